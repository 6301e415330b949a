"""The inputs tests/test_gpu_template_match.py runs hipdsp_template_match on, built on the host so that
tests/test_template_match_host.py can check, without a GPU, what the GPU test relies on: that with min_std = MIN_STD_DB
no window of the dB slab lies near the mask threshold."""

import numpy as np

FRAMES, CHANNELS = 300, 3
# (nfreq, k0, Fb, Tt): a band that is no multiple of 4 and narrower than a chunk; a band of several chunks and a
# remainder of one bin under 32 frames; the full band, again with a one-bin remainder; one tap; windows of 256 frames,
# longer than a tile (the chunk narrows to keep the tile in LDS).  300 - Tt + 1 windows: a tail tile everywhere, more
# than one tile for all but the last.
SHAPES = [(33, 3, 27, 7), (129, 5, 97, 32), (129, 0, 129, 5), (1025, 100, 1, 1), (33, 0, 33, 256)]
FLOOR_LEVEL_DB, SPREAD_DB = -90.0, 5.0
FLOOR_DB = -120.0                 # the floor the dB cases pass: the zero frames sit there
MIN_STD_DB = 0.1
MIN_STD_LINEAR = 1e-11            # in power units: the floor's own spread is some 1e-10
CONSTANT = slice(100, 140)
ZEROS = slice(200, 215)
NAN_FRAME, INF_FRAME = 30, 250


def slab(shape):
    """(CHANNELS, FRAMES, nfreq) float32 powers: a noise floor at FLOOR_LEVEL_DB of SPREAD_DB spread, bumps of up to
    40 dB, 40 constant frames, 15 zero frames; in channel 1 a NaN and in channel 2 a +inf just inside the band, and in
    every channel NaN and +inf in the bins just outside it (where there are any)."""
    nfreq, k0, Fb, Tt = shape
    rng = np.random.default_rng(nfreq*1000 + Fb)
    db = FLOOR_LEVEL_DB + rng.uniform(-SPREAD_DB/2, SPREAD_DB/2, (CHANNELS, FRAMES, nfreq))
    f = np.arange(FRAMES)[:, None]
    k = np.arange(nfreq)[None, :]
    for c in range(CHANNELS):
        for _ in range(12):
            fc, kc = rng.uniform(0, FRAMES), rng.uniform(k0, k0 + Fb)
            sf, sk = rng.uniform(2, 8), rng.uniform(0.7, 6)
            db[c] += rng.uniform(10, 40)*np.exp(-0.5*((f - fc)/sf)**2 - 0.5*((k - kc)/sk)**2)
    p = (10.0**(db/10.0)).astype(np.float32)
    p[:, CONSTANT, :] = np.float32(1e-9)
    p[:, ZEROS, :] = 0.0
    if k0 > 0:
        p[:, 10::17, k0 - 1] = np.nan
        p[:, 11::17, k0 - 1] = np.inf
    if k0 + Fb < nfreq:
        p[:, 12::17, k0 + Fb] = np.nan
        p[:, 13::17, k0 + Fb] = np.inf
    p[1, NAN_FRAME, k0 + Fb//2] = np.nan
    p[2, INF_FRAME, k0] = np.inf
    return p


def decibel_host(p, floor=FLOOR_DB):
    """10 log10(p) in float64, rounded to float32 and floored: NOT hipdsp_decibel's bits, only near them -- for the
    host-side check of the mask margins (the GPU test takes v from hipdsp_decibel itself)."""
    with np.errstate(all='ignore'):
        v = (10.0*np.log10(p.astype(np.float64))).astype(np.float32)
    return np.where(v < floor, np.float32(floor), v)


def templates(shape, K=16, integer=False):
    """K templates (K, Tt, Fb) float64: dB-like patches (a ridge that sweeps through the band plus noise), or small
    integers."""
    nfreq, k0, Fb, Tt = shape
    rng = np.random.default_rng(7*nfreq + Tt)
    if integer:
        return rng.integers(-4, 5, (K, Tt, Fb)).astype(np.float64)
    a = np.arange(Tt)[:, None]/max(Tt - 1, 1)
    b = np.arange(Fb)[None, :]/max(Fb - 1, 1)
    out = np.empty((K, Tt, Fb))
    for j in range(K):
        sweep = rng.uniform(-0.6, 0.6)
        out[j] = FLOOR_LEVEL_DB + 30.0*np.exp(-0.5*((b - 0.5 - sweep*(a - 0.5))/0.15)**2) + rng.uniform(-2.5, 2.5, (Tt, Fb))
    return out
