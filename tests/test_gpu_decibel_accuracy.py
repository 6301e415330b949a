"""The decibel kernels, element by element: hipdsp_decibel, hipdsp_decibel_image, hipdsp_decibel_image_decimate,
hipdsp_mean_spectrum_db and the dB epilogue of hipdsp_band_power under the pattern rules and the bound of
tests/decibel_bound.py (calibrated on the CPU by tests/test_decibel_bound.py), at every (ref_power, min_power) of
decibel_bound.PAIRS: the defaults, three min_power whose float32 cast rounds up (a power equal to that float is above
min_power and finite), denormal powers alive, and four ref_power whose float32 reciprocal or product leaves the normal
range.  One sweep of powers (every binade, the neighbours of every ref_power and min_power, 0, -0.0, a negative power,
NaN, +inf) feeds every entry point; every output buffer is filled with a sentinel first and must come back untouched
outside the written range.  test_zz_worst_per_entry_point prints the worst ratio error / bound measured (run with -s).
"""

import numpy as np
import pytest

import decibel_bound as dbb
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

SENTINEL = 0x7f7f7f7f
PAD = 8
P = dbb.sweep()
EDGES = dbb.edges()
WORST = {}


def note(entry, worst):
    WORST[entry] = max(WORST.get(entry, 0.0), worst)


def fresh(c, n):
    """n + PAD float32 on the device, every byte 0x7f."""
    from audian_amd import hipdsp
    a = hipdsp.DeviceArray(c, (n + PAD,), np.float32)
    hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(a), 0x7f, 4*(n + PAD))
    return a


def untouched(a, what):
    assert np.all(np.asarray(a).view(np.uint32) == SENTINEL), what + ': wrote outside its range'


def fill(shape, seed):
    """The sweep, cyclically from a seeded position, in `shape`."""
    n = int(np.prod(shape))
    return np.resize(np.roll(P, -17*seed), n).reshape(shape).copy()


# ---- hipdsp_decibel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ref_power,min_power', dbb.PAIRS)
def test_decibel(ref_power, min_power):
    """The 16-byte body and the scalar tail: every length modulo 4 at every pointer offset modulo 4; one value; 70001."""
    from audian_amd import hipdsp
    c = gh.ctx()
    big = np.resize(P, 70001 + 3)
    dp, dl = hipdsp.DeviceArray.from_host(c, P), hipdsp.DeviceArray.from_host(c, big)
    cases = [(dp, P, len(P) - 3 - off - k, off) for k in range(4) for off in range(4)]
    cases += [(dp, P, 1, off) for off in range(4)] + [(dl, big, 70001, 3), (dl, big, 70000, 0)]
    for src, host, n, off in cases:
        out = fresh(c, n + off)
        hipdsp.decibel(c, src.view(off, (n,)), out.view(off, (n,)), n, ref_power, min_power)
        got = out.to_host()
        what = 'hipdsp_decibel, n %d, offset %d' % (n, off)
        note('hipdsp_decibel', dbb.assert_within(got[off:off + n], host[off:off + n], ref_power, min_power, what))
        untouched(np.concatenate([got[:off], got[off + n:]]), what)


# ---- hipdsp_decibel_image ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('frames,F', [(70, 129), (33, 33), (1, 1), (32, 64)])
def test_decibel_image(frames, F):
    """Tile edges on both axes; the transposition is judged by position."""
    from audian_amd import hipdsp
    c = gh.ctx()
    for k, (ref_power, min_power) in enumerate(dbb.PAIRS):
        spec = fill((frames, F), frames + k)
        ds = hipdsp.DeviceArray.from_host(c, spec)
        out = fresh(c, frames*F)
        hipdsp.decibel_image(c, ds, out, frames, F, ref_power, min_power)
        got = out.to_host()
        what = 'hipdsp_decibel_image, %d x %d' % (frames, F)
        note('hipdsp_decibel_image', dbb.assert_within(got[:frames*F].reshape(F, frames), spec.T, ref_power, min_power, what))
        untouched(got[frames*F:], what)


# ---- hipdsp_decibel_image_decimate -------------------------------------------------------------------------------

DECIMATE = [(70, 129, 0, 70, 1), (1000, 1025, 3, 997, 28), (5000, 513, 100, 4999, 64), (33, 33, 32, 33, 4),
            (400, 2049, 0, 400, 400), (10, 5, 4, 4, 3)]                       # test_decimated_db_image's
DECIMATE += [(61, 33, 1, 60, step) for step in (7, 8, 9, 10, 11, 12)]          # the CPB switch; (b - a - 1) % 4 = 0 .. 3


@pytest.mark.parametrize('frames,F,start,stop,step', DECIMATE)
def test_decibel_image_decimate(frames, F, start, stop, step):
    """The column maximum is np.maximum.reduceat of the float32 slab, NaN included (NaNs sit first, last and inside
    segments); the dB of that is judged by position.  Whole segments hold one value around a min_power each, so the
    threshold values come out of the reduction."""
    from audian_amd import hipdsp
    c = gh.ctx()
    ncols = (stop - start + step - 1)//step
    spec = fill((frames, F), frames + step)
    for j in range(min(ncols, len(EDGES))):
        spec[start + j*step:min(start + (j + 1)*step, stop), j % F] = EDGES[j]
    for j, col in enumerate(range(1, ncols, 3)):
        a, b = start + col*step, min(start + (col + 1)*step, stop)
        spec[(a, b - 1, (a + b)//2)[j % 3], (5*j + 2) % F] = np.nan
    ds = hipdsp.DeviceArray.from_host(c, spec)
    if ncols:
        with np.errstate(invalid='ignore'):
            top = np.maximum.reduceat(spec[start:stop], np.arange(0, stop - start, step), axis=0)
        assert top.dtype == np.float32 and top.shape == (ncols, F)
    for ref_power, min_power in dbb.PAIRS:
        out = fresh(c, F*ncols)
        hipdsp.decibel_image_decimate(c, ds, out, frames, F, start, stop, step, ref_power, min_power)
        got = out.to_host()
        what = 'hipdsp_decibel_image_decimate, %d x %d, [%d, %d) by %d' % (frames, F, start, stop, step)
        if ncols:
            note('hipdsp_decibel_image_decimate',
                 dbb.assert_within(got[:F*ncols].reshape(F, ncols), top.T, ref_power, min_power, what))
        untouched(got[F*ncols:], what)


# ---- hipdsp_mean_spectrum_db -------------------------------------------------------------------------------------

def mean_case(frames, F):
    """(frames, F) powers: log-uniform random columns; from column 0 on constant columns around every min_power (their
    mean is the value itself); then one 1e30 among 1e-10s, a column that passes FLT_MAX as a sum but not as a mean, a
    NaN column, a +inf column, a zero column."""
    rng = np.random.default_rng([frames, F])
    spec = (10.0**rng.uniform(-24, 2, size=(frames, F))).astype(np.float32)
    if F > 1:
        nconst = min(len(EDGES), F - 6)
        spec[:, :nconst] = EDGES[:nconst]
        k = nconst
        spec[:, k] = 1e-10
        spec[frames//2, k] = 1e30
        spec[:, k + 1] = 3e38
        spec[frames//3, k + 2] = np.nan
        spec[frames - 1, k + 3] = np.inf
        spec[:, k + 4] = 0.0
    return spec


@pytest.mark.parametrize('F', [1, 129, 257])
@pytest.mark.parametrize('frames', [1, 63, 64, 65, 1000])
def test_mean_spectrum_db(frames, F):
    """Against the exact mean (longdouble over the float32 values), one rounding more than the stand-alone kernel; the
    slices change at 64 frames.  The floor replaces -inf and whatever lies under it: -200 and -37.5."""
    from audian_amd import hipdsp
    c = gh.ctx()
    spec = mean_case(frames, F)
    ds = hipdsp.DeviceArray.from_host(c, spec)
    for i0, i1 in sorted({(0, frames), (frames//3, frames)}):
        with np.errstate(all='ignore'):
            mean = np.sum(spec[i0:i1].astype(np.longdouble), axis=0)/np.longdouble(i1 - i0)
            p32 = mean.astype(np.float32)
        for k, (ref_power, min_power) in enumerate(dbb.PAIRS):
            floor_db = (-200.0, -37.5)[k % 2]
            out = fresh(c, F)
            hipdsp.mean_spectrum_db(c, ds, F, i0, i1, out, ref_power, min_power, floor_db)
            got = out.to_host()
            what = 'hipdsp_mean_spectrum_db, %d x %d, frames [%d, %d), floor %g' % (frames, F, i0, i1, floor_db)
            note('hipdsp_mean_spectrum_db', dbb.assert_within(got[:F], p32, ref_power, min_power, what, extra=1, arg=mean,
                                                              floor_db=floor_db))
            untouched(got[F:], what)


# ---- hipdsp_band_power, db ---------------------------------------------------------------------------------------

BAND_CASES = [(5, len(P), [(0, 1), (1, 5), (0, 5), (2, 2)]),                          # band_short_kernel, 4 bands
              (300, 2048, [(7, 8), (0, 300), (100, 164), (8, 9), (7, 7)]),            # a wave per frame, 16 band slots
              (8192, 64, [(4000, 8192)])]                                             # a workgroup per frame, 1 band


@pytest.mark.parametrize('ref_power,min_power', dbb.PAIRS)
def test_band_power_db(ref_power, min_power):
    """The first bin of the first band carries the sweep, so a one-bin band at scale 1 hands every sweep value to the
    threshold unchanged; the wider bands and scale 46.875 are judged against the exact band sum with one rounding more
    (the float32 rounding of scale * sum)."""
    from audian_amd import hipdsp
    c = gh.ctx()
    for nfreq, frames, bands in BAND_CASES:
        rng = np.random.default_rng([nfreq, frames])
        spec = (10.0**rng.uniform(-12, 2, size=(2, frames, nfreq))).astype(np.float32)
        k0, k1 = bands[0]
        spec[0, :, k0] = np.resize(P, frames)
        spec[1, :, k0] = np.resize(P[::-1], frames)
        ds = hipdsp.DeviceArray.from_host(c, spec)
        wide = spec.astype(np.longdouble)
        n = len(bands)*2*frames
        for scale in (1.0, 46.875):
            with np.errstate(all='ignore'):
                arg = np.stack([np.longdouble(scale)*np.sum(wide[:, :, k0:k1], axis=2) for k0, k1 in bands])
                p32 = arg.astype(np.float32)
            out = fresh(c, n)
            hipdsp.band_power(c, ds, 0, 2, frames, nfreq, bands, scale, out, db=True, ref_power=ref_power,
                              min_power=min_power)
            got = out.to_host()
            what = 'hipdsp_band_power, db, nfreq %d, scale %g' % (nfreq, scale)
            note('hipdsp_band_power, db', dbb.assert_within(got[:n].reshape(arg.shape), p32, ref_power, min_power, what,
                                                            extra=1, arg=arg))
            untouched(got[n:], what)
            if scale == 1.0 and k1 - k0 == 1:     # the one-bin band is the sweep itself: the threshold sees its values
                assert np.array_equal(p32[0], spec[:, :, k0], equal_nan=True)


def test_zz_worst_per_entry_point():
    for entry in sorted(WORST):
        print('%-34s worst error / bound %.3f' % (entry, WORST[entry]))
    assert all(w <= 1.0 for w in WORST.values())
