"""The definition of hipdsp_power_envelope (include/hip_dsp.h) -- the reference's envelope() (songdetector.py:57-69) -- on
top of tests/iir_bound.py, the wrong versions its calibration must catch and the reference's step rule.

For one row v of float32 samples, a table of S <= 2 sections and scipy's default pad length:

    u    = float64(v)**2                      exact: 24 + 24 bits
    f    = sosfiltfilt(sos, u)                scipy's odd extension OF u, zi-scaled forward and backward pass:
                                              iir_bound.sosfiltfilt(sos, u, gain=1, rectify=False, clamp=False)
    p[j] = float32(gain * max(f[first + j*step], 0)),  j < n_out         the product in float64, ONE rounding
    y[j] = p[j] (root == 0), np.sqrt(p[j]) in float32 (root != 0): the correctly rounded root

Arrays are (T, lanes) as everywhere in iir_bound.  Nothing here imports scipy."""

import numpy as np

import iir_bound as ib

LD = ib.LD

# label: (order, Wn, btype, rate, families)                              sections, padlen
FAMILIES = ('stepdown', 'stepup', 'offset', 'burst')
FILTERS = {
    'lp1 500 Hz @ 96 kHz': (1, 500.0, 'lowpass', 96000.0, FAMILIES),       # 1, 6
    'lp1 20 Hz @ 96 kHz': (1, 20.0, 'lowpass', 96000.0, FAMILIES),         # 1, 6
    'lp2 500 Hz @ 48 kHz': (2, 500.0, 'lowpass', 48000.0, FAMILIES),       # 1, 9
    'lp3 200 Hz @ 44.1 kHz': (3, 200.0, 'lowpass', 44100.0, FAMILIES),     # 2, 12
    'lp4 300 Hz @ 48 kHz': (4, 300.0, 'lowpass', 48000.0, FAMILIES),       # 2, 15
}
T_CASE = 3*4096 + 5
WRONG = ('float32 squares', 'float32 between the passes', 'float32 state every 2048 samples', 'extension of the samples')


def design(case):
    """(sos, rate, families) of a case of FILTERS."""
    return ib.design(case, FILTERS)


def first_order_sos(cutoff, rate):
    """butter(1, cutoff/(rate/2)) as ONE section with b2 = a2 = 0 (padlen 6), the reference's filter; None where scipy
    would reject the design."""
    from audian_amd.design import butter_sos
    try:
        return butter_sos(1, float(cutoff), 'lowpass', float(rate))
    except ValueError:
        return None


def reference_step(rate, cutoff):
    """songdetector.py:63-66: envrate = min(10 cutoff, rate), step = int(np.round(rate / envrate))."""
    envrate = cutoff*10
    if envrate > rate:
        envrate = rate
    return int(np.round(rate/envrate))


def grid_size(frames, first, step):
    """How many samples first + j*step lie in [0, frames): len(range(first, frames, step))."""
    return max(0, -(-(frames - first)//step))


def squares(x, dtype=LD):
    x = np.asarray(x)
    assert x.dtype == np.float32
    u = x.astype(np.float64)**2
    assert np.array_equal(u, (x.astype(LD)**2).astype(np.float64)), 'a square of a float32 is exact in float64'
    return u.astype(dtype)


def filtered_squares(sos, x, dtype=LD):
    """f of the definition, (T, lanes) in `dtype`, unclamped."""
    return ib.sosfiltfilt(sos, squares(x, np.float64), dtype, gain=1.0, rectify=False, clamp=False)


def power_envelope(sos, x, first=0, step=1, n_out=None, gain=4.0, root=True, dtype=LD):
    """The definition, (n_out, lanes) float32."""
    f = filtered_squares(sos, x, dtype)
    if n_out is None:
        n_out = grid_size(len(f), first, step)
    assert n_out == 0 or first + (n_out - 1)*step < len(f)
    picked = f[first::step][:n_out]
    p = (dtype(gain)*np.where(picked < 0, dtype(0), picked)).astype(np.float32)
    return np.sqrt(p) if root else p


def runs(sos, x):
    """(reference f in longdouble, the sequential float64 run), cached per (filter, input)."""
    return ib._cached(ib._key(sos, x, 'power envelope'),
                      lambda: (filtered_squares(sos, x, LD), filtered_squares(sos, x, np.float64)))


def case(sos, x):
    """(reference f, q per lane) of the unclamped filtered squares of x."""
    ref, run = runs(sos, x)
    return ref, ib.allowance(run, ref)


def wrong(sos, x, which):
    """The float64 run of f with one of the mistakes of WRONG in it, (T, lanes) float64.  For the calibration only."""
    assert which in WRONG, which
    x = np.asarray(x)
    edge = ib.padlen(sos)
    u = squares(x, np.float64)
    if which == 'float32 squares':
        u = (x*x).astype(np.float64)                                    # the float32 product
    if which == 'extension of the samples':
        v = x.astype(np.float64)
        left, right = (2*v[0] - v[edge:0:-1])**2, (2*v[-1] - v[-2:-(edge + 2):-1])**2
    else:
        left, right = 2*u[0] - u[edge:0:-1], 2*u[-1] - u[-2:-(edge + 2):-1]
    ext = np.concatenate([left, u, right])
    zi = ib.sosfilt_zi(sos, np.float64)
    every = 2048 if which == 'float32 state every 2048 samples' else 0
    y = ib.sosfilt(sos, ext, np.float64, zi=zi[:, :, None]*ext[0][None, None, :], round_state_every=every)
    if which == 'float32 between the passes':
        y = y.astype(np.float32).astype(np.float64)
    back = ib.sosfilt(sos, y[::-1], np.float64, zi=zi[:, :, None]*y[-1][None, None, :], round_state_every=every)
    return back[::-1][edge:edge + len(x)]


def host_power_envelope(sos, slab, first=0, step=1, n_out=None, gain=4.0, root=True):
    """audian_amd.bufferedpowerenvelope.power_envelope_host, for the tests that compare with it."""
    from audian_amd.bufferedpowerenvelope import power_envelope_host
    return power_envelope_host(sos, slab, first, step, n_out, gain, root)
