"""The FIR bank's definition (include/hip_dsp.h: hipdsp_fir_bank) written out in numpy float64 -- the comparator of
tests/test_kernelfilter_host.py and tests/test_gpu_firbank.py, never the code under test."""

import numpy as np


def fir_windows(x, n_taps, t):
    """(len(t), n_taps) array W with W[i, j] = x[t[i] + (n_taps-1)//2 - (n_taps-1) + j], zero outside [0, len(x)):
    the window under output t[i], oldest sample first (tap n_taps-1-j meets column j)."""
    x = np.asarray(x)
    t = np.asarray(t, dtype=np.int64)
    lead = (n_taps - 1)//2
    if len(t) == 0:
        return np.zeros((0, n_taps), dtype=x.dtype)
    tail = max(0, int(t.max()) + lead + 1 - len(x))
    padded = np.concatenate((np.zeros(n_taps - 1, dtype=x.dtype), x, np.zeros(tail, dtype=x.dtype)))
    rows = np.lib.stride_tricks.sliding_window_view(padded, n_taps)
    return rows[t + lead]                               # row r starts at padded[r] = x[r - (n_taps-1)]


def fir_definition(x, taps, first=0, step=1, n=None, with_abs=False, chunk=1 << 22):
    """y[k, c, i] = sum_j taps[k, j] * x[c, first + i*step + (L-1)//2 - j], x zero outside its frames.
    x: (channels, frames), taps: (kernels, L); float64 unless both are integer arrays (then int64, exact).
    with_abs: returns (y, M), M the same sum over |taps| and |x| (the M of the error bound)."""
    x, taps = np.atleast_2d(x), np.atleast_2d(taps)
    exact = np.issubdtype(x.dtype, np.integer) and np.issubdtype(taps.dtype, np.integer)
    dt = np.int64 if exact else np.float64
    x, taps = x.astype(dt), taps.astype(dt)
    frames, n_taps = x.shape[1], taps.shape[1]
    if n is None:
        n = max(0, -(-(frames - first)//step))
    t = first + step*np.arange(n, dtype=np.int64)
    y = np.zeros((len(taps), len(x), n), dtype=dt)
    m = np.zeros_like(y) if with_abs else None
    flipped = np.ascontiguousarray(taps[:, ::-1])
    rows = max(1, chunk//n_taps)
    for c in range(len(x)):
        for a in range(0, n, rows):
            w = fir_windows(x[c], n_taps, t[a:a + rows])
            y[:, c, a:a + rows] = flipped @ w.T
            if with_abs:
                m[:, c, a:a + rows] = np.abs(flipped) @ np.abs(w).T
    return (y, m) if with_abs else y


def fir_bound(abs_sum, n_taps, threshold=None):
    """The header's bound on |out - y_float64|: n u / (1 - n u) * M with u = 2^-24, n = L + 2; rectified:
    (n+1) u / (1 - (n+1) u) * (M + |threshold|)."""
    u = 2.0**-24
    n = n_taps + 2 + (0 if threshold is None else 1)
    extra = 0.0 if threshold is None else np.abs(threshold)
    return n*u/(1.0 - n*u)*(abs_sum + extra)
