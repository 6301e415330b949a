"""Writes tests/golden/find_peaks.npz: what scipy.signal.find_peaks (scipy 1.15.3 when the file was made) returns for
short rows of small integers with repeated samples, NaN and +-inf, under every combination of open and closed borders
of height, threshold and prominence and several wlen.  Run it by hand when the file has to be made again:

    python tests/golden/make_peaks_golden.py

Layout (flat arrays, one zip member each): rows / row_offsets -- the float32 rows back to back; cases (N, 8) float64
-- row index, hmin, hmax, tmin, tmax, pmin, pmax (-inf / +inf: the border was None), wlen (0: None); peaks /
peak_offsets -- the positions of every case back to back; props (sum K, 4) float64 -- peak_heights, prominences,
left_bases, right_bases."""

import os
import warnings

import numpy as np
import scipy
import scipy.signal

CLOSED = [0.0, 2.0, 1.0, 3.0, 1.0, 4.0]           # hmin, hmax, tmin, tmax, pmin, pmax where a border is closed
WLENS = [0, 2, 3, 4, 7, 100]
N_ROWS, COMBOS_PER_ROW = 32, 32


def make_row(rng, k):
    n = int(rng.integers(3, 200)) if k >= 4 else k          # rows 0 .. 3: 0, 1, 2 and 3 samples
    x = rng.integers(-3, 4, size=n).astype(np.float32)
    if k % 3 == 1:
        x = np.repeat(x, rng.integers(1, 4, size=n))[:n]    # longer plateaus
    if k % 2 == 1:
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random(n) < 0.04] = value
    if k % 8 == 7 and n > 20:
        x[5:5 + n//3] = np.inf                              # a +inf plateau wider than the small windows
        x[4] = 1.0
        x[5 + n//3] = 0.0
    return x


def main():
    rng = np.random.default_rng(20240611)
    rows, cases, peaks, props = [], [], [], []
    for k in range(N_ROWS):
        x = make_row(rng, k)
        rows.append(x)
        for q in range(COMBOS_PER_ROW):
            combo = ((k + k//8)*COMBOS_PER_ROW + q) % 64    # bit b: border b is closed (k//8: no kind of row misses a half)
            wlen = WLENS[(k + q) % len(WLENS)]
            b = [CLOSED[i] if combo >> i & 1 else None for i in range(6)]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                p, pr = scipy.signal.find_peaks(x.astype(np.float64), height=(b[0], b[1]), threshold=(b[2], b[3]),
                                                prominence=(b[4], b[5]), wlen=wlen if wlen else None)
            open_ = [-np.inf, np.inf]*3
            cases.append([k] + [open_[i] if b[i] is None else b[i] for i in range(6)] + [wlen])
            peaks.append(p.astype(np.int64))
            props.append(np.stack((pr['peak_heights'], pr['prominences'], pr['left_bases'].astype(np.float64),
                                   pr['right_bases'].astype(np.float64)), axis=1).reshape(-1, 4))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'find_peaks.npz')
    np.savez_compressed(
        out, rows=np.concatenate(rows), row_offsets=np.cumsum([0] + [len(r) for r in rows]),
        cases=np.asarray(cases, dtype=np.float64), peaks=np.concatenate(peaks),
        peak_offsets=np.cumsum([0] + [len(p) for p in peaks]), props=np.concatenate(props),
        scipy_version=np.asarray(scipy.__version__))
    print(out, os.path.getsize(out), 'bytes,', len(cases), 'cases,', sum(len(p) for p in peaks), 'peaks')


if __name__ == '__main__':
    main()
