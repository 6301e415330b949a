"""Writes tests/golden/region_xcorr.npz: what np.corrcoef returns, in float64, for windows of a small array against
shifted windows of its rows -- the pin of tests/xcorr_definition.py.  numpy only.  Run it by hand when the file has to be
made again:

    python tests/golden/make_xcorr_golden.py

Layout: x (3, 700) float32, the array (xcorr_definition.slab('small') when the file was made, with a constant stretch
and one NaN put in); cases (N, 5) int64 -- channel, start, stop, partner, max_lag; rows / row_offsets -- per case the 2
max_lag + 1 float64 values np.corrcoef(a, b_l)[0, 1] back to back, NaN where the shifted window leaves the row (and where
numpy itself gives NaN: a constant window, a NaN sample)."""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import xcorr_definition as xd  # noqa: E402

CASES = [(0, 10, 310, 1, 12), (0, 10, 310, 0, 3), (2, 0, 700, 1, 5), (1, 350, 355, 2, 300), (1, 3, 40, 0, 9),
         (2, 660, 700, 2, 9), (0, 400, 430, 1, 20), (1, 400, 430, 0, 20), (0, 480, 540, 2, 30), (1, 100, 100, 0, 2),
         (1, 100, 101, 0, 2)]


def main():
    x = xd.slab('small').copy()
    x[1, 405:445] = 0.5                                 # constant: partner windows of case 6, the event window of case 7
    x[2, 520] = np.nan                                  # inside some partner windows of case 8
    rows = []
    for c, a, b, p, L in CASES:
        row = np.full(2*L + 1, np.nan)
        for l in range(-L, L + 1):
            if b - a >= 1 and a + l >= 0 and b + l <= x.shape[1]:
                with warnings.catch_warnings(), np.errstate(all='ignore'):
                    warnings.simplefilter('ignore')
                    row[L + l] = np.corrcoef(x[c, a:b].astype(np.float64), x[p, a + l:b + l].astype(np.float64))[0, 1]
        rows.append(row)
    out = os.path.join(HERE, 'region_xcorr.npz')
    np.savez_compressed(out, x=x, cases=np.array(CASES, dtype=np.int64), rows=np.concatenate(rows),
                        row_offsets=np.cumsum([0] + [len(r) for r in rows]))
    print('%s: %d cases, %d values, %d of them NaN, numpy %s, %d bytes'
          % (out, len(CASES), sum(len(r) for r in rows), int(sum(np.isnan(r).sum() for r in rows)), np.__version__,
             os.path.getsize(out)))


if __name__ == '__main__':
    main()
