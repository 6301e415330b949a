"""The definition of hipdsp_find_peaks (include/hip_dsp.h) as plain loops over one row, written from its sentences and
sharing nothing with audian_amd/peaks.py: the comparator of tests/test_peaks_host.py and tests/test_gpu_peaks.py.
tests/golden/find_peaks.npz pins it to scipy.signal.find_peaks (scipy 1.15.3)."""

import math

import numpy as np

OPEN = (-math.inf, math.inf)


def inside(value, lo, hi):
    """An open border is not compared; NaN fails any comparison that is made."""
    if lo != -math.inf and not lo <= value:
        return False
    if hi != math.inf and not value <= hi:
        return False
    return True


def local_maxima(v):
    """[(l, r)] of the runs of equal samples that are peaks, ascending."""
    n = len(v)
    out = []
    l = 0
    while l < n:
        r = l
        while r + 1 < n and v[r + 1] == v[r]:
            r += 1
        if l >= 1 and r <= n - 2 and v[l - 1] < v[l] and v[r + 1] < v[r]:
            out.append((l, r))
        l = r + 1
    return out


def walk(v, m, limit, step):
    """(minimum, base) of the walk from m towards limit while v[i] <= v[m]."""
    h = v[m]
    low, base = h, m
    i = m
    while (i >= limit if step < 0 else i <= limit) and v[i] <= h:
        if v[i] < low:
            low, base = v[i], i
        i += step
    return low, base


def find_peaks(row, height=OPEN, threshold=OPEN, prominence=OPEN, wlen=0, first=0):
    """(positions, properties): lists of ints and of [height, prominence, left_base, right_base] (floats and ints),
    `first` added to positions and bases.  Every condition is a (lower, upper) pair, -inf / +inf an open border."""
    v = [float(s) for s in np.asarray(row, dtype=np.float32)]
    n = len(v)
    positions, properties = [], []
    for l, r in local_maxima(v):
        m = (l + r)//2
        h = v[m]
        if not inside(h, *height):
            continue
        tl, tr = h - v[m - 1], h - v[m + 1]
        if not (inside(tl, *threshold) and inside(tr, *threshold)):       # min and max that pass a NaN on
            continue
        lo, hi = 0, n - 1
        if wlen >= 2:
            lo, hi = max(m - wlen//2, 0), min(m + wlen//2, n - 1)
        left_min, left_base = walk(v, m, lo, -1)
        right_min, right_base = walk(v, m, hi, +1)
        prom = h - max(left_min, right_min)
        if not inside(prom, *prominence):
            continue
        positions.append(m + first)
        properties.append([h, prom, left_base + first, right_base + first])
    return positions, properties


def same(got_positions, got_properties, want):
    """Exact equality of a (positions array, (K, 4) array) result with find_peaks' lists, NaN equal to NaN."""
    positions, properties = want
    got_positions = np.asarray(got_positions)
    got_properties = np.asarray(got_properties, dtype=np.float64).reshape(-1, 4)
    if got_positions.tolist() != list(positions):
        return False
    want_props = np.asarray(properties, dtype=np.float64).reshape(-1, 4)
    return bool(np.array_equal(got_properties, want_props, equal_nan=True))
