"""The definition of hipdsp_common_reference (include/hip_dsp.h) in numpy, and the comparator its tests share.

Per group g and sample t, members(g) = {c : group[c] == g}, refs(g) = {c in members(g) : use[c]} in ascending c:
    y[c, t] = float32(float64(x[c, t]) - ref_g[t])              for every member c, one rounding at the end
    mean:   ref = s / n, s the float64 sum of float64(x[k, t]) over refs(g), added one by one in ascending channel order
            from 0.0, n = |refs| as a float64
    median: the refs values ordered by value, the middle one for odd n, (float64(a) + float64(b)) * 0.5 for even n
A NaN among the refs values makes ref NaN; infinities follow IEEE arithmetic; channels of group -1 are copied."""

import numpy as np

MEAN, MEDIAN = 'mean', 'median'


def common_reference(x, group, use=None, mode=MEAN):
    """x: (channels, frames) float32.  Returns (channels, frames) float32."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    C, T = x.shape
    group = np.asarray(group, dtype=np.int64)
    use = np.ones(C, dtype=bool) if use is None else np.asarray(use).astype(bool)
    assert group.shape == (C,) and use.shape == (C,) and np.all((group >= -1) & (group < max(C, 1)))
    y = x.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        for g in sorted(set(group[group >= 0].tolist())):
            members = [c for c in range(C) if group[c] == g]
            refs = [c for c in members if use[c]]
            assert refs, 'a group with members and no reference channel'
            n = len(refs)
            if mode == MEAN:
                s = np.zeros(T, dtype=np.float64)
                for k in refs:                                   # one by one, ascending
                    s = s + x[k].astype(np.float64)
                ref = s/np.float64(n)
            else:
                assert mode == MEDIAN
                v = np.sort(x[refs].astype(np.float64), axis=0)  # NaNs last
                ref = v[n//2].copy() if n % 2 else (v[n//2 - 1] + v[n//2])*0.5
                ref[np.isnan(v[-1])] = np.nan
            for c in members:
                y[c] = (x[c].astype(np.float64) - ref).astype(np.float32)
    return y


def assert_same(got, want, what=''):
    """An equal NaN pattern, equal float32 bits elsewhere; a zero on both sides passes whatever its sign."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), '%s: NaN pattern differs at %s' % (what, np.argwhere(gn != wn)[:4].tolist())
    zero = (got == 0) & (want == 0)
    same = gn | zero | (got.view(np.uint32) == want.view(np.uint32))
    if not np.all(same):
        at = np.argwhere(~same)
        i = tuple(at[0])
        raise AssertionError('%s: %d of %d values differ, first at %s: got %r, want %r'
                             % (what, len(at), got.size, list(i), got[i], want[i]))
