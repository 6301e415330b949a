"""The definition of hipdsp_bin_quantiles and hipdsp_spec_equalize (include/hip_dsp.h) in numpy, and the cases both
noise-profile test files share.  Nothing here imports the code under test.

bin_quantiles_column is the sequential definition of one column: drop the NaNs, sort, pos = q*(n - 1) as one double
multiply, the two elements and the count.  bin_quantiles is the same thing for a whole slab with one np.sort along the
frames (numpy sorts NaN behind everything, so the first n of a sorted column are its values); the host tests hold the
two to each other and to np.percentile."""

import numpy as np

NAN32 = np.float32(np.nan)


def bin_quantiles_column(values, q):
    """(lo, hi, n) of one column of float32 values."""
    v = np.asarray(values, dtype=np.float32)
    v = np.sort(v[~np.isnan(v)])
    n = len(v)
    if n == 0:
        return NAN32, NAN32, 0
    pos = float(q)*float(n - 1)
    k_lo = int(np.floor(pos))
    k_hi = min(k_lo + 1, n - 1)
    return v[k_lo], v[k_hi], n


def bin_quantiles(spec, first, n_frames, frame_step, k0, k1, q):
    """spec (channels, frames, nfreq) float32 -> lo_hi (channels, k1 - k0, 2) float32, count (channels, k1 - k0) int32."""
    spec = np.asarray(spec, dtype=np.float32)
    C = spec.shape[0]
    W = k1 - k0
    rows = first + frame_step*np.arange(n_frames)
    x = np.sort(spec[:, rows, k0:k1], axis=1)                     # NaN last
    count = np.sum(~np.isnan(x), axis=1).astype(np.int32)         # (C, W)
    lo_hi = np.full((C, W, 2), np.nan, dtype=np.float32)
    if n_frames == 0 or W == 0 or C == 0:
        return lo_hi, count
    n = count.astype(np.int64)
    pos = float(q)*(n - 1).astype(np.float64)
    k_lo = np.clip(np.floor(pos).astype(np.int64), 0, None)
    k_hi = np.clip(np.minimum(k_lo + 1, n - 1), 0, None)
    lo = np.take_along_axis(x, k_lo[:, None, :], axis=1)[:, 0, :]
    hi = np.take_along_axis(x, k_hi[:, None, :], axis=1)[:, 0, :]
    lo_hi[:, :, 0] = np.where(n > 0, lo, NAN32)
    lo_hi[:, :, 1] = np.where(n > 0, hi, NAN32)
    return lo_hi, count


def finish_percentile(lo_hi, count, q):
    """The percentile the host makes of the two order statistics, float64: lo when frac == 0 or hi == lo, else
    lo + frac*(hi - lo) (what np.percentile's linear interpolation gives)."""
    lo = np.asarray(lo_hi[..., 0], dtype=np.float64)
    hi = np.asarray(lo_hi[..., 1], dtype=np.float64)
    n = np.asarray(count, dtype=np.int64)
    pos = float(q)*np.maximum(n - 1, 0).astype(np.float64)
    frac = pos - np.floor(pos)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where((frac == 0) | (hi == lo), lo, lo + frac*(hi - lo))


def equalize(spec, profile, mode):
    """spec (channels, frames, nfreq) float32, profile (channels, nfreq) float32, in numpy's float32 arithmetic:
    'divide' spec/profile; 'subtract' spec - profile, then 0 where that is < 0."""
    spec = np.asarray(spec, dtype=np.float32)
    prof = np.asarray(profile, dtype=np.float32)[:, None, :]
    with np.errstate(all='ignore'):
        if mode == 'divide':
            return (spec/prof).astype(np.float32)
        if mode == 'subtract':
            d = (spec - prof).astype(np.float32)
            return np.where(d < 0, np.float32(0), d)
    raise ValueError(mode)


def canonical_bits(a):
    """The uint32 bits of float32 values with -0 turned into +0 and every NaN into one pattern."""
    a = np.array(a, dtype=np.float32)
    a[a == 0] = 0.0
    a[np.isnan(a)] = NAN32
    return a.view(np.uint32)


def same_bits(got, want):
    """Equal bit for bit, where the sign of a zero and the payload of a NaN are left open."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(canonical_bits(got), canonical_bits(want))


def exact_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float32).view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))


# ---- cases ------------------------------------------------------------------------------------------------------

def _bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def _noise(rng, n):
    return np.power(10.0, rng.uniform(-12.0, 6.0, n)).astype(np.float32)


def _equal(rng, n):
    return np.full(n, 3.25, dtype=np.float32)


def _ties(rng, n):
    # five values on both sides of a boundary of the second, third and fourth radix digit
    pool = _bits([0x3effffff, 0x3f000000, 0x3f7fffff, 0x3f800000, 0x3f800001])
    return pool[rng.integers(0, len(pool), n)]


def _low_byte(rng, n):
    return _bits(0x3f800000 | rng.integers(0, 256, n).astype(np.uint32))


def _high_byte(rng, n):
    # (exponent 0xfe at most: finite, both signs)
    return _bits((rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456))


def _signed(rng, n):
    v = rng.normal(0.0, 1.0, n).astype(np.float32)
    special = np.concatenate((np.array([0.0, -0.0, np.inf, -np.inf], dtype=np.float32),
                              _bits([0x00000001, 0x007fffff, 0x80000001, 0x807fffff])))
    where = rng.random(n) < 0.3
    v[where] = special[rng.integers(0, len(special), int(where.sum()))]
    return v


def _nan_some(rng, n):
    v = _noise(rng, n)
    v[rng.random(n) < 0.3] = np.nan
    return v


def _nan_all(rng, n):
    return np.full(n, np.nan, dtype=np.float32)


def _nan_but_one(rng, n):
    v = np.full(n, np.nan, dtype=np.float32)
    if n:
        v[int(rng.integers(0, n))] = 2.5
    return v


KINDS = (_noise, _equal, _ties, _low_byte, _high_byte, _signed, _nan_some, _nan_all, _nan_but_one)


def mixed_slab(rng, channels, frames, nfreq, rot=0):
    """(channels, frames, nfreq) float32: column (c, k) holds the kind (c*nfreq + k + rot) mod len(KINDS), so every kind
    of value meets every tile position once the slab is wider than the list."""
    spec = np.empty((channels, frames, nfreq), dtype=np.float32)
    for c in range(channels):
        for k in range(nfreq):
            spec[c, :, k] = KINDS[(c*nfreq + k + rot) % len(KINDS)](rng, frames)
    return spec


def exact_q(n):
    """A q strictly inside (0, 1) whose pos = q*(n - 1) is an exact integer for n values: 0.25 when n - 1 is a multiple
    of four, else 0.5 for an odd n (None when neither holds)."""
    if n >= 5 and (n - 1) % 4 == 0:
        return 0.25
    if n >= 3 and (n - 1) % 2 == 0:
        return 0.5
    return None


QS = (0.0, 0.05, 0.5, 0.95, 1.0)
