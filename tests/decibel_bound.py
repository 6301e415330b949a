"""A per-element bound for the decibel kernels, and the sweep of powers it is applied to.

The contract (include/hip_dsp.h): out = 10 log10(p / ref_power), -inf where p <= min_power, with ref_power and min_power
doubles and p a float32.  The suite's older checks are absolute (1e-4 or 1e-3 dB) at ref_power 1 on log-uniform random
powers: near 0 dB 1e-4 dB is 2.3e-5 of the argument, 390 float32 roundings.  Here every element is judged.

The pattern, exact, no element exempt:  -inf exactly where float64(p) <= min_power (negative p and -0.0 included), NaN
exactly where p is NaN, +inf exactly where p is +inf, finite everywhere else.

The finite elements, against ref = 10 log10(p / ref_power) in np.longdouble from the exact float32 p:

    |got - ref| <= a (10 / ln 10) 2^-24 + b ulp32(ref)

a counts the float32 roundings of the logarithm's argument (each moves the result by at most (10 / ln 10) 2^-24 dB):
0 at ref_power == 1, where the reciprocal and the product are exact, otherwise 2 (the float32 reciprocal, the product);
one more for hipdsp_mean_spectrum_db (its float64 mean, rounded to float32 once; the float64 sum of at most 2^31 float32
terms costs under 2^-22 of a rounding) and one more for hipdsp_band_power with db (the one rounding of scale * sum its
header states); where that rounding lands on a denormal float it is absolute, 2^-150, and counts as such (rounding_db).  b = 1.25 u + 0.5: u the ulp bound of log10f, 1.25 from the multiplication by ten (ten ulps of y are at
most 1.25 ulps of 10 y: the worst case is 10 y just above a power of two), 0.5 the product's own rounding.  u = 2 is
what HIP documents for log10f; the ROCm tree this was written against carries no document that states another figure
(its headers and the device library declare log10f without one), so 2 stands.  u is never read off a kernel's output.
tests/test_decibel_bound.py calibrates the bound on the CPU.
"""

import math

import numpy as np

U_LOG10F = 2.0
B = 1.25*U_LOG10F + 0.5
DB_PER_ROUNDING = 10.0/math.log(10.0)*2.0**-24

# (ref_power, min_power): the defaults; three min_power whose float32 cast rounds up; denormal powers alive; four
# ref_power whose float32 reciprocal or product with a float32 power leaves the normal range
PAIRS = ((1.0, 1e-20), (2.5, 1e-7), (1e-6, 0.1), (3.0, 1e-10), (1e12, 0.0),
         (1e-39, 1e-20), (1e39, 1e-20), (1e-30, 1e-20), (1e30, 1e-20))


def roundings(ref_power, extra=0):
    return (0 if ref_power == 1 else 2) + extra


def ulp32(x):
    """The float32 spacing at |x| (2^-149 at and below the denormals), for float64 / longdouble x."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(np.where(np.isfinite(x), x, 1.0))[1]           # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def rounding_db(p, arg):
    """What the float32 rounding of the argument `arg` to `p` may move the result by, in dB: (10 / ln 10) 2^-24 for a
    normal p; a denormal p is rounded absolutely, by up to 2^-150, which is 2^-150 / arg of the argument."""
    with np.errstate(all='ignore'):
        rel = (2.0**-150/np.abs(np.asarray(arg, dtype=np.longdouble))).astype(np.float64)
        wide = -10.0*np.log10(1.0 - np.minimum(rel, 1.0))
    return np.where(np.abs(p) < np.finfo(np.float32).tiny, wide, DB_PER_ROUNDING)


def reference(arg, ref_power):
    """10 log10(arg / ref_power) in longdouble; meaningful where arg is finite and positive."""
    with np.errstate(all='ignore'):
        return 10.0*np.log10(np.asarray(arg, dtype=np.longdouble)/np.longdouble(ref_power))


def neighbours(x, k):
    """The k float32 values on each side of float32(x), and float32(x) itself, ascending."""
    x = np.float32(x)
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out = [lo] + out + [hi]
    return np.array(out, dtype=np.float32)


def edges(pairs=PAIRS):
    """The three float32 values around every min_power of `pairs` (below, float32(min_power), above), ascending."""
    return np.unique(np.concatenate([neighbours(mp, 1) for mp in sorted({mp for _, mp in pairs})]))


def sweep(seed=0, pairs=PAIRS):
    """About 20k float32 powers, one vector for every test: every binade from the smallest denormal to FLT_MAX with the
    mantissas 1, 1 + 2^-23, 2 - 2^-23 and random ones (the denormal binades: their first, second, last and random
    members), the 16 float32 neighbours on each side of every ref_power of `pairs`, the three float32 values around
    every min_power, 0, -0.0, a negative power, NaN and +inf; shuffled."""
    rng = np.random.default_rng(seed)
    bits = []
    for e in range(1, 255):                                       # the normal binades
        m = np.concatenate([[0, 1, 0x7fffff], rng.integers(2, 0x7fffff, 73)])
        bits.append((e << 23) | m)
    for k in range(23):                                           # the denormal binades [2^k, 2^(k+1)) in units of 2^-149
        lo, n = 1 << k, 1 << k
        m = np.unique(np.concatenate([[0, min(1, n - 1), n - 1], rng.integers(0, n, 8)]))
        bits.append(lo + m)
    p = np.concatenate(bits).astype(np.uint32).view(np.float32)
    with np.errstate(over='ignore'):
        edge = [neighbours(rp, 16) for rp in sorted({rp for rp, _ in pairs})]
    p = np.concatenate([p] + edge + [edges(pairs), np.array([0.0, -0.0, -1.5, np.nan, np.inf], dtype=np.float32)])
    return p[rng.permutation(len(p))]


def failures(got, p, ref_power, min_power, extra=0, arg=None, floor_db=None):
    return judge(got, p, ref_power, min_power, extra, arg, floor_db)[:2]


def judge(got, p, ref_power, min_power, extra=0, arg=None, floor_db=None):
    """failures() and, third, the mask of the elements that break a pattern rule or the bound.  Judges `got` (float32) for the float32 powers `p`: returns (worst ratio of the finite elements, list of messages,
    empty when all is well).  `arg` is the exact argument of the logarithm where that is not p itself (the exact mean
    or band sum, longdouble) -- p is then its float32 rounding, which the threshold sees.  With `floor_db`
    (hipdsp_mean_spectrum_db) -inf has become exactly the floor, nothing lies below it, and the reference is
    max(ref, floor): a result pulled up to the floor is no further from that than it was from ref."""
    got = np.asarray(got)
    p = np.asarray(p, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == p.shape
    bad, mask = [], np.zeros(p.shape, bool)
    ninf = p.astype(np.float64) <= min_power
    nan = np.isnan(p)
    pinf = np.isposinf(p) & ~ninf
    fin = ~(ninf | nan | pinf)
    if floor_db is None:
        checks = (('-inf', ninf, np.isneginf(got)), ('finite', fin, np.isfinite(got)))
    else:
        with np.errstate(invalid='ignore'):
            checks = (('floor at -inf', ninf, ninf & (got == np.float32(floor_db))),
                      ('finite', fin | ninf, np.isfinite(got)),
                      ('nothing under the floor', np.zeros(p.shape, bool), got < np.float32(floor_db)))
    for name, want, have in checks + (('NaN', nan, np.isnan(got)), ('+inf', pinf, np.isposinf(got))):
        mask |= want != have
        wrong = np.nonzero(want != have)
        if len(wrong[0]):
            i = tuple(int(w[0]) for w in wrong)
            bad.append('%d element(s) break the %s pattern, first at %s: power %r (min_power %r) gave %r'
                       % (len(wrong[0]), name, i, float(p[i]), min_power, float(got[i])))
    ok = fin & np.isfinite(got)
    worst = 0.0
    if ok.any():
        ref = reference(p if arg is None else arg, ref_power)[ok]
        if floor_db is not None:
            ref = np.maximum(ref, np.longdouble(floor_db))
        err = np.abs(got[ok].astype(np.longdouble) - ref).astype(np.float64)
        bound = roundings(ref_power)*DB_PER_ROUNDING + B*ulp32(ref)
        if extra:
            bound = bound + extra*rounding_db(p[ok], (p if arg is None else arg)[ok])
        ratio = err/bound
        j = int(np.argmax(ratio))
        worst = float(ratio[j])
        mask[ok] |= ratio > 1.0
        if worst > 1.0:
            i = tuple(int(w[j]) for w in np.nonzero(ok))
            bad.append('%d element(s) over the bound, worst at %s: power %r gave %r dB, reference %.9g, error %.3g = '
                       '%.3g of the bound (a = %d, b = %g)' % (int(np.sum(ratio > 1.0)), i, float(p[i]), float(got[i]),
                                                               float(ref[j]), err[j], worst,
                                                               roundings(ref_power, extra), B))
    return worst, bad, mask


def assert_within(got, p, ref_power, min_power, what, extra=0, arg=None, floor_db=None):
    """Asserts pattern and bound; returns the worst ratio error / bound of the finite elements."""
    worst, bad = failures(got, p, ref_power, min_power, extra, arg, floor_db)
    assert not bad, '%s, ref_power %r, min_power %r: %s' % (what, ref_power, min_power, '; '.join(bad))
    return worst
