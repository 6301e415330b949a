"""Calibration of tests/decibel_bound.py on the CPU, before anybody trusts it on the GPU: a float32 NumPy emulation of
the kernels' intended arithmetic passes at every parameter pair (worst ratio printed with -s), and each injected defect
fails the new bound while it passes the suite's older check (-inf pattern, |error| < 1e-4 dB at ref_power 1 on
log-uniform random powers).  NumPy's float32 log10 stands in for log10f.  Last, the package's host fallback
(audian_amd.bufferedspectrogram.decibel) is held to the C oracle exactly."""

import numpy as np
import pytest

import decibel_bound as dbb

F32 = np.float32
TINY = float(np.finfo(F32).tiny)
FLT_MAX = float(np.finfo(F32).max)


def threshold_down(min_power):
    """The largest float32 not above min_power."""
    with np.errstate(over='ignore'):
        t = F32(min_power)
    return np.nextafter(t, F32(-np.inf)) if float(t) > min_power else t


def emulate(p, ref_power, min_power, defect=None):
    """The kernels' arithmetic in float32 NumPy: the threshold rounded down, the float32 reciprocal and product where
    the product is a normal float, the float64 quotient elsewhere; `defect` injects one fault."""
    p = np.asarray(p, dtype=F32)
    if defect == 'ref_power ignored':
        ref_power = 1.0
    with np.errstate(all='ignore'):
        thr = F32(min_power) if defect == 'threshold rounded to nearest' else threshold_down(min_power)
        inv = F32(1.0/ref_power)
        if not float(inv) >= TINY:
            inv = F32(0.0)
        q = p*inv
        if defect == '16 mantissa bits':
            q = (q.view(np.uint32) & np.uint32(0xffffff80)).view(F32)
        fast = (q >= F32(TINY)) & (q <= F32(FLT_MAX))
        narrow = F32(10.0)*np.log10(np.where(fast, q, F32(1.0)))
        assert narrow.dtype == F32
        wide = (10.0*np.log10(p.astype(np.float64)/ref_power)).astype(F32)
        out = np.where(fast, narrow, wide)
        if defect == 'flushed to 0 dB':
            out = np.where(np.abs(p.astype(np.float64)/ref_power - 1.0) < 2e-5, F32(0.0), out)
        if defect == 'offset of 5e-5 dB':
            out = (out + F32(5e-5)).astype(F32)
        below = p < thr if defect == '< for <=' else p <= thr
        return np.where(below, F32(-np.inf), out).astype(F32)


def old_inputs():
    """What test_decibel_any_length_and_alignment and its siblings draw."""
    return (10.0**np.random.default_rng(8).uniform(-25, 3, size=100001)).astype(F32)


def passes_old_check(got, p, oracle):
    want = oracle.decibel(p.astype(np.float64))
    fin = np.isfinite(want)
    return (np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
            and float(np.max(np.abs(got[fin] - want[fin]))) < 1e-4)


@pytest.mark.parametrize('ref_power,min_power', dbb.PAIRS)
def test_faithful_emulation_passes(oracle, ref_power, min_power):
    p = dbb.sweep()
    assert 15000 < len(p) < 25000
    worst = dbb.assert_within(emulate(p, ref_power, min_power), p, ref_power, min_power, 'emulation')
    print('faithful emulation, ref_power %g, min_power %g: worst ratio %.3f' % (ref_power, min_power, worst))
    assert passes_old_check(emulate(old_inputs(), 1.0, 1e-20), old_inputs(), oracle)


def test_random_arguments_stay_under_the_bound(monkeypatch):
    """Two million random normal powers per ref_power: b = 3 is not slack, the same samples break b = 2."""
    rng = np.random.default_rng(1)
    p = (rng.integers(1 << 23, 255 << 23, 2_000_000).astype(np.uint32)).view(F32)
    over = []
    for ref_power in (1.0, 3.0, 2.5, 1e-6, 1e12):
        got = emulate(p, ref_power, 0.0)
        worst = dbb.assert_within(got, p, ref_power, 0.0, 'emulation, random powers')
        monkeypatch.setattr(dbb, 'B', 2.0)
        over.append(dbb.failures(got, p, ref_power, 0.0)[0])
        monkeypatch.undo()
        print('faithful emulation, random powers, ref_power %g: worst ratio %.3f, against b = 2 %.3f'
              % (ref_power, worst, over[-1]))
    assert max(over) > 1.0


# the defect, and the parameter pair whose sweep shows it
DEFECTS = (('ref_power ignored', (2.5, 1e-7)),
           ('< for <=', (1.0, 1e-20)),
           ('threshold rounded to nearest', (2.5, 1e-7)),
           ('16 mantissa bits', (1.0, 1e-20)),
           ('flushed to 0 dB', (1.0, 1e-20)),
           ('offset of 5e-5 dB', (1.0, 1e-20)))


@pytest.mark.parametrize('defect,pair', DEFECTS, ids=[d for d, _ in DEFECTS])
def test_defect_fails_the_bound_and_passes_the_old_check(oracle, defect, pair):
    ref_power, min_power = pair
    p = dbb.sweep()
    worst, bad = dbb.failures(emulate(p, ref_power, min_power, defect), p, ref_power, min_power)
    assert bad, '%s: not noticed (worst ratio %.3f)' % (defect, worst)
    print('%s: %s' % (defect, bad[0]))
    old = old_inputs()
    assert passes_old_check(emulate(old, 1.0, 1e-20, defect), old, oracle), defect + ': the old check sees it too'


def test_todays_threshold_fails_exactly_where_the_cast_rounds_up():
    """(float)min_power as the threshold: wrong at 1e-7, 0.1 and 1e-10, right at 1e-20 and 0."""
    for ref_power, min_power in dbb.PAIRS[:5]:
        p = dbb.sweep()
        _, bad = dbb.failures(emulate(p, ref_power, min_power, 'threshold rounded to nearest'), p, ref_power, min_power)
        assert bool(bad) == (float(F32(min_power)) > min_power), (min_power, bad)


def test_ulp32():
    assert dbb.ulp32(1.0) == 2.0**-23 and dbb.ulp32(0.999) == 2.0**-24 and dbb.ulp32(-3.0) == 2.0**-22
    assert dbb.ulp32(0.0) == 2.0**-149 and dbb.ulp32(1e-40) == 2.0**-149 and dbb.ulp32(2.0**-126) == 2.0**-149
    assert dbb.ulp32(2.0**-125) == 2.0**-148


@pytest.mark.parametrize('ref_power,min_power', dbb.PAIRS)
def test_host_fallback_equals_the_oracle(oracle, ref_power, min_power):
    """bufferedspectrogram.decibel (NumPy) against the C oracle, bit for bit: the sweep, the float64 neighbours of
    min_power (the tie itself among them) and of ref_power."""
    from audian_amd.bufferedspectrogram import decibel
    p = dbb.sweep().astype(np.float64)
    ties = [np.nextafter(min_power, -np.inf), min_power, np.nextafter(min_power, np.inf),
            np.nextafter(ref_power, 0.0), ref_power, np.nextafter(ref_power, np.inf)]
    p = np.concatenate([p, ties])
    with np.errstate(all='ignore'):
        got = decibel(p, ref_power, min_power)
    want = oracle.decibel(p, ref_power, min_power)
    assert got.dtype == np.float64
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (p[~same][:5], got[~same][:5], want[~same][:5])
    assert np.array_equal(np.isnan(got), np.isnan(p))
    assert np.array_equal(np.isneginf(got), (p <= min_power) | (p/ref_power == 0))      # (5e-324 / 1e12 is 0 in float64)
    assert decibel(min_power, ref_power, min_power) == -np.inf
