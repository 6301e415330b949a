"""The three kernels behind playback and the colour-range estimate, each on its own: hipdsp_max_nonneg and
hipdsp_stride_copy exactly, hipdsp_channel_mean under derived bounds.  Until now they ran only inside two facade tests,
under a relative 1e-4 of the peak.

hipdsp_channel_mean without a carrier: the float64 sum of at most 64 float32 samples, divided and rounded to float32
once: |got - m| <= (0.5 + 2^-20) ulp32(m), m the exact mean.  With the heterodyne carrier the reference is
m sin(2 pi f k / rate) in longdouble (the expression oracle.play_data restates) and the bound

    |m| (2 pi (2^-25 + k cps 2^-52) + 5 2^-24),        cps = f / rate as a double

2 pi 2^-25 for the float32 cast of the phase fraction, k cps 2^-52 for the float64 product cps * k with cps itself
rounded once, 5 2^-24 for sinpif at the 2 ulp HIP documents plus the rounding of the product (the ROCm tree this was
written against carries no document with another figure).  The CPU tests below calibrate that bound: a NumPy emulation
of the kernel's arithmetic passes, a phase kept in float32 and a sample index cast to float32 fail.
"""

import numpy as np
import pytest

import gpu_helpers as gh

gpu = pytest.mark.gpu
SENTINEL = 0x7f7f7f7f
F32 = np.float32
RATIOS = ((40000.0, 192000.0), (25000.0, 192000.0), (12345.678, 44100.0))    # the facade test's two, and an awkward one
N_LONG = 2**24 + 4097                                                         # the sample index passes 2^24
PI_LD = 4*np.arctan(np.longdouble(1))                                         # (np.pi is a double)
WORST = {}


def fresh(c, n):
    from audian_amd import hipdsp
    a = hipdsp.DeviceArray(c, (max(n, 1),), np.float32)
    hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(a), 0x7f, 4*max(n, 1))
    return a


def untouched(a):
    return bool(np.all(np.asarray(a).view(np.uint32) == SENTINEL))


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(x)[1]
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


# ---- hipdsp_max_nonneg -------------------------------------------------------------------------------------------

def max_cases():
    """(name, array): the grid is min(ceil(n / 4096), 1024) workgroups of 256 threads striding over the array, so 257
    values already take a second pass; 4096 * 1025 + 1 reaches the cap of 1024 workgroups (17 passes)."""
    rng = np.random.default_rng(5)
    out = [('n = 0', np.zeros(0, F32))]
    for n in (1, 255, 256, 257, 4097, 4096*1025 + 1):
        x = rng.uniform(0.0, 1.0, n).astype(F32)
        threads = 256*min(-(-n//4096), 1024)
        for name, at in (('first', 0), ('last', n - 1), ('second pass', min(threads + n//7, n - 1))):
            y = x.copy()
            y[at] = 2.5
            out.append(('n = %d, maximum %s' % (n, name), y))
    x = rng.uniform(0.0, 1.0, 1000).astype(F32)
    for name, at, v in (('NaN first', 0, np.nan), ('NaN last', 999, np.nan), ('NaN in the second pass', 700, np.nan),
                        ('+inf', 300, np.inf)):
        y = x.copy()
        y[at] = v
        out.append((name, y))
    y = x.copy()
    y[[3, 500]] = np.inf, np.nan
    out.append(('NaN over +inf', y))
    out.append(('all zeros', np.zeros(777, F32)))
    tiny = np.full(600, -0.0, F32)
    tiny[::2] = 0.0
    tiny[411] = 3e-42
    tiny[77] = 1e-45
    out.append(('denormals among 0 and -0.0', tiny))
    return out


@gpu
def test_max_nonneg():
    """Bit for bit np.max of the float32 array; NaN wins; nothing but out[0] is written."""
    from audian_amd import hipdsp
    c = gh.ctx()
    for name, x in max_cases():
        dx = hipdsp.DeviceArray.from_host(c, x) if len(x) else None
        out = fresh(c, 4)
        hipdsp.max_nonneg(c, dx, len(x), out.view(1, (1,)))
        got = out.to_host()
        with np.errstate(invalid='ignore'):
            want = F32(np.max(x)) if len(x) else F32(0.0)
        assert got[1:2].view(np.uint32)[0] == np.array([want]).view(np.uint32)[0], (name, got[1], want)
        assert untouched(got[[0, 2, 3]]), name


@gpu
def test_max_nonneg_twice_into_the_same_word():
    """The second call, with the smaller maximum, must not see the first one's result."""
    from audian_amd import hipdsp
    c = gh.ctx()
    rng = np.random.default_rng(6)
    big, small = (rng.uniform(0.0, s, 5000).astype(F32) for s in (100.0, 0.01))
    db, dsm = hipdsp.DeviceArray.from_host(c, big), hipdsp.DeviceArray.from_host(c, small)
    out = fresh(c, 1)
    hipdsp.max_nonneg(c, db, 5000, out)
    assert out.to_host()[0] == np.max(big)
    hipdsp.max_nonneg(c, dsm, 5000, out)
    assert out.to_host()[0] == np.max(small)
    hipdsp.max_nonneg(c, None, 0, out)
    assert out.to_host()[0] == 0.0


# ---- hipdsp_stride_copy ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('n,step', [(1000, 1), (1001, 2), (1000, 2), (1003, 5), (1, 1), (3, 7), (7, 7), (8, 7), (0, 3),
                                    (2*(4096*256 + 1000) + 1, 2)])
def test_stride_copy(n, step):
    """out[i] = x[i * step] for i < ceil(n / step), exactly, and nothing behind it; the last case strides the grid's
    4096 x 256 threads a second time."""
    from audian_amd import hipdsp
    c = gh.ctx()
    x = np.random.default_rng(n + step).standard_normal(max(n, 1)).astype(F32)
    m = -(-n//step)
    dx = hipdsp.DeviceArray.from_host(c, x)
    out = fresh(c, m + 8)
    hipdsp.stride_copy(c, dx, n, step, out)
    got = out.to_host()
    assert np.array_equal(got[:m].view(np.uint32), x[:n][::step].view(np.uint32))
    assert untouched(got[m:])


# ---- hipdsp_channel_mean -----------------------------------------------------------------------------------------

CHANNELS, PITCH, START, N = 70, 6000, 371, 5003
GROUPS = ([5], [0, 69], [69, 3, 1], list(range(64)), [7, 7, 7], [60, 41, 41, 2], list(range(69, 5, -1)))


def mean_data():
    """(CHANNELS, PITCH) float32: audio-like samples in (-1, 1), one channel under an offset of 100, one at 1e-3 of the
    rest.  The float64 sum of 64 such samples is exact or off by a few 2^-41, far inside the 2^-20 ulp32 of the bound."""
    rng = np.random.default_rng(9)
    x = rng.uniform(-1.0, 1.0, (CHANNELS, PITCH)).astype(F32)
    x[41] += F32(100.0)
    x[7] *= F32(1e-3)
    return x


def exact_mean(x, group, start, n):
    return np.sum(x[group, start:start + n].astype(np.longdouble), axis=0)/np.longdouble(len(group))


@gpu
def test_channel_mean():
    """Counts 1, 2, 3 and 64, repeated and descending channels, start > 0, a pitch above the frames read."""
    from audian_amd import hipdsp
    c = gh.ctx()
    x = mean_data()
    dx = hipdsp.DeviceArray.from_host(c, x)
    for group in GROUPS:
        for start, n in ((START, N), (0, PITCH), (PITCH - 1, 1)):
            out = fresh(c, n + 8)
            hipdsp.channel_mean(c, dx, PITCH, group, start, n, out)
            got = out.to_host()
            m = exact_mean(x, group, start, n)
            ratio = np.abs(got[:n].astype(np.longdouble) - m).astype(np.float64)/((0.5 + 2.0**-20)*ulp32(m))
            WORST['mean'] = max(WORST.get('mean', 0.0), float(ratio.max()))
            assert ratio.max() <= 1.0, (group, start, n, int(np.argmax(ratio)), float(ratio.max()))
            assert untouched(got[n:]), (group, start, n)
    out = fresh(c, 8)
    for group in ([], list(range(65))):
        with pytest.raises(ValueError):
            hipdsp.channel_mean(c, dx, PITCH, group, 0, 8, out)
    assert untouched(out.to_host())


def carrier_ratio(got, m, k, f, rate):
    """error / bound of got (float32) at the sample indices k for the exact means m (longdouble) and the carrier f /
    rate; the kernel is handed cps = f / rate as a double."""
    cps = f/rate
    kl = k.astype(np.longdouble)
    t = np.longdouble(f)*kl/np.longdouble(rate)
    t -= np.floor(t)
    ref = m*np.sin(2*PI_LD*t)
    bound = np.abs(m).astype(np.float64)*(2*np.pi*(2.0**-25 + k.astype(np.float64)*cps*2.0**-52) + 5*2.0**-24)
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bound > 0, err/bound, np.where(err == 0, 0.0, np.inf))


@gpu
@pytest.mark.parametrize('f,rate', RATIOS)
def test_channel_mean_with_carrier(f, rate):
    from audian_amd import hipdsp
    c = gh.ctx()
    x = mean_data()
    dx = hipdsp.DeviceArray.from_host(c, x)
    for group in ([5], [69, 3, 1], list(range(64))):
        out = fresh(c, N + 8)
        hipdsp.channel_mean(c, dx, PITCH, group, START, N, out, heterodyne_cycles_per_sample=f/rate)
        got = out.to_host()
        ratio = carrier_ratio(got[:N], exact_mean(x, group, START, N), np.arange(N), f, rate)
        WORST['carrier'] = max(WORST.get('carrier', 0.0), float(ratio.max()))
        assert ratio.max() <= 1.0, (group, int(np.argmax(ratio)), float(ratio.max()))
        assert untouched(got[N:]), group


@gpu
def test_channel_mean_with_carrier_past_2_to_24_samples():
    """One channel of 2^24 + 4097 samples: the first 8192, the last 8192 and 8192 random positions."""
    from audian_amd import hipdsp
    c = gh.ctx()
    f, rate = RATIOS[0]
    rng = np.random.default_rng(11)
    x = rng.random(N_LONG, dtype=F32) - F32(0.5)
    dx = hipdsp.DeviceArray.from_host(c, x)
    out = fresh(c, N_LONG + 8)
    hipdsp.channel_mean(c, dx, N_LONG, [0], 0, N_LONG, out, heterodyne_cycles_per_sample=f/rate)
    got = out.to_host()
    k = np.unique(np.concatenate([np.arange(8192), np.arange(N_LONG - 8192, N_LONG), rng.integers(0, N_LONG, 8192)]))
    ratio = carrier_ratio(got[k], x[k].astype(np.longdouble), k, f, rate)
    WORST['carrier, long'] = float(ratio.max())
    assert ratio.max() <= 1.0, (int(k[np.argmax(ratio)]), float(ratio.max()))
    assert untouched(got[N_LONG:])


@gpu
def test_zz_worst_ratios():
    for name in sorted(WORST):
        print('hipdsp_channel_mean, %-14s worst error / bound %.3f' % (name, WORST[name]))


# ---- the carrier bound, calibrated on the CPU --------------------------------------------------------------------

def emulate_carrier(v, k, cps, defect=None):
    """channel_mean_kernel's carrier arithmetic on float32 means v at sample indices k: the phase cps * k in float64,
    its fraction cast to float32, sinpif (here the float64 sine, rounded), the float32 product."""
    v = np.asarray(v, dtype=F32)
    if defect == 'phase in float32':
        ph = F32(cps)*k.astype(F32)
        ph = ph - np.floor(ph)
    elif defect == 'index cast to float32':
        ph = cps*k.astype(F32).astype(np.float64)
        ph = ph - np.floor(ph)
    else:
        ph = cps*k.astype(np.float64)
        ph = ph - np.floor(ph)
    arg = F32(2.0)*ph.astype(F32)
    return v*np.sin(np.pi*arg.astype(np.float64)).astype(F32)


def carrier_positions():
    rng = np.random.default_rng(12)
    k = np.unique(np.concatenate([np.arange(8192), np.arange(N_LONG - 8192, N_LONG), rng.integers(0, N_LONG, 8192)]))
    return k, (rng.random(len(k), dtype=F32) - F32(0.5))


@pytest.mark.parametrize('f,rate', RATIOS)
def test_carrier_bound_passes_a_faithful_emulation(f, rate):
    k, v = carrier_positions()
    ratio = carrier_ratio(emulate_carrier(v, k, f/rate), v.astype(np.longdouble), k, f, rate)
    print('carrier %g / %g: worst error / bound of the emulation %.3f' % (f, rate, ratio.max()))
    assert ratio.max() <= 1.0


@pytest.mark.parametrize('defect', ['phase in float32', 'index cast to float32'])
@pytest.mark.parametrize('f,rate', RATIOS)
def test_carrier_bound_fails_the_defects(f, rate, defect):
    k, v = carrier_positions()
    ratio = carrier_ratio(emulate_carrier(v, k, f/rate, defect), v.astype(np.longdouble), k, f, rate)
    assert ratio.max() > 1.0, defect
    if defect == 'index cast to float32':                     # exact up to 2^24: only the long case can see it
        assert ratio[k < 2**24].max() <= 1.0
