"""hipdsp_region_stats, BufferedData.region_stats and the analyzers on the GPU.  The comparator is never the code under
test: exact rational arithmetic (fractions.Fraction) up to 4096 samples, math.fsum in float64 beyond, numpy itself for
the counts, extrema, positions and special values.

The kernel cuts a region into chunks of 16384 elements from the region's own start, one workgroup per chunk and
channel; inside a chunk a thread takes whole 16-byte vectors u*256 + t (1024 elements per row of the workgroup) plus
the up to three single samples before the first 16-byte boundary and after the last whole vector.  So of the lengths
used here 1 ... 4097 stay in one chunk (1, 2, 3 are single samples only at most starts; 255 ... 257 and 4095, 4097
straddle vector rows), 2^17 + 1 spans 9 chunks (the second launch merges 9 records in its tree) and 2^22 + 3 spans 257:
thread 0 of the second launch adds two records before the tree, the first size at which that loop runs twice."""

import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import gpu_helpers as gh

pytestmark = pytest.mark.gpu

U = Fraction(1, 2**53)
CHUNK = 16384
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4097]
STARTS = [0, 1, 2, 3, 5]                       # every 16-byte phase, and 5 = 1 again one vector on
BASE = 3                                       # elements between the allocation and x
FAMILIES = ['normal', 'dc_half', 'dc_three', 'outlier_pivot', 'constant', 'int16']


def family(name, rng, C, n):
    if name == 'normal':
        x = rng.standard_normal((C, n))
    elif name == 'dc_half':
        x = 0.5 + 1e-4*rng.standard_normal((C, n))
    elif name == 'dc_three':
        x = 3.0 + 1e-3*rng.standard_normal((C, n))
    elif name == 'outlier_pivot':
        x = rng.standard_normal((C, n))        # the caller puts 1000 at every region's first sample
    elif name == 'constant':
        x = np.full((C, n), 0.1) + np.arange(C)[:, None]
    else:
        x = rng.integers(-32768, 32768, size=(C, n)).astype(np.float64)
    return x.astype(np.float32)


class Slab(object):
    """A host (C, frames) float32 array on the device with a base offset of 3 elements and pitch = frames + 7."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(BASE + self.C*self.pitch, 12345.0, dtype=np.float32)
        for c in range(self.C):
            host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(BASE, (1,))

    def stats(self, regions, channels=None, out=None):
        from audian_amd import hipdsp
        return hipdsp.region_stats(self.ctx, self.view, self.pitch, self.C if channels is None else channels,
                                   self.frames, regions, out=out)


def numpy_slots(v):
    """All eight slots as numpy gives them on the float64 copy (the special-value contract)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return np.array([0, np.nan, np.nan, np.nan, np.nan, -1, -1, 0])
    with np.errstate(all='ignore'):
        return np.array([v.size, np.mean(v), np.std(v), np.min(v), np.max(v), np.argmin(v), np.argmax(v), 0])


def exact_moments(v):
    """(mu, sigma^2, D1, D2) of float32 samples as exact Fractions: every float32 is an integer times 2^-149."""
    m, e = np.frexp(v.astype(np.float64))
    assert (e[m != 0] + 125 >= 0).all()                         # no denormals in these tests
    ints = [int(a) << int(b) for a, b in zip((m*2.0**24).astype(np.int64).tolist(), np.where(m != 0, e + 125, 0).tolist())]
    n, scale = len(ints), 2**149
    s1, s2 = sum(ints), sum(i*i for i in ints)
    k = ints[0]
    return (Fraction(s1, n*scale), Fraction(n*s2 - s1*s1, n*n*scale*scale),
            Fraction(sum(abs(i - k) for i in ints), n*scale), Fraction(sum((i - k)**2 for i in ints), n*scale*scale))


def fsum_moments(v):
    """The same in float64 with math.fsum (each sum exact to one rounding): for n > 4096."""
    x = v.astype(np.float64)
    n = len(x)
    mu = math.fsum(x.tolist())/n
    var = math.fsum(((x - mu)**2).tolist())/n
    d = x - x[0]
    return (Fraction(mu), Fraction(var), Fraction(math.fsum(np.abs(d).tolist())/n), Fraction(math.fsum((d*d).tolist())/n))


def sqrt_fraction(q):
    with localcontext() as c:
        c.prec = 80
        return Fraction((Decimal(q.numerator)/Decimal(q.denominator)).sqrt())


def check_contract(slots, v, what):
    """The header's contract on one (region, channel) of finite float32 samples v (n >= 1)."""
    n = len(v)
    ref = numpy_slots(v)
    for k in (0, 3, 4, 5, 6, 7):
        assert slots[k] == ref[k], '%s: slot %d is %r, numpy gives %r' % (what, k, slots[k], ref[k])
    if n <= 4096:
        mu, var, d1, d2 = exact_moments(v)
        own_mu = own_var = Fraction(0)
    else:
        mu, var, d1, d2 = fsum_moments(v)
        own_mu, own_var = 16*U*abs(mu), 16*U*var               # the comparator's own rounding
    g = (n + 3)*U/(1 - (n + 3)*U)
    mean, std = Fraction(float(slots[1])), Fraction(float(slots[2]))
    err_mean, bound_mean = abs(mean - mu), g*d1 + U*abs(mu) + own_mu
    E = 3*g*d2 + 4*U*var + own_var
    err_var = abs(std*std - var)
    figures = tuple(float(q) for q in (err_mean, bound_mean, err_var, E))
    print('%s: n %d  mean err/bound %.3g/%.3g  var err/bound %.3g/%.3g' % ((what, n) + figures))
    assert err_mean <= bound_mean, '%s: |mean - mu| = %.3g > %.3g' % ((what,) + figures[:2])
    assert std >= 0
    assert err_var <= E, '%s: |std^2 - sigma^2| = %.3g > %.3g' % ((what,) + figures[2:])
    if var == 0:
        assert std == 0, '%s: std of equal samples is %r' % (what, slots[2])
    sigma = sqrt_fraction(var)
    bound_std = min(sqrt_fraction(E), E/sigma) if sigma > 0 else sqrt_fraction(E)
    bound_std += Fraction(1, 10**70)                            # the 80-digit square roots above
    assert abs(std - sigma) <= bound_std, '%s: |std - sigma| = %.3g > %.3g' % (what, float(abs(std - sigma)), float(bound_std))


def layout(shift, disjoint):
    """The eleven lengths, region k at start STARTS[(k + shift) % 5]; disjoint: one after the other instead (each on a
    multiple of 8 plus that start, the same 16-byte phase), for data that wants every region's first sample to itself."""
    regions, at = [], 0
    for k, n in enumerate(LENGTHS):
        a = at + STARTS[(k + shift) % len(STARTS)]
        regions.append((a, a + n))
        if disjoint:
            at = (a + n + 7)//8*8
    return regions


@pytest.mark.parametrize('name', FAMILIES)
def test_contract_small_lengths_every_phase(name):
    """Lengths 1 ... 4097 (one chunk) at starts 0, 1, 2, 3, 5 against exact rational arithmetic, two channels."""
    rng = np.random.default_rng(FAMILIES.index(name))
    for shift in range(len(STARTS)):
        regions = layout(shift, name == 'outlier_pivot')
        x = family(name, rng, 2, max(b for a, b in regions) + 3)
        if name == 'outlier_pivot':
            x[:, [a for a, b in regions]] = 1000.0              # first sample 1000, the rest N(0, 1)
        got = Slab(x).stats(regions)
        assert got.shape == (len(regions), 2, 8)
        for r, (a, b) in enumerate(regions):
            for c in range(2):
                check_contract(got[r, c], x[c, a:b], '%s start %d n %d ch %d' % (name, a, b - a, c))
                if name == 'constant':
                    assert got[r, c, 2] == 0.0 and got[r, c, 1] == float(x[c, a])
                if name == 'int16' and b - a <= 4096:
                    # the sums of integers are exact, so the mean is exact up to the two last roundings: S1/n (at most
                    # D1 in magnitude) and K + S1/n
                    mu, var, d1, d2 = exact_moments(x[c, a:b])
                    assert abs(Fraction(float(got[r, c, 1])) - mu) <= U*(1 + U)*d1 + U*abs(mu)


@pytest.fixture(scope='module')
def long_slab():
    """Two channels of 2^22 + 3 + 5 samples: N(0, 1) and 0.5 + 1e-4 N, with runs of equal extrema in different
    chunks (the first one must win)."""
    rng = np.random.default_rng(77)
    n = 2**22 + 3 + 5
    x = np.empty((2, n), dtype=np.float32)
    x[0] = rng.standard_normal(n).astype(np.float32)
    x[1] = (0.5 + 1e-4*rng.standard_normal(n)).astype(np.float32)
    for c, (lo, hi) in enumerate([(-9.0, 9.0), (0.25, 0.75)]):
        x[c, 3*CHUNK + 50:3*CHUNK + 60] = hi          # the maximum: chunks 3, 4 and 200 of a region starting at 0 or 5
        x[c, 4*CHUNK + 100:4*CHUNK + 103] = hi
        x[c, 200*CHUNK + 7:200*CHUNK + 9] = hi
        x[c, 5*CHUNK + 1000:5*CHUNK + 1003] = lo      # the minimum: chunks 5 and 255
        x[c, 255*CHUNK + 16000:255*CHUNK + 16384] = lo
    return x, Slab(x)


def test_contract_many_chunks_and_ties(long_slab):
    """2^17 + 1 (9 chunks) at two phases and 2^22 + 3 (257 chunks) on two channels, against math.fsum; equal extrema
    in two chunks give the first position."""
    x, slab = long_slab
    regions = [(5, 5 + 2**22 + 3), (0, 2**17 + 1), (3, 3 + 2**17 + 1), (3*CHUNK + 55, 5*CHUNK)]
    got = slab.stats(regions)
    for r, (a, b) in enumerate(regions):
        for c in range(2):
            check_contract(got[r, c], x[c, a:b], 'long region %d ch %d' % (r, c))
    assert got[0, 0, 6] == 3*CHUNK + 50 - 5 and got[0, 0, 5] == 5*CHUNK + 1000 - 5
    assert got[0, 1, 6] == 3*CHUNK + 50 - 5 and got[0, 1, 5] == 5*CHUNK + 1000 - 5
    assert got[3, 0, 6] == 0 and got[3, 1, 6] == 0          # the region starts inside the first run


def poisoned(base, where):
    x = base.copy()
    for i, v in where:
        x[1, i] = v
    return x


N_SPECIAL = 2**17 + 1
SPECIAL = {
    'nan_first': [(4, np.nan)],
    'nan_middle': [(4 + 3*CHUNK + 777, np.nan)],
    'nan_last': [(4 + N_SPECIAL - 1, np.nan)],
    'two_nans': [(4 + 5*CHUNK + 1, np.nan), (4 + 2*CHUNK + 9, np.nan)],
    'pinf': [(4 + CHUNK + 3, np.inf)],
    'ninf': [(4 + 7*CHUNK + 16383, -np.inf)],
    'both_inf': [(4 + 10, np.inf), (4 + 6*CHUNK, -np.inf)],
    'inf_first': [(4, np.inf)],
    'ninf_first_and_pinf': [(4, -np.inf), (4 + 8*CHUNK, np.inf)],
    'nan_after_inf': [(4 + 10, np.inf), (4 + 50000, np.nan)],
    'nan_before_inf': [(4 + 10, np.nan), (4 + 50000, -np.inf)],
}


@pytest.fixture(scope='module')
def special_base():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, N_SPECIAL + 9)).astype(np.float32)
    regions = [(4, 4 + N_SPECIAL), (9, 9), (4 + CHUNK, 4 + 2*CHUNK), (0, 3)]
    return x, regions, Slab(x).stats(regions)


@pytest.mark.parametrize('case', sorted(SPECIAL))
def test_special_values_are_numpys(special_base, case):
    """NaN / inf in channel 1 of a 9-chunk region: all eight slots are numpy's; channels 0 and 2, the empty region and
    the regions the poison is not in keep their bits."""
    base, regions, clean = special_base
    x = poisoned(base, SPECIAL[case])
    got = Slab(x).stats(regions)
    for r, (a, b) in enumerate(regions):
        want = numpy_slots(x[1, a:b])
        if not np.isfinite(x[1, a:b]).all():
            assert np.array_equal(got[r, 1], want, equal_nan=True), (case, r, got[r, 1], want)
        else:
            assert got[r, 1].tobytes() == clean[r, 1].tobytes(), (case, r)
        for c in (0, 2):
            assert got[r, c].tobytes() == clean[r, c].tobytes(), (case, r, c)
    assert np.array_equal(got[1], np.tile(numpy_slots([]), (3, 1)), equal_nan=True)        # n = 0
    assert np.signbit(got[1, :, 5:7]).all()


def test_special_value_rules_spelled_out(special_base):
    base, regions, clean = special_base
    nan = Slab(poisoned(base, SPECIAL['nan_after_inf'])).stats(regions[:1])[0, 1]
    assert np.isnan(nan[1:5]).all() and nan[5] == 50000 and nan[6] == 50000 and nan[0] == N_SPECIAL
    both = Slab(poisoned(base, SPECIAL['both_inf'])).stats(regions[:1])[0, 1]
    assert np.isnan(both[1]) and np.isnan(both[2]) and both[3] == -np.inf and both[4] == np.inf
    assert both[5] == 6*CHUNK and both[6] == 10
    pinf = Slab(poisoned(base, SPECIAL['pinf'])).stats(regions[:1])[0, 1]
    assert pinf[1] == np.inf and np.isnan(pinf[2]) and pinf[4] == np.inf and pinf[3] == clean[0, 1, 3]
    ninf = Slab(poisoned(base, SPECIAL['ninf'])).stats(regions[:1])[0, 1]
    assert ninf[1] == -np.inf and np.isnan(ninf[2]) and ninf[3] == -np.inf and ninf[5] == 7*CHUNK + 16383


SIXTEEN = [(0, 40000), (7, 39999), (7, 39999), (100, 100), (16384, 32768), (16383, 32769), (1, 2), (5, 16389),
           (0, 16384), (20000, 20003), (39999, 40000), (40000, 40000), (3, 20000), (2, 33000), (12345, 23456), (0, 1)]


@pytest.fixture(scope='module')
def wide_slab():
    rng = np.random.default_rng(9)
    x = (0.3 + rng.standard_normal((65, 40000))).astype(np.float32)
    return x, Slab(x)


def test_determinism(wide_slab):
    """Twice the same bits; 16 regions (overlapping, nested, identical, empty) in one call = 16 calls of one; the rows
    that calls with 1, 3 and 65 channels share have the same bits."""
    x, slab = wide_slab
    first = slab.stats(SIXTEEN)
    assert first.shape == (16, 65, 8)
    assert slab.stats(SIXTEEN).tobytes() == first.tobytes()
    for r, region in enumerate(SIXTEEN):
        assert slab.stats([region], channels=3)[0].tobytes() == first[r, :3].tobytes(), region
    assert slab.stats(SIXTEEN, channels=1).tobytes() == first[:, :1].tobytes()
    assert slab.stats(SIXTEEN[::-1], channels=3)[::-1].tobytes() == first[:, :3].tobytes()
    assert first[2].tobytes() == first[1].tobytes()
    for r, (a, b) in enumerate(SIXTEEN):
        for c in (0, 64):
            ref = numpy_slots(x[c, a:b])
            assert np.array_equal(first[r, c, [0, 3, 4, 5, 6, 7]], ref[[0, 3, 4, 5, 6, 7]], equal_nan=True)
            if b > a:
                assert abs(first[r, c, 1] - ref[1]) <= 1e-12 and abs(first[r, c, 2] - ref[2]) <= 1e-12
    assert slab.stats([(0, 10)], channels=0).shape == (1, 0, 8)


def test_errors(wide_slab):
    from audian_amd import hipdsp
    x, slab = wide_slab
    with pytest.raises(NotImplementedError, match='at most 16 regions'):
        slab.stats([(0, 10)]*17)
    with pytest.raises(ValueError, match=r'region 1: elements \[10, 9\)'):
        slab.stats([(0, 10), (10, 9)])
    with pytest.raises(ValueError, match=r'not inside \[0, 40000\]'):
        slab.stats([(0, 40001)])
    with pytest.raises(ValueError, match='not inside'):
        slab.stats([(-1, 5)])
    with pytest.raises(ValueError, match='at least one region'):
        slab.stats([])
    with pytest.raises(ValueError, match='too many channels'):
        hipdsp.region_stats(slab.ctx, slab.view, slab.pitch, 65536, slab.frames, [(0, 1)],
                            out=hipdsp.DeviceArray(slab.ctx, (8,), np.float64))
    assert slab.stats([(0, 10)], channels=2).shape == (1, 2, 8)          # the context still works


def test_writes_exactly_its_block(wide_slab):
    from audian_amd import hipdsp
    x, slab = wide_slab
    R, C, pad = 5, 7, 16
    sentinel = -4242.5
    host = np.full(pad + R*C*8 + pad, sentinel)
    dev = hipdsp.DeviceArray.from_host(slab.ctx, host)
    out = dev.view(pad, (R, C, 8))
    assert slab.stats(SIXTEEN[:R], channels=C, out=out) is out
    back = dev.to_host()
    assert (back[:pad] == sentinel).all() and (back[-pad:] == sentinel).all()
    inner = back[pad:-pad].reshape(R, C, 8)
    assert not (inner == sentinel).any()
    assert inner.tobytes() == slab.stats(SIXTEEN[:R], channels=C).tobytes()
    untouched = hipdsp.DeviceArray.from_host(slab.ctx, host)
    slab.stats(SIXTEEN[:R], channels=0, out=untouched.view(pad, (R, 1, 8)))
    assert (untouched.to_host() == sentinel).all()                        # channels == 0 writes nothing


@pytest.mark.parametrize('F', [129, 1025])
def test_spectrogram_slab(F):
    """(C, frames', F) with odd F: frames [3, 40) of a channel are one contiguous element range; positions are flat."""
    rng = np.random.default_rng(F)
    C, frames = 3, 48
    spec = np.power(10.0, rng.uniform(-12, 2, size=(C, frames, F))).astype(np.float32)
    slab = Slab(spec.reshape(C, frames*F))
    regions = [(3*F, 40*F), (0, frames*F), (47*F, 48*F)]
    got = slab.stats(regions)
    for r, (a, b) in enumerate(regions):
        for c in range(C):
            flat = spec[c].reshape(-1)[a:b]
            check_contract(got[r, c], flat, 'F %d region %d ch %d' % (F, r, c))
    assert got[0, 1, 6] == np.argmax(spec[1, 3:40])


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def test_facade_analyzers_stay_on_the_device():
    """filter + envelope + spectrogram on 4 channels x 6 s: analyze_region is one launch and leaves the host copy
    as stale as it was; 20 regions x 4 channels are two launches."""
    from audian_amd import hipdsp
    from audian_amd.analyzer import Region, StatisticsAnalyzer
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.tracegraph import TraceGraph
    rate, seconds, C = 16000.0, 6.0, 4
    rng = np.random.default_rng(21)
    n = int(rate*seconds)
    t = np.arange(n)/rate
    x = 0.4*rng.uniform(-1, 1, size=(n, C)) + 0.4*np.sin(2*np.pi*900.0*t)[:, None] + 0.05
    g = TraceGraph(30.0, 5.0)
    for tr in (BufferedFilter(), BufferedSpectrogram(nfft=256), BufferedEnvelope(envelope_cutoff=200.0)):
        g.add_trace(tr)
    g.setup_traces()
    g.open(x.astype(np.float32).astype(np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g['filtered'].highpass_cutoff, g['filtered'].lowpass_cutoff = 300.0, 3000.0
    g['filtered'].update()
    g.update_times(0.0, 6.0)
    f, s = g['filtered'], g['spectrogram']
    a = StatisticsAnalyzer(g)
    e = StatisticsAnalyzer(g, 'envelope')
    stale = {tr.name: [list(r) for r in tr._stale] for tr in g.traces[1:]}
    assert stale['filtered'] and stale['spectrogram'] and stale['envelope']
    before, made = dict(hipdsp.launches), Region.materialised
    g.analyze_region(1.0, 2.5, 2)
    assert hipdsp.launches['region_stats'] == before.get('region_stats', 0) + 2        # one per analyzer
    assert Region.materialised == made
    assert {tr.name: [list(r) for r in tr._stale] for tr in g.traces[1:]} == stale     # nothing crossed
    a.clear()
    e.clear()
    g.analyzers.remove(e)
    before = dict(hipdsp.launches)
    g.analyze_region(1.0, 2.5, 2)
    assert hipdsp.launches['region_stats'] == before['region_stats'] + 1
    assert {k: v for k, v in hipdsp.launches.items() if k != 'region_stats'} == \
        {k: v for k, v in before.items() if k != 'region_stats'}
    (mean, std), = a.rows()
    # a spectrogram region: numpy's values of the (frames, F) block
    sr = g.get_region(1.0, 2.5, 1)['spectrogram'][2]
    smax, sarg, smean = np.max(sr), np.argmax(sr), np.mean(sr)
    assert Region.materialised == made and hipdsp.launches['region_stats'] == before['region_stats'] + 2
    regions = [(0.25*k, 0.25*k + 0.5) for k in range(20)]
    a.clear()
    before = dict(hipdsp.launches)
    g.analyze_regions(regions)
    assert hipdsp.launches['region_stats'] == before['region_stats'] + 2
    assert {tr.name: [list(r) for r in tr._stale] for tr in g.traces[1:]} == stale
    rows = a.rows()
    assert len(rows) == 20*C
    # the host copy last
    i0, i1 = g.region_frames(f, 1.0, 2.5)
    host = np.asarray(f[i0:i1, 2])
    assert (i0, i1) == (16000, 40001)
    check_contract(np.array([i1 - i0, mean, std, host.min(), host.max(), host.argmin(), host.argmax(), 0]),
                   host.astype(np.float32), 'filtered region')
    assert np.array_equal(host.astype(np.float32).astype(np.float64), host)            # the mirror's float32, widened
    # numpy's own pairwise float64 sums are good to n u max|x|
    own = (i1 - i0)*2.0**-53*np.max(np.abs(host))
    assert abs(mean - np.mean(host)) <= own and abs(std - np.std(host)) <= 3*own*np.max(np.abs(host))/np.std(host)
    j0, j1 = g.region_frames(s, 1.0, 2.5)
    block = np.asarray(s[j0:j1, 1])
    assert smax == block.max() and sarg == block.argmax() and abs(smean - block.mean()) <= 1e-12*abs(block.mean())
    k = 0
    for t0, t1 in regions:
        i0, i1 = g.region_frames(f, t0, t1)
        for c in range(C):
            v = np.asarray(f[i0:i1, c])
            assert abs(rows[k][0] - v.mean()) <= 1e-12 and abs(rows[k][1] - v.std()) <= 1e-12, (t0, c)
            k += 1
