"""hipdsp_histogram, hipdsp_masked_stats and BufferedData.histogram / masked_stats / threshold_estimates on the GPU.
The comparator is never the code under test: np.histogram and plain counting for the histogram (exact integer
equality), exact rational arithmetic (fractions.Fraction) up to 4096 selected samples and math.fsum in float64 beyond
for the masked moments, and the thresholds the reference's own function gave (tests/golden/threshold_estimates.npz)
for the facade.

Both kernels cut [start, stop) into chunks of 16384 elements from `start`, one workgroup of four waves per chunk and
channel; inside a chunk a thread takes whole 16-byte vectors u*256 + t plus the up to three single samples before the
first 16-byte boundary and after the last whole vector.  So of the lengths used here 1 ... 4097 stay in one chunk (1, 2,
3 are single samples only at most starts; 255 ... 257 and 4095, 4097 straddle vector rows) and 2^17 + 1 spans 9 chunks:
9 workgroups add to one row of counts, and the second launch of the masked moments merges 9 records.  The edges reach
the device 256 per launch: 1, 49 and 64 bins need one launch, 1024 bins five.  Every slab has a base offset of 3
elements and pitch = frames + 7, and whatever lies outside [start, stop) would be counted or selected if it were
looked at."""

import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import gpu_helpers as gh
import threshold_definition as td
from conftest import load_golden

pytestmark = pytest.mark.gpu

U = Fraction(1, 2**53)
CHUNK = 16384
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4097]
LONG = 2**17 + 1
STARTS = [0, 1, 2, 3, 5]                       # every 16-byte phase, and 5 = 1 again one vector on
BASE = 3                                       # elements between the allocation and x
BINS = [1, 49, 64, 1024]
HIST_FAMILIES = ['uniform', 'constant', 'on_edges', 'linspace_max', 'duplicates', 'cubic', 'special']


class Slab(object):
    """A host (C, frames) float32 array on the device with a base offset of 3 elements and pitch = frames + 7."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(BASE + self.C*self.pitch, 0.5, dtype=np.float32)
        for c in range(self.C):
            host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(BASE, (1,))

    def rows(self, channel):
        """(device view, channels): all rows, or a one-channel call on the view of row `channel`."""
        if channel is None:
            return self.view, self.C
        return self.dev.view(BASE + channel*self.pitch, (1,)), 1

    def hist(self, start, stop, edges, channel=None, **kwargs):
        from audian_amd import hipdsp
        view, C = self.rows(channel)
        return hipdsp.histogram(self.ctx, view, self.pitch, C, start, stop, edges, **kwargs)

    def masked(self, start, stop, bounds, channel=None, **kwargs):
        from audian_amd import hipdsp
        view, C = self.rows(channel)
        bounds = np.asarray(bounds, dtype=np.float64).reshape(-1, 3)
        return hipdsp.masked_stats(self.ctx, view, self.pitch, C, start, stop,
                                   bounds if channel is None else bounds[channel:channel + 1], **kwargs)


# ---- the histogram -------------------------------------------------------------------------------------------------

def hist_case(name, rng, C, n, B, start, stop):
    """(samples (C, n) float32, edges (B + 1,) float64) of a family; [start, stop) is what will be counted."""
    if name == 'uniform':
        x = rng.uniform(-1.0, 3.0, size=(C, n))
        e = np.linspace(-1.0, 3.0, B + 1)
    elif name == 'constant':
        x = np.full((C, n), 0.3) + 0.125*np.arange(C)[:, None]         # every lane of every wave in one bin
        e = np.linspace(0.0, 1.0, B + 1)
    elif name == 'on_edges':
        m = max(1, 1024//B)
        e = -2.0 + np.arange(B + 1)*m/64.0                              # multiples of 1/64 from -2 to 14
        x = rng.integers(-160, 930, size=(C, n))/64.0                   # multiples of 1/64 from -2.5 to 14.5
    elif name == 'linspace_max':
        x = np.abs(rng.normal(0.0, 0.01, size=(C, n))) + 0.02
        x[:, start + (stop - start)//2] = 0.2 + 0.1*np.arange(C)        # the maximum is inside the range, in the last row
        x = x.astype(np.float32)
        e = np.linspace(0.0, float(np.max(x[:, start:stop])), B + 1)    # the last bin is closed: the maximum counts
    elif name == 'duplicates':
        e = np.sort(np.round(rng.uniform(-1.0, 1.0, size=B + 1)*8)/8)   # 17 distinct values: zero-width bins
        if B > 1:
            e[-2] = e[-1]                                               # the last bin has zero width too
        x = rng.integers(-20, 21, size=(C, n))/16.0
    elif name == 'cubic':
        e = 4.0*np.linspace(0.0, 1.0, B + 1)**3 - 1.0                   # the guess is far off: the binary search
        x = rng.uniform(-1.2, 3.2, size=(C, n))
    else:
        x = rng.standard_normal((C, n))
        e = np.linspace(-1.0, 1.0, B + 1)
    x = np.asarray(x, dtype=np.float32)
    if name == 'special':
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random((C, n)) < 0.05] = value
    return x, e


def check_hist(got, x, start, stop, e, what):
    assert got.dtype == np.int64 and got.shape == (x.shape[0], len(e) + 2), what
    for c in range(x.shape[0]):
        want = td.numpy_slots(x[c, start:stop], e)
        assert got[c].tolist() == want.tolist(), what + ' channel %d' % c
    assert (got.sum(axis=1) == stop - start).all(), what


@pytest.mark.parametrize('name', HIST_FAMILIES)
def test_histogram_small_lengths_every_start(name):
    """Lengths 1 ... 4097 at starts 0, 1, 2, 3, 5 with 1, 49, 64 and 1024 bins, three channels: numpy's counts."""
    rng = np.random.default_rng(HIST_FAMILIES.index(name))
    for shift in range(len(STARTS)):
        for k, n in enumerate(LENGTHS):
            start = STARTS[(k + shift) % len(STARTS)]
            B = BINS[(k + shift) % len(BINS)]
            x, e = hist_case(name, rng, 3, start + n + 3, B, start, start + n)
            got = Slab(x).hist(start, start + n, e)
            check_hist(got, x, start, start + n, e, '%s start %d n %d bins %d' % (name, start, n, B))
            if name == 'linspace_max':
                assert got[2, B - 1] >= 1 and got[:, B + 1].sum() == 0  # the maximum: in the last bin, not above
            if name == 'special' and n >= 255:
                assert got[:, B:].min() > 0                             # below, above and NaN all occur


@pytest.fixture(scope='module')
def long_cases():
    """Three channels of 5 + 2^17 + 1 + 2 samples per family, every family with all four bin counts."""
    rng = np.random.default_rng(101)
    out = {}
    for name in HIST_FAMILIES:
        for B in BINS:
            x, e = hist_case(name, rng, 3, 5 + LONG + 2, B, 5, 5 + LONG)
            out[name, B] = (x, e)
    return out


@pytest.mark.parametrize('name', HIST_FAMILIES)
def test_histogram_many_chunks(long_cases, name):
    """2^17 + 1 samples (9 chunks) at start 5, one channel of them also alone at start 0: nine workgroups add to a row."""
    for B in BINS:
        x, e = long_cases[name, B]
        slab = Slab(x)
        got = slab.hist(5, 5 + LONG, e)
        check_hist(got, x, 5, 5 + LONG, e, '%s bins %d' % (name, B))
        if B == 49:
            one = slab.hist(0, LONG, e, channel=1)
            check_hist(one, x[1:2], 0, LONG, e, '%s one channel' % name)


def test_histogram_single_channel_calls():
    """One channel: every length and start once more, and x_pitch is not looked at."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(5)
    for k, n in enumerate(LENGTHS + [LONG]):
        start = STARTS[k % len(STARTS)]
        x, e = hist_case('uniform', rng, 1, start + n + 3, 49, start, start + n)
        slab = Slab(x)
        check_hist(slab.hist(start, start + n, e), x, start, start + n, e, 'one channel n %d' % n)
        got = hipdsp.histogram(slab.ctx, slab.view, 0, 1, start, start + n, e)
        check_hist(got, x, start, start + n, e, 'one channel, pitch 0, n %d' % n)


def test_histogram_same_bytes_twice_channel_independence_and_its_block():
    from audian_amd import hipdsp
    rng = np.random.default_rng(6)
    n, start = 3*CHUNK + 77, 3
    x = (np.abs(rng.normal(0.0, 0.01, size=(3, start + n + 2))) + 0.02).astype(np.float32)
    x[0, 1000:1400] += 0.3
    slab = Slab(x)
    for B in (49, 1024):
        e = np.linspace(0.0, float(x.max()), B + 1)
        first = slab.hist(start, start + n, e)
        check_hist(first, x, start, start + n, e, 'bins %d' % B)
        assert slab.hist(start, start + n, e).tobytes() == first.tobytes()
        for c in range(3):
            assert slab.hist(start, start + n, e, channel=c).tobytes() == first[c:c + 1].tobytes()
        # into a sentinel-filled array with a row pitch of B + 3 + 5: all B + 3 slots of a row, nothing else
        pad, pitch, sentinel = 4, B + 3 + 5, -77
        host = np.full(pad + 3*pitch + pad, sentinel, dtype=np.int64)
        dev = hipdsp.DeviceArray.from_host(slab.ctx, host)
        out = dev.view(pad, (3*pitch,))
        assert slab.hist(start, start + n, e, out=out, out_pitch=pitch) is out
        back = dev.to_host()
        assert (back[:pad] == sentinel).all() and (back[-pad:] == sentinel).all()
        rows = back[pad:-pad].reshape(3, pitch)
        assert rows[:, :B + 3].tobytes() == first.tobytes() and (rows[:, B + 3:] == sentinel).all()
        # an empty range writes zeros; no channels: nothing
        dev2 = hipdsp.DeviceArray.from_host(slab.ctx, host)
        slab.hist(7, 7, e, out=dev2.view(pad, (3*pitch,)), out_pitch=pitch)
        rows = dev2.to_host()[pad:-pad].reshape(3, pitch)
        assert (rows[:, :B + 3] == 0).all() and (rows[:, B + 3:] == sentinel).all()
        dev3 = hipdsp.DeviceArray.from_host(slab.ctx, host)
        hipdsp.histogram(slab.ctx, slab.view, slab.pitch, 0, start, start + n, e, out=dev3)
        assert (dev3.to_host() == sentinel).all()
    assert slab.hist(start, start + n, [0.0, 1.0]).tolist() == [[n, 0, 0, 0]]*3


def test_histogram_errors():
    from audian_amd import hipdsp
    slab = Slab(np.zeros((3, 100), dtype=np.float32))
    for bad in ([1.0, 0.0], [0.0, np.nan], [0.0, np.inf], [-np.inf, 0.0], [0.0, 1.0, 0.5], [0.0]):
        with pytest.raises(ValueError):
            slab.hist(0, 100, bad)
    with pytest.raises(ValueError):
        slab.hist(10, 9, [0.0, 1.0])
    with pytest.raises(ValueError):
        slab.hist(-1, 9, [0.0, 1.0])
    with pytest.raises(ValueError):
        slab.hist(0, slab.pitch + 1, [0.0, 1.0])                       # x_pitch < stop with three channels
    with pytest.raises(ValueError):
        slab.hist(0, 100, [0.0, 1.0], out=hipdsp.DeviceArray(slab.ctx, (3, 4), np.int64), out_pitch=3)
    with pytest.raises(NotImplementedError, match='at most 1024 bins'):
        slab.hist(0, 100, np.arange(1026.0))
    with pytest.raises(NotImplementedError, match='at most 65535 channels'):
        hipdsp.histogram(slab.ctx, slab.view, slab.pitch, 65536, 0, 10, [0.0, 1.0],
                         out=hipdsp.DeviceArray(slab.ctx, (4,), np.int64))
    assert slab.hist(0, 100, [0.0, 1.0]).tolist() == [[100, 0, 0, 0]]*3       # the context still works


def test_indices_past_two_to_the_31():
    """Two rows 2^30 + 20000 elements apart in one allocation of 2^31 + 40000 floats: the range of row 1 lies behind
    element 2^31 of the allocation.  Only the ranges are written; nothing else is looked at."""
    from audian_amd import hipdsp
    c = gh.ctx()
    pitch = 2**30 + 20000
    start, stop = 2**30 - 10000, 2**30 + 19001
    rng = np.random.default_rng(8)
    x = rng.uniform(0.0, 1.0, size=(2, stop - start)).astype(np.float32)
    dev = hipdsp.DeviceArray(c, (2*pitch,), np.float32)
    for ch in range(2):
        dev.view(ch*pitch + start, (stop - start,)).copy_from_host(x[ch])
    e = np.linspace(0.0, 1.0, 50)
    got = hipdsp.histogram(c, dev, pitch, 2, start, stop, e)
    check_hist(got, x, 0, stop - start, e, 'past 2^31')
    stats = hipdsp.masked_stats(c, dev, pitch, 2, start, stop, [[0.25, 0.75, 0.25]]*2)
    for ch in range(2):
        check_masked(stats[ch], x[ch], 0.25, 0.75, 0.25, 'past 2^31 channel %d' % ch)
    dev.free()


# ---- the masked moments --------------------------------------------------------------------------------------------

SCALE_BITS = 1074                              # every finite float64 is an integer times 2^-1074


def as_ints(values):
    out = []
    for v in values:
        a, b = float(v).as_integer_ratio()
        out.append(a*((1 << SCALE_BITS)//b))
    return out


def exact_moments(sel, K):
    """(mu, sigma^2, D1, D2) of the selected samples about the pivot K as exact Fractions."""
    ints, (k,) = as_ints(sel.tolist()), as_ints([K])
    n, scale = len(ints), 1 << SCALE_BITS
    s1, s2 = sum(ints), sum(i*i for i in ints)
    return (Fraction(s1, n*scale), Fraction(n*s2 - s1*s1, n*n*scale*scale),
            Fraction(sum(abs(i - k) for i in ints), n*scale), Fraction(sum((i - k)**2 for i in ints), n*scale*scale))


def fsum_moments(sel, K):
    """The same in float64 with math.fsum (each sum exact to one rounding): for more than 4096 selected samples."""
    n = len(sel)
    mu = math.fsum(sel.tolist())/n
    var = math.fsum(((sel - mu)**2).tolist())/n
    d = sel - K
    return (Fraction(mu), Fraction(var), Fraction(math.fsum(np.abs(d).tolist())/n), Fraction(math.fsum((d*d).tolist())/n))


def sqrt_fraction(q):
    with localcontext() as c:
        c.prec = 80
        return Fraction((Decimal(q.numerator)/Decimal(q.denominator)).sqrt())


def check_masked(slots, v, lo, hi, K, what):
    """The header's contract on one channel: v = the float32 samples of [start, stop), N = len(v) enters g."""
    N = len(v)
    sel = td.selected(v, lo, hi)
    n = len(sel)
    assert slots[0] == n and slots[3] == 0, '%s: [0] is %r, %d samples are selected' % (what, slots[0], n)
    if n == 0:
        assert np.isnan(slots[1]) and np.isnan(slots[2]), what
        return
    if n <= 4096:
        mu, var, d1, d2 = exact_moments(sel, K)
        own_mu = own_var = Fraction(0)
    else:
        mu, var, d1, d2 = fsum_moments(sel, K)
        own_mu, own_var = 16*U*abs(mu), 16*U*var                # the comparator's own rounding
    g = (N + 3)*U/(1 - (N + 3)*U)
    mean, std = Fraction(float(slots[1])), Fraction(float(slots[2]))
    err_mean, bound_mean = abs(mean - mu), g*d1 + U*abs(mu) + own_mu
    E = 3*g*d2 + 4*U*var + own_var
    err_var = abs(std*std - var)
    figures = tuple(float(q) for q in (err_mean, bound_mean, err_var, E))
    print('%s: N %d n %d  mean err/bound %.3g/%.3g  var err/bound %.3g/%.3g' % ((what, N, n) + figures))
    assert err_mean <= bound_mean, '%s: |mean - mu| = %.3g > %.3g' % ((what,) + figures[:2])
    assert std >= 0
    assert err_var <= E, '%s: |std^2 - sigma^2| = %.3g > %.3g' % ((what,) + figures[2:])
    sigma = sqrt_fraction(var)
    bound_std = min(sqrt_fraction(E), E/sigma) if sigma > 0 else sqrt_fraction(E)
    bound_std += Fraction(1, 10**70)                            # the 80-digit square roots above
    assert abs(std - sigma) <= bound_std, '%s: |std - sigma| = %.3g > %.3g' % (what, float(abs(std - sigma)), float(bound_std))


MASK_FAMILIES = ['normal', 'dc_three', 'special']
# lo, hi, pivot of the three channels: one-sided below, one-sided above, two-sided
WINDOWS = {
    'normal': [(-np.inf, 0.25, 0.25), (0.5, np.inf, 0.5), (-0.75, 0.5, -0.75)],
    'dc_three': [(-np.inf, 3.0005, 3.0005), (2.9995, np.inf, 2.9995), (2.999, 3.001, 2.999)],
    'special': [(-np.inf, 0.25, 0.25), (0.5, np.inf, 0.5), (-np.inf, np.inf, 0.0)],
}


def mask_family(name, rng, C, n):
    if name == 'dc_three':
        x = 3.0 + 1e-3*rng.standard_normal((C, n))
    else:
        x = rng.standard_normal((C, n))
    x = x.astype(np.float32)
    if name == 'special':
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random((C, n)) < 0.05] = value
    return x


@pytest.mark.parametrize('name', MASK_FAMILIES)
def test_masked_stats_small_lengths_every_start(name):
    """Lengths 1 ... 4097 at starts 0, 1, 2, 3, 5 against exact rational arithmetic; the three channels carry a
    window below, a window above and a two-sided one (for 'special' the open window: NaN and inf stay out)."""
    rng = np.random.default_rng(20 + MASK_FAMILIES.index(name))
    bounds = WINDOWS[name]
    for shift in range(len(STARTS)):
        for k, n in enumerate(LENGTHS):
            start = STARTS[(k + shift) % len(STARTS)]
            x = mask_family(name, rng, 3, start + n + 3)
            got = Slab(x).masked(start, start + n, bounds)
            assert got.shape == (3, 4)
            for c, (lo, hi, K) in enumerate(bounds):
                check_masked(got[c], x[c, start:start + n], lo, hi, K, '%s start %d n %d ch %d' % (name, start, n, c))


@pytest.fixture(scope='module')
def long_masked():
    rng = np.random.default_rng(31)
    out = {}
    for name in MASK_FAMILIES:
        x = mask_family(name, rng, 3, 5 + LONG + 2)
        out[name] = (x, Slab(x))
    return out


@pytest.mark.parametrize('name', MASK_FAMILIES)
def test_masked_stats_many_chunks(long_masked, name):
    """2^17 + 1 samples (9 chunks, 9 records merged) against math.fsum; twice the same bytes; a channel alone gives the
    bytes it gives among three."""
    x, slab = long_masked[name]
    bounds = WINDOWS[name]
    got = slab.masked(5, 5 + LONG, bounds)
    for c, (lo, hi, K) in enumerate(bounds):
        check_masked(got[c], x[c, 5:5 + LONG], lo, hi, K, '%s long ch %d' % (name, c))
    assert slab.masked(5, 5 + LONG, bounds).tobytes() == got.tobytes()
    for c in range(3):
        assert slab.masked(5, 5 + LONG, bounds, channel=c).tobytes() == got[c:c + 1].tobytes()
    short = slab.masked(3, 3 + 4097, bounds)
    for c in range(3):
        assert slab.masked(3, 3 + 4097, bounds, channel=c).tobytes() == short[c:c + 1].tobytes()


def test_masked_stats_empty_selections_and_nan_bounds(long_masked):
    from audian_amd import hipdsp
    x, slab = long_masked['special']
    nothing = [(5.0, 6.0, 5.0), (1.0, 1.0, 1.0), (np.nan, 1.0, 0.0)]
    for start, stop in [(5, 5 + LONG), (3, 300), (9, 9)]:
        got = slab.masked(start, stop, nothing)
        assert (got[:, 0] == 0).all() and np.isnan(got[:, 1:3]).all() and (got[:, 3] == 0).all()
    got = slab.masked(3, 300, [(0.0, np.nan, 0.0), (-np.inf, np.inf, 0.0), (0.0, 1.0, 0.0)])
    assert got[0, 0] == 0 and got[1, 0] == np.isfinite(x[1, 3:300]).sum()
    assert got[2, 0] == ((x[2, 3:300] > 0) & (x[2, 3:300] < 1)).sum()
    # strict on both sides: the bounds themselves are samples
    y = np.array([[0.0, 0.5, 1.0, 0.5, 0.25]], dtype=np.float32)
    got = Slab(y).masked(0, 5, [(0.0, 1.0, 0.0)])[0]
    assert got[0] == 3 and got[1] == 1.25/3 and abs(got[2] - np.std([0.5, 0.5, 0.25])) <= 1e-15 and got[3] == 0
    assert Slab(y).masked(0, 5, [(0.25, 0.5, 0.25)])[0, 0] == 0
    # out= fills a device array and returns it; no channels: nothing is written
    sentinel = -4242.5
    dev = hipdsp.DeviceArray.from_host(slab.ctx, np.full(3*4 + 4, sentinel))
    out = dev.view(2, (3, 4))
    assert slab.masked(3, 300, nothing, out=out) is out
    back = dev.to_host()
    assert (back[:2] == sentinel).all() and (back[-2:] == sentinel).all() and not (back[2:-2] == sentinel).any()
    hipdsp.masked_stats(slab.ctx, slab.view, slab.pitch, 0, 3, 300, hipdsp.DeviceArray(slab.ctx, (1, 3), np.float64),
                        out=dev.view(2, (3, 4)))
    assert dev.to_host().tobytes() == back.tobytes()
    with pytest.raises(ValueError):
        slab.masked(10, 9, nothing)
    with pytest.raises(ValueError):
        slab.masked(0, slab.pitch + 1, nothing)
    with pytest.raises(NotImplementedError, match='at most 65535 channels'):
        hipdsp.masked_stats(slab.ctx, slab.view, slab.pitch, 65536, 0, 10,
                            hipdsp.DeviceArray(slab.ctx, (1, 3), np.float64), out=dev)


def test_both_calls_inside_a_captured_graph():
    """Legal inside hipdsp_graph_begin/end once the scratch is there: a replay gives the bytes of the plain calls."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(41)
    n = 2*CHUNK + 9
    x = rng.uniform(0.0, 1.0, size=(2, n)).astype(np.float32)
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    dx = hipdsp.DeviceArray.from_host(c, x)
    e = np.linspace(0.0, 1.0, 50)
    bounds = hipdsp.DeviceArray.from_host(c, np.array([[0.25, 0.75, 0.25], [-np.inf, 0.5, 0.5]]))
    want_h = hipdsp.histogram(c, dx, n, 2, 1, n, e)                     # (also: the scratch now holds both sizes)
    want_m = hipdsp.masked_stats(c, dx, n, 2, 1, n, bounds)
    for ch in range(2):
        assert want_h[ch].tolist() == td.numpy_slots(x[ch, 1:], e).tolist()
    dh = hipdsp.DeviceArray(c, (2, 52), np.int64)
    dm = hipdsp.DeviceArray(c, (2, 4), np.float64)
    c.synchronize()
    c.graph_begin()
    hipdsp.histogram(c, dx, n, 2, 1, n, e, out=dh)
    hipdsp.masked_stats(c, dx, n, 2, 1, n, bounds, out=dm)
    graph = c.graph_end()
    dh.copy_from_host(np.full((2, 52), -1, dtype=np.int64))
    c.graph_launch(graph)
    c.synchronize()
    assert dh.to_host().tobytes() == want_h.tobytes() and dm.to_host().tobytes() == want_m.tobytes()
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)


# ---- the facade ----------------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def device_copy_trace():
    from audian_amd import hipdsp
    from audian_amd.buffereddata import BufferedData

    class DeviceCopy(BufferedData):
        """A derived trace whose process() copies its source on the device: the mirror holds the source's float32
        samples bit for bit, and the host copy is stale."""

        def __init__(self):
            super().__init__('copy', 'data')

        def open(self, source):
            super().open(source, 1)

        def process(self, source, dest, nbefore):
            call = self._take_call(source, dest)
            if len(dest) == 0:
                return
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            dsrc, spitch, keep = self._device_source(source, call)
            hipdsp.memcpy2d(self.ctx, ddst, 4*dpitch, hipdsp.DeviceArray(self.ctx, (1,), np.float32,
                                                                          ptr=hipdsp._p(dsrc).value + 4*nbefore),
                            4*spitch, 4*len(dest), self.channels)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            self.ctx.synchronize()

    return DeviceCopy()


def open_copy_graph(x, rate):
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(buffer_time=len(x)/rate + 10.0, back_time=0.0)
    g.add_trace(device_copy_trace())
    g.setup_traces()
    g.open(np.asarray(x, dtype=np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g.update_times(0.0, len(x)/rate)
    return g


@pytest.fixture(scope='module')
def golden():
    g = load_golden('threshold_estimates')
    return g, td.tiled(g['x'], int(g['tiled_times']), int(g['tiled_frames']))


@pytest.mark.parametrize('case', ['stored', 'tiled'])
def test_facade_threshold_estimates_match_the_reference(golden, case):
    """BufferedData.threshold_estimates on a device-resident trace against the reference's thresholds at rtol 1e-9:
    with n <= 2^20 the header's contract gives (n + 3) 2^-53 <= 1.2e-10 per moment, and the fixtures' margins (no sample
    within 1e-7 of mean + 3 std, the branch 1e-2 clear) rule out a flipped sample or branch.  Four reductions run on
    the mirror and nothing is read back."""
    from audian_amd import hipdsp
    from audian_amd.bufferedarray import BufferedArray
    g, tiled = golden
    x, want = (g['x'], g['thresholds']) if case == 'stored' else (tiled, g['tiled_thresholds'])
    graph = open_copy_graph(x, 1000.0)
    tr = graph['copy']
    assert tr._dev is not None and len(tr._buf()) == len(x) and tr.offset == 0
    assert any(r[0] == 0 and r[1] == len(x) for r in tr._dev_valid)
    stale = [list(r) for r in tr._stale]
    assert stale
    before = dict(hipdsp.launches)
    got = tr.threshold_estimates()
    assert {k: hipdsp.launches[k] - before.get(k, 0) for k in ('region_stats', 'histogram', 'masked_stats')} == \
        {'region_stats': 1, 'histogram': 1, 'masked_stats': 2}
    assert [list(r) for r in tr._stale] == stale                        # nothing crossed but counts and moments
    print(case, 'relative differences', np.abs(got - want)/np.abs(want))
    assert got.dtype == np.float64 and got.shape == (4,)
    assert np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
    assert np.array_equal(tr.event_thresholds(3.0, method='histogram'), got)
    assert np.array_equal(graph.event_thresholds('copy', 3.0, method='histogram'), got)
    # the primitives on the mirror against the host fallback on the same frames (absolute frame indices)
    e = np.linspace(0.0, float(x.max()), 50)
    a, b = 7, len(x) - 5
    h = tr.histogram(e, a, b)
    m = tr.masked_stats([0.03, 0.02, -np.inf, 0.1], [np.inf, 0.04, 0.05, 0.2], start=a, stop=b)
    assert tr.histogram(e, a, b, channel=2).tolist() == h[2].tolist()
    assert [list(r) for r in tr._stale] == stale
    for c in range(4):
        assert h[c].tolist() == td.numpy_slots(x[a:b, c], e).tolist()
    launches = dict(hipdsp.launches)
    assert BufferedArray.histogram(tr, e, a, b).tolist() == h.tolist()           # this reads the mirror back
    fb = BufferedArray.masked_stats(tr, [0.03, 0.02, -np.inf, 0.1], [np.inf, 0.04, 0.05, 0.2], start=a, stop=b)
    assert hipdsp.launches.get('histogram') == launches.get('histogram')
    assert m[3, 0] == 0 and np.isnan(m[3, 1:3]).all()                   # nothing of the odd channel lies in (0.1, 0.2)
    assert np.array_equal(m[:, 0], fb[:, 0]) and np.allclose(m[:, 1:3], fb[:, 1:3], rtol=1e-9, atol=0, equal_nan=True)
    # a sub-range: the definition on that range; a range without a positive maximum: the ValueError
    sub = tr.threshold_estimates(100, 4100)
    assert np.allclose(sub, td.threshold_estimates(x[100:4100])[0], rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match='maximum'):
        tr.threshold_estimates(50, 50)


def test_facade_histogram_thresholds_to_events_to_the_table(golden):
    """event_thresholds(method='histogram') -> detect_events -> analyze_events on the device against the host fallback
    path: the bursts of the even channels are found, the odd channels (threshold max + std) have no event."""
    from audian_amd import hipdsp
    from audian_amd.analyzer import StatisticsAnalyzer
    from audian_amd.bufferedarray import BufferedArray
    g, tiled = golden
    rate = 1000.0
    graph = open_copy_graph(tiled, rate)
    tr = graph['copy']
    a = StatisticsAnalyzer(graph, 'copy')
    t1 = 40.0
    before = dict(hipdsp.launches)
    thr = graph.event_thresholds('copy', 1.0, 0.0, t1, method='histogram')
    ev = graph.detect_events('copy', thr, min_gap=0.01, min_duration=0.02, t0=0.0, t1=t1)
    assert hipdsp.launches['histogram'] == before.get('histogram', 0) + 1
    assert hipdsp.launches['detect_events'] == before.get('detect_events', 0) + 1
    graph.analyze_events(ev)
    rows = a.rows()
    i0, i1 = graph.region_frames(tr, 0.0, t1)
    assert np.allclose(thr, td.threshold_estimates(tiled[i0:i1])[0], rtol=1e-9, atol=0)
    host = np.asarray(tr[i0:i1])                                        # the host values last (this reads back)
    assert np.array_equal(host, tiled[i0:i1].astype(np.float64))
    fb = BufferedArray.detect_events(tr, thr, 0.01, 0.02, i0, i1)
    k = 0
    for c in range(4):
        assert ev.frames(c).tolist() == fb.frames(c).tolist()
        assert (len(ev.onsets[c]) >= 3) == (c % 2 == 0) and (c % 2 == 0 or len(ev.onsets[c]) == 0)
        for p, q in ev.frames(c).tolist():
            v = host[p - i0:q - i0, c]
            assert abs(rows[k][0] - v.mean()) <= 1e-12 and abs(rows[k][1] - v.std()) <= 1e-12, (c, p, q)
            k += 1
    assert k == len(rows) == len(ev)
