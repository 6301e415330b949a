"""hipdsp_find_peaks, BufferedData.find_peaks and TraceGraph.find_peaks / mark_peaks on the GPU.  The comparator is
never the code under test: tests/peaks_definition.py, the definition as plain loops (pinned to scipy by
tests/golden/find_peaks.npz), and for the long rows audian_amd.peaks.host_find_peaks, which tests/test_peaks_host.py
holds to that definition.  Every comparison is exact: integer positions, float64 heights, prominences (NaN equal to
NaN) and bases.

The kernels cut [start, stop) into chunks of C = hipdsp.PEAKS_CHUNK samples from `start`, one 64-lane wave per chunk
and channel, lane l owning the bits of samples 64*l ... 64*l + 63 of the chunk; a run of equal samples that enters a
chunk brings its first sample along through a scan over the chunks in which each of 256 threads walks
ceil(chunks/256) chunks.  The prominence search skips whole blocks of B samples, B in hipdsp.PEAKS_BLOCKS, that hold
nothing higher than the peak.  The shapes below follow those constants."""

import ctypes
import math

import numpy as np
import pytest

import gpu_helpers as gh
import peaks_definition as pd

pytestmark = pytest.mark.gpu

INF = math.inf
OPEN6 = [-INF, INF]*3
MIXED = [0.0, 2.0, -INF, 3.0, 1.0, INF]        # hmin, hmax, tmin, tmax, pmin, pmax
SENTINEL = -77


def constants():
    from audian_amd import hipdsp
    return hipdsp.PEAKS_CHUNK, hipdsp.PEAKS_BLOCKS


def expected(row, borders, wlen, first=0):
    """The definition on a short row, its vectorised form on a long one: (positions, (K, 4) properties)."""
    from audian_amd.peaks import host_find_peaks
    b = [float(v) for v in borders]
    if len(row) <= 3000:
        pos, props = pd.find_peaks(row, (b[0], b[1]), (b[2], b[3]), (b[4], b[5]), wlen, first=first)
        return np.asarray(pos, dtype=np.int64), np.asarray(props, dtype=np.float64).reshape(-1, 4)
    return host_find_peaks(row, (b[0], b[1]), (b[2], b[3]), (b[4], b[5]), wlen, first=first)


def same(got, want):
    return got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1], equal_nan=True)


def small_integers(rng, C, n, special=True):
    x = rng.integers(-3, 4, size=(C, n)).astype(np.float32)
    if n:
        x[1 % C] = np.repeat(x[1 % C], rng.integers(1, 4, size=n))[:n]        # runs
    if special:
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random((C, n)) < 0.03] = value
    return x


class Slab(object):
    """A host (C, frames) float32 array on the device, `base` elements into its allocation, pitch = frames + 7; the
    elements around the rows are +inf: higher than everything, they must not be looked at."""

    def __init__(self, x, base=3, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.base, self.pitch = base, self.frames + pitch_extra
        host = np.full(base + self.C*self.pitch + 1, np.inf, dtype=np.float32)
        for c in range(self.C):
            host[base + c*self.pitch:base + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(base, (1,))

    def peaks(self, start, stop, borders, wlen=0, capacity=None, channels=None, props=True):
        """[(positions, properties)] per channel; channels=(a, b): a call on the view of rows a ... b-1."""
        from audian_amd import hipdsp
        a, b = (0, self.C) if channels is None else channels
        view = self.dev.view(self.base + a*self.pitch, (1,))
        got = hipdsp.find_peaks(self.ctx, view, self.pitch, b - a, start, stop, borders, wlen, props=props,
                                capacity=capacity)
        assert len(got) == b - a and all(p.dtype == np.int64 and p.ndim == 1 for p, q in got)
        assert all(q is None for p, q in got) if not props else all(q.shape == (len(p), 4) for p, q in got)
        return got

    def check(self, start, stop, borders, wlen=0, note=None):
        """One call against the comparator, every channel; `borders` six values or six per channel.  Returns the
        number of peaks."""
        got = self.peaks(start, stop, borders, wlen)
        per = np.broadcast_to(np.asarray(borders, dtype=np.float64), (self.C, 6))
        for c in range(self.C):
            want = expected(self.x[c, start:stop], per[c], wlen, first=start)
            assert same(got[c], want), (note, c, start, stop, wlen, got[c][0][:8], want[0][:8])
        return sum(len(p) for p, q in got)

    def raw(self, start, stop, borders, wlen, capacity, props=True, pitch_extra=0):
        """One call through the C ABI into sentinel-filled device arrays: (peaks (C, pitch), props (C, 4*capacity +
        pitch_extra) or None, counts with a sentinel on either side)."""
        from audian_amd import hipdsp
        dborders = None
        if np.ndim(borders) == 2:
            dborders = hipdsp.DeviceArray.from_host(self.ctx, np.asarray(borders, dtype=np.float64))
        ppitch, qpitch = capacity + pitch_extra, 4*capacity + pitch_extra
        dp = hipdsp.DeviceArray.from_host(self.ctx, np.full((self.C, max(1, ppitch)), SENTINEL, dtype=np.int64))
        dq = hipdsp.DeviceArray.from_host(self.ctx, np.full((self.C, max(1, qpitch)), SENTINEL, dtype=np.float64))
        counts = hipdsp.DeviceArray.from_host(self.ctx, np.full(self.C + 2, SENTINEL, dtype=np.int64))
        hipdsp.find_peaks_into(self.ctx, self.view, self.pitch, self.C, start, stop,
                               dborders if dborders is not None else borders, wlen, capacity,
                               dp if capacity > 0 else None, dq if props and capacity > 0 else None,
                               counts.view(1, (self.C,)), peaks_pitch=ppitch if capacity > 0 else 0,
                               props_pitch=qpitch if capacity > 0 else 0)
        return dp.to_host(), dq.to_host(), counts.to_host()


# ---- 1. small lengths --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('borders', [OPEN6, MIXED], ids=['open', 'mixed'])
def test_small_lengths_every_offset(borders):
    """n = 0 ... 200 at every row offset 0 ... 3 (the address of the row modulo 16 bytes) and start 0 ... 3, three
    channels, wlen 0, 2, 3, 4, 5 in turn.  Small integers with runs, NaN and +-inf."""
    rng = np.random.default_rng(len(borders) + int(borders[0] == 0.0))
    seen = 0
    for n in range(0, 201):
        for base in range(4):
            start = (n + base) % 4
            x = small_integers(rng, 3, start + n + 2)
            slab = Slab(x, base=base)
            seen += slab.check(start, start + n, borders, [0, 2, 3, 4, 5][(n + base) % 5], note=('small', n, base))
    assert seen > (1000 if borders is MIXED else 10000)


# ---- 2. chunk and carry borders ----------------------------------------------------------------------------------

def border_rows(C, s, total):
    """Rows over a floor of small negative integers, one feature each, at the borders of the chunks of a call that
    starts at s; positions relative to s."""
    rng = np.random.default_rng(7)
    feats = []
    for p in range(C - 2, C + 2):
        feats.append([(p, p, 1.0)])                                    # a sharp peak at C-2 ... C+1
    for k, j in [(1, 0), (1, 1), (2, 0), (0, 1), (0, 2), (3, 1), (2, 2), (64, 0), (65, 63)]:
        feats.append([(C - k, C + j, 1.0)])                            # flat peaks over the border, even and odd width
    feats.append([(C, 2*C - 1, 1.0)])                                  # exactly one whole chunk
    feats.append([(C, 4*C - 1, 1.0)])                                  # three whole chunks: the middle holds no end
    feats.append([(C - 1, 4*C - 1, 1.0)])
    feats.append([(C, 4*C, 1.0)])
    feats.append([(C + 1, 4*C - 2, 2.0), (4*C + 5, 4*C + 5, 1.0)])
    feats.append([(0, 9, 1.0)])                                        # touches start: no peak
    feats.append([(0, C + 3, 1.0)])
    feats.append([(C - 5, C + 5, 1.0), (C - 6, C - 6, np.nan)])        # a NaN right before, right after: no peak
    feats.append([(C - 5, C + 5, 1.0), (C + 6, C + 6, np.nan)])
    feats.append([(C - 1, C - 1, np.nan), (C, C + 5, 1.0)])
    feats.append([(C - 6, C - 1, 1.0), (C, C, np.nan)])
    feats.append([(2*C - 3, 2*C + 2, np.inf), (5, 5, -np.inf)])
    x = rng.integers(-40, 0, size=(len(feats), s + total)).astype(np.float32)      # (40 levels: the walks of the floor stay short)
    for c, row in enumerate(feats):
        for a, b, value in row:
            x[c, s + a:s + b + 1] = value
    return x


@pytest.fixture(scope='module')
def border_slab():
    C, blocks = constants()
    x = border_rows(C, 3, 5*C + 3)
    return x, Slab(x), 3


@pytest.mark.parametrize('chunks, extra', [(1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 5), (4, 0), (5, 3)])
def test_chunk_borders(border_slab, chunks, extra):
    """Sizes around one, two and three chunks, and 4C and 5C + 3 for the plateau of three chunks; a plateau that is cut
    by `stop` touches stop - 1: no peak."""
    C, blocks = constants()
    x, slab, s = border_slab
    n = chunks*C + extra
    assert slab.check(s, s + n, OPEN6, 0, note=('borders', n)) > 1000
    if chunks in (3, 5):
        slab.check(s, s + n, [-0.5, INF, -INF, INF, 1.5, INF], 0, note=('borders closed', n))


def test_chunk_borders_spelled_out(border_slab):
    C, blocks = constants()
    x, slab, s = border_slab
    got = slab.peaks(s, s + 5*C + 3, [0.5, INF] + OPEN6[2:])
    assert [g[0].tolist() for g in got[:4]] == [[s + p] for p in range(C - 2, C + 2)]
    assert got[13][0].tolist() == [s + C + (C - 1)//2] and got[14][0].tolist() == [s + (5*C - 1)//2]
    assert got[15][0].tolist() == [s + (5*C - 2)//2] and got[16][0].tolist() == [s + (5*C)//2]
    assert got[17][0].tolist() == [s + (5*C - 1)//2, s + 4*C + 5]
    assert all(len(g[0]) == 0 for g in got[18:24]) and got[24][0].tolist() == [s + 2*C - 1]
    assert all(len(g[0]) == 0 for g in slab.peaks(s, s + 4*C, [0.5, INF] + OPEN6[2:])[14:17])      # cut by stop


@pytest.fixture(scope='module')
def many_chunks():
    """One row of 600 chunks + 3: spikes of random height some 1500 samples apart over a floor of -1, a plateau from
    chunk 100 to chunk 400 (its first sample comes to its last through 300 chunks of the scan); and a row of flat peaks
    of random height, each half a chunk and three samples wide."""
    C, blocks = constants()
    rng = np.random.default_rng(9)
    s, n = 2, 600*C + 3
    x = np.full((2, s + n + 1), -1.0, dtype=np.float32)
    at = rng.integers(10, 1500)
    while at < n - 10:
        x[0, s + at] = float(rng.integers(0, 40))
        at += int(rng.integers(2, 3000))
    x[0, s + 100*C + 5:s + 400*C + 9] = 50.0
    run = np.arange(s + n + 1)//(C//2 + 3)                            # runs of C/2 + 3 samples: a flat peak every 7 runs
    x[1] = np.where(run % 7 == 6, 10 + rng.integers(0, 30, size=run[-1] + 1)[run], run % 7)
    return x, Slab(x), s


@pytest.mark.parametrize('chunks', [255, 256, 257, 600])
def test_many_chunks(many_chunks, chunks):
    C, blocks = constants()
    x, slab, s = many_chunks
    for n in (chunks*C, chunks*C + 3):
        assert slab.check(s, s + n, OPEN6, 0, note=('chunks', n)) > 300
        slab.check(s, s + n, [-INF, INF, 0.5, INF, 3.0, 60.0], 0, note=('chunks closed', n))
    if chunks == 600:
        assert s + (500*C + 13)//2 in slab.peaks(s, s + 600*C, OPEN6)[0][0].tolist()


# ---- 3. prominence searches --------------------------------------------------------------------------------------

def test_staircases():
    """Descending: every right-hand search runs to the end of the row; ascending: every left-hand one to its start.
    The valleys hold equal minima: the nearest one is the base."""
    C, blocks = constants()
    n, s = 2*C + 77, 1
    x = np.zeros((2, s + n), dtype=np.float32)
    k = np.arange(s + n)
    steps = 300 - k//29                                               # a peak every 29 samples, each lower than the last
    x[0] = np.where(k % 29 == 7, steps, np.where(k % 29 == 20, -2.0, -1.0))
    x[1] = x[0, ::-1]
    slab = Slab(x)
    assert slab.check(s, s + n, OPEN6, 0, note='stairs') > 500
    slab.check(s, s + n, [-INF, INF, -INF, INF, 100.0, 250.0], 0, note='stairs closed')
    slab.check(s + 5, s + n - 9, OPEN6, 2*C, note='stairs wlen')


@pytest.mark.parametrize('level', [0, 1, 2])
def test_stoppers_at_block_borders(level):
    """For the table level of B samples: a peak whose walk to the right ends at a stopper B-1, B, B+1 ... past a block
    border (at 2B-1, 2B, 2B+1: inside the last block that could be skipped, right after it, one further) and one whose
    walk to the left ends at B+1, B, B-1; the stopper a higher sample or a NaN.  Equal minima lie in different blocks."""
    C, blocks = constants()
    B = blocks[level]
    n, s = 2*B + 100, 1
    rows = []
    for stopper in (9.0, np.nan):
        for side in (+1, -1):
            for d in (-1, 0, 1):
                x = np.full(s + n, -1.0, dtype=np.float32)
                m, q = (10, 2*B + d) if side > 0 else (2*B + 90, B + d)
                x[s + m] = 5.0
                x[s + q] = stopper
                for p in (B//2, B + B//2, B + B//2 + 1, B - 3, B + 7, 2*B + 50, 30):
                    if abs(p - q) > 1 and abs(p - m) > 1:
                        x[s + p] = -3.0                                # equal minima: the nearest is the base
                x[s + 2*B + 95] = 2.0                                  # small peaks near both ends
                x[s + 3] = 2.0
                rows.append(x)
    slab = Slab(np.stack(rows))
    assert slab.check(s, s + n, OPEN6, 0, note=('stoppers', B)) >= 12*3
    slab.check(s, s + n, [-INF, INF, -INF, INF, 7.5, INF], 0, note=('stoppers closed', B))
    slab.check(s, s + n, OPEN6, 2*B - 30, note=('stoppers wlen', B))
    # no lower sample on one side: the base is the peak itself
    flat = np.full((1, s + n), -1.0, dtype=np.float32)
    flat[0, s + 40:s + B + 40] = 3.0
    got = Slab(flat).peaks(s, s + n, OPEN6, B//2)[0]
    m = s + 40 + (B - 1)//2
    assert got[0].tolist() == [m] and got[1].tolist() == [[3.0, 0.0, m, m]]


def test_window_lengths():
    """wlen around one and two 64-blocks and two chunks, and larger than the row; a window that ends inside a plateau;
    a +inf plateau wider than wlen has a NaN prominence: kept under open borders, dropped under a closed one."""
    C, blocks = constants()
    rng = np.random.default_rng(13)
    n, s = 3*C + 5, 2
    x = np.zeros((3, s + n + 1), dtype=np.float32)
    x[0] = np.round(4*rng.standard_normal(s + n + 1))/4
    x[1] = np.repeat(rng.integers(-3, 4, size=(s + n)//40 + 2), 40)[:s + n + 1]          # plateaus of 40
    x[2] = np.repeat(rng.integers(-3, 4, size=(s + n)//700 + 2), 700)[:s + n + 1]        # plateaus of 700
    x[2, s + 1000:s + 1300] = np.inf
    x[2, s + C - 100:s + C + 200] = np.inf
    slab = Slab(x)
    nan = 0
    for wlen in [2, 3, 63, 64, 65, 127, 128, 129, 2*C - 1, 2*C, 2*C + 1, 5*C]:
        slab.check(s, s + n, OPEN6, wlen, note='wlen open')
        slab.check(s, s + n, [-INF, INF, -INF, INF, 0.5, INF], wlen, note='wlen closed')
        got = slab.peaks(s, s + n, OPEN6, wlen)[2]
        kept = slab.peaks(s, s + n, [-INF, INF, -INF, INF, -1e300, INF], wlen)[2]
        assert np.isnan(got[1][:, 1]).sum() == (2 if wlen < 300 else 0)
        assert len(kept[0]) == len(got[0]) - np.isnan(got[1][:, 1]).sum()
        nan += int(np.isnan(got[1][:, 1]).sum())
    assert nan == 16


# ---- 4. random ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def noise():
    C, blocks = constants()
    rng = np.random.default_rng(21)
    x = rng.standard_normal((5, 3*C + 77)).astype(np.float32)
    x[3:] = np.round(4*x[3:])/4                                        # quarters: many ties
    x[4, rng.integers(0, x.shape[1], size=40)] = np.nan
    return x, Slab(x)


def test_random_rows_and_per_channel_borders(noise):
    x, slab = noise
    start, stop = 2, x.shape[1] - 3
    assert slab.check(start, stop, OPEN6) > 5*(stop - start)//5
    per = np.array([[0.0, INF, -INF, INF, 0.5, INF], OPEN6, [-INF, 1.0, 0.25, 2.0, -INF, 3.0],
                    [0.5, INF, -INF, INF, 1.0, 2.0], [-INF, INF, -INF, INF, math.nan, INF]])
    assert slab.check(start, stop, per, 0, note='per channel') > 1000
    slab.check(start, stop, per, 301, note='per channel wlen')
    full = slab.peaks(start, stop, per, 301)
    for c in range(5):                                                  # the by-value form, channel by channel
        assert same(slab.peaks(start, stop, per[c], 301, channels=(c, c + 1))[0], full[c])
    assert len(full[4][0]) == 0


# ---- 5. capacity -------------------------------------------------------------------------------------------------

def test_capacity(noise):
    from audian_amd import hipdsp
    x, slab = noise
    start, stop = 2, x.shape[1] - 3
    borders = [0.0, INF, -INF, INF, 0.5, INF]
    want = [expected(x[c, start:stop], borders, 0, first=start) for c in range(5)]
    counts = [len(w[0]) for w in want]
    for cap in [min(counts) - 10, min(counts), max(counts), max(counts) + 5]:
        dp, dq, dc = slab.raw(start, stop, borders, 0, cap, pitch_extra=6)
        assert dc.tolist() == [SENTINEL] + counts + [SENTINEL]                          # always the true counts
        for c in range(5):
            k = min(counts[c], cap)
            assert dp[c, :k].tolist() == want[c][0][:k].tolist() and (dp[c, k:] == SENTINEL).all()
            assert np.array_equal(dq[c, :4*k].reshape(k, 4), want[c][1][:k]) and (dq[c, 4*k:] == SENTINEL).all()
    # a capacity of 0 with NULL outputs: counts only; props NULL with peaks given
    dp, dq, dc = slab.raw(start, stop, borders, 0, 0)
    assert dc.tolist() == [SENTINEL] + counts + [SENTINEL] and (dp == SENTINEL).all() and (dq == SENTINEL).all()
    dp, dq, dc = slab.raw(start, stop, borders, 0, max(counts), props=False)
    assert all(dp[c, :counts[c]].tolist() == want[c][0].tolist() for c in range(5)) and (dq == SENTINEL).all()
    # an empty range: zero counts, nothing else
    dp, dq, dc = slab.raw(7, 7, borders, 0, 10)
    assert dc.tolist() == [SENTINEL] + [0]*5 + [SENTINEL] and (dp == SENTINEL).all() and (dq == SENTINEL).all()
    # the Python call: a fixed capacity truncates in one launch, None counts first and stores second
    before = hipdsp.launches.get('find_peaks', 0)
    got = slab.peaks(start, stop, borders, capacity=100)
    assert all(same(g, (w[0][:100], w[1][:100])) for g, w in zip(got, want))
    assert hipdsp.launches['find_peaks'] == before + 1
    got = slab.peaks(start, stop, borders, props=False)
    assert [g[0].tolist() for g in got] == [w[0].tolist() for w in want]
    assert hipdsp.launches['find_peaks'] == before + 3


# ---- 6. determinism and independence -----------------------------------------------------------------------------

def test_same_bytes_twice_and_independence(noise):
    from audian_amd import hipdsp
    x, slab = noise
    start, stop = 5, x.shape[1] - 40
    borders = [-INF, INF, -INF, INF, 0.25, INF]
    cap = (stop - start)//2
    first = slab.raw(start, stop, borders, 77, cap)
    again = slab.raw(start, stop, borders, 77, cap)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    full = slab.peaks(start, stop, borders, 77)
    part = slab.peaks(start, stop, borders, 77, channels=(1, 3))
    assert same(part[0], full[1]) and same(part[1], full[2])
    # start > 0 and stop < frames: the call on a copy of the slice, positions shifted
    cut = Slab(x[:, start:stop], base=1).peaks(0, stop - start, borders, 77)
    shift = np.array([0.0, 0.0, start, start])
    assert all(same((p + start, q + shift), f) for (p, q), f in zip(cut, full))
    assert sum(len(p) for p, q in full) > 1000


def test_inside_a_captured_graph(noise):
    """Legal between hipdsp_graph_begin and hipdsp_graph_end once the scratch is there: a replay gives the bytes of
    the plain call."""
    from audian_amd import hipdsp
    x, slab = noise
    C, n = x.shape
    borders = [-INF, INF, -INF, INF, 0.25, INF]
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    dx = hipdsp.DeviceArray.from_host(c, x)
    cap = n//2
    arrays = [[hipdsp.DeviceArray.from_host(c, np.full(shape, SENTINEL, dtype=dt)) for shape, dt in
               (((C, cap), np.int64), ((C, cap, 4), np.float64), ((C,), np.int64))] for k in range(2)]
    hipdsp.find_peaks_into(c, dx, n, C, 1, n - 1, borders, 500, cap, *arrays[0])       # (also: the scratch is there now)
    c.synchronize()
    c.graph_begin()
    hipdsp.find_peaks_into(c, dx, n, C, 1, n - 1, borders, 500, cap, *arrays[1])
    graph = c.graph_end()
    c.graph_launch(graph)
    c.synchronize()
    for plain, replay in zip(*arrays):
        assert plain.to_host().tobytes() == replay.to_host().tobytes()
    assert arrays[1][2].to_host().min() > 100
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)


# ---- 7. errors ---------------------------------------------------------------------------------------------------

def test_errors(noise):
    """Every HIPDSP_ERR_INVALID and HIPDSP_ERR_UNSUPPORTED case of the header: the status, the text of
    hipdsp_last_error() and outputs that stay as they were."""
    from audian_amd import _lib, hipdsp
    x, slab = noise
    C, n, cap = 5, x.shape[1], 50
    dp = hipdsp.DeviceArray.from_host(slab.ctx, np.full((C, cap + 1), SENTINEL, dtype=np.int64))
    dq = hipdsp.DeviceArray.from_host(slab.ctx, np.full((C, 4*cap + 1), SENTINEL, dtype=np.float64))
    dc = hipdsp.DeviceArray.from_host(slab.ctx, np.full(C + 1, SENTINEL, dtype=np.int64))
    db = hipdsp.DeviceArray.from_host(slab.ctx, np.tile(np.asarray(OPEN6), (C + 1, 1)))
    good = dict(ctx=slab.ctx.handle, x=slab.view.ptr, x_pitch=slab.pitch, channels=C, start=0, stop=n, borders=0,
                wlen=0, capacity=cap, peaks=dp.ptr, peaks_pitch=0, props=dq.ptr, props_pitch=0, counts=dc.ptr)

    def call(**changes):
        a = dict(good, **changes)
        vp, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
        return _lib.lib.hipdsp_find_peaks(a['ctx'], vp(a['x']), i64(a['x_pitch']), i64(a['channels']), i64(a['start']),
                                          i64(a['stop']), vp(a['borders']), *[dbl(v) for v in OPEN6], i64(a['wlen']),
                                          i64(a['capacity']), vp(a['peaks']), i64(a['peaks_pitch']), vp(a['props']),
                                          i64(a['props_pitch']), vp(a['counts']))

    invalid = [
        (dict(ctx=None), 'ctx is NULL'), (dict(counts=0), 'counts is NULL'), (dict(peaks=0), 'peaks is NULL'),
        (dict(x=0), 'NULL data pointer'), (dict(channels=-1), 'negative number of channels'),
        (dict(capacity=-1), 'negative capacity'), (dict(wlen=-1), 'negative wlen'),
        (dict(start=-1), 'no range'), (dict(start=10, stop=9), 'no range'),
        (dict(stop=slab.pitch + 1), 'x_pitch smaller than stop'), (dict(peaks_pitch=cap - 1), 'peaks_pitch smaller'),
        (dict(props_pitch=4*cap - 1), 'props_pitch smaller'), (dict(x=slab.view.ptr + 2), 'x is not aligned'),
        (dict(counts=dc.ptr + 4), 'not aligned to 8'), (dict(peaks=dp.ptr + 4), 'not aligned to 8'),
        (dict(props=dq.ptr + 4), 'not aligned to 8'), (dict(borders=db.ptr + 4), 'not aligned to 8')]
    for changes, text in invalid:
        assert call(**changes) == _lib.ERR_INVALID, changes
        assert text in _lib.last_error(), (changes, _lib.last_error())
    unsupported = [(dict(channels=65536), 'at most 65535 channels'),
                   (dict(channels=1, stop=2**40 + 1, x_pitch=2**40 + 1), 'at most 2^40 elements')]
    for changes, text in unsupported:
        assert call(**changes) == _lib.ERR_UNSUPPORTED, changes
        assert text in _lib.last_error(), (changes, _lib.last_error())
    assert call(channels=0) == _lib.OK                                  # writes nothing
    slab.ctx.synchronize()
    assert (dp.to_host() == SENTINEL).all() and (dq.to_host() == SENTINEL).all() and (dc.to_host() == SENTINEL).all()
    with pytest.raises(ValueError):
        slab.peaks(10, 9, OPEN6)
    with pytest.raises(NotImplementedError, match='at most 65535 channels'):
        hipdsp.find_peaks_into(slab.ctx, slab.view, slab.pitch, 65536, 0, 10, OPEN6, 0, 0, None, None, dc)
    assert call(borders=db.ptr) == _lib.OK                              # and the same arguments are a good call
    counts = dc.to_host()[:C]
    assert counts.tolist() == [len(expected(x[c], OPEN6, 0)[0]) for c in range(C)]


# ---- 8. the facade -----------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


@pytest.fixture(scope='module')
def scrolled_graph():
    """filter + envelope on 3 channels x 60 s x 16 kHz with bursts of a 900 Hz tone; windows of 5 s in buffers of 30 s
    plus the margins the filter and the envelope ask for, after two scrolls (the second keeps an overlap)."""
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.tracegraph import TraceGraph
    rate, seconds, C = 16000.0, 60.0, 3
    rng = np.random.default_rng(31)
    n = int(rate*seconds)
    t = np.arange(n)/rate
    x = 0.02*rng.uniform(-1, 1, size=(n, C))
    for c in range(C):
        for t0 in np.arange(0.3 + 0.1*c, seconds, 0.7 + 0.2*c):
            on = slice(int(t0*rate), int((t0 + 0.15 + 0.05*c)*rate))
            x[on, c] += 0.5*np.sin(2*np.pi*900.0*t[on])*np.sin(2*np.pi*25.0*t[on])**2
    g = TraceGraph(30.0, 2.0)
    for tr in (BufferedFilter(), BufferedEnvelope(envelope_cutoff=200.0)):
        g.add_trace(tr)
    g.setup_traces()
    g.open(x.astype(np.float32).astype(np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g['filtered'].highpass_cutoff, g['filtered'].lowpass_cutoff = 300.0, 3000.0
    g['filtered'].update()
    g.update_times(0.0, 5.0)
    g.update_times(40.0, 45.0)
    g.update_times(52.0, 58.0)                                         # the scrolls: the buffers move
    return g


def peaks_of(pk, c):
    return pk.indices[c], np.stack((pk.heights[c], pk.prominences[c], pk.left_bases[c], pk.right_bases[c]), axis=1)


def test_facade_envelope_mirror_against_the_definition(scrolled_graph):
    from audian_amd import hipdsp
    from audian_amd.bufferedarray import BufferedArray
    g = scrolled_graph
    env = g['envelope']
    assert env.offset > 0 and env._dev is not None and env._dev_valid
    a, b = env._dev_valid[0]
    assert b - a >= 5*16000
    start, stop = env.offset + a, env.offset + b
    stale = [list(r) for r in env._stale]
    assert stale
    before = hipdsp.launches.get('find_peaks', 0)
    heights = np.array([0.05, 0.06, 0.04])
    pk = env.find_peaks(height=heights, prominence=(0.02, None), wlen=0.0625, start=start, stop=stop)
    assert hipdsp.launches['find_peaks'] == before + 2                 # on the mirror: one call counts, one stores
    assert [list(r) for r in env._stale] == stale                      # nothing crossed but counts, positions, properties
    assert pk.rate == env.rate and pk.channels == 3 and pk.trace_name == 'envelope'
    host = np.asarray(env[start:stop])                                 # the host values last (this reads back)
    assert np.array_equal(host.astype(np.float32).astype(np.float64), host)
    for c in range(3):
        want = pd.find_peaks(host[:, c], (heights[c], INF), pd.OPEN, (0.02, INF), 1000, first=start)
        assert pd.same(*peaks_of(pk, c), want) and len(want[0]) >= 10
    fb = BufferedArray.find_peaks(env, heights, None, (0.02, None), 0.0625, start, stop)
    assert all(same(peaks_of(fb, c), peaks_of(pk, c)) for c in range(3))
    assert hipdsp.launches['find_peaks'] == before + 2
    # a mirror that is valid over less than the range: the host buffer serves, no launch
    valid = [list(r) for r in env._dev_valid]
    env._dev_valid = [[a, b - 1000]]
    try:
        pk = env.find_peaks(height=0.05, start=start, stop=stop)
    finally:
        env._dev_valid = valid
    assert hipdsp.launches['find_peaks'] == before + 2
    assert pd.same(*peaks_of(pk, 0), pd.find_peaks(host[:, 0], (0.05, INF), first=start))


def test_facade_find_mark_and_count_in_events(scrolled_graph):
    """TraceGraph.find_peaks with t0 and t1 moves the buffers and returns absolute frames; mark_peaks fills the
    analyzer's point store; Peaks.in_events(detect_events(...)) counts the pulses of every song."""
    from audian_amd import hipdsp
    from audian_amd.analyzer import Analyzer
    from audian_amd.bufferedarray import BufferedArray
    g = scrolled_graph
    env = g['envelope']
    before = dict(hipdsp.launches)
    pk = g.find_peaks('envelope', height=0.05, prominence=0.02, t0=20.0, t1=26.0)
    assert hipdsp.launches['find_peaks'] == before.get('find_peaks', 0) + 2
    i0, i1 = g.region_frames(env, 20.0, 26.0)
    assert env.offset <= i0 and i1 <= env.offset + len(env._hostbuf)
    fb = BufferedArray.find_peaks(env, 0.05, None, 0.02, None, i0, i1)
    for c in range(3):
        assert same(peaks_of(pk, c), peaks_of(fb, c)) and len(pk.indices[c]) >= 10
        assert pk.indices[c].min() >= i0 and pk.indices[c].max() < i1
    a = Analyzer(g, 'pulses', 'envelope')
    try:
        a.make_trace_events('pulse', 'envelope', 'o', '#ff0000', 8)
        g.mark_peaks(a, 'pulse', pk)
        for c in range(3):
            t, h = a.events['pulse'][c]
            assert t.tolist() == (pk.indices[c]/env.rate).tolist() and h.tolist() == pk.heights[c].tolist()
        ev = g.detect_events('envelope', 0.03, min_gap=0.05, min_duration=0.05, t0=20.0, t1=26.0)
        host_ev = BufferedArray.detect_events(env, 0.03, 0.05, 0.05, i0, i1)
        for c in range(3):
            assert ev.frames(c).tolist() == host_ev.frames(c).tolist() and len(ev.onsets[c]) >= 3
            want = [int(((fb.indices[c] >= p) & (fb.indices[c] < q)).sum()) for p, q in host_ev.frames(c).tolist()]
            assert pk.in_events(ev, c).tolist() == want and sum(want) >= 10
    finally:
        if a in g.analyzers:
            g.analyzers.remove(a)
