"""hipdsp_detect_events, BufferedData.detect_events and TraceGraph.detect_events / analyze_events on the GPU.  The
comparator is never the code under test: tests/events_definition.py, a plain loop that finds the runs, merges them and
filters them (np.diff for the runs of the million-sample rows).  Every comparison is exact integer equality.

The kernels cut [start, stop) into chunks of CHUNK = 4096 samples from `start`, one 64-lane wave per chunk and channel,
lane l owning the 64-bit word of `above` bits of samples 64*l ... 64*l + 63 of the chunk; what a chunk needs from
outside itself (the last above sample before it, the first after it, the last onset before it, its first output slot)
comes from scans over the chunks in which each of 256 threads walks ceil(chunks/256) chunks.  So of the sizes here
  1, 2, 3               less than one word, at every start (the chunk grid and the words move with `start`);
  63, 64, 65            one word, and one sample past it: runs and gaps that cross a word border (a lane border);
  255 ... 257           four words;
  4095, 4097            one chunk less a sample, and the first size with a second chunk;
  2*CHUNK + 5, 3*CHUNK + 5   three and four chunks: runs, single samples and gaps at and across chunk borders, and a
                        whole chunk without an above sample between two runs (the carries cross an empty chunk);
  257*CHUNK + 3         258 chunks: a thread of the scans walks two chunks (the per-thread loop first runs twice at
                        257 chunks, 256*CHUNK + 1 samples; this is the next size up and has a partial last chunk), and
                        with alternating samples one chunk emits 2048 events, 32 per lane."""

import numpy as np
import pytest

import events_definition as ed
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

CHUNK = 4096
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4097]
STARTS = [0, 1, 2, 3, 5]
BASE = 3                                       # elements between the allocation and x
GAPS = [0, 1, 5]
MIN_LENS = [0, 1, 4]
FAMILIES = ['normal', 'integers', 'spikes', 'special']
THRESHOLDS = [0.25, 0.0, 1.0]                  # one per channel; the integer family ties at 0 and 1


def family(name, rng, C, n):
    if name == 'integers':
        x = np.round(1.5*rng.standard_normal((C, n)))
    elif name == 'spikes':
        x = np.where(rng.random((C, n)) < 0.04, 2.0, -1.0)
    else:
        x = rng.standard_normal((C, n))
    x = x.astype(np.float32)
    if name == 'special':
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random((C, n)) < 0.03] = value
    return x


class Slab(object):
    """A host (C, frames) float32 array on the device with a base offset of 3 elements and pitch = frames + 7."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(BASE + self.C*self.pitch, 12345.0, dtype=np.float32)       # above every threshold used here
        for c in range(self.C):
            host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(BASE, (1,))

    def events(self, start, stop, thresholds, min_gap, min_len, capacity=None, channel=None):
        """Per-channel lists of (onset, offset) tuples; channel=c: a one-channel call on the view of row c."""
        from audian_amd import hipdsp
        view, C = (self.view, self.C) if channel is None else (self.dev.view(BASE + channel*self.pitch, (1,)), 1)
        got = hipdsp.detect_events(self.ctx, view, self.pitch, C, start, stop, thresholds, min_gap, min_len, capacity)
        assert len(got) == C and all(g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2 for g in got)
        return [[tuple(p) for p in g.tolist()] for g in got]

    def raw(self, start, stop, thresholds, min_gap, min_len, capacity, sentinel=-77, pitch_extra=0):
        """One call through the C ABI into sentinel-filled device arrays: (events bytes as int64 (C, pitch), counts)."""
        from audian_amd import hipdsp
        pitch = 2*capacity + pitch_extra
        dthr = hipdsp.DeviceArray.from_host(self.ctx, np.asarray(thresholds, dtype=np.float32))
        dev = hipdsp.DeviceArray.from_host(self.ctx, np.full((self.C, max(1, pitch)), sentinel, dtype=np.int64))
        counts = hipdsp.DeviceArray.from_host(self.ctx, np.full(self.C + 2, sentinel, dtype=np.int64))
        hipdsp.detect_events_into(self.ctx, self.view, self.pitch, self.C, start, stop, dthr, min_gap, min_len, capacity,
                                  dev if capacity > 0 else None, counts.view(1, (self.C,)),
                                  events_pitch=pitch if capacity > 0 else 0)
        return dev.to_host(), counts.to_host()


@pytest.mark.parametrize('name', FAMILIES)
def test_small_lengths_every_start(name):
    """Lengths 1 ... 4097 at starts 0, 1, 2, 3, 5, three channels with a threshold each, min_gap 0, 1, 5 and min_len
    0, 1, 4.  Samples past `stop` and before `start` are above every threshold: they must not be looked at."""
    rng = np.random.default_rng(FAMILIES.index(name))
    seen = 0
    for shift in range(len(STARTS)):
        for k, n in enumerate(LENGTHS):
            start = STARTS[(k + shift) % len(STARTS)]
            x = family(name, rng, 3, start + n + 3)
            x[:, :start] = 50.0
            x[:, start + n:] = 50.0
            slab = Slab(x)
            runs = [ed.runs_by_loop(ed.above_of(x[c, start:start + n], THRESHOLDS[c]), start) for c in range(3)]
            for G in GAPS:
                for L in MIN_LENS:
                    got = slab.events(start, start + n, THRESHOLDS, G, L)
                    want = [ed.merge_and_filter(runs[c], G, L) for c in range(3)]
                    assert got == want, (name, start, n, G, L)
                    seen += sum(len(w) for w in want)
    assert seen > 1000


def border_rows(n, s):
    """Rows of 0 / 1 (threshold 0.5) with their runs at the borders of the chunks of a call that starts at s."""
    C = CHUNK
    spans = [
        [(s + C - 10, s + C + 10)],                                    # a run that spans a border
        [(s + C - 1, s + C)],                                          # one sample, the last of a chunk
        [(s + C, s + C + 1)],                                          # one sample, the first of the next
        [(s + C - 1, s + C + 1), (s + 2*C - 1, s + 2*C)],              # both; and the last of the next chunk
        [(s + C - 20, s + C - 3), (s + C + 4, s + C + 30)],            # a gap of 7 that straddles a border
        [(s + 5, s + C - 5), (s + 2*C + 1, s + 2*C + 4)],              # a gap of C + 6: a whole chunk without a sample
        [(s, s + n)],                                                  # all above
        [],                                                            # none above
        [(s, s + 1), (s + n - 1, s + n)],                              # the first and the last sample only
        [(s + 63, s + 65), (s + 2*C - 64, s + 2*C + 5)],               # a word border, and a run over a chunk border
    ]
    x = np.zeros((len(spans), s + n + 2), dtype=np.float32)
    x[:, :s] = 1.0
    x[:, s + n:] = 1.0
    for c, row in enumerate(spans):
        for a, b in row:
            x[c, a:b] = 1.0
    return x, spans


@pytest.mark.parametrize('n', [2*CHUNK + 5, 3*CHUNK + 5])
def test_chunk_borders(n):
    s = 3
    x, spans = border_rows(n, s)
    slab = Slab(x)
    runs = [ed.runs_by_loop(ed.above_of(x[c, s:s + n], 0.5), s) for c in range(len(spans))]
    assert runs == spans                                               # the rows are what the comments say
    longest = n
    for G in [0, 6, 7, CHUNK + 5, CHUNK + 6, n]:
        for L in [0, 1, 2, 18, CHUNK - 9, CHUNK - 10, longest, longest + 1]:
            got = slab.events(s, s + n, 0.5, G, L)
            want = [ed.merge_and_filter(runs[c], G, L) for c in range(len(spans))]
            assert got == want, (n, G, L)
    # spelled out: the gap that straddles a border merges at G = 7 and not at 6, the carry crosses an empty chunk at
    # G = CHUNK + 6 and not at CHUNK + 5, and L one more than the longest event leaves nothing
    assert slab.events(s, s + n, 0.5, 7, 0)[4] == [(s + CHUNK - 20, s + CHUNK + 30)]
    assert slab.events(s, s + n, 0.5, 6, 0)[4] == spans[4]
    assert slab.events(s, s + n, 0.5, CHUNK + 6, 0)[5] == [(s + 5, s + 2*CHUNK + 4)]
    assert slab.events(s, s + n, 0.5, CHUNK + 5, 0)[5] == spans[5]
    assert slab.events(s, s + n, 0.5, 0, n)[6] == [(s, s + n)]
    assert slab.events(s, s + n, 0.5, n, n + 1) == [[] for c in range(len(spans))]


@pytest.fixture(scope='module')
def long_slab():
    """Two channels of 5 + 257*CHUNK + 3 + 2 samples.  Channel 0: bursts of 1 ... 300 samples some 20000 apart over
    the first part, then alternating samples from chunk 200 on; channel 1: normal noise with the alternating part in
    chunks 3 ... 5 only."""
    rng = np.random.default_rng(11)
    s, n = 5, 257*CHUNK + 3
    x = np.zeros((2, s + n + 2), dtype=np.float32)
    at = s + 17
    while at < s + 200*CHUNK - 400:
        x[0, at:at + int(rng.integers(1, 301))] = 1.0
        at += int(rng.integers(2000, 40000))
    x[0, s + 200*CHUNK + 1::2] = 1.0
    x[1] = (0.3*rng.standard_normal(x.shape[1])).astype(np.float32)
    x[1, s + 3*CHUNK:s + 6*CHUNK:2] = 1.0
    x[1, s + 3*CHUNK + 1:s + 6*CHUNK:2] = 0.0
    x[:, :s] = 1.0
    x[:, s + n:] = 1.0
    slab = Slab(x)
    runs = [ed.runs_by_diff(ed.above_of(x[c, s:s + n], 0.5), s) for c in range(2)]
    return x, slab, s, n, runs


@pytest.mark.parametrize('G, L', [(0, 0), (0, 2), (1, 0), (1999, 5), (40000, 0), (5000, 250)])
def test_many_chunks_sparse_and_dense(long_slab, G, L):
    x, slab, s, n, runs = long_slab
    got = slab.events(s, s + n, 0.5, G, L)
    want = [ed.merge_and_filter(runs[c], G, L) for c in range(2)]
    assert got == want
    if (G, L) == (0, 0):
        assert len(want[0]) > 57*CHUNK//2 and want[0][-1] == (s + n - 2, s + n - 1)
        assert want == [ed.detect(x[c], s, s + n, 0.5, 0, 0, sparse=True) for c in range(2)]
    if (G, L) == (1, 0):
        assert want[0][-1] == (s + 200*CHUNK + 1, s + n - 1)           # the dense part is one event of 57 chunks


@pytest.fixture(scope='module')
def medium():
    rng = np.random.default_rng(4)
    x = family('normal', rng, 3, 3*CHUNK + 100)
    slab = Slab(x)
    want = [ed.detect(x[c], 2, 3*CHUNK + 90, THRESHOLDS[c], 1, 2) for c in range(3)]
    return x, slab, want


def test_capacity(medium):
    from audian_amd import hipdsp
    x, slab, want = medium
    start, stop, cap, sentinel = 2, 3*CHUNK + 90, 100, -77
    assert min(len(w) for w in want) > cap
    ev, counts = slab.raw(start, stop, THRESHOLDS, 1, 2, cap, pitch_extra=6)
    assert counts.tolist() == [sentinel] + [len(w) for w in want] + [sentinel]          # the true counts
    for c in range(3):
        assert ev[c, :2*cap].reshape(cap, 2).tolist() == [list(p) for p in want[c][:cap]]
        assert (ev[c, 2*cap:] == sentinel).all()                                        # nothing beyond is touched
    # a capacity of 0 with a NULL events pointer: counts only
    ev0, counts0 = slab.raw(start, stop, THRESHOLDS, 1, 2, 0)
    assert counts0.tolist() == counts.tolist() and (ev0 == sentinel).all()
    # an empty range: zero counts, nothing else
    ev1, counts1 = slab.raw(7, 7, THRESHOLDS, 1, 2, cap)
    assert counts1.tolist() == [sentinel, 0, 0, 0, sentinel] and (ev1 == sentinel).all()
    # the Python call: a fixed capacity truncates, None recovers everything after one repeat
    assert slab.events(start, stop, THRESHOLDS, 1, 2, capacity=cap) == [w[:cap] for w in want]
    dense = np.zeros((1, 3*4096 + 20), dtype=np.float32)
    dense[0, ::2] = 1.0
    before = hipdsp.launches.get('detect_events', 0)
    got = Slab(dense).events(0, dense.shape[1], 0.5, 0, 0)
    assert got == [[(i, i + 1) for i in range(0, dense.shape[1], 2)]] and len(got[0]) > 4096
    assert hipdsp.launches['detect_events'] == before + 2


def test_same_bytes_twice_and_channel_independence(medium):
    x, slab, want = medium
    start, stop = 2, 3*CHUNK + 90
    cap = max(len(w) for w in want) + 3
    first = slab.raw(start, stop, THRESHOLDS, 1, 2, cap)
    again = slab.raw(start, stop, THRESHOLDS, 1, 2, cap)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    full = slab.events(start, stop, THRESHOLDS, 1, 2)
    assert full == want
    for c in range(3):
        assert slab.events(start, stop, THRESHOLDS[c], 1, 2, channel=c) == [full[c]]


def test_errors(medium):
    from audian_amd import hipdsp
    x, slab, want = medium
    with pytest.raises(ValueError):
        slab.events(10, 9, 0.5, 0, 0)
    with pytest.raises(ValueError):
        slab.events(0, 10, 0.5, -1, 0)
    with pytest.raises(ValueError):
        slab.events(0, slab.pitch + 1, 0.5, 0, 0)                     # x_pitch < stop with three channels
    with pytest.raises(NotImplementedError, match='at most 65535 channels'):
        hipdsp.detect_events_into(slab.ctx, slab.view, slab.pitch, 65536, 0, 10, 0.5, 0, 0, 0, None,
                                  hipdsp.DeviceArray(slab.ctx, (4,), np.int64))
    assert slab.events(2, 3*CHUNK + 90, THRESHOLDS, 1, 2) == want     # the context still works


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


@pytest.fixture(scope='module')
def scrolled_graph():
    """filter + envelope on 3 channels x 60 s x 16 kHz with bursts of a 900 Hz tone; windows of 5 s in buffers of 30 s plus
    the 11 s of margin the filter and the envelope ask for (the raw buffer starts back_time + 2*11 s before a window, so
    it has to be that much longer than the window to hold it), after two scrolls (the second keeps an overlap)."""
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
            x[on, c] += 0.5*np.sin(2*np.pi*900.0*t[on])
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
    before = hipdsp.launches.get('detect_events', 0)
    thr = [0.1, 0.12, 0.08]
    ev = env.detect_events(thr, min_gap=0.01, min_duration=0.05, start=start, stop=stop)
    assert hipdsp.launches['detect_events'] == before + 1              # on the mirror, one call
    assert [list(r) for r in env._stale] == stale                      # nothing crossed but counts and pairs
    assert ev.rate == env.rate and ev.channels == 3
    host = np.asarray(env[start:stop])                                 # the host values last (this reads back)
    assert np.array_equal(host.astype(np.float32).astype(np.float64), host)
    for c in range(3):
        want = ed.detect(host[:, c], 0, stop - start, thr[c], int(0.01*env.rate), int(0.05*env.rate), sparse=True)
        assert ev.frames(c).tolist() == [[p + start, q + start] for p, q in want]
        assert len(want) >= 3
    # the numpy fallback on the same frames gives the same events
    fb = BufferedArray.detect_events(env, thr, 0.01, 0.05, start, stop)
    assert all(fb.frames(c).tolist() == ev.frames(c).tolist() for c in range(3))
    assert hipdsp.launches['detect_events'] == before + 1


def test_facade_detect_and_analyze_events_fill_the_table(scrolled_graph):
    """TraceGraph.detect_events + analyze_events on the device against the host fallback path: the same events
    exactly, one table row per event, mean and std within 1e-12 of numpy's (the figure tests/test_gpu_regionstats.py
    holds region_stats to on traces of this size)."""
    from audian_amd import hipdsp
    from audian_amd.analyzer import StatisticsAnalyzer
    from audian_amd.bufferedarray import BufferedArray
    g = scrolled_graph
    env = g['envelope']
    a = StatisticsAnalyzer(g, 'envelope')
    try:
        thr = g.event_thresholds('envelope', 0.5, 52.0, 58.0)
        before = dict(hipdsp.launches)
        ev = g.detect_events('envelope', thr, min_gap=0.01, min_duration=0.05, t0=52.0, t1=58.0)
        assert hipdsp.launches['detect_events'] == before.get('detect_events', 0) + 1
        g.analyze_events(ev)
        rows = a.rows()
        i0, i1 = g.region_frames(env, 52.0, 58.0)
        host = np.asarray(env[i0:i1])
        stats = BufferedArray.region_stats(env, [(i0, i1)])[0]
        assert np.allclose(thr, stats[:, 1] + 0.5*stats[:, 2], rtol=1e-12, atol=1e-12)
        fb = BufferedArray.detect_events(env, thr, 0.01, 0.05, i0, i1)
        k = 0
        for c in range(3):
            assert ev.frames(c).tolist() == fb.frames(c).tolist() and len(ev.onsets[c]) >= 3
            for p, q in ev.frames(c).tolist():
                v = host[p - i0:q - i0, c]
                assert abs(rows[k][0] - v.mean()) <= 1e-12 and abs(rows[k][1] - v.std()) <= 1e-12, (c, p, q)
                k += 1
        assert k == len(rows) == len(ev)
    finally:
        g.analyzers.remove(a)
