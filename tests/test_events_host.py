"""Host side of event detection (no GPU): the numpy fallback of BufferedData.detect_events against the sequential
definition (tests/events_definition.py), the seconds-to-frames conversion, the Events.regions() / region_frames round
trip, TraceGraph.detect_events -> analyze_events, the Analyzer's event store and the ctypes signature.  The traces here
compute on the host, so no device mirror exists and every detect_events call takes the numpy path.  All comparisons
are exact integer equality."""

import ctypes

import numpy as np
import pytest

import events_definition as ed
from audian_amd.analyzer import Analyzer, StatisticsAnalyzer
from audian_amd.buffereddata import BufferedData
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.events import Events, host_detect_events
from audian_amd.tracegraph import TraceGraph


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


class HostFilter(BufferedData):
    """A derived trace computed on the host: dest = source - 0.5."""

    def __init__(self, name='filtered'):
        super().__init__(name, 'data')

    def open(self, source):
        super().open(source, 1)

    def process(self, source, dest, nbefore):
        dest[:] = np.asarray(source[nbefore:nbefore + len(dest)]) - 0.5


class HostSpectrogram(BufferedSpectrogram):
    def process(self, source, dest, nbefore):
        dest[:] = 0


def random_row(rng, n, kind):
    if kind == 0:
        x = rng.standard_normal(n)
    elif kind == 1:
        x = np.round(2*rng.standard_normal(n))              # integers: ties at the thresholds 0 and 1
    else:
        x = np.where(rng.random(n) < 0.1, 3.0, -1.0)        # sparse spikes
    x = x.astype(np.float32)
    for value in (np.nan, np.inf, -np.inf):
        if n and rng.random() < 0.5:
            x[rng.integers(0, n, size=max(1, n//20))] = value
    return x


def test_fallback_is_the_definition():
    rng = np.random.default_rng(1)
    seen = 0
    for case in range(1500):
        n = int(rng.integers(0, 201))
        x = random_row(rng, n, case % 3)
        thr = float(rng.choice([-0.5, 0.0, 0.5, 1.0]))
        G, L = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        first = int(rng.integers(0, 50))
        got = host_detect_events(x, thr, G, L, first=first)
        assert got.dtype == np.int64 and got.shape[1:] == (2,)
        want = [(a + first, b + first) for a, b in ed.detect(x, 0, n, thr, G, L)]
        assert [tuple(p) for p in got.tolist()] == want, (case, n, thr, G, L)
        assert want == [(a + first, b + first) for a, b in ed.detect(x, 0, n, thr, G, L, sparse=True)]
        seen += len(want)
    assert seen > 3000
    # the rules one by one
    x = np.array([0, 2, 2, 0, 0, 2, 0, 0, 0, 2, np.nan, 2, 1, np.inf], dtype=np.float32)
    assert ed.detect(x, 0, len(x), 1.0, 0, 0) == [(1, 3), (5, 6), (9, 10), (11, 12), (13, 14)]     # equal to thr, NaN: not above
    assert ed.detect(x, 0, len(x), 1.0, 1, 0) == [(1, 3), (5, 6), (9, 14)]
    assert ed.detect(x, 0, len(x), 1.0, 2, 2) == [(1, 6), (9, 14)]
    assert ed.detect(x, 1, 12, 1.0, 0, 0) == [(1, 3), (5, 6), (9, 10), (11, 12)]                   # cut off at both ends
    for G, L in [(0, 0), (1, 0), (2, 2), (3, 6)]:
        assert [tuple(p) for p in host_detect_events(x, 1.0, G, L).tolist()] == ed.detect(x, 0, len(x), 1.0, G, L)


def open_graph(x, rate, traces=(), **kwargs):
    g = TraceGraph(buffer_time=40.0, back_time=5.0)
    for t in traces:
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate, **kwargs)
    for t in traces:
        t.plot_items = [Item()]*x.shape[1]
    g.set_need_update()
    g.update_times(0.0, 10.0)
    return g


def test_seconds_become_frames_as_in_the_reference():
    """min_gap and min_duration are int(seconds*rate) frames (songdetector.py:137-139), thresholds one per channel."""
    rate = 96000/7
    rng = np.random.default_rng(2)
    x = np.where(rng.random((4000, 2)) < 0.02, 1.0, 0.0) + np.array([0.0, 5.0])
    g = open_graph(x, rate)
    for gap, dur in [(0.0, 0.0), (0.001, 0.0), (0.0049, 0.0003), (0.01, 0.002)]:
        ev = g.data.detect_events([0.5, 5.5], gap, dur)
        assert isinstance(ev, Events) and ev.rate == rate and ev.channels == 2
        for c, thr in enumerate([0.5, 5.5]):
            want = ed.detect(x[:, c], 0, 4000, thr, int(gap*rate), int(dur*rate))
            assert ev.frames(c).tolist() == [list(p) for p in want]
    assert int(0.0049*rate) == 67 and int(0.0003*rate) == 4
    # a scalar threshold serves every channel; a frame range is absolute
    ev = g.data.detect_events(0.5, start=100, stop=900)
    assert ev.frames(0).tolist() == [list(p) for p in ed.detect(x[:, 0], 100, 900, 0.5, 0, 0)]
    assert ev.frames(1).tolist() == [[100, 900]]
    assert len(g.data.detect_events(0.5, start=7, stop=7)) == 0
    with pytest.raises(IndexError):
        g.data.detect_events(0.5, start=0, stop=4001)
    with pytest.raises(ValueError):
        g.data.detect_events([0.5, 0.5, 0.5])


@pytest.mark.parametrize('rate', [100.0, 44100.0, 96000/7])
def test_regions_round_trip_through_region_frames(rate):
    class Trace:
        def __len__(self):
            return 10**8 + 10

    trace = Trace()
    trace.rate = rate
    rng = np.random.default_rng(3)
    onsets = np.concatenate(([0, 1, 2, 10**8 - 1, 10**8], rng.integers(0, 10**8, size=20000)))
    offsets = onsets + np.concatenate(([1, 1, 5, 1, 3], rng.integers(1, 10**6, size=20000)))
    offsets = np.minimum(offsets, 10**8 + 10)
    ev = Events([np.stack((onsets, offsets), axis=1)], rate)
    back = [TraceGraph.region_frames(trace, t0, t1) for t0, t1 in ev.regions(0)]
    assert back == list(zip(onsets.tolist(), offsets.tolist()))


def test_detect_and_analyze_events_fill_one_row_per_event():
    rate = 100.0
    rng = np.random.default_rng(5)
    x = 0.1*rng.standard_normal((3000, 3))
    for c, spans in enumerate([[(100, 180), (200, 260), (1500, 1510)], [(5, 50)], []]):
        for a, b in spans:
            x[a:b, c] += 2.0
    f = HostFilter()
    g = open_graph(x, rate, [f])
    assert f._dev is None                                   # host-only graph: the numpy path
    a = StatisticsAnalyzer(g)
    thr = g.event_thresholds('filtered', 1.0, 0.0, 25.0)
    want_thr = (x[:2501] - 0.5).mean(axis=0) + (x[:2501] - 0.5).std(axis=0)
    assert np.allclose(thr, want_thr, rtol=1e-12, atol=0)
    ev = g.detect_events('filtered', 0.5, min_gap=0.25, min_duration=0.2, t0=0.0, t1=25.0)
    want = [ed.detect(x[:, c] - 0.5, 0, 2501, 0.5, 25, 20) for c in range(3)]
    assert [ev.frames(c).tolist() for c in range(3)] == [[list(p) for p in w] for w in want]
    assert want[0] == [(100, 260)] and want[1] == [(5, 50)] and want[2] == []
    g.analyze_events(ev)
    rows = a.rows()
    assert len(rows) == 2
    assert rows[0] == [np.mean(x[100:260, 0] - 0.5), np.std(x[100:260, 0] - 0.5)]
    assert rows[1] == [np.mean(x[5:50, 1] - 0.5), np.std(x[5:50, 1] - 0.5)]
    a.clear()
    g.analyze_events(ev, channels=[1])
    assert len(a.rows()) == 1
    # without times: the buffer as it is
    assert g.detect_events('data', 1.0).frames(1).tolist() == [[5, 50]]


def test_spectrogram_shaped_traces_are_refused():
    s = HostSpectrogram(nfft=16, source='data')
    g = open_graph(np.zeros((500, 2)), 100.0, [s])
    with pytest.raises(TypeError):
        s.detect_events(0.0)


def test_analyzer_event_store_and_clear():
    g = open_graph(np.zeros((100, 3)), 100.0)
    a = Analyzer(g, 'songs', 'data')
    assert a.events == {}
    a.make_trace_events('onset', 'data', 'o', '#ff0000', 8)
    a.make_panel_events('peak', 'xt', 't', '#00ff00', 6)
    assert sorted(a.events) == ['onset', 'peak'] and len(a.events['onset']) == 3
    assert a.event_styles['onset']['trace'] == 'data' and a.event_styles['peak']['panel'] == 'xt'
    a.set_events('onset', 1, [0.1, 0.2], [1.0, 2.0])
    assert [len(x) for x, y in a.events['onset']] == [0, 2, 0]
    a.add_events('onset', 1, [0.3], [3.0])
    a.add_events('onset', 2, [0.4], [4.0])
    assert a.events['onset'][1][0].tolist() == [0.1, 0.2, 0.3] and a.events['onset'][1][1].tolist() == [1.0, 2.0, 3.0]
    assert a.events['onset'][2][0].tolist() == [0.4]
    a.set_events('onset', 0, [0.5], [5.0])                   # erases the other channels
    assert [len(x) for x, y in a.events['onset']] == [1, 0, 0]
    a.set_events('peak', -1, [0.7], [7.0])
    assert [x.tolist() for x, y in a.events['peak']] == [[0.7]]*3
    a.make_column('n')
    a.store(1)
    a.clear()
    assert a.rows() == [] and all(len(x) == 0 and len(y) == 0 for name in a.events for x, y in a.events[name])
    assert sorted(a.events) == ['onset', 'peak']


def test_ctypes_signature():
    from audian_amd import _lib
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    args, res = _lib._SIGNATURES['hipdsp_detect_events']
    assert args == [vp, vp, i64, i64, i64, i64, vp, ctypes.c_double, i64, i64, i64, vp, i64, vp] and res is ctypes.c_int
    assert _lib.lib.hipdsp_detect_events.argtypes == args
