"""Host side of region analysis (no GPU): the numpy fallback of BufferedData.region_stats, TraceGraph.get_region's
index arithmetic (src/audian/data.py:102-118 of the reference), the lazy Region and the Analyzer surface
(src/audian/analyzer.py, src/audian/statisticsanalyzer.py).  The traces here compute on the host, so no device mirror
exists and every region_stats call takes the numpy path."""

import warnings

import numpy as np
import pytest

from audian_amd.analyzer import Analyzer, PlainAnalyzer, Region, StatisticsAnalyzer
from audian_amd.buffereddata import BufferedData
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.tracegraph import TraceGraph

RATE = 100.0
FRAMES = 3000


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
    """A spectrogram-shaped trace computed on the host: dest[k, c, f] = source[k*hop, c] + f."""

    def process(self, source, dest, nbefore):
        src = np.asarray(source[nbefore::self.hop])[:len(dest)]
        dest[:len(src)] = src[:, :, None] + np.arange(dest.shape[2])[None, None, :]
        dest[len(src):] = 0


def signal():
    rng = np.random.default_rng(5)
    return rng.standard_normal((FRAMES, 3))*0.2 + np.array([0.0, 0.5, -3.0])


@pytest.fixture()
def graph():
    g = TraceGraph(buffer_time=20.0, back_time=5.0)
    f, s = HostFilter(), HostSpectrogram(nfft=16, source='filtered')
    g.add_trace(f)
    g.add_trace(s)
    g.setup_traces()
    g.open(signal(), RATE, ampl_max=1.0)
    for t in (f, s):
        t.plot_items = [Item()]*3
    g.set_need_update()
    g.update_times(0.0, 10.0)
    return g


def numpy_slots(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return [0, np.nan, np.nan, np.nan, np.nan, -1, -1, 0]
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return [v.size, np.mean(v), np.std(v), np.min(v), np.max(v), np.argmin(v), np.argmax(v), 0]


def test_fallback_slots_shapes_and_empty(graph):
    f = graph['filtered']
    assert f._dev is None                                   # host-only graph: the numpy path
    want = signal() - 0.5
    regions = [(10, 500), (0, 1), (700, 700), (f.offset, f.offset + len(f.buffer))]
    got = f.region_stats(regions)
    assert got.shape == (4, 3, 8) and got.dtype == np.float64
    for k, (a, b) in enumerate(regions):
        for c in range(3):
            assert np.array_equal(got[k, c], numpy_slots(want[a:b, c]), equal_nan=True)
    assert np.isnan(got[2, :, 1:5]).all() and (got[2, :, 5:7] == -1).all() and (got[2, :, 0] == 0).all()
    one = f.region_stats(regions, channel=1)
    assert one.shape == (4, 8) and np.array_equal(one, got[:, 1], equal_nan=True)
    assert f.region_stats([]).shape == (0, 3, 8)
    # more than 16 regions: chunked, same values
    many = [(k, k + 40) for k in range(0, 400, 20)]
    assert np.array_equal(f.region_stats(many, 2), np.array([numpy_slots(want[a:b, 2]) for a, b in many]))
    with pytest.raises(IndexError):
        f.region_stats([(0, len(f.buffer) + f.offset + 1)])
    with pytest.raises(IndexError):
        f.region_stats([(5, 4)])
    # the raw recording has the same method
    assert np.array_equal(graph.data.region_stats([(3, 90)], 0)[0], numpy_slots(signal()[3:90, 0]))


def test_fallback_spectrogram_flat_positions(graph):
    s = graph['spectrogram']
    F = s.shape[2]
    got = s.region_stats([(3, 40)], channel=2)
    block = np.asarray(s.buffer[3:40, 2])
    assert block.shape == (37, F)
    assert np.array_equal(got[0], numpy_slots(block))
    assert got[0, 0] == 37*F


@pytest.mark.parametrize('values', [
    [1.0, np.nan, 3.0], [np.nan, 1.0], [2.0, 1.0, np.nan], [1.0, np.inf, 2.0], [-np.inf, 1.0, 2.0],
    [np.inf, 0.0, -np.inf], [np.inf, np.nan, -np.inf], [np.inf, np.inf], [np.nan, np.nan]])
def test_fallback_special_values_follow_numpy(values):
    """The NaN and inf rules of hipdsp_region_stats are numpy's own: checked on the numpy path against the
    literal statement of the rules."""
    g = TraceGraph(10.0, 0.0)
    g.setup_traces()
    x = np.zeros((50, 2))
    x[:, 1] = np.linspace(-1, 1, 50)
    x[7:7 + len(values), 0] = values
    g.open(x, RATE)
    got = g.data.region_stats([(7, 7 + len(values))])[0]
    v = np.array(values)
    assert np.array_equal(got[0], numpy_slots(v), equal_nan=True)
    if np.isnan(v).any():
        first = int(np.flatnonzero(np.isnan(v))[0])
        assert np.isnan(got[0, 1:5]).all() and got[0, 5] == first and got[0, 6] == first
    else:
        assert np.isnan(got[0, 2])
        pos, neg = (v == np.inf).any(), (v == -np.inf).any()
        assert np.isnan(got[0, 1]) if pos and neg else got[0, 1] == (np.inf if pos else -np.inf)
        assert got[0, 3] == v.min() and got[0, 4] == v.max()
    assert np.array_equal(got[1], numpy_slots(x[7:7 + len(values), 1]))          # the other channel


def reference_indices(t, t0, t1):
    """data.py:105-110, verbatim in meaning."""
    i0 = int(t0*t.rate)
    if i0 < 0:
        i0 = 0
    i1 = int(t1*t.rate) + 1
    if i1 > len(t):
        i1 = len(t)
    return i0, i1


@pytest.mark.parametrize('t0, t1', [(1.0, 2.5), (-3.0, 0.7), (28.5, 99.0), (0.013, 0.019)])
def test_get_region_indices_keys_and_tuples(graph, t0, t1):
    traces = graph.get_region(t0, t1, 1)
    assert list(traces) == ['data', 'filtered', 'spectrogram']
    for t in graph.traces:
        i0, i1 = reference_indices(t, t0, t1)
        entry = traces[t.name]
        assert len(entry) == (3 if isinstance(t, BufferedSpectrogram) else 2)
        time, data = entry[0], entry[-1]
        assert np.array_equal(time, np.arange(i0, i1)/t.rate)
        assert isinstance(data, Region) and len(data) == i1 - i0 and data.dtype == np.float64
        assert data.shape == (i1 - i0,) + tuple(t.shape[2:]) and data.ndim == len(data.shape)
        assert np.array_equal(np.asarray(data), t[i0:i1, 1])
    assert traces['spectrogram'][1] is graph['spectrogram'].frequencies


def test_region_reductions_do_not_materialise(graph):
    want = (signal() - 0.5)[120:381, 2]
    before = Region.materialised
    r = graph.get_region(1.2, 3.8, 2)['filtered'][1]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = [np.mean(r), np.std(r), np.min(r), np.max(r), np.argmin(r), np.argmax(r)]
    assert got == [np.mean(want), np.std(want), np.min(want), np.max(want), np.argmin(want), np.argmax(want)]
    assert isinstance(got[0], np.float64) and isinstance(got[4], np.integer)
    assert Region.materialised == before and r._data is None
    # the six share one region_stats call
    calls = []
    f = graph['filtered']
    f.region_stats = lambda *a, **k: calls.append(a) or BufferedData.region_stats(f, *a, **k)
    r = graph.get_region(1.2, 3.8, 2)['filtered'][1]
    assert (np.mean(r), np.std(r), np.max(r)) == (np.mean(want), np.std(want), np.max(want))
    assert len(calls) == 1 and Region.materialised == before
    # anything else becomes the array, once
    assert np.sum(r) == np.sum(want) and Region.materialised == before + 1
    assert np.array_equal(r[3:5], want[3:5]) and np.array_equal(r[3:5], f[123:125, 2])
    assert r.std(ddof=1) == np.std(want, ddof=1) and np.mean(r, dtype=np.float32) == np.mean(want, dtype=np.float32)
    assert Region.materialised == before + 1
    # a spectrogram region: numpy's flat argmax
    s = graph.get_region(1.2, 3.8, 0)['spectrogram'][2]
    i0, i1 = reference_indices(graph['spectrogram'], 1.2, 3.8)
    block = graph['spectrogram'][i0:i1, 0]
    assert np.argmax(s) == np.argmax(block) and np.mean(s) == np.mean(block) and Region.materialised == before + 1
    # an empty region is numpy's business
    e = Region(f, 50, 50, 0)
    with pytest.raises(ValueError):
        np.argmin(e)


@pytest.mark.parametrize('ampl_max, fmt', [(1.0, '%.5f'), (32768.0, '%.1f')])
def test_statistics_analyzer_columns(ampl_max, fmt):
    g = TraceGraph(20.0, 5.0)
    g.add_trace(HostFilter())
    g.setup_traces()
    g.open(signal(), RATE, ampl_max=ampl_max, unit='mV')
    a = StatisticsAnalyzer(g)
    assert g.analyzers == [a] and a.name == 'statistics' and a.source is g['filtered']
    assert a.data.labels == ['filtered mean', 'filtered stdev']
    assert a.data.units == ['mV', 'mV'] and a.data.formats == [fmt, fmt]
    assert a.traces() == ['data', 'filtered'] and a.trace('nothing') is None
    p = PlainAnalyzer(g)
    assert p.data.labels == ['tstart', 'tend', 'duration', 'channel'] and p.data.formats[0] == '%.2f'


def test_analyze_region_and_regions(graph, tmp_path):
    a, p = StatisticsAnalyzer(graph), PlainAnalyzer(graph)
    want = signal() - 0.5
    before = Region.materialised
    graph.analyze_region(-1.0, 2.0, 1)                       # t0 is clipped to 0 (databrowser.py:1761-1764)
    assert a.rows() == [[np.mean(want[0:201, 1]), np.std(want[0:201, 1])]]
    assert p.rows() == [[0, 2.0, 2.0, 1]]
    assert Region.materialised == before
    a.clear()
    p.clear()
    assert a.rows() == [] and a.data.rows() == 0 and a.data.columns() == 2
    regions = [(0.5*k, 0.5*k + 1.0) for k in range(20)]
    graph.analyze_regions(regions)
    rows = a.rows()
    assert len(rows) == 20*3 and len(p.rows()) == 20*3
    k = 0
    for t0, t1 in regions:                                   # region-major
        i0, i1 = reference_indices(graph['filtered'], t0, t1)
        for c in range(3):
            assert rows[k] == [np.mean(want[i0:i1, c]), np.std(want[i0:i1, c])]
            assert p.rows()[k] == [t0, t1, t1 - t0, c]
            k += 1
    a.clear()
    graph.analyze_regions(regions[:2], channels=[2, 0])
    assert len(a.rows()) == 4 and a.rows()[1][0] == np.mean(want[0:101, 0])
    path = tmp_path/'table.csv'
    a.save_csv(path)
    lines = path.read_text().splitlines()
    assert lines[0] == 'filtered mean/a.u.,filtered stdev/a.u.' and len(lines) == 5
    assert lines[2] == '%.5f,%.5f' % tuple(a.rows()[1])


def test_custom_analyzer_goes_region_by_region(graph):
    class Peak(Analyzer):
        def __init__(self, g):
            super().__init__(g, 'peak', 'filtered')
            self.make_column('peak time', 's', '%.3f')

        def analyze(self, t0, t1, channel, traces):
            time, data = traces[self.source_name]
            self.store(time[np.argmax(data)])

    a = Peak(graph)
    want = signal() - 0.5
    graph.analyze_regions([(1.0, 2.0), (4.0, 4.5)], channels=[1])
    assert a.rows() == [[(100 + np.argmax(want[100:201, 1]))/RATE], [(400 + np.argmax(want[400:451, 1]))/RATE]]
