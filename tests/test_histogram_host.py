"""Host side of the amplitude histogram, the masked moments and the histogram threshold (no GPU): the numpy fallbacks
of BufferedArray against np.histogram and tests/threshold_definition.py, threshold_estimates against the thresholds the
reference's function gave (tests/golden/threshold_estimates.npz, written by tests/golden/make_threshold_golden.py),
TraceGraph.event_thresholds(method='histogram'), the unchanged 'std' path and the ctypes signatures.  The traces here
live on the host, so no device mirror exists and every call takes the numpy path."""

import ctypes

import numpy as np
import pytest

import threshold_definition as td
from conftest import load_golden
from audian_amd.bufferedarray import ArrayLoader
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.tracegraph import TraceGraph


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


class HostSpectrogram(BufferedSpectrogram):
    def process(self, source, dest, nbefore):
        dest[:] = 0


def open_graph(x, rate, traces=()):
    g = TraceGraph(buffer_time=40.0, back_time=5.0)
    for t in traces:
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for t in traces:
        t.plot_items = [Item()]*x.shape[1]
    g.set_need_update()
    g.update_times(0.0, 10.0)
    return g


def samples(rng, n, channels):
    x = np.round(rng.uniform(-1.5, 2.5, size=(n, channels))*64)/64          # many land exactly on edges k/64
    x = x.astype(np.float32)
    for value in (np.nan, np.inf, -np.inf):
        x[rng.random((n, channels)) < 0.02] = value
    return x


EDGES = {
    'one_bin': [0.0, 1.0],
    'uniform': np.linspace(0.0, 2.0, 50),
    'sixtyfourths': np.arange(-32, 97)/64.0,
    'duplicates': [-1.0, 0.0, 0.0, 0.5, 0.5, 0.5, 1.0, 1.0],
    'all_equal': [0.25, 0.25, 0.25],
    'uneven': [-1.0, -0.99, 0.0, 1e-3, 0.7, 2.0],
}


@pytest.mark.parametrize('name', sorted(EDGES))
def test_histogram_is_numpys_plus_the_outside_counts(name):
    rng = np.random.default_rng(sorted(EDGES).index(name))
    x = samples(rng, 3000, 3)
    x[5, 0], x[6, 1] = 0.25, 2.0                                            # the only edge of 'all_equal'; the last edge
    a = ArrayLoader(x, 100.0)
    e = np.asarray(EDGES[name], dtype=np.float64)
    for start, stop in [(None, None), (0, 3000), (7, 2001), (40, 40), (2999, 3000)]:
        got = a.histogram(e, start, stop)
        lo, hi = (0 if start is None else start), (3000 if stop is None else stop)
        assert got.dtype == np.int64 and got.shape == (3, len(e) + 2)
        for c in range(3):
            assert got[c].tolist() == td.numpy_slots(x[lo:hi, c], e).tolist(), (name, start, stop, c)
            assert got[c].tolist() == td.histogram_slots(x[lo:hi, c], e).tolist()
            assert a.histogram(e, start, stop, channel=c).tolist() == got[c].tolist()
        assert (got.sum(axis=1) == hi - lo).all()
    assert a.histogram(e)[:, -3:].min() > 0                                 # below, above and NaN all occur


def test_histogram_closes_the_last_bin_and_checks_its_edges():
    x = np.array([[0.0], [0.5], [1.0], [1.0], [0.99]], dtype=np.float32)
    a = ArrayLoader(x, 10.0)
    assert a.histogram([0.0, 0.5, 1.0]).tolist() == [[1, 4, 0, 0, 0]]
    assert a.histogram([0.0, 0.5, 1.0, 1.0]).tolist() == [[1, 2, 2, 0, 0, 0]]         # a zero-width LAST bin takes x == e[B]
    assert a.histogram([0.0, 0.5, 0.5, 1.0]).tolist() == [[1, 0, 4, 0, 0, 0]]         # any other one is empty
    for bad in ([0.0], [1.0, 0.0], [0.0, np.nan], [0.0, np.inf], []):
        with pytest.raises(ValueError):
            a.histogram(bad)
    with pytest.raises(NotImplementedError):
        a.histogram(np.arange(1026.0))
    assert a.histogram(np.arange(1025.0)).shape == (1, 1027)
    with pytest.raises(IndexError):
        a.histogram([0.0, 1.0], 0, 6)


def test_masked_stats_is_the_definition():
    rng = np.random.default_rng(11)
    x = samples(rng, 2500, 3)
    a = ArrayLoader(x, 100.0)
    windows = [(-np.inf, 0.5), (0.25, np.inf), (-0.5, 1.0), (-np.inf, np.inf), (5.0, 6.0), (1.0, 1.0), (np.nan, 1.0),
               (0.0, np.nan), ([-np.inf, 0.0, 0.5], [0.0, 0.5, np.inf])]
    for lo, hi in windows:
        for start, stop in [(None, None), (3, 2000), (9, 9)]:
            got = a.masked_stats(lo, hi, start=start, stop=stop)
            assert got.shape == (3, 4)
            first, last = (0 if start is None else start), (2500 if stop is None else stop)
            for c in range(3):
                want = td.masked_slots(x[first:last, c], np.broadcast_to(lo, 3)[c], np.broadcast_to(hi, 3)[c])
                assert got[c, 0] == want[0] and got[c, 3] == 0
                assert np.allclose(got[c, 1:3], want[1:3], rtol=1e-13, atol=0, equal_nan=True), (lo, hi, start, c)
    assert a.masked_stats(5.0, 6.0)[:, 0].tolist() == [0, 0, 0] and np.isnan(a.masked_stats(5.0, 6.0)[:, 1:3]).all()
    # strict on both sides
    b = ArrayLoader(np.array([[0.0], [0.5], [1.0]], dtype=np.float32), 10.0)
    assert b.masked_stats(0.0, 1.0).tolist() == [[1.0, 0.5, 0.0, 0.0]]
    # the default pivot: the finite bound, lo when both are, 0 when neither is; it must be finite
    assert a._masked_bounds(-np.inf, 2.0, None)[:, 2].tolist() == [2.0]*3
    assert a._masked_bounds(1.0, np.inf, None)[:, 2].tolist() == [1.0]*3
    assert a._masked_bounds(1.0, 2.0, None)[:, 2].tolist() == [1.0]*3
    assert a._masked_bounds(-np.inf, np.inf, None)[:, 2].tolist() == [0.0]*3
    assert a._masked_bounds(0.0, 1.0, [1.0, 2.0, 3.0])[:, 2].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        a.masked_stats(0.0, 1.0, pivot=np.inf)
    with pytest.raises(ValueError):
        a.masked_stats([0.0, 1.0], 2.0)


@pytest.fixture(scope='module')
def golden():
    g = load_golden('threshold_estimates')
    assert g['x'].dtype == np.float32 and g['x'].shape == (5000, 4)
    tiled = td.tiled(g['x'], int(g['tiled_times']), int(g['tiled_frames']))
    assert tiled.shape[0] >= 40000
    return g, tiled


def test_threshold_estimates_match_the_reference(golden):
    g, tiled = golden
    for x, name in ((g['x'], ''), (tiled, 'tiled_')):
        want = g[name + 'thresholds']
        assert g[name + 'gap'] >= 1e-7 and g[name + 'branch_margin'] >= 1e-2
        assert g[name + 'upper_branch'].any() and not g[name + 'upper_branch'].all()
        a = ArrayLoader(x, 1000.0, buffer_time=100.0)
        got = a.threshold_estimates()
        assert got.dtype == np.float64 and got.shape == (4,)
        assert np.allclose(got, want, rtol=1e-12, atol=0), (name, got, want)
        assert np.allclose(td.threshold_estimates(x)[0], want, rtol=1e-12, atol=0)
        assert np.array_equal(a.event_thresholds(10.0, method='histogram'), got)
        assert np.array_equal(a.event_thresholds(0.0, None, None, 'histogram'), got)      # the factor is ignored
    # a sub-range: the definition on that range
    a = ArrayLoader(g['x'], 1000.0, buffer_time=100.0)
    assert np.allclose(a.threshold_estimates(100, 4100), td.threshold_estimates(g['x'][100:4100])[0], rtol=1e-12, atol=0)


def test_tracegraph_passes_the_method_through(golden):
    g, tiled = golden
    x = g['x'].astype(np.float64)
    graph = open_graph(x, 1000.0)
    want = td.threshold_estimates(x[:3001])[0]
    got = graph.event_thresholds('data', 1.0, 0.0, 3.0, method='histogram')
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert np.allclose(graph.event_thresholds('data', 1.0, method='histogram'), g['thresholds'], rtol=1e-12, atol=0)
    # 'std' and the positional call are what they were
    std = x[:3001].mean(axis=0) + 2.5*x[:3001].std(axis=0)
    assert np.allclose(graph.event_thresholds('data', 2.5, 0.0, 3.0), std, rtol=1e-12, atol=0)
    assert np.array_equal(graph.event_thresholds('data', 2.5, 0.0, 3.0, method='std'),
                          graph.event_thresholds('data', 2.5, 0.0, 3.0))
    assert np.array_equal(graph.data.event_thresholds(2.5, 0, 3001), graph.data.event_thresholds(2.5, 0, 3001, 'std'))
    stats = graph.data.region_stats([(0, 3001)])[0]
    assert np.array_equal(graph.data.event_thresholds(2.5, 0, 3001), stats[:, 1] + 2.5*stats[:, 2])
    with pytest.raises(ValueError):
        graph.event_thresholds('data', 1.0, method='median')


def test_ranges_without_a_positive_finite_maximum_are_value_errors():
    x = np.abs(np.random.default_rng(3).normal(0.0, 0.1, size=(400, 2))).astype(np.float32)
    x[100:200] = 0.0
    a = ArrayLoader(x, 100.0)
    assert np.isfinite(a.threshold_estimates()).all()
    with pytest.raises(ValueError, match='maximum'):
        a.threshold_estimates(100, 200)                                     # all zero
    with pytest.raises(ValueError, match='maximum'):
        a.threshold_estimates(150, 150)                                     # empty
    with pytest.raises(ValueError, match='maximum'):
        ArrayLoader(-x - 1.0, 100.0).threshold_estimates()                  # negative
    for value in (np.nan, np.inf):
        y = x.copy()
        y[300, 1] = value
        with pytest.raises(ValueError, match='maximum'):
            ArrayLoader(y, 100.0).event_thresholds(1.0, method='histogram')
        assert np.isfinite(ArrayLoader(y, 100.0).threshold_estimates(0, 300)).all()
    y = x.copy()
    y[:, 1] = -1.0
    with pytest.raises(ValueError, match='no sample'):
        ArrayLoader(y, 100.0).threshold_estimates()


def test_spectrogram_shaped_traces_are_refused():
    s = HostSpectrogram(nfft=16, source='data')
    open_graph(np.zeros((500, 2)), 100.0, [s])
    with pytest.raises(TypeError):
        s.histogram([0.0, 1.0])
    with pytest.raises(TypeError):
        s.masked_stats(0.0, 1.0)
    with pytest.raises(TypeError):
        s.threshold_estimates()
    with pytest.raises(TypeError):
        s.event_thresholds(1.0, method='histogram')


def test_ctypes_signatures():
    from audian_amd import _lib
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    args, res = _lib._SIGNATURES['hipdsp_histogram']
    assert args == [vp, vp, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_double), ctypes.c_int, vp, i64]
    assert res is ctypes.c_int and _lib.lib.hipdsp_histogram.argtypes == args
    args, res = _lib._SIGNATURES['hipdsp_masked_stats']
    assert args == [vp, vp, i64, i64, i64, i64, vp, vp] and res is ctypes.c_int
    assert _lib.lib.hipdsp_masked_stats.argtypes == args
