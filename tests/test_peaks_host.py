"""Host side of peak detection (no GPU).  tests/peaks_definition.py -- the definition of hipdsp_find_peaks as plain
loops -- must reproduce tests/golden/find_peaks.npz, which scipy.signal.find_peaks (1.15.3) wrote, and live scipy
where it is installed; audian_amd.peaks.host_find_peaks, the vectorised fallback, must equal the definition; then the
argument handling of BufferedArray.find_peaks, the Peaks object, TraceGraph.find_peaks / mark_peaks on host-computed
traces (no device mirror exists: every call takes the numpy path) and the ctypes signature.  Every comparison is exact:
integer positions, and float64 values with NaN equal to NaN."""

import ctypes
import math
import os
import time

import numpy as np
import pytest

import peaks_definition as pd
from audian_amd.analyzer import Analyzer
from audian_amd.buffereddata import BufferedData
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.events import Events
from audian_amd.peaks import Peaks, host_find_peaks
from audian_amd.tracegraph import TraceGraph

INF = math.inf
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'find_peaks.npz')
CONDITIONS = [(pd.OPEN, pd.OPEN, pd.OPEN), ((0.0, INF), pd.OPEN, (1.0, INF)), ((-INF, 2.0), (1.0, INF), pd.OPEN),
              (pd.OPEN, (-INF, 3.0), (1.0, 4.0)), ((0.0, 2.0), (1.0, 3.0), (-INF, 4.0)), (pd.OPEN, pd.OPEN, (math.nan, INF))]
WLENS = [0, 2, 3, 4, 7, 100]


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
    x = rng.integers(-3, 4, size=n).astype(np.float32)          # small integers: ties and flat peaks
    if kind % 3 == 1 and n:
        x = np.repeat(x, rng.integers(1, 5, size=n))[:n]
    if kind % 3 == 2:
        x = rng.standard_normal(n).astype(np.float32)
    if kind % 2 == 1:
        for value in (np.nan, np.inf, -np.inf):
            x[rng.random(n) < 0.03] = value
    return x


def golden_cases():
    g = np.load(GOLDEN)
    for i, case in enumerate(g['cases']):
        k = int(case[0])
        row = g['rows'][g['row_offsets'][k]:g['row_offsets'][k + 1]]
        a, b = g['peak_offsets'][i], g['peak_offsets'][i + 1]
        yield i, row, (case[1], case[2]), (case[3], case[4]), (case[5], case[6]), int(case[7]), g['peaks'][a:b], \
            g['props'][a:b]


def test_definition_reproduces_the_golden_file():
    """Positions, heights, prominences (NaN equal to NaN) and bases of scipy 1.15.3, every case of the file."""
    n = kept = nan = 0
    combos = set()
    for i, row, height, threshold, prominence, wlen, peaks, props in golden_cases():
        want = pd.find_peaks(row, height, threshold, prominence, wlen)
        assert pd.same(peaks, props, want), (i, height, threshold, prominence, wlen)
        n += 1
        kept += len(peaks)
        nan += int(np.isnan(props[:, 1]).sum())
        combos.add(tuple(np.isinf([*height, *threshold, *prominence]).tolist()))
    assert n >= 500 and kept > 4000 and nan > 0 and len(combos) == 64       # every combination of open and closed
    assert os.path.getsize(GOLDEN) < 200000


def test_definition_is_live_scipy():
    signal = pytest.importorskip('scipy.signal')
    import warnings
    rng = np.random.default_rng(17)
    seen = 0
    for case in range(600):
        x = random_row(rng, int(rng.integers(0, 150)), case)
        height, threshold, prominence = CONDITIONS[case % 5]
        wlen = WLENS[case % 6]
        none = [None if math.isinf(b) else b for b in (*height, *threshold, *prominence)]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            p, pr = signal.find_peaks(x.astype(np.float64), height=tuple(none[0:2]), threshold=tuple(none[2:4]),
                                      prominence=tuple(none[4:6]), wlen=wlen if wlen else None)
        props = np.stack((pr['peak_heights'], pr['prominences'], pr['left_bases'], pr['right_bases']), axis=1)
        assert pd.same(p, props, pd.find_peaks(x, height, threshold, prominence, wlen)), case
        seen += len(p)
    assert seen > 2000


def test_fallback_is_the_definition():
    rng = np.random.default_rng(1)
    seen = 0
    for case in range(1500):
        n = int(rng.integers(0, 201))
        x = random_row(rng, n, case)
        height, threshold, prominence = CONDITIONS[case % len(CONDITIONS)]
        wlen = WLENS[(case//7) % 6]
        first = int(rng.integers(0, 50))
        pos, props = host_find_peaks(x, height, threshold, prominence, wlen, first=first)
        assert pos.dtype == np.int64 and props.dtype == np.float64 and props.shape == (len(pos), 4)
        assert pd.same(pos, props, pd.find_peaks(x, height, threshold, prominence, wlen, first=first)), (case, n)
        seen += len(pos)
    assert seen > 5000
    # the golden rows too, and None for an open condition or an open side
    for i, row, height, threshold, prominence, wlen, peaks, props in golden_cases():
        assert pd.same(*host_find_peaks(row, height, threshold, prominence, wlen), (peaks.tolist(), props)), i
    x = random_row(rng, 300, 0)
    assert pd.same(*host_find_peaks(x, None, (1.0, None), None, None), pd.find_peaks(x, threshold=(1.0, INF)))
    # the rules one by one
    x = np.array([0, 1, 0, 2, 2, 0, 3, 3, 3, 1, np.nan, 5, 4, -1, 0, -0.0, -1, 2, 2], dtype=np.float32)
    assert pd.find_peaks(x)[0] == [1, 3, 7, 14]             # flat peaks at (l + r)//2; next to NaN, at the end: none
    assert pd.find_peaks(x)[1][2] == [3.0, 2.0, 5, 9]       # of equal minima the nearest; the walk stops at the NaN
    assert pd.find_peaks(x, wlen=2)[1][1] == [2.0, 0.0, 2, 3]             # nothing lower on the right: the peak itself
    assert pd.find_peaks(x, prominence=(1.5, INF))[0] == [3, 7]
    assert pd.find_peaks(x, threshold=(1.0, INF))[0] == [1]
    assert pd.find_peaks(x, prominence=(math.nan, INF))[0] == []


def test_fallback_on_long_rows():
    """Some hundred thousand samples: white noise (a peak at every third sample), quarters (ties) and a slow wave with
    far-reaching walks; the vectorised form has to be fast enough to serve as the comparator of the GPU tests."""
    rng = np.random.default_rng(2)
    n = 300000
    noise = rng.standard_normal(n).astype(np.float32)
    rows = [noise, np.round(4*noise[:100000])/4, (np.sin(np.arange(60000)/2000.0) + 0.01*noise[:60000]).astype(np.float32)]
    rows[1][rng.integers(0, 100000, size=50)] = np.nan
    cases = [(0.25, 0), (0.25, 1001), (0.02, 0)]
    t0 = time.perf_counter()
    got = [host_find_peaks(x, None, None, (pmin, None), wlen) for x, (pmin, wlen) in zip(rows, cases)]
    seconds = time.perf_counter() - t0
    for x, (pmin, wlen), (pos, props) in zip(rows, cases, got):
        assert pd.same(pos, props, pd.find_peaks(x, prominence=(pmin, INF), wlen=wlen))
        assert len(pos) > 100
    assert len(got[0][0]) > n//5
    assert seconds < 10.0, seconds


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


def definition_of(peaks, c):
    props = np.stack((peaks.heights[c], peaks.prominences[c], peaks.left_bases[c], peaks.right_bases[c]), axis=1)
    return peaks.indices[c], props


def test_arguments_of_buffered_array_find_peaks():
    rate = 96000/7
    rng = np.random.default_rng(3)
    x = np.round(2*rng.standard_normal((4000, 2))) + np.array([0.0, 5.0])
    g = open_graph(x, rate)
    d = g.data
    pk = d.find_peaks()
    assert isinstance(pk, Peaks) and pk.rate == rate and pk.channels == 2 and pk.trace_name == d.name
    for c in range(2):
        assert pd.same(*definition_of(pk, c), pd.find_peaks(x[:, c]))
        assert pk.indices[c].dtype == np.int64 and pk.left_bases[c].dtype == np.int64
        assert pk.heights[c].dtype == np.float64 and pk.prominences[c].dtype == np.float64
    assert len(pk) == sum(len(i) for i in pk.indices) > 500
    # a scalar is the lower border, a pair is (min, max) with None for an open side, arrays are per channel
    for args, want in [
            (dict(height=1.0), [dict(height=(1.0, INF))]*2),
            (dict(height=(None, 6.0), prominence=2.0), [dict(height=(-INF, 6.0), prominence=(2.0, INF))]*2),
            (dict(height=np.array([1.0, 6.0])), [dict(height=(1.0, INF)), dict(height=(6.0, INF))]),
            (dict(threshold=(np.array([1.0, 2.0]), 3.0)), [dict(threshold=(1.0, 3.0)), dict(threshold=(2.0, 3.0))]),
            (dict(prominence=(1.0, np.array([4.0, 2.0])), height=(0.0, None)),
             [dict(prominence=(1.0, 4.0), height=(0.0, INF)), dict(prominence=(1.0, 2.0), height=(0.0, INF))]),
            (dict(threshold=[1.0, None]), [dict(threshold=(1.0, INF))]*2)]:
        pk = d.find_peaks(**args)
        for c in range(2):
            assert pd.same(*definition_of(pk, c), pd.find_peaks(x[:, c], **want[c])), (args, c)
    # wlen in seconds, rounded up to frames
    assert math.ceil(0.0049*rate) == 68 and math.ceil(0.0003*rate) == 5
    for seconds, frames in [(0.0049, 68), (0.0003, 5), (2/rate, 2), (1.01/rate, 2)]:
        pk = d.find_peaks(prominence=1.0, wlen=seconds)
        assert pd.same(*definition_of(pk, 0), pd.find_peaks(x[:, 0], prominence=(1.0, INF), wlen=frames))
    for seconds in [1/rate, 0.5/rate, 0.0]:
        with pytest.raises(ValueError):
            d.find_peaks(wlen=seconds)
    with pytest.raises(ValueError):
        d.find_peaks(height=[1.0, 2.0, 3.0])
    # a frame range is absolute, positions and bases too; empty, one and two samples have no peak
    pk = d.find_peaks(prominence=1.0, start=100, stop=900)
    assert pd.same(*definition_of(pk, 1), pd.find_peaks(x[100:900, 1], prominence=(1.0, INF), first=100))
    assert pk.indices[1].min() > 100 and pk.left_bases[1].min() >= 100 and pk.right_bases[1].max() < 900
    for stop in (7, 8, 9):
        assert len(d.find_peaks(start=7, stop=stop)) == 0
    with pytest.raises(IndexError):
        d.find_peaks(start=0, stop=4001)


def test_spectrogram_shaped_traces_are_refused():
    s = HostSpectrogram(nfft=16, source='data')
    open_graph(np.zeros((500, 2)), 100.0, [s])
    with pytest.raises(TypeError):
        s.find_peaks()


def test_peaks_object_against_hand_made_events():
    props = np.array([[1.0, 0.5, 2, 9], [3.0, 2.5, 9, 30], [2.0, 1.0, 30, 50], [4.0, 4.0, 0, 99]])
    pk = Peaks([(np.array([5, 20, 40, 60]), props), (np.zeros(0, dtype=np.int64), np.zeros((0, 4)))], 10.0, 'envelope')
    assert pk.channels == 2 and len(pk) == 4 and pk.trace_name == 'envelope'
    assert pk.times(0).tolist() == [0.5, 2.0, 4.0, 6.0] and pk.times(1).tolist() == []
    t, h = pk.points(0)
    assert t.tolist() == [0.5, 2.0, 4.0, 6.0] and h.tolist() == [1.0, 3.0, 2.0, 4.0]
    assert pk.prominences[0].tolist() == [0.5, 2.5, 1.0, 4.0]
    assert pk.left_bases[0].tolist() == [2, 9, 30, 0] and pk.right_bases[0].tolist() == [9, 30, 50, 99]
    # events are frames [onset, offset): a peak at the onset is inside, one at the offset is not
    ev = Events([[(0, 5), (5, 21), (21, 40), (39, 100), (61, 70)], [(0, 100)]], 10.0)
    assert pk.in_events(ev, 0).tolist() == [0, 2, 0, 2, 0] and pk.in_events(ev, 0).dtype == np.int64
    assert pk.in_events(ev, 1).tolist() == [0]


def test_tracegraph_find_peaks_and_mark_peaks_on_the_host():
    rate = 100.0
    rng = np.random.default_rng(5)
    x = np.round(3*rng.standard_normal((3000, 3)))
    f = HostFilter()
    g = open_graph(x, rate, [f])
    assert f._dev is None                                   # host-only graph: the numpy path
    pk = g.find_peaks('filtered', height=0.0, prominence=(2.0, None), wlen=0.5, t0=2.0, t1=25.0)
    i0, i1 = g.region_frames(f, 2.0, 25.0)
    assert (i0, i1) == (200, 2501)
    for c in range(3):
        want = pd.find_peaks(x[i0:i1, c] - 0.5, height=(0.0, INF), prominence=(2.0, INF), wlen=50, first=i0)
        assert pd.same(*definition_of(pk, c), want) and len(want[0]) > 20
    # without times: the buffer as it is
    assert pd.same(*definition_of(g.find_peaks('data', 1.0), 1), pd.find_peaks(x[:, 1], height=(1.0, INF)))
    a = Analyzer(g, 'pulses', 'filtered')
    a.make_trace_events('peak', 'filtered', 'o', '#ff0000', 8)
    a.set_events('peak', -1, [9.0], [9.0])                  # whatever was there goes
    g.mark_peaks(a, 'peak', pk)
    for c in range(3):
        t, h = a.events['peak'][c]
        assert t.tolist() == (pk.indices[c]/rate).tolist() and h.tolist() == pk.heights[c].tolist() and len(t) > 20
    # the pulses per event
    ev = g.detect_events('filtered', 1.4, min_gap=0.05, min_duration=0.0, t0=2.0, t1=25.0)
    for c in range(3):
        want = [int(((pk.indices[c] >= p) & (pk.indices[c] < q)).sum()) for p, q in ev.frames(c).tolist()]
        assert pk.in_events(ev, c).tolist() == want and sum(want) > 0


def test_ctypes_signature_and_constants():
    from audian_amd import _lib, hipdsp
    i64, vp, dbl = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    args, res = _lib._SIGNATURES['hipdsp_find_peaks']
    assert args == [vp, vp, i64, i64, i64, i64, vp, dbl, dbl, dbl, dbl, dbl, dbl, i64, i64, vp, i64, vp, i64, vp]
    assert res is ctypes.c_int and _lib.lib.hipdsp_find_peaks.argtypes == args
    assert hipdsp.PEAKS_CHUNK == 4096 and hipdsp.PEAKS_BLOCKS == (64, 4096, 262144)
    assert _lib.lib.hipdsp_version() == 102
