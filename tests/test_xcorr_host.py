"""Event cross-correlation on the host: the definition (tests/xcorr_definition.py) against the golden file made by
np.corrcoef and against scipy.signal.correlate, the condition T < 2^-30 on every input of the GPU tests, the numpy fallback
(audian_amd/xcorr.py, BufferedArray.region_xcorr) against the definition, the argument refusals, the accessors of
CrossCorrelation and the sign convention, the attribution rule on hand-made arrays, CrossCorrelationAnalyzer and
TraceGraph.attribute_events on host-computed traces, and the binding's signature.  No GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import xcorr_definition as xd
from audian_amd.analyzer import CrossCorrelationAnalyzer
from audian_amd.buffereddata import BufferedData
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.events import Events
from audian_amd.tracegraph import TraceGraph
from audian_amd.xcorr import CrossCorrelation, attribute_events, attribute_table, event_table, host_region_xcorr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'region_xcorr.npz')


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


class HostFilter(BufferedData):
    """A derived trace computed on the host: dest = source."""

    def __init__(self, name='filtered'):
        super().__init__(name, 'data')

    def open(self, source):
        super().open(source, 1)

    def process(self, source, dest, nbefore):
        dest[:] = np.asarray(source[nbefore:nbefore + len(dest)])


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


def golden_cases():
    g = np.load(GOLDEN)
    for i, (c, a, b, p, L) in enumerate(g['cases'].tolist()):
        yield g['x'], c, a, b, p, L, g['rows'][g['row_offsets'][i]:g['row_offsets'][i + 1]]


def test_definition_against_numpy_golden():
    seen_nan = seen_value = 0
    for x, c, a, b, p, L, want in golden_cases():
        q = xd.region_xcorr(x, c, a, b, p, L)
        got = q['r'].astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (c, a, b, p, L)
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 64*2.0**-53*np.sqrt(b - a + 1)), (c, a, b, p, L)
        seen_nan += int((~ok).sum())
        seen_value += int(ok.sum())
        # the float64 fallback meets the same numbers and the definition's info
        r, info = host_region_xcorr(x[c], x[p], a, b, L)
        assert xd.compare(q, r, info, 'host') <= 1.0
    assert seen_nan > 50 and seen_value > 500


def test_definition_against_scipy_correlate():
    """At interior lags sum((a - mean a)(b_l - mean b_l)) is scipy.signal.correlate of the window of the partner, taken
    wide enough for every lag, with the centred event window -- minus the part that the moving mean of b takes out."""
    from scipy import signal
    x = xd.slab('small')
    c, a, b, p, L = 0, 100, 400, 2, 25
    q = xd.region_xcorr(x, c, a, b, p, L)
    n = b - a
    ev = x[c, a:b].astype(np.float64)
    ev -= ev.mean()
    wide = x[p, a - L:b + L].astype(np.float64)
    cc = signal.correlate(wide, ev, mode='valid')               # cc[k] = sum ev[i] wide[k + i]: lag k - L
    assert len(cc) == 2*L + 1
    for k in range(2*L + 1):
        w = wide[k:k + n]
        r = cc[k]/n/(ev.std()*w.std())                          # sum ev = 0: the mean of w drops out of the covariance
        assert abs(r - float(q['r'][k])) <= 1e-12


@pytest.mark.parametrize('name', sorted(xd.GPU_CASES))
def test_gpu_inputs_meet_the_condition_on_T(name):
    x, regions, partners, L = xd.case(name)
    values = 0
    for c, a, b in regions.tolist():
        for p in partners:
            T = xd.bound_T(xd.region_xcorr(x, c, a, b, p, L))
            ok = ~np.isnan(T)
            values += int(ok.sum())
            assert np.all(T[ok] < xd.T_LIMIT), (name, c, a, b, p, float(np.max(T[ok])))
    assert values > 0


def test_bound_separates_float32_sums_under_an_offset():
    """The case that tells float64 pivot-shifted sums from float32 ones: n = 65536 under an offset of 10^4 sigma.  The
    float64 fallback is within the contract; the same sums carried in float32 miss it by far."""
    x, regions, partners, L = xd.case('dc')
    c, a, b = regions[0].tolist()
    q = xd.region_xcorr(x, c, a, b, partners[0], L)
    r, info = host_region_xcorr(x[c], x[partners[0]], a, b, L)
    assert xd.compare(q, r, info, 'float64') <= 1.0
    d = x[c, a:b] - x[c, a]
    e = x[partners[0], a:b] - x[partners[0], a]
    n = np.float32(b - a)
    s = [np.cumsum(v, dtype=np.float32)[-1] for v in (d, d*d, e, e*e, d*e)]          # sequential float32 sums
    va, vb = s[1]/n - (s[0]/n)**2, s[3]/n - (s[2]/n)**2
    r32 = np.float32((s[4]/n - (s[0]/n)*(s[2]/n))/np.sqrt(va*vb))
    assert abs(float(r32) - float(q['r'][L])) > 8*2.0**-24*abs(float(q['r'][L]))


def test_buffered_array_region_xcorr_against_the_definition():
    x = xd.slab('small')
    g = open_graph(x.T.astype(np.float64), 100.0)
    d = g.data
    regions = [(0, 10, 310), (2, 0, 700), (1, 350, 355), (1, 690, 700), (0, 5, 5)]
    xc = d.region_xcorr(regions, max_lag=12)
    assert isinstance(xc, CrossCorrelation) and len(xc) == 5 and xc.partners.tolist() == [0, 1, 2]
    assert xc.r.shape == (5, 3, 25) and xc.info.shape == (5, 3, 4) and xc.table.tolist() == [list(r) for r in regions]
    assert xd.compare_call(x, regions, [0, 1, 2], 12, xc.r, xc.info, 'host') <= 1.0
    xc = d.region_xcorr(regions[:2], partners=[2, 2, 0], max_lag=0)
    assert xc.r.shape == (2, 3, 1) and np.array_equal(xc.r[:, 0], xc.r[:, 1])
    assert xc.r[1, 0, 0] == 1.0                                         # a channel against itself, lag 0
    assert len(d.region_xcorr([], max_lag=3)) == 0 and d.region_xcorr([], max_lag=3).r.shape == (0, 3, 7)
    assert d.region_xcorr(regions, partners=[], max_lag=3).r.shape == (5, 0, 7)


def test_buffered_data_without_a_mirror_takes_any_iterable():
    """The fallback of BufferedData.region_xcorr gets the table it has already read, not the caller's iterator again."""
    x = xd.slab('small')
    f = HostFilter()
    open_graph(x.T.astype(np.float64), 100.0, [f])
    assert f._dev is None
    regions = [(0, 10, 310), (1, 350, 355)]
    xc = f.region_xcorr(iter(regions), partners=iter([2, 0]), max_lag=3)
    assert len(xc) == 2 and xc.table.tolist() == [list(r) for r in regions] and xc.partners.tolist() == [2, 0]
    assert xd.compare_call(x, regions, [2, 0], 3, xc.r, xc.info, 'host') <= 1.0


def test_argument_refusals():
    x = xd.slab('small')
    s = HostSpectrogram(nfft=16, source='data')
    g = open_graph(x.T.astype(np.float64), 100.0, [s])
    d = g.data
    with pytest.raises(TypeError):
        s.region_xcorr([(0, 0, 100)])
    for bad in (-1, 1025, 2.5):
        with pytest.raises(ValueError):
            d.region_xcorr([(0, 0, 100)], max_lag=bad)
    for partners in ([3], [-1], [0, 7]):
        with pytest.raises(ValueError):
            d.region_xcorr([(0, 0, 100)], partners=partners)
    for region in ((3, 0, 10), (-1, 0, 10), (0, -1, 10), (0, 0, 701), (0, 20, 10)):
        with pytest.raises(IndexError):
            d.region_xcorr([region])
    with pytest.raises(ValueError, match='1024'):
        g.event_cross_correlation(Events([[(0, 100)], [], []], 100.0, 'data'), max_delay=11.0)
    with pytest.raises(ValueError):
        attribute_events(Events([[(0, 100)], [], []], 100.0, 'data'), d.region_xcorr([]))


def test_accessors_and_the_sign_convention():
    """A partner that is the event's channel k samples later has its peak at lag +k."""
    rng = np.random.default_rng(5)
    k, rate = 4, 200.0
    x = np.zeros((3, 600), dtype=np.float32)
    x[0] = rng.standard_normal(600)
    x[1, k:] = x[0, :-k]                                                # the same waveform, k samples later
    x[2, :-2] = 0.5*x[0, 2:]                                            # two samples earlier, half as loud
    g = open_graph(x.T.astype(np.float64), rate)
    xc = g.data.region_xcorr([(0, 100, 400), (1, 100, 400)], max_lag=6)
    assert xc.lags.tolist() == list(range(-6, 7)) and xc.max_lag == 6 and xc.rate == rate
    assert xc.best_lag(0).tolist() == [0.0, float(k), -2.0]
    assert xc.best_r(0).tolist() == [1.0, 1.0, 1.0]
    assert np.array_equal(xc.delays(0), np.array([0.0, k, -2.0])/rate)
    assert xc.best_lag(1).tolist() == [-float(k), 0.0, -2.0 - k]
    sd = float(np.std(x[0, 100:400].astype(np.float64)))
    assert np.allclose(xc.std_event(0), sd, rtol=1e-12) and np.allclose(xc.std_partner(0), [sd, sd, 0.5*sd], rtol=1e-12)
    # undefined: a constant partner
    x[2] = 1.0
    g = open_graph(x.T.astype(np.float64), rate)
    xc = g.data.region_xcorr([(0, 100, 400)], max_lag=6)
    assert np.isnan(xc.best_lag(0)[2]) and np.isnan(xc.best_r(0)[2]) and np.isnan(xc.std_partner(0)[2])
    assert np.isnan(xc.delays(0)[2]) and xc.info[0, 2, 0] == 0 and xc.info[0, 2, 1] == -1


def hand_made(table, partners, best_r, best_lag, std_event, std_partner, L=5, rate=100.0):
    """A CrossCorrelation whose accessors give these arrays."""
    R, P = len(table), len(partners)
    r = np.full((R, P, 2*L + 1), np.nan, dtype=np.float32)
    info = np.zeros((R, P, 4))
    for i in range(R):
        for j in range(P):
            if np.isnan(best_r[i][j]):
                info[i, j] = [0, -1, std_event[i], np.nan]
            else:
                pos = L + int(best_lag[i][j])
                r[i, j, pos] = best_r[i][j]
                info[i, j] = [1, pos, std_event[i], std_partner[i][j]]
    return CrossCorrelation(table, partners, r, info, L, rate)


def test_attribution_rule_on_hand_made_arrays():
    nan = np.nan
    table = [(0, 0, 10), (0, 20, 30), (0, 40, 50), (0, 60, 70), (0, 80, 90), (1, 0, 10), (2, 5, 15)]
    partners = [2, 1, 0, 3]
    best_r = [[0.2, 0.4, 1.0, 0.1],             # own: nobody correlates
              [0.9, 0.8, 1.0, 0.1],             # crosstalk: 2 and 1 pass, 1 is louder
              [0.9, 0.9, 1.0, 0.9],             # a tie between 2 and 1 in loudness: the lower channel, 1
              [nan, 0.9, 1.0, nan],             # NaN never passes; 1 passes r but is quieter: own
              [0.3, 0.49, 1.0, 0.2],            # channel 1 is far louder but uncorrelated: own
              [0.7, 1.0, 0.6, 0.4],             # on channel 1: its own row is skipped, 2 and 0 pass, 0 louder
              [1.0, 0.5, 0.5, 0.5]]             # on channel 2: r == min_r and ratio == min_ratio pass: 0, 1 and 3 tie, 0
    best_lag = [[0, 0, 0, 0], [2, -3, 0, 1], [2, -3, 0, 1], [0, 1, 0, 0], [0, 1, 0, 0], [1, 0, 4, 0], [0, 1, -1, 5]]
    std_event = [1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0]
    std_partner = [[3.0, 3.0, 1.0, 3.0], [2.0, 2.5, 1.0, 9.0], [2.5, 2.5, 1.0, 2.0], [nan, 0.9, 1.0, nan],
                   [1.0, 50.0, 1.0, 1.0], [2.5, 2.0, 3.0, 9.0], [1.0, 1.0, 1.0, 1.0]]
    xc = hand_made(table, partners, best_r, best_lag, std_event, std_partner)
    src, delay, corr = attribute_table(xc)
    assert src.tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert np.allclose(delay, [0, -0.03, -0.03, 0, 0, 0.04, -0.01])
    assert np.allclose(corr, [1, 0.8, 0.9, 1, 1, 0.6, 0.5])
    # the sequential form of the definition file agrees, row by row, also with other thresholds
    for min_r, min_ratio in ((0.5, 1.0), (0.85, 1.0), (0.1, 3.0), (0.5, 0.5)):
        src, delay, corr = attribute_table(xc, min_r, min_ratio)
        for i in range(len(table)):
            s, lag = xd.attribute(table[i][0], partners, xc.best_r(i), xc.best_lag(i), xc.std_event(i), xc.std_partner(i),
                                  min_r, min_ratio)
            assert (s, lag/xc.rate) == (src[i], delay[i]), (i, min_r, min_ratio)
    # through Events: the events that are their own source stay, sources and delays cover all
    ev = Events([[(0, 10), (20, 30), (40, 50), (60, 70), (80, 90)], [(0, 10)], [(5, 15)]], 100.0, 'data')
    assert event_table(ev).tolist() == [list(r) for r in table]
    own, sources, delays = attribute_events(ev, xc)
    assert [s.tolist() for s in sources] == [[0, 1, 1, 0, 0], [0], [0]]
    assert own.frames(0).tolist() == [[0, 10], [60, 70], [80, 90]] and len(own.onsets[1]) == 0 and len(own.onsets[2]) == 0
    assert own.rate == 100.0 and own.trace_name == 'data' and np.allclose(delays[1], [0.04])


def crosstalk_recording(rate=1000.0, n=10000, shift=5, gain=0.3):
    """Four channels of weak noise; a song on channel 1 at 2-3 s that channel 2 carries `shift` samples later at `gain`
    times the amplitude, and a song of its own on channel 3 at 6-7 s."""
    rng = np.random.default_rng(21)
    x = 0.01*rng.standard_normal((n, 4))
    song = rng.standard_normal(1000)
    x[2000:3000, 1] += song
    x[2000 + shift:3000 + shift, 2] += gain*song
    x[6000:7000, 3] += rng.standard_normal(1000)
    return x


def test_tracegraph_attribute_events_and_the_analyzer_on_a_host_graph():
    rate, shift = 1000.0, 5
    x = crosstalk_recording(rate, shift=shift)
    f = HostFilter()
    g = open_graph(x, rate, [f])
    assert f._dev is None                                               # host-only graph: the numpy path
    ev = Events([[], [(2000, 3000)], [(2004, 3006)], [(6000, 7000)]], rate, 'filtered')
    xc = g.event_cross_correlation(ev, max_delay=0.008)
    assert xc.max_lag == 8 and xc.table.tolist() == [[1, 2000, 3000], [2, 2004, 3006], [3, 6000, 7000]]
    own, sources, delays = g.attribute_events(ev, max_delay=0.008)
    assert [s.tolist() for s in sources] == [[], [1], [1], [3]]
    assert delays[2].tolist() == [-shift/rate] and delays[1].tolist() == [0.0] and delays[3].tolist() == [0.0]
    assert [len(o) for o in own.onsets] == [0, 1, 0, 1]
    # the definition's rule over the definition's numbers gives the same sources
    x32 = np.ascontiguousarray(x.T, dtype=np.float32)
    for i, (c, a, b) in enumerate(xc.table.tolist()):
        qs = [xd.region_xcorr(x32, c, a, b, p, 8) for p in range(4)]
        s, lag = xd.attribute(c, [0, 1, 2, 3], [float(q['r'][int(q['info'][1])]) for q in qs],
                              [q['info'][1] - 8 for q in qs], [q['info'][2] for q in qs], [q['info'][3] for q in qs])
        assert s == sources[c][0] and lag/rate == delays[c][0]
    # the analyzer: one row per event through analyze_events, the same through analyze_region
    a = CrossCorrelationAnalyzer(g, 'filtered', max_delay=0.008)
    assert a.data.labels == ['source channel', 'delay', 'correlation'] and a.data.units[1] == 's'
    g.analyze_events(ev)
    rows = a.rows()
    assert [r[0] for r in rows] == [1, 1, 3] and [r[1] for r in rows] == [0.0, -shift/rate, 0.0]
    assert rows[0][2] == 1.0 and 0.99 < rows[1][2] <= 1.0
    a.clear()
    g.analyze_region(2.004, 3.0055, 2)
    assert a.rows() == [rows[1]]
    with pytest.raises(ValueError):
        CrossCorrelationAnalyzer(g, 'filtered', max_delay=2.0)


def test_ctypes_signature_and_constants():
    from audian_amd import _lib, hipdsp, xcorr
    i64, vp, cint = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    args, res = _lib._SIGNATURES['hipdsp_region_xcorr']
    assert args == [vp, vp, i64, i64, i64, ctypes.POINTER(i64), i64, ctypes.POINTER(cint), cint, cint, vp, i64, vp]
    assert res is ctypes.c_int and _lib.lib.hipdsp_region_xcorr.argtypes == args
    header = open(os.path.join(HERE, '..', 'include', 'hip_dsp.h')).read()
    proto = re.search(r'int hipdsp_region_xcorr\(([^;]*)\);', header).group(1)
    kinds = [re.sub(r'\s*\w+$', '', a.strip()) for a in proto.replace('\n', ' ').split(',')]
    assert kinds == ['hipdsp_ctx *', 'const float *', 'int64_t', 'int64_t', 'int64_t', 'const int64_t *', 'int64_t',
                     'const int *', 'int', 'int', 'float *', 'int64_t', 'double *']
    assert (hipdsp.XCORR_TILE, hipdsp.XCORR_CHUNK, hipdsp.XCORR_LAGS, hipdsp.XCORR_MAX_LAG) == \
        (xd.TILE, xd.CHUNK, xd.LAGS_PER_THREAD, xd.MAX_LAG) and xcorr.MAX_LAG == xd.MAX_LAG
    # the scratch formula of the header: the tables rounded up to 8 bytes, then the float64 rows
    assert hipdsp.region_xcorr_scratch([(0, 0, 10), (1, 5, 5), (0, 0, xd.CHUNK + 1)], 3, 4) == 48*4 + 16 + 8*(4 + 27)*9
    assert hipdsp.region_xcorr_scratch([(0, 0, 10)], 2, 0) == 48*2 + 8 + 8*(4 + 27)*2
