"""Host side of the event refinement (no GPU): the golden file against the definitions, the case list of the GPU
accuracy test against the cap, audian_amd.refine against tests/refine_definition.py, and BufferedEventFilter /
TraceGraph.refine_events on traces without a device mirror."""

import numpy as np
import pytest

import iir_bound as ib
import refine_definition as rd
from audian_amd import refine
from audian_amd.bufferedeventfilter import BufferedEventFilter
from audian_amd.design import butter_sos
from audian_amd.events import Events
from audian_amd.tracegraph import TraceGraph
from conftest import load_golden


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


# ---- the filter ------------------------------------------------------------------------------------------------------------

def test_definitions_against_the_golden_file():
    """iir_bound.sosfiltfilt in float64 and refine.host_region_filtfilt against scipy's sosfiltfilt -- and, for the
    reference's first-order filters, scipy's filtfilt(b, a, v) -- per 64-sample window, within Q_CAP roundings of
    float32 (measured: 0.0 for the float64 run)."""
    g = load_golden('region_filtfilt')
    off, ffo = g['offsets'], g['ff_offsets']
    assert len(g['sections']) == 12 and sorted(set(np.diff(off))) == [7, 16, 65, 4099]
    worst = 0.0
    for i, S in enumerate(g['sections']):
        v, sos = g['x'][off[i]:off[i + 1]], g['sos'][i][:S]
        assert v.dtype == np.float32
        want = [g['y_sosfiltfilt'][off[i]:off[i + 1]]]
        if S == 1:
            assert sos[0, 2] == 0.0 and sos[0, 5] == 0.0 and ib.padlen(sos) == 6
            want.append(g['y_filtfilt'][ffo[i]:ffo[i + 1]])
        run = ib.sosfiltfilt(sos, v[:, None], np.float64, gain=1.0, rectify=False, clamp=False)
        for y in want:
            assert len(y) == len(v)
            rho = float(np.max(ib.ratios(run, y[:, None])))
            worst = max(worst, rho)
            assert rho <= ib.Q_CAP, (i, rho)
            host = refine.host_region_filtfilt(v, sos)
            assert host.dtype == np.float32
            # one rounding to float32 on top
            assert float(np.max(ib.ratios(host[:, None], y[:, None]))) <= 1.0 + ib.Q_CAP, i
    print('largest e_w / (2^-24 r_w) of the float64 definition against scipy: %.3g' % worst)


@pytest.mark.parametrize('label', list(rd.CASES))
def test_case_list_meets_the_cap(label):
    """Every (filter, family) of the GPU accuracy test has q <= Q_CAP and a reference the bound can be met on, at the
    lengths padlen + 1, 65, 4097 and 3 * 4096 + 5."""
    sos, rate, fams = rd.case_design(label)
    assert len(sos) == (2 if label.startswith('lp4') else 1)
    pad = ib.padlen(sos)
    for L in (pad + 1, 65, 4097, 3*4096 + 5):
        x = rd.case_signal(label, L)
        ref, q = rd.filtfilt_case(sos, x)
        ib.assert_in_range(ref, '%s, L %d' % (label, L))
        assert np.all(q <= ib.Q_CAP), (label, L, q)


def test_too_short_exactly_at_padlen():
    sos = butter_sos(1, 40.0, 'lowpass', 5000.0)
    v = np.linspace(0, 1, 7, dtype=np.float32)
    assert ib.padlen(sos) == 6 and refine.padlen(sos) == 6
    assert refine.host_region_filtfilt(v, sos).shape == (7,)
    with pytest.raises(ValueError, match='padlen'):
        refine.host_region_filtfilt(v[:6], sos)
    with pytest.raises(ValueError, match='padlen'):
        ib.sosfiltfilt(sos, v[:6, None], np.float64, gain=1.0, rectify=False, clamp=False)
    four = butter_sos(4, 300.0, 'lowpass', 48000.0)
    assert refine.padlen(four) == ib.padlen(four) == 15 and refine.padlen(np.array([four, four])).tolist() == [15, 15]
    with pytest.raises(ValueError, match='padlen'):
        refine.host_region_filtfilt(np.ones(15, dtype=np.float32), four)


def test_host_filter_special_values_and_clamp():
    sos = butter_sos(1, 400.0, 'lowpass', 5000.0)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(100).astype(np.float32)
    y = refine.host_region_filtfilt(v, sos)
    assert np.any(y < 0)
    assert np.array_equal(refine.host_region_filtfilt(v, sos, clamp=True), np.where(y < 0, np.float32(0), y))
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[17] = bad
        assert np.all(np.isnan(refine.host_region_filtfilt(w, sos)))
    for wrong in ([[1, 1, 0, 2, 0, 0]], [[1, 1, 0, 1, -1.0, 0]], [[np.nan, 1, 0, 1, 0, 0]], [[1, 1, 0, 1, 0.5, 1.0]]):
        with pytest.raises(ValueError):
            refine.check_sos(np.array([wrong], dtype=np.float64))
    with pytest.raises(NotImplementedError):
        refine.check_sos(np.zeros((1, 3, 6)))


def test_host_crossings_against_the_definition():
    rng = np.random.default_rng(8)
    row = rng.standard_normal(300).astype(np.float32)
    row[40] = row[41] = row.max() + 1                       # a plateau at the maximum
    cases = [(0, 300, 0.0), (5, 5, 0.0), (10, 200, float(row[40])), (10, 200, np.nan), (10, 200, np.inf), (10, 200, -np.inf),
             (42, 300, 1.0), (0, 1, -10.0)]
    for a, b, thr in cases:
        assert np.array_equal(refine.host_region_crossings(row, a, b, thr), rd.region_crossings(row, a, b, thr),
                              equal_nan=True), (a, b, thr)
    bad = row.copy()
    bad[[60, 90]] = np.nan
    bad[70] = np.inf
    got = refine.host_region_crossings(bad, 50, 100, 0.0)
    assert np.array_equal(got, rd.region_crossings(bad, 50, 100, 0.0), equal_nan=True)
    assert np.isnan(got[4]) and got[5] == 60


# ---- the bookkeeping -------------------------------------------------------------------------------------------------------

def test_widen_events():
    n = 1000
    on, off = np.array([5, 100, 130, 400, 990]), np.array([20, 120, 300, 500, 998])
    won, woff = refine.widen_events(on, off, n, 10)
    assert won.tolist() == [0, 90, 125, 390, 980] and woff.tolist() == [30, 125, 310, 510, 1000]     # (120 + 130)//2
    for width in (0, 1, 7, 10, 45, 200, 5000):
        won, woff = refine.widen_events(on, off, n, width)
        dn, df = rd.widen_events(on, off, n, width)
        assert np.array_equal(won, dn) and np.array_equal(woff, df)
        assert won[0] >= 0 and woff[-1] <= n and np.all(woff[:-1] <= won[1:]) and np.all(won <= on) and np.all(woff >= off)
    e = refine.widen_events([], [], n, 5)
    assert len(e[0]) == 0 and len(e[1]) == 0


def random_events(rng, n, k):
    cuts = np.sort(rng.choice(np.arange(1, n), size=2*k, replace=False))
    return cuts[0::2].astype(np.int64), cuts[1::2].astype(np.int64)


def test_clean_event_freqs_against_the_definition():
    rng = np.random.default_rng(21)
    for trial in range(20):
        pairs, freqs = [], []
        for c in range(3):
            on, off = random_events(rng, 5000, int(rng.integers(0, 9)))
            f = 40.0 + rng.standard_normal(len(on))
            f[rng.random(len(on)) < 0.2] = np.nan
            f[rng.random(len(on)) < 0.1] = 400.0
            pairs.append(np.stack((on, off), axis=1))
            freqs.append(f)
        ev = Events(pairs, 1000.0, 'envelope')
        keep = [f.copy() for f in freqs]
        got, gf = refine.clean_event_freqs(ev, freqs, fac=6.0)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(freqs, keep))        # nothing in place
        don, doff, df = rd.clean_event_freqs(ev.onsets, ev.offsets, freqs, fac=6.0)
        for c in range(3):
            assert np.array_equal(got.onsets[c], don[c]) and np.array_equal(got.offsets[c], doff[c])
            assert np.array_equal(gf[c], df[c]) and not np.isnan(gf[c]).any()
        assert got.rate == 1000.0 and got.trace_name == 'envelope'
    empty = Events([np.zeros((0, 2))]*2, 10.0)
    got, gf = refine.clean_event_freqs(empty, [np.zeros(0)]*2)
    assert len(got) == 0 and [len(f) for f in gf] == [0, 0]


def test_event_filters():
    sos, valid = refine.event_filters([10.0, np.nan, 600.0, 625.0, 100.0], 5000.0)
    assert valid.tolist() == [True, False, True, False, True] and sos.shape == (5, 1, 6)
    assert np.array_equal(sos[0], butter_sos(1, 40.0, 'lowpass', 5000.0))
    assert np.array_equal(sos[1], [[1, 0, 0, 1, 0, 0]])
    sos, valid = refine.event_filters([10.0], 5000.0, factor=2.0, order=4)
    assert sos.shape == (1, 2, 6) and np.array_equal(sos[0], butter_sos(4, 20.0, 'lowpass', 5000.0))
    with pytest.raises(ValueError):
        refine.event_filters([10.0], 5000.0, order=5)


def env_with_songs(rng, n, on, off):
    env = (0.02 + 0.01*rng.random(n)).astype(np.float32)
    for a, b in zip(on, off):
        m = np.arange(a, b)
        env[a:b] += (0.5*np.sin(np.pi*(m - a + 0.5)/(b - a))).astype(np.float32)
    return env


def host_refine(env, on, off, freqs, threshold, w, fac):
    row = np.asarray(env, dtype=np.float32)

    def maxima(windows):
        return [refine.host_region_crossings(row, a, max(a, b), np.nan)[4] for a, b in windows]

    def crossings(windows, thresholds):
        res = np.array([refine.host_region_crossings(row, a, max(a, b), t) for (a, b), t in zip(windows, thresholds)])
        return res[:, 2].astype(np.int64), res[:, 3].astype(np.int64)

    return refine.refine(np.stack((on, off), axis=1), freqs, maxima, crossings, threshold, w, len(row), fac)


def test_refine_against_the_definition():
    rng = np.random.default_rng(77)
    n, w = 6000, 60
    lists = [random_events(rng, n, int(rng.integers(1, 12))) for trial in range(25)]
    lists.append((np.array([0, 700, 5800]), np.array([300, 900, n])))               # an event at either end of the trace
    lists.append((np.array([100, 420, 470, 3000]), np.array([400, 450, 900, 3300])))  # windows shorter than w/2: carried over
    carried = False
    for on, off in lists:
        env = env_with_songs(rng, n, on, off)
        freqs = 30.0 + rng.random(len(on))
        freqs[rng.random(len(on)) < 0.15] = np.nan
        wide, before, after = refine.noise_windows(np.stack((on, off), axis=1), freqs, w, n)
        ok = ~np.isnan(freqs)
        carried = carried or bool(np.any((before[ok, 1] - before[ok, 0] <= w/2) | (after[ok, 1] - after[ok, 0] <= w/2)))
        for fac in (1.0, 20.0):
            got = host_refine(env, on, off, freqs, 0.05, w, fac)
            want = rd.refine(on, off, freqs, env, 0.05, w, fac)
            assert got.tolist() == [list(p) for p in want], (on, off)
    assert carried


def test_refine_reports_an_event_at_the_window_border():
    """An envelope above the threshold over the whole widened event: [wide onset, wide offset), rule 2 of
    hipdsp_detect_events."""
    env = np.full(1000, 0.01, dtype=np.float32)
    env[300:700] = 1.0
    got = host_refine(env, np.array([400]), np.array([600]), np.array([30.0]), 0.05, 100, 1.0)
    assert got.tolist() == [[300, 700]]
    assert rd.refine([400], [600], [30.0], env, 0.05, 100) == [(300, 700)]


# ---- the traces, without a device ----------------------------------------------------------------------------------------

RATE = 1000.0


def host_graph(x, buffer_time, back_time=0.0):
    g = TraceGraph(buffer_time, back_time)
    g.add_trace(BufferedEventFilter(source='data'))
    g.setup_traces()
    g.open(x, RATE)
    g['eventfiltered'].plot_items = [Item()]*x.shape[1]
    g.set_need_update()
    return g


def songs(n=8000):
    rng = np.random.default_rng(5)
    x = np.zeros((n, 2))
    on = [np.array([0, 2000, 5000]), np.array([1000, 6500])]
    off = [np.array([600, 3000, 6000]), np.array([1800, 7600])]
    for c in range(2):
        x[:, c] = env_with_songs(rng, n, on[c], off[c])
    ev = Events([np.stack((on[c], off[c]), axis=1) for c in range(2)], RATE, 'data')
    freqs = [np.array([20.0, np.nan, 35.0]), np.array([25.0, 30.0])]
    return x.astype(np.float32).astype(np.float64), ev, freqs


def test_event_filter_trace_on_the_host():
    x, ev, freqs = songs()
    g = host_graph(x, 20.0)
    g.update_times(0.0, 8.0)
    t = g['eventfiltered']
    assert t._dev is None and np.array_equal(np.asarray(t.buffer), x)            # no events yet: a copy
    t.set_events(ev, freqs, 0.05)
    width = 100
    assert t.regions.tolist() == [[0, 0, 700], [0, 4900, 6100], [1, 900, 1900], [1, 6400, 7700]] and width == round(2*0.05*RATE)
    assert t.skipped == []
    got = np.asarray(t.buffer)
    mask = np.ones(x.shape, dtype=bool)
    for (c, a, b), f in zip(t.regions.tolist(), (20.0, 35.0, 25.0, 30.0)):
        sos = butter_sos(1, 4.0*f, 'lowpass', RATE)
        want = ib.sosfiltfilt(sos, x[a:b, c:c + 1].astype(np.float32), np.float64, gain=1.0, rectify=False, clamp=False)
        assert np.array_equal(got[a:b, c], want[:, 0].astype(np.float32).astype(np.float64))
        mask[a:b, c] = False
    assert np.array_equal(got[mask], x[mask])                                   # bit-identical outside the regions
    assert np.array_equal(np.asarray(g.data.buffer), x)                          # the source is left alone


def test_event_filter_trace_skips_regions_on_the_border():
    x, ev, freqs = songs()
    g = host_graph(x, 5.0)
    g.update_times(0.0, 5.0)
    t = g['eventfiltered']
    t.set_events(ev, freqs, 0.05)
    lo, hi = t.offset, t.offset + len(t.buffer)
    assert lo == 0 and 4900 < hi < 6100
    assert t.skipped == [(0, 4900, 6100)]
    got = np.asarray(t.buffer)
    assert np.array_equal(got[4900:hi], x[4900:hi])                          # the cut region is unfiltered
    assert not np.array_equal(got[0:700, 0], x[0:700, 0]) and not np.array_equal(got[900:1900, 1], x[900:1900, 1])
    g.update_times(3.0, 8.0)                                                     # the buffer moves: everything again
    lo, hi = t.offset, t.offset + len(t.buffer)
    assert lo > 1900 and hi == 8000 and t.skipped == []
    got = np.asarray(t.buffer)
    sos = butter_sos(1, 140.0, 'lowpass', RATE)
    want = ib.sosfiltfilt(sos, x[4900:6100, 0:1].astype(np.float32), np.float64, gain=1.0, rectify=False, clamp=False)
    assert np.array_equal(got[4900 - lo:6100 - lo, 0], want[:, 0].astype(np.float32).astype(np.float64))
    assert np.array_equal(got[:4900 - lo, 0], x[lo:4900, 0])


def test_refine_events_on_the_host():
    x, ev, freqs = songs()
    g = host_graph(x, 20.0)
    g.update_times(0.0, 8.0)
    g['eventfiltered'].set_events(ev, freqs, 0.05)
    clean, cf = g.clean_event_freqs(ev, freqs)
    assert [len(o) for o in clean.onsets] == [2, 2] and [f.tolist() for f in cf] == [[20.0, 35.0], [25.0, 30.0]]
    got = g.refine_events(ev, freqs, [0.05, 0.05], 'eventfiltered', min_duration=0.05, min_thresh_fac=2.0)
    assert got.trace_name == 'eventfiltered' and got.rate == RATE
    env = np.asarray(g['eventfiltered'].buffer)
    for c in range(2):
        want = rd.refine(ev.onsets[c], ev.offsets[c], freqs[c], env[:, c], 0.05, 50, 2.0)
        assert got.frames(c).tolist() == [list(p) for p in want]
        assert len(want) == int(np.sum(~np.isnan(freqs[c])))
    assert got.onsets[0][0] == 0 or got.onsets[0][0] < 50                       # the song at the very start
