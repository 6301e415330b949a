"""The event refinement on device mirrors: BufferedEventFilter, BufferedData.region_filtfilt / region_crossings and
TraceGraph.refine_events on a synthetic three-channel envelope -- pulse trains of known rates on a noise floor, three
songs per channel, one at the very start.  The comparators are the definitions: iir_bound.sosfiltfilt (longdouble) for
the filter, tests/refine_definition.py for the bookkeeping."""

import functools

import numpy as np
import pytest

import iir_bound as ib
import refine_definition as rd

pytestmark = pytest.mark.gpu

RATE = 2000.0
N = 100000
C = 3
MIN_DURATION = 0.1
SONGS = {0: [(0.0, 1.5, 20.0), (10.0, 11.2, 25.0), (30.0, 32.0, 30.0)],
         1: [(2.0, 3.0, 22.0), (20.0, 21.5, 27.0), (40.0, 41.0, 32.0)],
         2: [(5.0, 6.5, 24.0), (15.0, 16.0, 29.0), (47.5, 49.0, 34.0)]}


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def envelope():
    rng = np.random.default_rng(41)
    t = np.arange(N)/RATE
    x = 0.02 + 0.01*rng.random((N, C))
    for c, songs in SONGS.items():
        for t0, t1, f in songs:
            on = (t >= t0) & (t < t1)
            x[on, c] += 0.5*(1.0 + 0.8*np.sin(2*np.pi*f*(t[on] - t0)))
    return x.astype(np.float32).astype(np.float64)


def device_copy():
    """A derived trace that is its source, uploaded: the synthetic envelope with a device mirror."""
    from audian_amd import hipdsp
    from audian_amd.buffereddata import BufferedData

    class DeviceCopy(BufferedData):
        def __init__(self):
            BufferedData.__init__(self, 'envelope', 'data')

        def open(self, source):
            BufferedData.open(self, source, 1)

        def process(self, source, dest, nbefore):
            call = self._take_call(source, dest)
            if len(dest) == 0:
                return
            dsrc, spitch, up = self._device_source(source, call)
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            hipdsp.memcpy2d(self.ctx, ddst, 4*dpitch, dsrc.view(nbefore, (1,)), 4*spitch, 4*len(dest), self.channels)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)

    return DeviceCopy()


def make_graph(buffer_time):
    from audian_amd.bufferedeventfilter import BufferedEventFilter
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(buffer_time, 0.0)
    g.add_trace(device_copy())
    g.add_trace(BufferedEventFilter(source='envelope'))
    g.setup_traces()
    g.open(envelope(), RATE)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    return g


@functools.lru_cache(maxsize=None)
def scene():
    """(graph, events, pulse rates) with the whole trace resident and the events' filters set."""
    g = make_graph(60.0)
    g.update_times(0.0, N/RATE)
    ev = g.detect_events('envelope', 0.2, min_gap=0.05, min_duration=0.05)
    freqs = g.event_peak_freqs(ev, freq_resolution=2.0, step=1)
    return g, ev, freqs


def filtered(g, ev, freqs):
    """The event-filtered trace of the scene with its events set."""
    t = g['eventfiltered']
    if len(t.regions) == 0:
        t.set_events(ev, freqs, MIN_DURATION)
    return t


def test_events_and_pulse_rates_of_the_scene():
    g, ev, freqs = scene()
    assert np.array_equal(np.asarray(g['envelope'].buffer), envelope())
    for c in range(C):
        assert len(ev.onsets[c]) == 3
        for j, (t0, t1, f) in enumerate(SONGS[c]):
            assert abs(ev.onsets[c][j] - t0*RATE) <= 0.03*RATE and abs(ev.offsets[c][j] - t1*RATE) <= 0.03*RATE
            assert abs(freqs[c][j] - f) <= 2.0
    assert ev.onsets[0][0] == 0


def test_event_filter_on_the_mirror():
    """ONE hipdsp_region_filtfilt call filters all nine widened events in place on the trace's mirror, each with its own
    low-pass; every window of every region within the bound of the definition; everything outside the regions is
    bit-identical to the source, and the source is left alone."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    g, ev, freqs = scene()
    t = g['eventfiltered']
    before = hipdsp.launches.get('region_filtfilt', 0)
    t.set_events(ev, freqs, MIN_DURATION)
    assert hipdsp.launches['region_filtfilt'] == before + 1
    assert t._dev is not None and t._stale and t.skipped == [] and len(t.regions) == 9
    x = envelope()
    got = np.asarray(t.buffer)
    mask = np.ones(x.shape, dtype=bool)
    width = int(round(2*MIN_DURATION*RATE))
    k = 0
    for c in range(C):
        for j in range(3):
            cc, a, b = t.regions[k].tolist()
            assert cc == c and a == max(ev.onsets[c][j] - width, 0) and b == ev.offsets[c][j] + width
            sos = butter_sos(1, 4.0*freqs[c][j], 'lowpass', RATE)
            assert np.array_equal(t.sos[k], sos)
            ref, q = rd.filtfilt_case(sos, x[a:b, c:c + 1].astype(np.float32))
            ib.assert_within(got[a:b, c:c + 1], ref, q, 'channel %d, event %d' % (c, j), first=0)
            mask[a:b, c] = False
            k += 1
    assert np.array_equal(got[mask], x[mask])
    assert np.array_equal(np.asarray(g['envelope'].buffer), x)
    assert t.regions[0, 1] == 0                                            # the song at the very start: clipped at 0


def test_region_filtfilt_splits_a_long_table():
    """BufferedData.region_filtfilt with a max_scratch that forces three calls gives the bytes of one call; out=None
    leaves the trace as it is."""
    from audian_amd import hipdsp
    g, ev, freqs = scene()
    e = g['envelope']
    t = filtered(g, ev, freqs)
    regions, sos = t.regions, t.sos
    assert e._dev is not None
    before = hipdsp.launches.get('region_filtfilt', 0)
    one = e.region_filtfilt(regions, sos)
    assert hipdsp.launches['region_filtfilt'] == before + 1
    sizes = [hipdsp.region_filtfilt_scratch(regions[k:k + 3], sos[k:k + 3]) for k in (0, 3, 6)]
    limit = max(sizes)
    assert limit < hipdsp.region_filtfilt_scratch(regions[0:4], sos[0:4])
    three = e.region_filtfilt(regions, sos, max_scratch=limit)
    calls = hipdsp.launches['region_filtfilt'] - before - 1
    assert calls == 3
    assert len(one) == len(three) == 9
    for (c, a, b), p, q in zip(regions.tolist(), one, three):
        assert p.dtype == np.float32 and p.shape == (b - a,) and p.tobytes() == q.tobytes()
    assert np.array_equal(np.asarray(e.buffer), envelope())
    # the clamp, and what the trace itself holds
    got = np.asarray(t.buffer)
    for (c, a, b), p in zip(regions.tolist(), one):
        assert np.array_equal(got[a:b, c], p.astype(np.float64))
    with pytest.raises(ValueError, match='overlap'):
        e.region_filtfilt([(0, 0, 100), (0, 50, 200)], sos[:2])
    with pytest.raises(ValueError, match='padlen'):
        e.region_filtfilt([(0, 0, 6)], sos[:1])


def test_refine_events_on_the_mirror():
    """Two hipdsp_region_crossings calls -- the maxima of all noise windows, then the borders of all widened events --
    give exactly what the sequential definition gives on the filtered trace; the new borders lie at the songs."""
    from audian_amd import hipdsp
    g, ev, freqs = scene()
    t = filtered(g, ev, freqs)
    clean, cf = g.clean_event_freqs(ev, freqs)
    assert len(clean) == 9
    before = hipdsp.launches.get('region_crossings', 0)
    stale = [list(r) for r in t._stale]
    new = g.refine_events(clean, cf, 0.2, 'eventfiltered', min_duration=MIN_DURATION, min_thresh_fac=1.0)
    assert hipdsp.launches['region_crossings'] == before + 2
    assert [list(r) for r in t._stale] == stale                             # nothing crossed to the host
    env = np.asarray(t.buffer)
    w = int(MIN_DURATION*RATE)
    for c in range(C):
        want = rd.refine(clean.onsets[c], clean.offsets[c], cf[c], env[:, c], 0.2, w, 1.0)
        assert new.frames(c).tolist() == [list(p) for p in want]
        assert len(want) == 3
        for (a, b), (t0, t1, f) in zip(want, SONGS[c]):
            assert abs(a - t0*RATE) <= 0.05*RATE and abs(b - t1*RATE) <= 0.05*RATE
    # one event without a frequency is dropped, and a factor that lifts the threshold over every sample drops all
    cf2 = [f.copy() for f in cf]
    cf2[1][1] = np.nan
    assert [len(o) for o in g.refine_events(clean, cf2, 0.2, 'eventfiltered', MIN_DURATION).onsets] == [3, 2, 3]
    assert len(g.refine_events(clean, cf, 0.2, 'eventfiltered', MIN_DURATION, min_thresh_fac=100.0)) == 0
    # region_crossings of the trace against the definition, positions absolute
    regions = [(0, 0, 5000), (2, 9000, 14000), (1, 3999, 4001)]
    got = t.region_crossings(regions, [0.3, 0.1, np.nan])
    for row, (c, a, b), thr in zip(got, regions, [0.3, 0.1, np.nan]):
        assert np.array_equal(row, rd.region_crossings(env[:, c].astype(np.float32), a, b, thr), equal_nan=True)


def test_regions_on_the_buffer_border_are_skipped_on_the_mirror():
    g, ev, freqs = scene()
    h = make_graph(25.0)
    h.update_times(0.0, 25.0)
    t = h['eventfiltered']
    t.set_events(ev, freqs, MIN_DURATION)
    lo, hi = t.offset, t.offset + len(t._hostbuf)
    assert lo == 0 and 20.0*RATE < hi < 30.0*RATE and t._dev is not None
    inside = [r for r in t.regions.tolist() if r[2] <= hi]
    assert len(inside) == 6 and t.skipped == []
    h.update_times(5.8, 30.8)                                              # cuts channel 2's first and channel 0's last song
    lo, hi = t.offset, t.offset + len(t._hostbuf)
    cut = [tuple(r) for r in t.regions.tolist() if r[1] < hi and r[2] > lo and not (r[1] >= lo and r[2] <= hi)]
    assert len(cut) == 2 and t.skipped == cut
    x = envelope()
    got = np.asarray(t.buffer)
    whole = np.asarray(filtered(g, ev, freqs).buffer)
    for c, a, b in cut:
        a2, b2 = max(a, lo), min(b, hi)
        assert np.array_equal(got[a2 - lo:b2 - lo, c], x[a2:b2, c])        # unfiltered
    for c, a, b in t.regions.tolist():
        if a >= lo and b <= hi:
            assert np.array_equal(got[a - lo:b - lo, c], whole[a:b, c])      # the same bytes wherever the buffer lies
