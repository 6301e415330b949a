"""Spectral contour features on the host: the definition (tests/spectral_features_definition.py) against the golden file
made with numpy's library functions, its array form against its loops, the float64 term of the bound on every input
of the GPU tests, the package's numpy path against the definition, the frame/event mapping and every field of Contours
on a hand-made feature table, ContourAnalyzer, the refusals before any launch, the binding's signature, units and
ranges, set_band / update on a host-only graph, and the interpolation against pure tones.  No GPU."""

import ctypes
import os
import re
from math import ceil

import numpy as np
import pytest

import spectral_features_definition as sd
from audian_amd import hipdsp
from audian_amd.analyzer import ContourAnalyzer
from audian_amd.bufferedarray import ArrayLoader
from audian_amd.bufferedspectralfeature import BufferedSpectralFeature, host_spectral_features
from audian_amd.bufferedspectrogram import BufferedSpectrogram, band_bins
from audian_amd.contours import CONTOUR_FEATURES, FIELDS, Contours, centre_frames, frame_table
from audian_amd.events import Events
from audian_amd.tracegraph import TraceGraph

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'spectral_features.npz')


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def host_spectrogram(oracle):
    class OSpectrogram(BufferedSpectrogram):
        """The facade's bookkeeping, computed on the host: no device mirror anywhere in the graph.  The bins are
        rounded to float32, what a device spectrogram holds and what the definition takes."""

        def process(self, source, dest, nbefore):
            self._pending = None
            oracle.spectrogram_process(np.asarray(source), dest, self.source.rate, self.nfft, self.hop)
            dest[...] = dest.astype(np.float32)

    return OSpectrogram


def test_definition_against_numpy_golden():
    g = np.load(GOLDEN)
    spec, scale, floor, ratio = g['spec'], float(g['scale']), float(g['min_power']), float(g['ratio'])
    seen_nan = seen_value = 0
    for (k0, k1), want in zip(g['bands'].tolist(), g['values']):
        V, T = sd.slab_features(spec, k0, k1, scale, floor, ratio)
        V64 = V.astype(np.float64)
        assert np.array_equal(np.isnan(V64), np.isnan(want)) and np.array_equal(np.isinf(V64), np.isinf(want)), (k0, k1)
        ok = np.isfinite(want)
        # numpy's float64 sums of at most 97 terms, its log, exp and sqrt: 2^-44 relative is generous and pins every formula
        assert np.all(np.abs(V64[ok] - want[ok]) <= 2.0**-44*np.maximum(np.abs(want[ok]), scale)), (k0, k1)
        for bit in sd.EXACT_BITS:
            assert np.array_equal(V64[bit][ok[bit]], want[bit][ok[bit]])
        seen_nan += int((~ok).sum())
        seen_value += int(ok.sum())
    assert seen_nan > 500 and seen_value > 1000


def test_array_form_of_the_definition_equals_its_loops():
    for F, k0, k1 in ((97, 10, 75), (97, 0, 97), (40, 7, 8), (300, 250, 300)):
        spec = sd.family_slab(F, len(sd.FAMILIES), 2, k0, k1, 5)
        for floor, ratio in ((0.0, 0.1), (1e-7, 1.0), (0.5, 1e-6)):
            V, T = sd.slab_features(spec, k0, k1, 3.5, floor, ratio)
            for c in range(spec.shape[0]):
                for t in range(spec.shape[1]):
                    v, tt = sd.row_features(spec[c, t], k0, k1, 3.5, floor, ratio)
                    a, b = np.array([float(x) for x in v]), V[:, c, t].astype(np.float64)
                    assert np.array_equal(np.isnan(a), np.isnan(b)), (F, k0, k1, c, t)
                    ok = np.isfinite(a)
                    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.allclose(a[ok], b[ok], rtol=2.0**-50, atol=0)
                    assert np.allclose(np.array(tt), T[:, c, t], rtol=1e-6, atol=0), (F, k0, k1, c, t)


def test_gpu_inputs_keep_the_float64_term_small_and_numpy_float64_is_inside_the_bound():
    """On every slab and band the GPU tests judge: T < 2^-30 of the value (of one bin where a frequency is smaller),
    finite everywhere, and the package's numpy path -- a float64 restatement with numpy's own summation order -- inside
    the bound.  Its worst |error| / allowed measured 0.9992: the float32 rounding of the result, which the bound grants
    in full, is all that shows; the float64 term stayed below 0.61 of its limit."""
    worst_term = worst_host = 0.0
    cases = 0
    for label, spec, k0, k1 in sd.gpu_cases():
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, 0.0, 0.1)
        assert np.all(np.isfinite(T)), label
        ref = sd.term_scale(V, sd.SCALE)
        ok = np.isfinite(V.astype(np.float64)) & (ref > 0)
        if ok.any():
            worst_term = max(worst_term, float((T[ok]/ref[ok]).max()))
        assert worst_term < sd.T_LIMIT, label
        got = host_spectral_features(spec, k0, k1, sd.ALL, sd.SCALE, 0.0, 10.0)
        worst_host = max(worst_host, sd.compare(got, V, T, sd.ALL, label))
        cases += 1
    assert cases > 150 and 0.5 < worst_host <= 1.0
    print('worst T / 2^-30: %.4f, worst host |error| / allowed: %.4f' % (worst_term/sd.T_LIMIT, worst_host))


def test_numpy_path_masks_and_selections():
    spec = sd.family_slab(97, 24, 2, 10, 75, 1)
    V, T = sd.slab_features(spec, 10, 75, 2.0, 1e-7, sd.drop_ratio(20.0))
    full = host_spectral_features(spec, 10, 75, sd.ALL, 2.0, 1e-7, 20.0)
    sd.compare(full, V, T, sd.ALL, 'all bits')
    for names in (('peak_freq',), ('flatness', 'peak_bin_freq'), ('freq_high', 'freq_low', 'centroid')):
        mask = hipdsp.feature_mask(names)
        got = host_spectral_features(spec, 10, 75, names, 2.0, 1e-7, 20.0)
        assert hipdsp.feature_names(mask) == tuple(n for n in sd.NAMES if n in names)
        assert np.array_equal(got, full[sd.bits_of(mask)], equal_nan=True)
    empty = host_spectral_features(spec, 30, 30, sd.ALL, 2.0)
    assert empty.shape == (8, 2, 24) and np.all(np.isnan(empty))
    assert host_spectral_features(spec[:, :0], 10, 75, 0x05, 2.0).shape == (2, 2, 0)
    assert hipdsp.SPECTRAL_FEATURES == sd.NAMES and hipdsp.feature_mask(0xFF) == 0xFF
    assert hipdsp.drop_ratio(10.0) == sd.drop_ratio(10.0) == 0.1


def test_frames_of_an_event():
    """An event [t_on, t_off) owns the frames whose centre (t*hop + nfft/2)/rate lies in it."""
    rate, nfft, hop, N = 1000.0, 100, 50, 40                             # centres at 0.05, 0.10, 0.15, ... s
    assert centre_frames(0.0, 0.05, rate, nfft, hop, N) == (0, 0)        # the centre of frame 0 is not < 0.05
    assert centre_frames(0.0, 0.051, rate, nfft, hop, N) == (0, 1)
    assert centre_frames(0.05, 0.15, rate, nfft, hop, N) == (0, 2)       # 0.05 is in, 0.15 is out
    assert centre_frames(0.051, 0.151, rate, nfft, hop, N) == (1, 3)
    assert centre_frames(0.26, 0.29, rate, nfft, hop, N) == (5, 5)       # between two centres: no frame
    assert centre_frames(1.9, 5.0, rate, nfft, hop, N) == (37, 40)       # clipped to the spectrogram
    assert centre_frames(-1.0, 0.11, rate, nfft, hop, N) == (0, 2)
    assert centre_frames(7.0, 8.0, rate, nfft, hop, N) == (40, 40)
    for t_on, t_off in ((0.123, 0.987), (0.3, 0.3), (0.049999, 1.000001)):
        a, b = centre_frames(t_on, t_off, rate, nfft, hop, N)
        want = [t for t in range(N) if t_on <= (t*hop + nfft/2)/rate < t_off]
        assert list(range(a, b)) == want
    tab = frame_table([(2, 0.05, 0.15), (0, 0.26, 0.29)], rate, nfft, hop, N)
    assert tab.dtype == np.int64 and tab.tolist() == [[2, 0, 2], [0, 5, 5]]
    assert frame_table([], rate, nfft, hop, N).shape == (0, 3)


def hand_made_features():
    nan = np.nan
    m, C = 12, 2
    f = {name: np.full((m, C), nan) for name in CONTOUR_FEATURES}
    # channel 1, frames 102 ... 108 (first = 100): masked, 1000, 1500, masked, 1400, 2000, masked
    rows = {2: (1000.0, 2.0, 1100.0, 50.0, 0.2, 900.0, 1200.0), 3: (1500.0, 6.0, 1450.0, 80.0, 0.4, 1300.0, 1600.0),
            5: (1400.0, 6.0, 1500.0, 20.0, 0.1, 800.0, 1450.0), 6: (2000.0, 1.0, 1900.0, 10.0, 0.9, 1950.0, 2600.0)}
    for t, values in rows.items():
        for name, v in zip(CONTOUR_FEATURES, values):
            f[name][t, 1] = v
    for t in range(m):                                                  # masked frames keep their peak power
        if np.isnan(f['peak_power'][t, 1]):
            f['peak_power'][t, 1] = 1e-25
    f['peak_power'][:, 0] = 0.0
    return f


def test_every_field_of_contours_on_a_hand_made_table():
    f = hand_made_features()
    table = [(1, 101, 108), (0, 100, 112), (1, 104, 105), (1, 103, 103), (1, 105, 107)]
    c = Contours(table, 100, f, t0=0.05, dt=0.01, trace_name='spectrogram')
    assert len(c) == 5 and c.table.tolist() == [list(r) for r in table] and c.trace_name == 'spectrogram'
    assert c.n_frames.tolist() == [7, 12, 1, 0, 2] and c.n_frames.dtype == np.int64
    assert np.allclose(c.voiced, [4/7, 0, 0, 0, 1.0])
    # event 0: four unmasked frames
    assert (c.start_freq[0], c.end_freq[0], c.min_freq[0], c.max_freq[0]) == (1000.0, 2000.0, 1000.0, 2000.0)
    assert c.peak_freq[0] == 1500.0                                      # powers 2, 6, 6, 1: the first of the largest
    assert (c.low_freq[0], c.high_freq[0]) == (800.0, 2600.0)
    w = np.array([2.0, 6.0, 6.0, 1.0])
    assert c.centroid[0] == np.sum(w*[1100.0, 1450.0, 1500.0, 1900.0])/15.0
    assert c.bandwidth[0] == np.sum(w*[50.0, 80.0, 20.0, 10.0])/15.0
    assert abs(c.flatness[0] - np.sum(w*[0.2, 0.4, 0.1, 0.9])/15.0) < 1e-15
    # events without an unmasked frame: a silent channel, one masked frame, no frame at all
    for i in (1, 2, 3):
        assert c.voiced[i] == 0 and all(np.isnan(getattr(c, name)[i]) for name in FIELDS[:10]), i
    # event 4: frames 105, 106
    assert c.row(4) == [1400.0, 2000.0, 1400.0, 2000.0, 1400.0, 800.0, 2600.0, (6*1500.0 + 1900.0)/7, (6*20.0 + 10.0)/7,
                        (6*0.1 + 0.9)/7, 2, 1.0]
    assert len(c.row(0)) == len(FIELDS) == 12
    t, pf = c.contour(0)
    assert np.allclose(t, 0.05 + 0.01*np.arange(101, 108)) and np.array_equal(pf, f['peak_freq'][1:8, 1], equal_nan=True)
    t, pf = c.contour(3)
    assert len(t) == 0 and len(pf) == 0
    assert len(Contours([], 100, f)) == 0


def sweep_recording(rate, seconds=4.0):
    """Channel 0: an up-sweep 1000 -> 3000 Hz between 1 s and 2 s; channel 1: the same sweep a hundred times weaker
    between 2.5 s and 3 s; faint noise everywhere."""
    rng = np.random.default_rng(8)
    n = int(rate*seconds)
    t = np.arange(n)/rate
    x = 1e-4*rng.standard_normal((n, 2))
    on = (t >= 1.0) & (t < 2.0)
    x[on, 0] += 0.5*np.sin(2*np.pi*(1000.0*(t[on] - 1.0) + 1000.0*(t[on] - 1.0)**2))
    on = (t >= 2.5) & (t < 3.0)
    x[on, 1] += 0.005*np.sin(2*np.pi*(1000.0*(t[on] - 2.5) + 2000.0*(t[on] - 2.5)**2))
    return x


def host_graph(oracle, x, rate, nfft=256, **feature):
    g = TraceGraph(10.0, 2.0)
    s = host_spectrogram(oracle)(source='data', nfft=nfft)
    t = BufferedSpectralFeature(**feature)
    g.add_trace(s)
    g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g.update_times(0.0, 4.0)
    return g, s, t


def test_trace_on_a_host_only_graph_recomputes_itself_and_not_its_source(oracle):
    rate = 16000.0
    x = sweep_recording(rate)
    g, s, t = host_graph(oracle, x, rate, fmin=500.0, fmax=6000.0, min_power=1e-10)
    assert [tr.name for tr in g.traces] == ['data', 'spectrogram', 'peakfreq'] and t._dev is None and s._dev is None

    def check():
        assert (t.rate, t.frames, t.offset, len(t.buffer)) == (s.rate, s.frames, s.offset, len(s.buffer))
        assert (t.k0, t.k1) == band_bins(t.fmin, t.fmax, s.fresolution, s.nfft//2 + 1) and t.scale == s.fresolution
        slab = np.asarray(s.buffer).transpose(1, 0, 2).astype(np.float32)
        V, T = sd.slab_features(slab, t.k0, t.k1, t.scale, t.min_power, sd.drop_ratio(t.drop_db))
        bit = sd.NAMES.index(t.feature)
        got = np.asarray(t.buffer).T.astype(np.float32)[None]
        assert np.array_equal(got[0].astype(np.float64), np.asarray(t.buffer).T, equal_nan=True)   # float32 values
        sd.compare(got, V, T, 1 << bit, t.feature)
        return np.asarray(t.buffer)

    pf = check()
    frames = np.arange(len(pf))
    centre = (frames*s.hop + s.nfft/2)/rate
    inside = (centre > 1.05) & (centre < 1.95)
    assert not np.any(np.isnan(pf[inside, 0])) and np.all(np.isnan(pf[centre < 0.9, 0])) and np.all(np.isnan(pf[centre > 2.1, 0]))
    want = 1000.0 + 2000.0*(centre[inside] - 1.0)
    assert np.all(np.abs(pf[inside, 0] - want) < s.fresolution)         # the contour follows the sweep within a bin
    calls = []
    real = s.process
    s.process = lambda *a: (calls.append(1), real(*a))
    t.set_band(1500.0, 2500.0)
    got = check()
    assert not calls and np.nanmin(got) >= 1500.0 and np.nanmax(got) <= 2500.0
    t.set_band(500.0, 6000.0)
    for feature in hipdsp.SPECTRAL_FEATURES:
        t.update(feature=feature)
        check()
    t.update(feature='freq_low', drop_db=3.0, min_power=1e-6)
    assert (t.feature, t.drop_db, t.min_power) == ('freq_low', 3.0, 1e-6)
    got = check()
    assert np.all(np.isnan(got[:, 1]))                                   # the weak sweep is below this floor
    assert not calls
    # refusals change nothing and compute nothing
    process_calls = []
    real_t = t.process
    t.process = lambda *a: (process_calls.append(1), real_t(*a))
    for kw in (dict(feature='peak'), dict(feature=None, drop_db=-0.5), dict(feature=3), dict(drop_db=float('nan'))):
        with pytest.raises(ValueError):
            t.update(**kw)
    assert (t.feature, t.drop_db, t.min_power) == ('freq_low', 3.0, 1e-6) and not process_calls and not calls
    # a scroll and a change of the spectrogram's window carry through
    g.update_times(1.0, 3.5)
    check()
    s.update(nfft=512, overlap_frac=0.75)
    assert calls and t.rate == rate/128 and t.frames == ceil(len(x)/128)
    check()


def test_units_ranges_and_constructor_refusals(oracle):
    src = ArrayLoader(np.zeros((100000, 3)), 48000.0, buffer_time=1.0, back_time=0.0, unit='V', ampl_max=2.0)
    s = host_spectrogram(oracle)(source='data', nfft=512)
    s.open(src)
    t = BufferedSpectralFeature(fmin=4000.0, fmax=6000.0)
    t.open(s)
    assert t.source is s and t in s.dests and t.shape == (s.frames, 3) and t.rate == s.rate == 48000.0/256
    assert (t.name, t.source_name, t.panel, t.panel_type, t.feature) == ('peakfreq', 'spectrogram', 'spectrogram', 'trace', 'peak_freq')
    assert (t.min_power, t.drop_db, t.fmin, t.fmax) == (1e-20, 10.0, 4000.0, 6000.0)
    assert (t.k0, t.k1) == band_bins(4000.0, 6000.0, 48000.0/512, 257) and t.scale == 48000.0/512
    for feature in ('peak_bin_freq', 'peak_freq', 'centroid', 'bandwidth', 'freq_low', 'freq_high'):
        t.feature = feature
        t._set_range()
        assert (t.unit, t.ampl_min, t.ampl_max) == ('Hz', 0, 24000.0) == ('Hz', s.ampl_min, s.ampl_max)
    t.feature = 'peak_power'
    t._set_range()
    assert t.unit == s.unit == 'V^2/Hz' and t.ampl_min == 0 and t.ampl_max == 4.0/(48000.0/512)
    t.feature = 'flatness'
    t._set_range()
    assert (t.unit, t.ampl_min, t.ampl_max) == ('', 0, 1)
    for kw in (dict(feature='entropy'), dict(drop_db=-1.0), dict(feature=('peak_freq',))):
        with pytest.raises(ValueError):
            BufferedSpectralFeature(**kw)
    with pytest.raises(ValueError):
        hipdsp.feature_mask(('peak_freq', 'peek'))
    for bad in ((), 0, 256, -1):
        with pytest.raises(ValueError):
            hipdsp.feature_mask(bad)
    with pytest.raises(ValueError):
        hipdsp.spectral_features(None, None, 0, 1, 1, 9, 0, 9, ('peak_freq',), 1.0, None, drop_db=-3.0)   # before any launch


def test_spectrogram_features_event_contours_and_the_analyzer_on_a_host_graph(oracle):
    rate = 16000.0
    x = sweep_recording(rate)
    g, s, t = host_graph(oracle, x, rate)
    n = len(s.buffer)
    feats = s.spectral_features(s.offset + 3, s.offset + n - 2, 500.0, 6000.0, ('centroid', 'peak_freq', 'flatness'),
                                min_power=1e-10, drop_db=6.0)
    assert list(feats) == ['peak_freq', 'centroid', 'flatness']           # bit order
    k0, k1 = band_bins(500.0, 6000.0, s.fresolution, 129)
    slab = np.asarray(s.buffer)[3:n - 2].transpose(1, 0, 2).astype(np.float32)
    V, T = sd.slab_features(slab, k0, k1, s.fresolution, 1e-10, sd.drop_ratio(6.0))
    got = np.stack([feats[name].T for name in feats])
    assert got.dtype == np.float32 and got.shape == (3, 2, n - 5)
    sd.compare(got, V, T, 0x2A, 'BufferedSpectrogram.spectral_features')
    assert s.spectral_features(s.offset, s.offset, features=('peak_power',))['peak_power'].shape == (0, 2)
    with pytest.raises(IndexError):
        s.spectral_features(s.offset - 1, s.offset + 2)
    with pytest.raises(ValueError):
        s.spectral_features(s.offset, s.offset + 2, features=('nothing',))
    with pytest.raises(ValueError):
        s.spectral_features(s.offset, s.offset + 2, drop_db=-1.0)
    # events at the rate of the raw data: the sweep, silence on the same channel, the weak sweep, silence
    ev = Events([[(16000, 32000), (40000, 48000)], [(40000, 48000), (8000, 12000)]], rate, 'data')
    c = g.event_contours(ev, fmin=500.0, fmax=6000.0, min_power=1e-10)
    assert len(c) == 4 and c.table[:, 0].tolist() == [0, 0, 1, 1]
    for i, (ch, a, b) in enumerate([(0, 16000, 32000), (0, 40000, 48000), (1, 40000, 48000), (1, 8000, 12000)]):
        want = [k for k in range(s.frames) if a/rate <= (k*s.hop + s.nfft/2)/rate < b/rate]
        assert c.table[i].tolist() == [ch, want[0], want[-1] + 1] and c.n_frames[i] == len(want)
    assert c.voiced[0] > 0.95 and abs(c.start_freq[0] - 1000.0) < 2*s.fresolution and abs(c.end_freq[0] - 3000.0) < 2*s.fresolution
    assert c.start_freq[0] < c.end_freq[0] and c.min_freq[0] <= c.start_freq[0] and c.max_freq[0] >= c.end_freq[0]
    assert c.low_freq[0] <= c.min_freq[0] and c.high_freq[0] >= c.max_freq[0] and 1000.0 < c.centroid[0] < 3000.0
    assert c.flatness[0] < 0.05 and c.bandwidth[0] < 10*s.fresolution
    for i in (1, 3):
        assert c.voiced[i] == 0 and all(np.isnan(getattr(c, name)[i]) for name in FIELDS[:10])
    assert 0.9 < c.voiced[2] <= 1.0 and abs(c.start_freq[2] - 1000.0) < 2*s.fresolution and c.end_freq[2] > 2500.0
    times, pf = c.contour(0)
    assert np.all(np.abs(pf[3:-3] - (1000.0 + 2000.0*(times[3:-3] - 1.0))) < s.fresolution)
    # the fields against the definition applied to the spectrogram's buffer
    a, b = int(c.table[0, 1]), int(c.table[0, 2])
    slab = np.asarray(s.buffer)[a - s.offset:b - s.offset, 0][None].astype(np.float32)
    V, T = sd.slab_features(slab, k0, k1, s.fresolution, 1e-10, 0.1)
    assert abs(c.max_freq[0] - np.nanmax(V[1].astype(np.float64))) <= 2.0**-23*c.max_freq[0]
    assert c.high_freq[0] == np.float32(np.nanmax(V[7].astype(np.float64)))
    # the analyzer: one row per event, through analyze_events and analyze_region
    an = ContourAnalyzer(g, 'spectrogram', fmin=500.0, fmax=6000.0, min_power=1e-10)
    assert an.data.labels == [name.replace('_', ' ') for name in FIELDS] and an.data.units[0] == 'Hz' and an.data.units[9] == ''
    g.analyze_events(ev)
    rows = an.rows()
    assert len(rows) == 4
    for c_, regions in ((0, ev.regions(0)), (1, ev.regions(1))):
        want = g.region_contours([(c_, t0, t1) for t0, t1 in regions], fmin=500.0, fmax=6000.0, min_power=1e-10)
        for i in range(len(want)):
            assert np.array_equal(np.array(rows.pop(0), dtype=np.float64), np.array(want.row(i), dtype=np.float64), equal_nan=True)
    an.clear()
    g.analyze_region(1.0, 2.0, 0)
    one = g.region_contours([(0, 1.0, 2.0)], fmin=500.0, fmax=6000.0, min_power=1e-10)
    assert np.array_equal(np.array(an.rows()[0]), np.array(one.row(0)), equal_nan=True) and one.start_freq[0] < one.end_freq[0]
    with pytest.raises(ValueError):
        ContourAnalyzer(g, 'spectrogram', drop_db=-2.0)


def test_interpolated_peak_on_hann_frames_of_pure_tones(oracle):
    """float32 Hann frames of a pure tone at nfft 256, bins 5 ... 100, offsets -0.5 ... 0.5 bin in steps of 0.05, three
    phases: |PEAK_FREQ - f0| <= 0.02 bin everywhere, and strictly smaller than |kp - f0/df| for offsets of at least 0.1
    bin -- a flipped sign of d fails both.  The float64 definition measured 0.0163 bin: the bias of log-parabolic
    interpolation under a Hann window; the cap is that figure plus a fifth."""
    nfft, rate = 256, 256.0                                              # df = 1: frequencies are bins
    bins, offsets, phases = np.arange(5, 101), np.round(np.arange(-0.5, 0.5001, 0.05), 2), (0.0, 1.0, 2.5)
    f0 = np.array([k + o for k in bins for o in offsets for p in phases])
    off = np.array([o for k in bins for o in offsets for p in phases])
    ph = np.array([p for k in bins for o in offsets for p in phases])
    t = np.arange(nfft)
    x = np.sin(2*np.pi*f0[None, :]*t[:, None]/nfft + ph[None, :]).astype(np.float32)
    freqs, times, Sxx = oracle.spectrogram_numpy(x.astype(np.float64), rate, nfft, 0)
    assert Sxx.shape == (129, 1, len(f0))
    spec = np.ascontiguousarray(Sxx[:, 0, :].T).astype(np.float32)[None]      # (1, tones, 129)
    V, T = sd.slab_features(spec, 0, 129, 1.0, 0.0, 0.1)
    kp, pf = V[0, 0].astype(np.float64), V[1, 0].astype(np.float64)
    err = np.abs(pf - f0)
    print('worst |PEAK_FREQ - f0|: %.4f bin' % err.max())
    assert err.max() <= 0.02
    far = np.abs(off) >= 0.1
    assert np.all(err[far] < np.abs(kp - f0)[far])
    got = host_spectral_features(spec, 0, 129, ('peak_freq',), 1.0)
    assert np.all(np.abs(got[0, 0] - f0) <= 0.02 + 2.0**-17)


def test_the_binding_declares_the_entry():
    from audian_amd import _lib
    i64, vp, dbl = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    args, res = _lib._SIGNATURES['hipdsp_spectral_features']
    assert args == [vp, vp, i64, i64, i64, i64, i64, i64, ctypes.c_uint, dbl, dbl, dbl, vp, i64, i64]
    assert res is ctypes.c_int and _lib.lib.hipdsp_spectral_features.argtypes == args
    header = open(os.path.join(HERE, '..', 'include', 'hip_dsp.h')).read()
    proto = re.search(r'int hipdsp_spectral_features\(([^;]*)\);', header).group(1)
    kinds = [re.sub(r'\s*\w+$', '', a.strip()) for a in proto.replace('\n', ' ').split(',')]
    assert kinds == ['hipdsp_ctx *', 'const float *', 'int64_t', 'int64_t', 'int64_t', 'int64_t', 'int64_t', 'int64_t',
                     'unsigned', 'double', 'double', 'double', 'float *', 'int64_t', 'int64_t']
    for bit, name in enumerate(sd.NAMES):
        assert re.search(r'#define HIPDSP_FEATURE_%s %du\b' % (name.upper(), 1 << bit), header), name
