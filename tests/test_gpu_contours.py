"""BufferedSpectralFeature, BufferedSpectrogram.spectral_features, TraceGraph.event_contours and ContourAnalyzer on the
GPU: the trace's buffer against tests/spectral_features_definition.py applied to the spectrogram's mirror read back,
what a move of the band costs in launches, what a scroll keeps, and the contours of synthetic sweeps."""

import numpy as np
import pytest

import spectral_features_definition as sd

pytestmark = pytest.mark.gpu

RATE = 16000.0


class Item:
    def isVisible(self):
        return True


def recording(seconds=20.0):
    """Channel 0: an up-sweep 1000 -> 3000 Hz in the first second of every 2 s; channel 1: faint noise only."""
    rng = np.random.default_rng(4)
    n = int(RATE*seconds)
    t = np.arange(n)/RATE
    x = 1e-4*rng.standard_normal((n, 2))
    tau = np.mod(t, 2.0)
    on = tau < 1.0
    x[on, 0] += 0.5*np.sin(2*np.pi*(1000.0*tau[on] + 1000.0*tau[on]**2))
    return x.astype(np.float32).astype(np.float64)


def graph(x, **feature):
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedspectralfeature import BufferedSpectralFeature
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(4.0, 1.0)
    g.add_trace(BufferedSpectrogram(source='data', nfft=256))
    g.add_trace(BufferedSpectralFeature(**feature))
    g.setup_traces()
    g.open(x, RATE)
    for t in g.traces:
        t.plot_items = [Item() for _ in range(t.channels)]
    g.set_need_update()
    return g


def check(g):
    """The trace's buffer against the definition on the spectrogram's own frames."""
    s, t = g['spectrogram'], g['peakfreq']
    assert (t.rate, t.frames, t.offset, len(t.buffer)) == (s.rate, s.frames, s.offset, len(s.buffer))
    slab = np.array(s.buffer).transpose(1, 0, 2)
    assert np.array_equal(slab, slab.astype(np.float32))
    V, T = sd.slab_features(slab.astype(np.float32), t.k0, t.k1, t.scale, t.min_power, sd.drop_ratio(t.drop_db))
    got = np.array(t.buffer).T
    assert np.array_equal(got, got.astype(np.float32), equal_nan=True)
    sd.compare(got.astype(np.float32)[None], V, T, 1 << sd.NAMES.index(t.feature), t.feature)
    return np.array(t.buffer)


def test_trace_walk_launches_and_scroll():
    from audian_amd import hipdsp
    x = recording()
    g = graph(x, fmin=500.0, fmax=6000.0, min_power=1e-10)
    s, t = g['spectrogram'], g['peakfreq']
    before = dict(hipdsp.launches)
    g.update_times(0.0, 2.0)
    assert hipdsp.launches['spectral_features'] >= before.get('spectral_features', 0) + 1
    assert t._dev is not None and t._stale                               # computed on the mirror, nothing read back yet
    pf = check(g)
    centre = ((t.offset + np.arange(len(pf)))*s.hop + s.nfft/2)/RATE
    inside = (np.mod(centre, 2.0) > 0.05) & (np.mod(centre, 2.0) < 0.95)
    assert not np.any(np.isnan(pf[inside, 0])) and np.all(np.isnan(pf[:, 1]))
    assert np.all(np.abs(pf[inside, 0] - (1000.0 + 2000.0*np.mod(centre[inside], 2.0))) < s.fresolution)
    # a scroll keeps the values that stay in the buffer and computes only the rest
    kept = {t.offset + i: pf[i].copy() for i in range(len(pf))}
    for t0, t1 in [(1.0, 3.0), (5.5, 7.5), (6.0, 8.5), (18.0, 20.0)]:
        before = dict(hipdsp.launches)
        g.update_times(t0, t1)
        assert hipdsp.launches['spectral_features'] <= before['spectral_features'] + 1
        now = check(g)
        for i in range(len(now)):
            if t.offset + i in kept:
                assert np.array_equal(now[i], kept[t.offset + i], equal_nan=True)
        kept = {t.offset + i: now[i].copy() for i in range(len(now))}
    # moving the band, the feature, the floor: one launch each, the spectrogram is neither computed nor read back
    g.update_times(4.0, 6.0)
    assert s._stale
    for change in (lambda: t.set_band(1500.0, 2500.0), lambda: t.set_band(0.0, None), lambda: t.update(feature='centroid'),
                   lambda: t.update(feature='flatness'), lambda: t.update(feature='freq_high', drop_db=3.0),
                   lambda: t.update(feature='peak_freq', min_power=1e-3, drop_db=10.0), lambda: t.set_band(3000.0, 1000.0)):
        stale, before = [list(r) for r in s._stale], dict(hipdsp.launches)
        change()
        after = dict(hipdsp.launches)
        assert after['spectral_features'] == before['spectral_features'] + 1
        assert all(after.get(k, 0) == before.get(k, 0) for k in ('spectrogram', 'chain_forward', 'unpack_spectrum', 'pack'))
        assert s._stale == stale
    assert t.k0 == t.k1 and np.all(np.isnan(np.array(t.buffer)))        # an empty band: no contour
    t.set_band(500.0, 6000.0)
    t.update(min_power=1e-10)
    check(g)
    with pytest.raises(ValueError):
        t.update(feature='peak')
    with pytest.raises(ValueError):
        t.update(drop_db=-1.0)


def test_spectrogram_features_in_one_launch():
    from audian_amd import hipdsp
    from audian_amd.bufferedspectrogram import band_bins
    x = recording(6.0)
    g = graph(x)
    g.update_times(0.0, 3.0)
    s = g['spectrogram']
    n = len(s.buffer)
    assert s._stale == [[0, n]]
    i0, i1 = s.offset + 2, s.offset + n - 1
    before = dict(hipdsp.launches)
    feats = s.spectral_features(i0, i1, 500.0, 6000.0, hipdsp.SPECTRAL_FEATURES, min_power=1e-10, drop_db=6.0)
    assert hipdsp.launches['spectral_features'] == before['spectral_features'] + 1      # ONE launch for all eight
    assert s._stale == [[0, n]]                                          # nothing of the spectrogram was read back
    assert tuple(feats) == sd.NAMES and all(v.shape == (i1 - i0, 2) and v.dtype == np.float32 for v in feats.values())
    k0, k1 = band_bins(500.0, 6000.0, s.fresolution, 129)
    slab = np.array(s.buffer)[2:n - 1].transpose(1, 0, 2).astype(np.float32)
    V, T = sd.slab_features(slab, k0, k1, s.fresolution, 1e-10, sd.drop_ratio(6.0))
    got = np.stack([feats[name].T for name in sd.NAMES])
    sd.compare(got, V, T, sd.ALL, 'device')
    s._dev_valid = []                                                    # without a mirror numpy serves, inside the same bound
    host = s.spectral_features(i0, i1, 500.0, 6000.0, hipdsp.SPECTRAL_FEATURES, min_power=1e-10, drop_db=6.0)
    sd.compare(np.stack([host[name].T for name in sd.NAMES]), V, T, sd.ALL, 'host')
    for bit in sd.EXACT_BITS:
        assert np.array_equal(host[sd.NAMES[bit]], feats[sd.NAMES[bit]], equal_nan=True)


def test_event_contours_and_the_analyzer():
    from audian_amd import hipdsp
    from audian_amd.analyzer import ContourAnalyzer
    from audian_amd.bufferedspectrogram import band_bins
    from audian_amd.contours import FIELDS
    from audian_amd.events import Events
    x = recording(8.0)
    g = graph(x)
    g.update_times(0.0, 4.0)
    s = g['spectrogram']
    # a sweep, the silence behind it, the next sweep on channel 0; the same stretch of channel 1, which is silent
    ev = Events([[(0, 16000), (17000, 31000), (32000, 48000)], [(0, 16000)]], RATE, 'data')
    before = dict(hipdsp.launches)
    c = g.event_contours(ev, fmin=500.0, fmax=6000.0, min_power=1e-10)
    assert hipdsp.launches['spectral_features'] == before['spectral_features'] + 1      # one call over all events
    assert len(c) == 4 and c.table[:, 0].tolist() == [0, 0, 0, 1]
    for i in (0, 2):
        assert c.voiced[i] > 0.95 and c.start_freq[i] < c.end_freq[i]
        assert abs(c.start_freq[i] - 1000.0) < 2*s.fresolution and abs(c.end_freq[i] - 3000.0) < 2*s.fresolution
        times, pf = c.contour(i)
        tau = np.mod(times, 2.0)
        assert np.all(np.abs(pf[3:-3] - (1000.0 + 2000.0*tau[3:-3])) < s.fresolution)      # within a bin of the sweep
        assert c.low_freq[i] <= c.min_freq[i] <= c.peak_freq[i] <= c.max_freq[i] <= c.high_freq[i]
        assert c.flatness[i] < 0.05 and 1000.0 < c.centroid[i] < 3000.0
    for i in (1, 3):
        assert c.voiced[i] == 0 and c.n_frames[i] > 50 and all(np.isnan(getattr(c, name)[i]) for name in FIELDS[:10])
    # the per-frame features the contours were reduced from, against the definition on the mirror read back
    a, b = int(c.table[:, 1].min()), int(c.table[:, 2].max())
    slab = np.array(s.buffer)[a - s.offset:b - s.offset].transpose(1, 0, 2).astype(np.float32)
    k0, k1 = band_bins(500.0, 6000.0, s.fresolution, 129)
    V, T = sd.slab_features(slab, k0, k1, s.fresolution, 1e-10, 0.1)
    got = np.stack([c.features[name].T.astype(np.float32) for name in sd.NAMES[1:]])
    sd.compare(got, V, T, 0xFE, 'event_contours')
    an = ContourAnalyzer(g, 'spectrogram', fmin=500.0, fmax=6000.0, min_power=1e-10)
    g.analyze_events(ev)
    rows = an.rows()
    assert len(rows) == 4
    for ch in (0, 1):
        want = g.region_contours([(ch, t0, t1) for t0, t1 in ev.regions(ch)], fmin=500.0, fmax=6000.0, min_power=1e-10)
        for i in range(len(want)):
            assert np.array_equal(np.array(rows.pop(0), dtype=np.float64), np.array(want.row(i), dtype=np.float64),
                                  equal_nan=True)
