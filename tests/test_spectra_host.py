"""Event spectra on the host: the definition (tests/spectra_definition.py) against the golden file made by
scipy.signal.welch / find_peaks, the numpy fallback (audian_amd/spectra.py) against the definition, the nfft rule, the
argument handling of BufferedArray.region_spectra / peak_freqs, PeakFrequencyAnalyzer and
TraceGraph.event_peak_freqs on host-computed traces, and the binding's signature.  No GPU."""

import ctypes
import os

import numpy as np
import pytest

import spectra_definition as sd
from audian_amd.analyzer import PeakFrequencyAnalyzer
from audian_amd.bufferedarray import BufferedArray
from audian_amd.buffereddata import BufferedData
from audian_amd.bufferedenvelope import BufferedEnvelope
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.events import Events
from audian_amd.spectra import Spectra, event_nfft, host_region_spectrum, pick_peak, welch_nfft
from audian_amd.tracegraph import TraceGraph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'region_spectra.npz')


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


class HostEnvelope(BufferedEnvelope):
    """An envelope computed on the host: the rectified source smoothed over 1/envelope_cutoff seconds."""

    def open(self, source):
        BufferedData.open(self, source)

    def update(self):
        pass

    def process(self, source, dest, nbefore):
        n = max(1, int(round(self.rate/self.envelope_cutoff)))
        x = np.abs(np.asarray(source, dtype=np.float64))
        for c in range(x.shape[1]):
            dest[:, c] = np.convolve(x[:, c], np.ones(n)/n, mode='same')[nbefore:nbefore + len(dest)]


class HostSpectrogram(BufferedSpectrogram):
    def process(self, source, dest, nbefore):
        dest[:] = 0


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


def golden_cases():
    g = np.load(GOLDEN)
    k = 0
    for i, (nfft, hop, step, start, stop, n) in enumerate(g['cases'].tolist()):
        row = None
        if n > 0:
            row = g['rows'][g['row_offsets'][k]:g['row_offsets'][k + 1]]
            k += 1
        yield i, nfft, hop, step, start, stop, n, float(g['fs'][i]), row, float(g['peak_plain'][i]), \
            float(g['peak_thresh'][i])


def same_hz(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9*abs(b)


def test_definition_reproduces_the_golden_file():
    """Every case of the file: n_frames, the row to 1e-9 of its peak, the peak frequency with and without thresh."""
    g = np.load(GOLDEN)
    thresh = float(g['thresh'])
    x = sd.golden_signal(5 + 7*2048)
    seen, shapes, with_peak = 0, set(), 0
    for i, nfft, hop, step, start, stop, n, fs, want, plain, above in golden_cases():
        row, frames, argmax = sd.region_spectrum(x, start, stop, nfft, hop, step, fs)
        assert frames == n == sd.count_frames(len(x[start:stop:step]), nfft, hop), i
        shapes.add((nfft, 'half' if hop == nfft//2 else 'full' if hop == nfft else hop, step))
        if n == 0:
            assert np.isnan(row).all() and argmax == -1 and len(row) == nfft//2 + 1
            assert np.isnan(sd.pick_peak(row, None, fs)) and np.isnan(sd.pick_peak(row, thresh, fs))
            continue
        assert np.max(np.abs(row - want)) <= 1e-9*np.max(want), (i, nfft, hop, step)
        assert argmax == np.argmax(want)
        assert same_hz(sd.pick_peak(row, None, fs), plain), i
        assert same_hz(sd.pick_peak(row, thresh, fs), above), i
        assert same_hz(sd.pick_peak(want, thresh, fs), above), i
        seen += 1
        with_peak += int(np.isfinite(above))
    assert seen == 108 and with_peak >= 50 and seen - with_peak >= 10
    assert shapes == {(nfft, hop, step) for nfft in (8, 16, 256, 1024) for hop in ('half', 'full', 3)
                      for step in (1, 2, 7)}
    assert os.path.getsize(GOLDEN) < 200000


def test_definition_is_live_scipy():
    signal = pytest.importorskip('scipy.signal')
    rng = np.random.default_rng(4)
    for case in range(40):
        nfft = int(2**rng.integers(3, 12))
        hop = [nfft//2, nfft, 3, 1][case % 4]
        step = [1, 2, 7][case % 3]
        frames = int(rng.integers(1, 6))
        n = ((frames - 1)*hop + nfft + int(rng.integers(0, hop)))*step
        x = (rng.standard_normal(n + 3) + 100.0).astype(np.float32)
        row, got_frames, _ = sd.region_spectrum(x, 3, 3 + n, nfft, hop, step, 48000.0/step)
        f, want = signal.welch(x[3:3 + n:step].astype(np.float64), 48000.0/step, 'hann', nperseg=nfft,
                               noverlap=nfft - hop, detrend='constant', scaling='density')
        assert got_frames == frames
        assert np.max(np.abs(row - want)) <= 1e-9*np.max(want), (nfft, hop, step)


def test_special_values_of_the_definition():
    x = np.full(100, 0.25, dtype=np.float32)
    row, n, argmax = sd.region_spectrum(x, 0, 100, 16, 8, 1, 10.0)
    assert n == 11 and (row == 0.0).all() and argmax == 0
    assert sd.pick_peak(row, None, 10.0) == 0.0 and np.isnan(sd.pick_peak(row, 10.0, 10.0))    # -inf dB everywhere
    x = sd.golden_signal(100)
    x[97] = np.nan                                              # 100 samples, hop 8: frames end at 96
    clean = sd.region_spectrum(sd.golden_signal(100), 0, 100, 16, 8, 1, 10.0)
    got = sd.region_spectrum(x, 0, 100, 16, 8, 1, 10.0)
    assert np.array_equal(got[0], clean[0]) and got[1:] == clean[1:]
    for bad in (np.nan, np.inf, -np.inf):
        x[40] = bad
        row, n, argmax = sd.region_spectrum(x, 0, 100, 16, 8, 1, 10.0)
        assert np.isnan(row).all() and n == 11 and argmax == 0
        assert np.isnan(sd.pick_peak(row, None, 10.0))


def random_row(rng, n, kind):
    x = rng.standard_normal(n)
    if kind % 3 == 1:
        x = x + 1e4
    if kind % 3 == 2:
        x = np.round(3*x)
    x = x.astype(np.float32)
    if kind % 7 == 3 and n:
        x[int(rng.integers(0, n))] = [np.nan, np.inf, -np.inf][kind % 3]
    return x


def test_fallback_is_the_definition():
    """host_region_spectrum and pick_peak against the definition: rows to 1e-12 of their peak (the fallback sums
    differently), n_frames, argmax and the peaks exactly."""
    rng = np.random.default_rng(6)
    nans = 0
    for case in range(300):
        nfft = int(2**rng.integers(3, 11))
        hop = [nfft//2, nfft, 3, 1][case % 4] if nfft <= 64 else [nfft//2, nfft, 3][case % 3]
        n = int(rng.integers(0, 4*nfft))
        x = random_row(rng, n, case)
        fs = float(rng.uniform(10.0, 1e5))
        want, frames, argmax = sd.region_spectrum(x, 0, n, nfft, hop, 1, fs)
        got, got_frames, got_argmax = host_region_spectrum(x, nfft, hop, fs)
        assert got.dtype == np.float64 and got.shape == (nfft//2 + 1,)
        assert got_frames == frames
        if np.isnan(want).all():
            assert np.isnan(got).all() and got_argmax == argmax
            nans += 1
            assert np.isnan(pick_peak(got, None, fs)) and np.isnan(pick_peak(got, 3.0, fs))
            continue
        assert np.max(np.abs(got - want)) <= 1e-12*np.max(want), case
        for thresh in (None, 3.0, 10.0):
            assert same_hz(pick_peak(got, thresh, fs), sd.pick_peak(got, thresh, fs)), (case, thresh)
    assert nans > 20
    # a float32 row (what the device returns) is picked like its float64 copy
    row = sd.region_spectrum(sd.golden_signal(4000), 0, 4000, 256, 128, 1, 1000.0)[0].astype(np.float32)
    assert pick_peak(row, 10.0, 1000.0) == sd.pick_peak(row.astype(np.float64), 10.0, 1000.0) == 21*1000.0/256


def test_welch_nfft_and_the_nfft_of_an_event():
    assert welch_nfft(48000.0, 100.0) == 512                    # 480 -> 512
    assert welch_nfft(48000.0, 93.75) == 512                    # exactly 512
    assert welch_nfft(48000.0, 93.0) == 1024
    assert welch_nfft(1000.0, 1.0) == 1024
    assert welch_nfft(96000.0, 1.0) == 8192                     # clamped: use step
    assert welch_nfft(100.0, 50.0) == 16 and welch_nfft(100.0, 50.0, min_nfft=8) == 8
    assert welch_nfft(96000.0, 1.0, max_nfft=2048) == 2048
    assert event_nfft(5000, 1024) == 1024 and event_nfft(1024, 1024) == 1024 and event_nfft(1023, 1024) == 512
    assert event_nfft(16, 1024) == 16 and event_nfft(15, 1024) == 0 and event_nfft(0, 1024) == 0
    assert event_nfft(15, 1024, min_nfft=8) == 8 and event_nfft(7, 1024, min_nfft=4) == 0


def two_tone_trace(rate, n):
    """Channel 0: 440 Hz, channel 1: 1250 Hz, both over weak noise and an offset."""
    rng = np.random.default_rng(8)
    t = np.arange(n)/rate
    x = 0.01*rng.standard_normal((n, 2)) + 0.25
    x[:, 0] += np.sin(2*np.pi*440.0*t)
    x[:, 1] += 0.5*np.sin(2*np.pi*1250.0*t)
    return x.astype(np.float32).astype(np.float64)


def test_buffered_array_region_spectra_and_peak_freqs():
    rate = 8000.0
    x = two_tone_trace(rate, 40000)
    g = open_graph(x, rate)
    d = g.data
    regions = [(0, 0, 4000), (1, 100, 4196), (1, 7, 7 + 255), (0, 5, 5), (1, 0, 40000)]
    sp = d.region_spectra(regions, 256)
    assert isinstance(sp, Spectra) and len(sp) == 5 and sp.nfft == 256 and sp.hop == 128 and sp.fs == rate
    assert sp.power.shape == (5, 129) and sp.regions.tolist() == [list(r) for r in regions]
    assert sp.frequencies(0).tolist() == (np.arange(129)*rate/256).tolist()
    for i, (c, a, b) in enumerate(regions):
        row, n, argmax = sd.region_spectrum(x[:, c].astype(np.float32), a, b, 256, 128, 1, rate)
        assert sp.n_frames[i] == n and sp.argmax[i] == argmax
        assert np.array_equal(np.isnan(sp.power[i]), np.isnan(row))
        if n:
            assert np.max(np.abs(sp.power[i] - row)) <= 1e-12*np.max(row)
    assert sp.n_frames.tolist() == [30, 31, 0, 0, 311]
    hz = sp.peak_freqs()
    assert abs(hz[0] - 440.0) <= rate/256 and abs(hz[1] - 1250.0) <= rate/256 and np.isnan(hz[2]) and np.isnan(hz[3])
    assert sp.peak_freqs(10.0).tolist()[:2] == hz.tolist()[:2]
    # step and hop
    sp = d.region_spectra([(0, 3, 39000)], 64, hop=3, step=7)
    row, n, argmax = sd.region_spectrum(x[:, 0].astype(np.float32), 3, 39000, 64, 3, 7, rate/7)
    assert sp.fs == rate/7 and sp.n_frames[0] == n and np.max(np.abs(sp.power[0] - row)) <= 1e-12*np.max(row)
    for bad in (dict(nfft=100), dict(nfft=4), dict(nfft=16384), dict(nfft=64, hop=65), dict(nfft=64, hop=0),
                dict(nfft=64, step=0)):
        with pytest.raises(ValueError):
            d.region_spectra([(0, 0, 100)], **bad)
    for region in [(2, 0, 10), (-1, 0, 10), (0, 0, 40001), (0, 10, 9), (0, -1, 5)]:
        with pytest.raises(IndexError):
            d.region_spectra([region], 64)
    assert len(d.region_spectra([], 64)) == 0

    # peak_freqs: the nfft of every event, NaN for the short ones, one call per nfft
    events = [(0, 0, 9000), (1, 50, 1074), (1, 1000, 1015), (0, 100, 1124), (1, 2000, 2700), (0, 0, 8192), (1, 5, 21)]
    calls = []
    original = BufferedArray._spectra_peaks

    def counted(self, regions, nfft, hop, step, thresh):
        calls.append((nfft, hop, [tuple(r) for r in regions]))
        return original(self, regions, nfft, hop, step, thresh)

    BufferedArray._spectra_peaks = counted
    try:
        hz = d.peak_freqs(events, 1.0)
    finally:
        BufferedArray._spectra_peaks = original
    assert [(nfft, hop) for nfft, hop, r in calls] == [(16, 8), (512, 256), (1024, 512), (8192, 4096)]
    assert calls[2][2] == [(1, 50, 1074), (0, 100, 1124)] and calls[3][2] == [(0, 0, 9000), (0, 0, 8192)]
    assert len(hz) == 2 and [len(h) for h in hz] == [3, 4]
    assert np.isnan(hz[1][1])                                   # 15 samples: shorter than min_nfft
    want = {0: [440.0, 440.0, 440.0], 1: [1250.0, np.nan, 1250.0, 1250.0]}
    sizes = {0: [8192, 1024, 8192], 1: [1024, 0, 512, 16]}
    for c in range(2):
        for k, (f, nfft) in enumerate(zip(want[c], sizes[c])):
            if nfft:
                assert abs(hz[c][k] - f) <= rate/nfft, (c, k, hz[c][k])
    # against the definition, with a threshold and a step, through an Events object
    ev = Events([[(0, 9000), (100, 1123)], [(50, 1074), (2000, 2700)]], rate, 'data')
    hz, power = d.peak_freqs(ev, 20.0, thresh=10.0, step=2, powers=True)
    top = welch_nfft(rate/2, 20.0)
    assert top == 256
    for c in range(2):
        for k, (a, b) in enumerate(ev.frames(c).tolist()):
            nfft = event_nfft(-(-(b - a)//2), top)
            row = sd.region_spectrum(x[:, c].astype(np.float32), a, b, nfft, nfft//2, 2, rate/2)[0]
            f = sd.pick_peak(row, 10.0, rate/2)
            assert same_hz(hz[c][k], f) and np.isfinite(f)
            assert abs(power[c][k] - row[int(round(f*nfft/(rate/2)))]) <= 1e-12*np.max(row)


def test_spectrogram_shaped_traces_are_refused():
    s = HostSpectrogram(nfft=16, source='data')
    open_graph(np.zeros((500, 2)), 100.0, [s])
    with pytest.raises(TypeError):
        s.region_spectra([(0, 0, 100)], 16)
    with pytest.raises(TypeError):
        s.peak_freqs([(0, 0, 100)], 1.0)


def test_analyzer_table_on_two_tones():
    rate = 8000.0
    x = two_tone_trace(rate, 40000)
    f = HostFilter()
    g = open_graph(x, rate, [f])
    assert f._dev is None                                       # host-only graph: the numpy path
    a = PeakFrequencyAnalyzer(g, 'filtered', freq_resolution=10.0)
    assert a.data.labels == ['peak frequency', 'peak power'] and a.data.units[0] == 'Hz'
    g.analyze_region(0.5, 1.5, 1)
    (hz, power), = a.rows()
    assert abs(hz - 1250.0) <= rate/1024
    i0, i1 = g.region_frames(f, 0.5, 1.5)
    row = sd.region_spectrum(x[:, 1].astype(np.float32), i0, i1, 1024, 512, 1, rate)[0]
    assert hz == sd.pick_peak(row, None, rate) and abs(power - row.max()) <= 1e-12*row.max()
    a.clear()
    regions = [(0.0, 0.5), (1.0, 1.01), (2.0, 4.0), (3.0, 3.001)]
    g.analyze_regions(regions)
    rows = a.rows()
    assert len(rows) == 8
    for k, (t0, t1) in enumerate(regions):
        for c, tone in enumerate((440.0, 1250.0)):
            hz, power = rows[2*k + c]
            if t1 - t0 < 16/rate:
                assert np.isnan(hz) and np.isnan(power)
            else:
                nfft = event_nfft(g.region_frames(f, t0, t1)[1] - g.region_frames(f, t0, t1)[0], 1024)
                assert abs(hz - tone) <= rate/nfft and power > 0, (k, c, hz)
    # one row per event, each on its own channel
    a.clear()
    ev = Events([[(0, 4000), (8000, 9000)], [(100, 8100)]], rate, 'filtered')
    g.analyze_events(ev)
    rows = a.rows()
    assert len(rows) == 3
    assert abs(rows[0][0] - 440.0) <= 8 and abs(rows[1][0] - 440.0) <= 16 and abs(rows[2][0] - 1250.0) <= 8
    # with a prominence threshold the same tones
    b = PeakFrequencyAnalyzer(g, 'filtered', freq_resolution=10.0, thresh=10.0)
    g.analyzers.remove(a)
    g.analyze_events(ev)
    assert [r[0] for r in b.rows()] == [r[0] for r in rows]


def test_tracegraph_event_peak_freqs_of_an_amplitude_modulated_tone():
    """Two songs of a 1 kHz carrier, modulated at 20 Hz and at 31 Hz: the events of the envelope give the modulation
    rate on the envelope (decimated to 10 x its cut-off, as the reference's envrate) and the carrier on the filtered
    trace, both within one bin."""
    rate, cutoff = 8000.0, 100.0
    n = int(10*rate)
    t = np.arange(n)/rate
    x = np.zeros((n, 2))
    for c, (t0, t1, fm) in enumerate([(1.0, 4.0, 20.0), (5.0, 8.5, 31.0)]):
        on = (t >= t0) & (t < t1)
        x[on, c] = ((1.0 + 0.8*np.sin(2*np.pi*fm*t[on]))*np.sin(2*np.pi*(1000.0 + 500.0*c)*t[on]))
    f, e = HostFilter(), HostEnvelope(envelope_cutoff=cutoff)
    g = open_graph(x, rate, [f, e])
    assert e._dev is None
    ev = g.detect_events('envelope', 0.05, min_gap=0.1, min_duration=0.5)
    assert [len(o) for o in ev.onsets] == [1, 1] and ev.trace_name == 'envelope'
    step = 8                                                    # round(8000 / (10 * 100))
    hz = g.event_peak_freqs(ev, freq_resolution=1.0)
    nfft = welch_nfft(rate/step, 1.0)
    assert nfft == 1024
    assert abs(hz[0][0] - 20.0) <= (rate/step)/nfft and abs(hz[1][0] - 31.0) <= (rate/step)/nfft
    for c in range(2):
        a, b = ev.frames(c)[0].tolist()
        env = np.asarray(e[a:b, c]).astype(np.float32)
        row = sd.region_spectrum(env, 0, b - a, nfft, nfft//2, step, rate/step)[0]
        assert hz[c][0] == sd.pick_peak(row, None, rate/step)
    assert g.event_peak_freqs(ev, thresh=10.0, freq_resolution=1.0)[0][0] == hz[0][0]
    assert g.event_peak_freqs(ev, step=4, freq_resolution=2.0)[1][0] == pytest.approx(31.0, abs=2000.0/1024)
    carrier = g.event_peak_freqs(ev, 'filtered', freq_resolution=10.0)
    assert abs(carrier[0][0] - 1000.0) <= rate/1024 and abs(carrier[1][0] - 1500.0) <= rate/1024
    none = g.event_peak_freqs(Events([[], []], rate, 'envelope'))
    assert [len(h) for h in none] == [0, 0]


def test_ctypes_signature_and_constants():
    from audian_amd import _lib, hipdsp, spectra
    i64, vp, dbl, cint = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    args, res = _lib._SIGNATURES['hipdsp_region_spectra']
    assert args == [vp, vp, i64, i64, i64, ctypes.POINTER(i64), i64, cint, cint, i64, dbl, vp, i64, vp]
    assert res is ctypes.c_int and _lib.lib.hipdsp_region_spectra.argtypes == args
    assert hipdsp.SPECTRA_GROUP == 16 and (spectra.MIN_NFFT, spectra.MAX_NFFT) == (8, 8192)
