"""Noise profiles and the equalised spectrogram without a GPU: the definition against numpy's percentiles, the numpy
restatements against the definition, NoiseProfile, the binding's signatures, and the facade on a host-only graph."""

from math import ceil

import numpy as np
import pytest

import noise_profile_definition as nd
import template_match_definition as td
from audian_amd.bufferedbandpower import BufferedBandPower
from audian_amd.bufferedequalizedspectrogram import BufferedEqualizedSpectrogram
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
from audian_amd.noiseprofile import NoiseProfile, finish_quantiles, host_bin_quantiles, host_equalize
from audian_amd.templates import host_values
from audian_amd.tracegraph import TraceGraph


# ---- the definition ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 2, 3, 17, 256, 257, 1000])
def test_definition_agrees_with_numpy_percentile(n):
    """NaN-free data: the two elements and the host's interpolation are np.percentile; with NaN, np.nanpercentile."""
    rng = np.random.default_rng(n)
    spec = rng.standard_normal((2, n, 7)).astype(np.float32)

    def agree(got, want, values):
        # numpy interpolates with its own formula (a + (b - a) t, or from b when t >= 0.5) and its own q = (100 q)/100:
        # a few roundings of size 2^-53 max|v| in either formula, and a position off by at most 2 n 2^-53
        top = np.nanmax(np.abs(values.astype(np.float64)), axis=1)
        return np.all(np.abs(got - want) <= (8 + 4*n)*2.0**-53*top)

    holes = spec.copy()
    holes[rng.random(spec.shape) < 0.2] = np.nan
    holes[0, 0, 0] = 1.0                                                  # (no column without a value)
    holes[1, 0, :] = 1.0
    holes[0, 0, :] = 1.0
    for q in nd.QS + (0.25, 1/3):
        lo_hi, count = nd.bin_quantiles(spec, 0, n, 1, 0, 7, q)
        assert np.all(count == n)
        got = nd.finish_percentile(lo_hi, count, q)
        want = np.percentile(spec.astype(np.float64), 100.0*q, axis=1)
        assert agree(got, want, spec)
        if n > 1 and q in (0.0, 1.0):
            assert np.array_equal(got, want)
        lo_hi, count = nd.bin_quantiles(holes, 0, n, 1, 0, 7, q)
        assert np.array_equal(count, np.sum(~np.isnan(holes), axis=1))
        want = np.nanpercentile(holes.astype(np.float64), 100.0*q, axis=1)
        assert agree(nd.finish_percentile(lo_hi, count, q), want, holes)


def test_vectorised_definition_is_the_sequential_one():
    rng = np.random.default_rng(1)
    C, frames, F = 3, 120, 20
    spec = nd.mixed_slab(rng, C, frames, F)
    for first, n_frames, step, k0, k1 in ((0, 120, 1, 0, F), (5, 38, 3, 2, 17), (7, 1, 1, 0, F), (3, 0, 2, 1, 4), (0, 2, 100, 0, 1)):
        for q in nd.QS + (0.25,):
            lo_hi, count = nd.bin_quantiles(spec, first, n_frames, step, k0, k1, q)
            assert lo_hi.shape == (C, k1 - k0, 2) and count.shape == (C, k1 - k0) and count.dtype == np.int32
            for c in range(C):
                for k in range(k0, k1):
                    lo, hi, n = nd.bin_quantiles_column(spec[c, first:first + n_frames*step:step, k][:n_frames], q)
                    assert n == count[c, k - k0]
                    assert nd.same_bits(lo_hi[c, k - k0], np.array([lo, hi], dtype=np.float32)), (first, n_frames, step, k, q)
    # ties across a digit boundary, -0 and +0 as one value, infinities inside the order
    col = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
    assert nd.bin_quantiles_column(col, 0.0)[::2] == (-np.inf, 6) and nd.bin_quantiles_column(col, 1.0)[::2] == (np.inf, 6)
    lo, hi, n = nd.bin_quantiles_column(col, 0.5)
    assert lo == 0 and hi == 0 and n == 6                                 # pos = 2.5: the two zeros
    assert nd.exact_q(257) == 0.25 and 0.25*256 == 64.0 and nd.exact_q(3) == 0.5 and nd.exact_q(256) is None


def test_host_restatements_are_the_definition():
    rng = np.random.default_rng(2)
    C, frames, F = 3, 130, 11
    spec = nd.mixed_slab(rng, C, frames, F)
    slab = spec.transpose(1, 0, 2).astype(np.float64)                     # the facade's (frames, channels, bins) buffer
    for first, n_frames, step, k0, k1 in ((0, 130, 1, 0, F), (4, 42, 3, 1, 9), (9, 1, 1, 0, F), (2, 0, 1, 0, F)):
        for q in nd.QS + (0.25,):
            got, gcnt = host_bin_quantiles(slab, first, n_frames, step, k0, k1, q)
            want, wcnt = nd.bin_quantiles(spec, first, n_frames, step, k0, k1, q)
            assert got.dtype == np.float32 and gcnt.dtype == np.int32
            assert np.array_equal(gcnt, wcnt) and nd.same_bits(got, want)
            a, b = finish_quantiles(got, gcnt, q), nd.finish_percentile(want, wcnt, q)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    for bad in (dict(q=1.5), dict(q=float('nan')), dict(step=0), dict(first=-1), dict(first=100, n_frames=31)):
        a = dict(first=0, n_frames=10, step=1, q=0.5)
        a.update(bad)
        with pytest.raises(ValueError):
            host_bin_quantiles(slab, a['first'], a['n_frames'], a['step'], 0, F, a['q'])
    prof = nd._noise(rng, C*F).reshape(C, F)
    prof[0, 1], prof[1, 2], prof[2, 3] = np.inf, 0.0, 3e38
    for mode in ('divide', 'subtract'):
        got = host_equalize(slab, prof, mode)
        want = nd.equalize(spec, prof, mode).transpose(1, 0, 2)
        assert got.dtype == np.float32 and got.shape == slab.shape
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))
    with np.errstate(all='ignore'):                                       # the header's formula for 'divide'
        q64 = (spec.astype(np.float64)/prof.astype(np.float64)[:, None, :]).astype(np.float32)
    want = nd.equalize(spec, prof, 'divide')
    assert np.array_equal(q64[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))
    with pytest.raises(ValueError):
        host_equalize(slab, prof, 'multiply')


# ---- NoiseProfile ---------------------------------------------------------------------------------------------------

class Shape(object):
    def __init__(self, channels, nfreq, fresolution):
        self.channels, self.shape, self.fresolution = channels, (100, channels, nfreq), fresolution


def test_noise_profile_object(tmp_path):
    values = np.array([[1e-3, 1e-25, 0.0], [2.0, 1e-20, 5e-21]])
    p = NoiseProfile(values, 62.5, 0.008, percentile=25.0, t0=1.0, t1=3.5)
    assert p.values.dtype == np.float32 and (p.channels, p.nfreq) == (2, 3)
    floor = np.float32(1e-20)
    assert np.array_equal(p.values, np.array([[1e-3, floor, floor], [2.0, floor, floor]], dtype=np.float32))
    assert (p.fresolution, p.tresolution, p.percentile, p.min_power, p.t0, p.t1) == (62.5, 0.008, 25.0, 1e-20, 1.0, 3.5)
    assert np.allclose(p.db(), 10*np.log10(p.values.astype(np.float64)), rtol=0, atol=1e-9) and p.db().shape == (2, 3)
    assert NoiseProfile(values, 1.0, 1.0, min_power=0.0).values[0, 2] == 0
    for c, k in ((0, 0), (1, 2)):
        bad = values.copy()
        bad[c, k] = np.nan
        with pytest.raises(ValueError, match='channel %d bin %d' % (c, k)):
            NoiseProfile(bad, 62.5, 0.008)
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((2, 0))):
        with pytest.raises(ValueError):
            NoiseProfile(bad, 1.0, 1.0)
    path = str(tmp_path/'profile.npz')
    p.save(path)
    back = NoiseProfile.load(path)
    assert vars(back).keys() == vars(p).keys() and all(np.array_equal(getattr(back, k), getattr(p, k)) for k in vars(p))
    assert back.values.dtype == np.float32
    assert p.fits(Shape(2, 3, 62.5)) and p.fits(Shape(2, 3, 62.5*(1 + 1e-12)))
    assert not p.fits(Shape(2, 4, 62.5)) and not p.fits(Shape(3, 3, 62.5)) and not p.fits(Shape(2, 3, 62.6))
    trace = Shape(2, 3, 62.5)
    trace.shape = (100, 2)
    assert not p.fits(trace)


def test_the_binding_declares_the_entries():
    import ctypes
    from audian_amd import _lib, hipdsp
    args, res = _lib._SIGNATURES['hipdsp_bin_quantiles']
    assert len(args) == 14 and res is _lib._int and args[11] is _lib._dbl
    assert all(a is _lib._i64 for a in args[2:11]) and all(a is _lib._vp for a in args[:2] + args[12:])
    args, res = _lib._SIGNATURES['hipdsp_spec_equalize']
    assert len(args) == 11 and res is _lib._int and args[10] is _lib._int
    assert [a is _lib._vp for a in args] == [True, True, False, True] + [False]*4 + [True, False, False]
    assert hipdsp.eq_mode('divide') == 0 and hipdsp.eq_mode('subtract') == 1 and hipdsp.eq_mode(1) == 1
    for bad in ('multiply', 2, None, True):
        with pytest.raises(ValueError):
            hipdsp.eq_mode(bad)
    import audian_amd
    assert audian_amd.NoiseProfile is NoiseProfile and audian_amd.BufferedEqualizedSpectrogram is BufferedEqualizedSpectrogram
    assert audian_amd.host_bin_quantiles is host_bin_quantiles and audian_amd.host_equalize is host_equalize
    assert ctypes.sizeof(_lib._i64) == 8


# ---- the facade on a host-only graph --------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def host_spectrogram(oracle):
    class OSpectrogram(BufferedSpectrogram):
        """The facade's bookkeeping, computed on the host: no device mirror anywhere in the graph."""

        def process(self, source, dest, nbefore):
            self._pending = None
            oracle.spectrogram_process(np.asarray(source), dest, self.source.rate, self.nfft, self.hop)
            dest[...] = dest.astype(np.float32)

    return OSpectrogram


RATE = 16000.0
SECONDS = 6.0
HUM = 3000.0                                   # a stationary band: louder than the chirps' band


def recording():
    """Channel 0: a stationary tone at 3000 Hz, noise, and three faint up-chirps 5000 -> 6500 Hz; channel 1: the tone
    and noise only, a hundred times fainter."""
    rng = np.random.default_rng(7)
    n = int(RATE*SECONDS)
    t = np.arange(n)/RATE
    x = 1e-3*rng.standard_normal((n, 2)) + 0.2*np.sin(2*np.pi*HUM*t)[:, None]
    for on in (1.0, 2.5, 4.2):
        m = (t >= on) & (t < on + 0.1)
        s = t[m] - on
        x[m, 0] += 0.02*np.hanning(m.sum())*np.sin(2*np.pi*(5000.0*s + 0.5*15000.0*s**2))
    x[:, 1] *= 0.01
    return x


def host_graph(oracle, x, **eq):
    g = TraceGraph(10.0, 2.0)
    s = host_spectrogram(oracle)(source='data', nfft=256)
    e = BufferedEqualizedSpectrogram(**eq)
    bp = BufferedBandPower(source='equalized', fmin=2500.0, fmax=3500.0)
    m = BufferedTemplateMatch(source='equalized')
    for tr in (s, e, bp, m):
        g.add_trace(tr)
    g.setup_traces()
    g.open(x, RATE)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g.update_times(0.0, SECONDS)
    return g, s, e, bp, m


def check_graph(s, e, bp, m):
    """Every trace below the spectrogram against its numpy definition on its own source's buffer."""
    src = np.asarray(s.buffer)
    got = np.asarray(e.buffer)
    assert (e.rate, e.frames, e.offset, len(e.buffer)) == (s.rate, s.frames, s.offset, len(s.buffer))
    assert (e.nfft, e.hop, e.fresolution, e.tresolution) == (s.nfft, s.hop, s.fresolution, s.tresolution)
    assert e.shape == s.shape and np.array_equal(e.frequencies, s.frequencies)
    assert e.spec_rect == [e.offset/e.rate, 0, len(e.buffer)/e.rate, RATE/2 + e.fresolution]
    if e.stale:
        assert np.all(np.isnan(got))
    elif e.profile is None:
        assert np.array_equal(got, src)
    else:
        want = nd.equalize(src.transpose(1, 0, 2), e.profile.values, e.mode).transpose(1, 0, 2)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got.astype(np.float32)[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)
    # band power under it: fresolution * the float64 sum of ITS source's bins
    assert (bp.rate, bp.offset, len(bp.buffer)) == (e.rate, e.offset, len(e.buffer))
    want = e.fresolution*np.sum(got[:, :, bp.k0:bp.k1], axis=2)
    assert np.array_equal(np.asarray(bp.buffer), want, equal_nan=True)
    # the template trace under it
    r = np.asarray(m.buffer).T
    if m.template is None or m.stale:
        assert np.all(np.isnan(r))
        return got
    tpl = m.template
    Tt = tpl.values.shape[0]
    v = host_values(got.transpose(1, 0, 2).astype(np.float32).astype(np.float64), tpl.log, tpl.floor).astype(np.float32)
    ref = td.scores(v, td.prepare(tpl.values, True)[0], m.k0, -(Tt//2), len(got), True, m.min_std)
    want = ref['value'][0]
    assert not ref['near'].any() and np.array_equal(np.isnan(r), np.isnan(want))
    ok = np.isfinite(want)
    assert np.all(np.abs(r[ok] - want[ok]) <= 2.0**-23*np.abs(want[ok]) + 1e-3*ref['bound'][0][ok] + 2.0**-149)
    return got


def test_profile_on_a_host_only_graph(oracle):
    x = recording()
    g, s, e, bp, m = host_graph(oracle, x)
    assert [tr.name for tr in g.traces] == ['data', 'spectrogram', 'equalized', 'bandpower', 'match']
    assert s._dev is None and e._dev is None
    n = len(s.buffer)
    done = s.complete_frames()
    assert done == (len(x) - 256)//128 + 1 and done < s.frames and np.all(np.asarray(s.buffer)[done:] == 0)
    prof = g.estimate_noise_profile(percentile=50.0)
    assert isinstance(prof, NoiseProfile) and prof.values.shape == (2, 129) and prof.fits(s) and prof.fits(e)
    assert (prof.fresolution, prof.tresolution, prof.percentile, prof.min_power) == (s.fresolution, s.tresolution, 50.0, 1e-20)
    assert (prof.t0, prof.t1) == (0.0, done/s.rate)                       # the zero tail frames are left out
    slab = np.asarray(s.buffer).transpose(1, 0, 2).astype(np.float32)
    lo_hi, count = nd.bin_quantiles(slab, 0, done, 1, 0, 129, 0.5)
    assert np.all(count == done)
    assert np.array_equal(prof.values, nd.finish_percentile(lo_hi, count, 0.5).astype(np.float32))
    assert np.allclose(prof.values, np.median(np.asarray(s.buffer)[:done], axis=0), rtol=1e-6, atol=0)
    hum = int(round(HUM/s.fresolution))
    assert np.all(np.argmax(prof.values, axis=1) == hum)                  # the stationary band owns the profile
    # a sub-range, every third frame, another percentile
    part = s.noise_profile(100, 400, percentile=95.0, frame_step=3)
    lo_hi, count = nd.bin_quantiles(slab, 100, 100, 3, 0, 129, 0.95)
    assert np.array_equal(part.values, nd.finish_percentile(lo_hi, count, 0.95).astype(np.float32))
    assert (part.t0, part.t1, part.percentile) == (100/s.rate, 400/s.rate, 95.0)
    t_prof = g.estimate_noise_profile(1.0, 3.0, percentile=10.0, frame_step=2)
    i0, i1 = g.region_frames(s, 1.0, 3.0)
    lo_hi, count = nd.bin_quantiles(slab, i0 - s.offset, ceil((i1 - i0)/2), 2, 0, 129, 0.10)
    assert np.array_equal(t_prof.values, nd.finish_percentile(lo_hi, count, 0.10).astype(np.float32))
    with pytest.raises(IndexError):
        s.noise_profile(0, n + 1)
    with pytest.raises(ValueError):
        s.noise_profile(0, n, frame_step=0)
    with pytest.raises(ValueError):
        s.noise_profile(0, n, percentile=101.0)
    with pytest.raises(ValueError):
        s.noise_profile(done, n)                                          # nothing but the zero tail: no valid frame


def test_equalized_trace_on_a_host_only_graph(oracle):
    x = recording()
    g, s, e, bp, m = host_graph(oracle, x)
    calls, mine = [], []
    real, real_e = s.process, e.process
    s.process = lambda *a: (calls.append(1), real(*a))
    e.process = lambda *a: (mine.append(1), real_e(*a))
    assert (e.mode, e.profile, e.stale, e.panel, e.panel_type) == ('divide', None, False, 'spectrogram', 'spectrogram')
    check_graph(s, e, bp, m)                                              # no profile: a copy of the source
    raw_band = np.asarray(bp.buffer).copy()
    prof = g.estimate_noise_profile()
    e.set_profile(prof)
    white = check_graph(s, e, bp, m)
    assert not calls and len(mine) == 1 and e.profile is prof and e.unit == ''
    done = s.complete_frames()
    assert np.allclose(np.median(white[:done], axis=0), 1.0, rtol=1e-6)   # whitened: the median of every bin is 1
    hum = int(round(HUM/s.fresolution))
    assert np.all(np.argmax(np.asarray(s.buffer)[:done, 0], axis=1) == hum)          # the raw peak sits in the hum ...
    on = int(1.05*e.rate)
    assert abs(np.argmax(white[on, 0])*e.fresolution - 5750.0) < 500.0               # ... the whitened one in the chirp
    assert not np.array_equal(raw_band, np.asarray(bp.buffer))
    # the consumers take the trace by name: a template cut from the equalised image, matched against it
    tm = g.cut_template(0.99, 1.11, 4800.0, 6800.0, 0, spec_name='equalized', floor_db=-20.0, name='chirp')
    assert tm.first_bin(e) == tm.first_bin(s)
    m.set_template(tm)
    check_graph(s, e, bp, m)
    r = np.asarray(m.buffer)
    Tt = tm.values.shape[0]
    for on in (1.0, 2.5, 4.2):
        k = int(on*e.rate) + Tt//2
        assert np.nanmax(r[k - 3:k + 4, 0]) > 0.7
    events, best, score = g.detect_calls([tm], 0.7, spec_name='equalized')
    assert len(events.onsets[0]) == 3 and len(events.onsets[1]) == 0
    scores, i0 = g.match_templates([tm], spec_name='equalized')
    assert scores.shape == (1, 2, len(e.buffer)) and i0 == e.offset
    contours = g.event_contours(events, spec_name='equalized', fmin=4000.0)
    raw_contours = g.event_contours(events, spec_name='spectrogram', fmin=4000.0)
    assert len(contours) == 3 and np.array_equal(contours.table, raw_contours.table)
    assert np.all(contours.peak_freq > 4500.0) and np.all(contours.peak_freq < 7000.0) and np.all(contours.n_frames > 0)
    feats = e.spectral_features(e.offset, e.offset + 50, features=('peak_freq',))
    assert feats['peak_freq'].shape == (50, 2)
    assert e.band_powers([(2500.0, 3500.0)], e.offset, e.offset + 10).shape == (1, 2, 10)
    assert e.decibel_image(0).shape == (129, len(e.buffer)) and e.mean_power_db(e.offset, e.offset + 20, 0).shape == (129,)
    assert e.decimated_image(e.offset, e.offset + 40, 4, 1).shape == (129, 10)
    # the other mode, and back
    before = len(mine)
    e.update(mode='subtract')
    sub = check_graph(s, e, bp, m)
    assert not calls and len(mine) == before + 1 and e.unit == s.unit and sub.min() == 0 and np.any(sub > 0)
    e.update(mode='divide')
    assert np.array_equal(check_graph(s, e, bp, m), white, equal_nan=True)
    # a scroll changes no value that stays in the buffer
    keep = {int(i) + e.offset: np.asarray(e.buffer)[int(i)].copy() for i in (5, 50, 200)}
    g.update_times(0.5, 5.5)
    check_graph(s, e, bp, m)
    for frame, row in keep.items():
        if e.offset <= frame < e.offset + len(e.buffer):
            assert np.array_equal(np.asarray(e.buffer)[frame - e.offset], row, equal_nan=True)
    # refusals: before any launch, nothing changed
    before = len(mine)
    wrong_bins = NoiseProfile(np.ones((2, 65)), s.fresolution, s.tresolution)
    wrong_res = NoiseProfile(np.ones((2, 129)), s.fresolution*1.001, s.tresolution)
    wrong_ch = NoiseProfile(np.ones((3, 129)), s.fresolution, s.tresolution)
    for bad in (wrong_bins, wrong_res, wrong_ch, prof.values):
        with pytest.raises(ValueError):
            e.set_profile(bad)
    with pytest.raises(ValueError):
        e.update(mode='multiply')
    assert e.profile is prof and e.mode == 'divide' and len(mine) == before and not calls
    fresh = BufferedEqualizedSpectrogram(name='other', profile=wrong_bins)
    with pytest.raises(ValueError):
        fresh.open(s)
    assert fresh not in s.dests
    with pytest.raises(ValueError):
        BufferedEqualizedSpectrogram(mode='multiply')
    with pytest.raises(ValueError):
        BufferedEqualizedSpectrogram(profile=np.ones((2, 129)))
    with pytest.raises(ValueError):
        BufferedEqualizedSpectrogram(name='onraw').open(g.data)           # the source must be a spectrogram
    assert e._fusable_with(None) is None
    # a change of the spectrogram's window: the profile is stale, the trace NaN, nothing raises
    s.update(nfft=512, overlap_frac=0.75)
    assert calls and e.stale and (e.nfft, e.hop) == (512, 128) and e.shape == s.shape and e.shape[2] == 257
    check_graph(s, e, bp, m)
    assert np.all(np.isnan(np.asarray(e.buffer))) and np.all(np.isnan(np.asarray(bp.buffer))) and m.stale
    e.set_profile(g.estimate_noise_profile(percentile=25.0))
    assert not e.stale
    check_graph(s, e, bp, m)
    e.set_profile(None)
    assert not e.stale and e.unit == s.unit
    check_graph(s, e, bp, m)
