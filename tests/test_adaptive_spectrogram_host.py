"""The adaptive spectrogram without a GPU: the longdouble definition against the scipy golden, smooth_for, host_adapt
and a numpy float64 model of the kernels' chunked hand-over against the definition and its bounds, the binding, and
BufferedAdaptiveSpectrogram on a host-only graph."""

import os

import numpy as np
import pytest

import adaptive_spectrogram_definition as ad
from conftest import ROOT, load_golden
from audian_amd.bufferedadaptivespectrogram import (BufferedAdaptiveSpectrogram, MODES, check_parameters, host_adapt,
                                                    smooth_for)
from audian_amd.bufferedbandpower import BufferedBandPower
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.tracegraph import TraceGraph


def test_definition_is_scipys_lfilter():
    g = load_golden('adaptive_spectrogram')
    kw = dict(gain=float(g['gain']), bias=float(g['bias']), power=float(g['power']), eps=float(g['eps']))
    d = ad.Definition(g['spec'], float(g['smooth']))
    rows = g['rows']
    assert g['spec'].shape == (2, 300, 9) and len(rows) > 100 and rows[-1] == 299
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'adaptive_spectrogram.npz')) < 100000
    for mode in ad.MODES:
        want = g[mode]
        got = d.value(mode, **kw)[:, rows]
        assert want.dtype == np.float64 and want.shape == got.shape
        # scipy's float64 recursion is itself inside the smoother bound; its own error is what the comparison allows
        tol = d.bound(mode, **kw)[:, rows] - ad.U*np.abs(got)
        assert np.all(np.abs(got - want.astype(ad.LD)) <= tol + 4*ad.W*np.abs(got)), mode
    assert np.all(g['pcen'][:, -3:] == 0) and np.all(g['divide'][:, -3:] == 0)


def test_smooth_for_is_the_formula():
    for tc, rate in ((0.4, 93.75), (0.4, 62.5), (0.06, 22050/512), (10.0, 1000.0), (1e-3, 10.0), (1e-7, 1.0)):
        T = ad.LD(tc)*ad.LD(rate)
        want = (np.sqrt(1 + 4*T*T) - 1)/(2*T*T) if T > 1e-3 else 2/(np.sqrt(1 + 4*T*T) + 1)
        s = smooth_for(tc, rate)
        assert 0 < s <= 1 and abs(ad.LD(s) - want) <= 4*ad.W*want, (tc, rate)
    assert abs(smooth_for(0.4, 22050/512) - 0.05638943879134889) < 1e-15        # at librosa's default rate and hop
    assert abs(ad.smooth_for(0.4, 62.5) - smooth_for(0.4, 62.5)) < 1e-16
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            smooth_for(bad, 100.0)


@pytest.mark.parametrize('smooth', [ad.smooth_for(0.4, 62.5), 1.0, 0.9, 1e-3])
def test_host_adapt_and_the_chunked_model_against_the_definition(smooth):
    """host_adapt (sequential float64) and the float64 model of the chunked hand-over (zero-state v, M' = a^n M + v)
    stay inside the bounds; the model's floor inside the smoother bound (4/s) w P_t."""
    rng = np.random.default_rng(3)
    frames = 3*ad.CHUNK + 7
    spec = ad.decades_slab(rng, 2, frames, 9, zero_tail=3)
    d = ad.Definition(spec, smooth)
    slab = spec.transpose(1, 0, 2)
    for mode in ad.MODES:
        for nb in (0, 1, ad.CHUNK, frames - 1, frames):
            got = host_adapt(slab, nb, smooth, mode)
            assert got.dtype == np.float32 and got.shape == (frames - nb, 2, 9)
            ok, worst = d.within(got.transpose(1, 0, 2), nb, mode)
            assert ok, (mode, nb, worst)
        assert np.all(host_adapt(slab, 0, smooth, mode)[-3:] == 0) or mode == 'background'
    for n in (ad.CHUNK, 2, 64):
        M = ad.chunked_model(spec, smooth, n)
        unit = (1/ad.LD(smooth))*ad.W*d.P
        ratio = float(np.max(np.abs(M.astype(ad.LD) - d.M)/np.where(unit > 0, unit, 1)))
        print('smooth %g chunk %d: worst |M - definition| = %.4f (1/s) w P_t' % (smooth, n, ratio))
        assert ratio <= 4.0


def test_handover_share_is_at_most_one():
    for n in (3, 16, ad.CHUNK, 4096):
        assert max(ad.handover_share(s, n) for s in np.linspace(1e-6, 1.0, 2001)) <= 1.0


def test_non_finite_pattern_of_host_adapt():
    rng = np.random.default_rng(4)
    spec = ad.decades_slab(rng, 1, 40, 5)
    spec[0, 7, 1], spec[0, 9, 2], spec[0, 30, 2], spec[0, 11, 3] = np.nan, np.inf, -np.inf, np.inf
    for mode in ad.MODES:
        got = host_adapt(spec.transpose(1, 0, 2), 2, 0.05, mode).transpose(1, 0, 2)
        want = ad.adapt(spec, 2, 0.05, mode, dtype=np.float64)
        assert ad.same_pattern(got, want) and np.array_equal(got, want, equal_nan=True)
        assert np.all(np.isfinite(got[0, :, 0])) and np.all(np.isfinite(got[0, :, 4]))
    back = ad.adapt(spec, 0, 0.05, 'background', dtype=np.float64)[0]
    assert np.all(np.isnan(back[7:, 1])) and np.all(np.isposinf(back[9:30, 2])) and np.all(np.isnan(back[30:, 2]))
    div = ad.adapt(spec, 0, 0.05, 'divide', dtype=np.float64)[0]
    assert np.isnan(div[11, 3]) and np.all(div[12:, 3] == 0)               # finite values after an inf: x/inf


def test_parameter_validation():
    ok = dict(mode='pcen', smooth=0.05, gain=0.98, bias=2.0, power=0.5, eps=1e-20)
    check_parameters(**ok)
    for kw in (dict(mode='log'), dict(smooth=0.0), dict(smooth=1.0000001), dict(smooth=np.nan), dict(eps=0.0),
               dict(eps=np.inf), dict(gain=-1e-9), dict(gain=1.5), dict(gain=np.nan), dict(bias=-1.0), dict(bias=np.inf),
               dict(power=0.0), dict(power=-1.0), dict(power=np.nan)):
        with pytest.raises(ValueError):
            check_parameters(**dict(ok, **kw))
    check_parameters(**dict(ok, mode='subtract', eps=0.0, gain=7.0, power=0.0))          # what a mode does not use
    check_parameters(**dict(ok, mode='divide', gain=7.0))
    with pytest.raises(ValueError):
        check_parameters(**dict(ok, mode='divide', eps=-1.0))
    with pytest.raises(ValueError):
        host_adapt(np.zeros((4, 1, 3)), 5, 0.1, 'divide')
    for kw in (dict(mode='log'), dict(time_constant=0.0), dict(warmup=-1.0), dict(gain=2.0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            BufferedAdaptiveSpectrogram(**kw)


def test_the_binding_declares_the_entry():
    import audian_amd
    from audian_amd import _lib, hipdsp
    args, res = _lib._SIGNATURES['hipdsp_spec_adapt']
    assert len(args) == 15 and res is _lib._int and args[10] is _lib._int
    assert [a is _lib._vp for a in args] == [True, True, False, True] + [False]*11
    assert all(a is _lib._i64 for a in (args[2],) + tuple(args[4:9])) and all(a is _lib._dbl for a in (args[9],) + tuple(args[11:]))
    assert [hipdsp.adapt_mode(m) for m in MODES] == [0, 1, 2, 3] and hipdsp.adapt_mode(2) == 2 and MODES == ad.MODES
    for bad in ('log', 4, -1, None, True):
        with pytest.raises(ValueError):
            hipdsp.adapt_mode(bad)
    header = open(os.path.join(ROOT, 'include', 'hip_dsp.h')).read()
    assert '#define HIPDSP_ADAPT_CHUNK %d\n' % hipdsp.ADAPT_CHUNK in header and hipdsp.ADAPT_CHUNK == ad.CHUNK
    for k, name in enumerate(('BACKGROUND', 'DIVIDE', 'SUBTRACT', 'PCEN')):
        assert '#define HIPDSP_ADAPT_%s %d\n' % (name, k) in header
    assert hipdsp.adapt_scratch_bytes(3, 3*ad.CHUNK + 7, 65) == 8*3*3*65 and hipdsp.adapt_scratch_bytes(3, ad.CHUNK, 65) == 0
    assert audian_amd.BufferedAdaptiveSpectrogram is BufferedAdaptiveSpectrogram and audian_amd.host_adapt is host_adapt


# ---- the facade on a host-only graph --------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


class HostSpectrogram(BufferedSpectrogram):
    """The facade's bookkeeping with a numpy periodogram: no device mirror anywhere in the graph."""

    def process(self, source, dest, nbefore):
        self._pending = None
        x = np.asarray(source, dtype=np.float64)
        win = np.hanning(self.nfft + 1)[:-1]
        dest[...] = 0.0
        for i in range(len(dest)):
            seg = x[i*self.hop:i*self.hop + self.nfft]
            if len(seg) == self.nfft:
                dest[i] = (np.abs(np.fft.rfft(seg*win[:, None], axis=0))**2).T.astype(np.float32)


RATE, SECONDS = 8000.0, 48.0


def recording():
    """Noise whose level swells and falls (rain), a short tone burst every second on channel 0."""
    rng = np.random.default_rng(11)
    n = int(RATE*SECONDS)
    t = np.arange(n)/RATE
    level = 1e-3*(1.0 + 30.0*np.exp(-0.5*((t - 12.0)/3.0)**2))
    x = level[:, None]*rng.standard_normal((n, 2))
    on = (t % 1.0 >= 0.3) & (t % 1.0 < 0.4)
    x[:, 0] += np.where(on, 0.01*np.sin(2*np.pi*2000.0*t), 0.0)
    return x


def host_graph(**kw):
    g = TraceGraph(6.0, 1.0)
    s = HostSpectrogram(source='data', nfft=256)
    a = BufferedAdaptiveSpectrogram(**kw)
    bp = BufferedBandPower(source='adaptive', fmin=1500.0, fmax=2500.0)
    for tr in (s, a, bp):
        g.add_trace(tr)
    g.setup_traces()
    g.open(recording(), RATE)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    calls = {'s': 0, 'a': [], 'bp': 0}
    real_s, real_a, real_bp = s.process, a.process, bp.process

    def a_process(source, dest, nbefore):
        first = a._pending.soffset
        real_a(source, dest, nbefore)
        calls['a'].append((first, len(source), nbefore, len(dest), np.array(np.asarray(source), dtype=np.float32)))

    s.process = lambda *args: (calls.__setitem__('s', calls['s'] + 1), real_s(*args))
    bp.process = lambda *args: (calls.__setitem__('bp', calls['bp'] + 1), real_bp(*args))
    a.process = a_process
    return g, s, a, bp, calls


def check_last_calls(a, calls, since=0):
    """What every process() call since `since` wrote equals the definition on the slab it saw."""
    for first, count, lead, n, slab in calls['a'][since:]:
        assert count == lead + n
        d = ad.Definition(slab.transpose(1, 0, 2), a.smooth)
        kw = dict(gain=a.gain, bias=a.bias, power=a.power, eps=a.eps)
        at = first + lead + a.source.offset - a.offset
        if at < 0 or at + n > len(a.buffer):
            continue                                                       # (scrolled out since)
        got = np.asarray(a.buffer)[at:at + n].transpose(1, 0, 2)
        ok, worst = d.within(got, lead, a.mode, **kw)
        assert ok, (a.mode, first, lead, worst)


def test_adaptive_trace_on_a_host_only_graph():
    g, s, a, bp, calls = host_graph(time_constant=0.2, warmup=5.0)
    assert [tr.name for tr in g.traces] == ['data', 'spectrogram', 'adaptive', 'bandpower']
    assert (a.mode, a.panel, a.unit, a.gain, a.bias, a.power, a.eps) == ('pcen', 'spectrogram', '', 0.98, 2.0, 0.5, 1e-20)
    g.update_times(0.0, 4.0)
    assert s._dev is None and a._dev is None
    assert (a.rate, a.frames, a.offset, len(a.buffer)) == (s.rate, s.frames, s.offset, len(s.buffer))
    assert (a.nfft, a.hop, a.fresolution, a.sample_rate) == (s.nfft, s.hop, s.fresolution, RATE) and a.shape == s.shape
    assert np.array_equal(a.frequencies, s.frequencies) and a.set_hop() is False and a._fusable_with(None) is None
    lead = a.warmup_frames()
    assert lead == int(np.ceil(5.0*0.2*s.rate)) == 63 and a.smooth == smooth_for(0.2, s.rate)
    # the recording's start: nothing ahead, the whole buffer in one call
    assert [(c[0], c[2], c[3]) for c in calls['a']] == [(0, 0, len(a.buffer))] and a.lead == 0
    check_last_calls(a, calls)
    # the band power below it takes the trace by name
    assert np.array_equal(np.asarray(bp.buffer), a.fresolution*np.sum(np.asarray(a.buffer)[:, :, bp.k0:bp.k1], axis=2))
    # PCEN does what it is for: the bursts stand out of the swelling noise by about the same amount, loud or quiet
    burst = np.asarray(bp.buffer)[:, 0]
    assert burst.max() > 3*np.median(burst)
    # a scroll: the strip asks for the whole warm-up, mid-buffer
    n0 = len(calls['a'])
    g.update_times(3.0, 7.5)
    strips = calls['a'][n0:]
    assert len(strips) == 1 and strips[0][3] < len(a.buffer) and strips[0][2] == lead == a.lead
    assert strips[0][0] + lead + s.offset == a.offset + len(a.buffer) - strips[0][3]         # the strip is the buffer's end
    check_last_calls(a, calls, n0)
    # a jump: the buffer starts where the source's does, the lead is clamped to nothing
    n0 = len(calls['a'])
    g.update_times(20.0, 24.0)
    assert [(c[0], c[2], c[3]) for c in calls['a'][n0:]] == [(0, 0, len(a.buffer))] and a.offset == s.offset > 0
    check_last_calls(a, calls, n0)
    # a scroll forward that keeps fewer frames of the buffer than the warm-up asks for: the strip is nearly the whole
    # buffer and its lead is clamped to what the source's buffer holds ahead of it
    n0 = len(calls['a'])
    old_end = a.offset + len(a.buffer)
    g.update_times(25.4, 27.0)
    strips = calls['a'][n0:]
    assert len(strips) == 1
    first, count, got_lead, n = strips[0][:4]
    kept = old_end - a.offset                                              # frames of the old buffer that stay
    assert 0 < kept < lead and a.offset == s.offset and n == len(a.buffer) - kept
    assert (first, got_lead, count) == (0, kept, kept + n) and a.lead == kept
    check_last_calls(a, calls, n0)
    # update(): this trace and its dests, never the source
    for kw in (dict(mode='divide'), dict(mode='subtract'), dict(mode='background'), dict(mode='pcen', gain=0.5, bias=1.0,
               power=0.25, eps=1e-12, time_constant=0.4)):
        n0, ns, nb = len(calls['a']), calls['s'], calls['bp']
        a.update(**kw)
        assert len(calls['a']) == n0 + 1 and calls['s'] == ns and calls['bp'] == nb + 1
        assert a.unit == ('' if a.mode in ('pcen', 'divide') else s.unit)
        check_last_calls(a, calls, n0)
    assert a.warmup_frames() == int(np.ceil(5.0*0.4*s.rate))
    n0, ns = len(calls['a']), calls['s']
    state = (a.mode, a.time_constant, a.gain, a.bias, a.power, a.eps, a.warmup)
    for kw in (dict(mode='log'), dict(gain=1.5), dict(eps=0.0), dict(power=0.0), dict(bias=-1.0), dict(time_constant=-1.0),
               dict(warmup=np.nan)):
        with pytest.raises(ValueError):
            a.update(**kw)
    assert len(calls['a']) == n0 and calls['s'] == ns
    assert state == (a.mode, a.time_constant, a.gain, a.bias, a.power, a.eps, a.warmup)
    with pytest.raises(ValueError):
        BufferedAdaptiveSpectrogram(name='onraw').open(g.data)             # the source must be spectrogram-shaped
    # the spectrogram's window changes: the geometry is redone in recompute()
    s.update(nfft=512, overlap_frac=0.75)
    assert (a.nfft, a.hop) == (512, 128) and a.shape == s.shape and a.shape[2] == 257 and len(a.buffer) == len(s.buffer)
    check_last_calls(a, calls, len(calls['a']) - 1)
