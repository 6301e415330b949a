"""Spectrogram template matching without a GPU: the definition (template_match_definition.py) against numpy, the
context-free preparation of the taps against the definition's, the binding against the header, the inputs of the GPU
test, and the facade (Template, BufferedTemplateMatch, TraceGraph.cut_template / match_templates / detect_calls) on a
host-only graph."""

import ctypes
import os
import re
from math import ceil

import numpy as np
import pytest

import template_match_cases as tc
import template_match_definition as td
from audian_amd import hipdsp
from audian_amd.bufferedbandpower import BufferedBandPower
from audian_amd.bufferedspectrogram import BufferedSpectrogram
from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
from audian_amd.templates import Template, default_pivot, host_template_scores, host_values, template_scores
from audian_amd.tracegraph import TraceGraph

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the definition ---------------------------------------------------------------------------------------------------

def test_definition_is_the_correlation_coefficient():
    rng = np.random.default_rng(0)
    v = rng.standard_normal((2, 40, 19))*5.0 - 90.0
    tm = rng.standard_normal((3, 6, 11))
    taps, h0, q = td.prepare(tm, True)
    r = td.scores(v, taps, 4, 0, 35, True, pivot=(-90.0, 0.0))
    raw = td.scores(v, taps, 4, 0, 35, False)
    for c in range(2):
        for t in range(35):
            w = v[c, t:t + 6, 4:15].ravel()
            for k in range(3):
                g = taps[k].ravel().astype(np.float64)
                assert abs(np.corrcoef(g, w)[0, 1] - r['value'][k, c, t]) <= 1e-12
                assert abs(np.dot(g, w) - raw['value'][k, c, t]) <= 1e-9
    assert np.all(np.abs(r['value']) <= 1) and not r['near'].any()
    assert np.all(r['bound'][0] < r['bound'][1])                         # a pivot 90 dB off costs accuracy
    assert r['bound'][0].max() < 1e-4 and r['bound'].min() > 0


def test_nan_rules_and_windows_outside_the_slab():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((1, 30, 9))
    v[0, 10:16] = 0.25                                                   # six flat frames
    v[0, 22, 3] = np.nan
    v[0, 27, 5] = np.inf
    v[0, :, 0] = np.nan                                                  # outside the band [1, 8)
    v[0, :, 8] = np.inf
    taps = td.prepare(rng.standard_normal((2, 3, 7)), True)[0]
    r = td.scores(v, taps, 1, -4, 40, True, min_std=0.01)
    val = r['value'][:, 0]
    t = np.arange(-4, 36)
    outside = (t < 0) | (t + 3 > 30)
    flat = (t >= 10) & (t + 3 <= 16)
    bad = ((t <= 22) & (t + 3 > 22)) | ((t <= 27) & (t + 3 > 27))
    want_nan = outside | flat | bad
    assert np.array_equal(np.isnan(val), np.broadcast_to(want_nan, val.shape))
    raw = td.scores(v, taps, 1, -4, 40, False)['value'][:, 0]
    assert np.all(np.isnan(raw[:, outside])) and np.all(np.isfinite(raw[:, ~outside & ~bad]))
    assert not np.any(np.isfinite(raw[:, bad & ~outside]))               # IEEE: NaN or an infinity
    # a window clear of every non-finite element is what it is without that element
    clean = v.copy()
    clean[0, 22, 3], clean[0, 27, 5] = 0.0, 0.0
    again = td.scores(clean, taps, 1, -4, 40, True, min_std=0.01)['value'][:, 0]
    assert np.array_equal(val[:, ~want_nan], again[:, ~want_nan])
    # the mask: min_std is the patch's standard deviation
    lo = td.scores(v, taps, 1, 0, 28, True, min_std=0.0)
    std = lo['std'][0]
    cut = float(np.nanmedian(std))
    hi = td.scores(v, taps, 1, 0, 28, True, min_std=cut)['value'][0, 0]
    assert np.array_equal(np.isnan(hi), ~(std > cut))


def test_gpu_inputs_keep_clear_of_the_mask_threshold():
    """What tests/test_gpu_template_match.py relies on: with MIN_STD_DB no window of the dB slabs lies within 1e-3
    relative of the threshold, none is undecided, and NaN and values both occur."""
    for shape in tc.SHAPES:
        nfreq, k0, Fb, Tt = shape
        if Tt*Fb == 1:
            continue
        v = tc.decibel_host(tc.slab(shape))
        taps = td.prepare(tc.templates(shape, K=1), True)[0]
        r = td.scores(v, taps, k0, 0, tc.FRAMES - Tt + 1, True, tc.MIN_STD_DB, (-90.0, -60.0))
        std = r['std'][np.isfinite(r['std'])]
        assert not r['near'].any() and np.all(np.abs(std - tc.MIN_STD_DB) > 1e-3*tc.MIN_STD_DB)
        assert std[std > tc.MIN_STD_DB].min() > 0.2, shape
        val = r['value']
        assert np.isnan(val).any() and np.isfinite(val).sum() > val.size//3
        assert np.all(np.isfinite(r['bound'])) and r['bound'].max() < 0.05


# ---- the preparation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('normalize', [True, False])
def test_prepare_host_equals_the_definition(normalize):
    rng = np.random.default_rng(2)
    for shape in ((1, 1, 2), (3, 7, 27), (16, 32, 97), (2, 256, 33)):
        tm = rng.standard_normal(shape)*7.0 - 80.0
        taps, h0, q = hipdsp.template_prepare(tm, normalize)
        want, wh0, wq = td.prepare(tm, normalize)
        assert taps.dtype == np.float32 and np.array_equal(taps.view(np.uint32), want.view(np.uint32))
        assert np.all(np.abs(h0 - wh0.astype(np.float64)) <= 2*np.spacing(np.abs(wh0.astype(np.float64))))
        assert np.all(np.abs(q - wq.astype(np.float64)) <= 2*np.spacing(wq.astype(np.float64)))
        if normalize:
            assert np.all(np.abs(q - 1.0) < 1e-6) and np.all(np.abs(h0) < 1e-4)
    one = hipdsp.template_prepare(rng.standard_normal((5, 9)), normalize)[0]          # a single 2-D template
    assert one.shape == (1, 5, 9)


def test_prepare_host_refusals():
    rng = np.random.default_rng(3)
    tm = rng.standard_normal((2, 4, 5))
    for bad in (np.nan, np.inf, -np.inf):
        t = tm.copy()
        t[1, 2, 3] = bad
        for normalize in (True, False):
            with pytest.raises(ValueError):
                hipdsp.template_prepare(t, normalize)
            with pytest.raises(ValueError):
                td.prepare(t, normalize)
    const = tm.copy()
    const[0] = 0.1                                                      # 0.1 * n / n is not 0.1 in every arithmetic
    with pytest.raises(ValueError):
        hipdsp.template_prepare(const, True)
    with pytest.raises(ValueError):
        td.prepare(const, True)
    taps = hipdsp.template_prepare(const, False)[0]                     # raw: a constant template is a box filter
    assert np.all(taps[0] == np.float32(0.1))
    with pytest.raises(ValueError):
        hipdsp.template_prepare(np.ones((1, 1, 1)), True)
    for shape in ((17, 2, 2), (1, 257, 2), (1, 256, 257)):
        with pytest.raises(NotImplementedError):
            hipdsp.template_prepare(rng.standard_normal(shape), True)
    with pytest.raises(ValueError):
        hipdsp.template_prepare(np.full((1, 2, 2), 1e300), False)      # overflows float32


def test_the_binding_declares_the_entries():
    from audian_amd import _lib
    i64, vp, dbl, flt, cint = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_float, ctypes.c_int
    header = open(os.path.join(HERE, '..', 'include', 'hip_dsp.h')).read()
    kinds_of = {'hipdsp_ctx *': vp, 'const hipdsp_tmplplan *': vp, 'hipdsp_tmplplan *': vp, 'hipdsp_tmplplan **': _lib._pp,
                'const float *': vp, 'float *': vp, 'const double *': vp, 'double *': vp, 'int64_t': i64, 'int': cint,
                'double': dbl, 'float': flt}
    want = {'hipdsp_template_prepare_host': 8, 'hipdsp_tmplplan_create': 2, 'hipdsp_tmplplan_destroy': 2,
            'hipdsp_tmplplan_set': 7, 'hipdsp_tmplplan_set_host': 7, 'hipdsp_tmplplan_upload': 2,
            'hipdsp_template_match': 19}
    for name, n_args in want.items():
        args, res = _lib._SIGNATURES[name]
        assert len(args) == n_args and res is cint and getattr(_lib.lib, name).argtypes == args
        proto = re.search(r'int %s\(([^;]*)\);' % name, header).group(1)
        kinds = [re.sub(r'\s*\w+$', '', a.strip()) for a in proto.replace('\n', ' ').split(',')]
        assert [kinds_of[k] for k in kinds] == args, name
    proto = re.search(r'int hipdsp_template_match\(([^;]*)\);', header).group(1)
    names = [re.search(r'(\w+)$', a.strip()).group(1) for a in proto.replace('\n', ' ').split(',')]
    assert names == ['ctx', 'plan', 'spec', 'spec_pitch', 'channels', 'frames', 'nfreq', 'k0', 'first', 'n_out', 'db',
                     'ref_power', 'min_power', 'floor', 'pivot', 'min_std', 'out', 'out_pitch', 'out_template_pitch']
    for sentence in ('v_mfma_f32_16x16x4_f32', 'D <= n*min_std^2', 'gamma*M/sqrt(Q*D)', 'bit for bit what 16 one-template calls'):
        assert sentence in header


# ---- the numpy path ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('normalize, log', [(True, True), (True, False), (False, True), (False, False)])
def test_numpy_path_is_inside_the_bound_of_the_definition(normalize, log):
    shape = tc.SHAPES[0]
    nfreq, k0, Fb, Tt = shape
    p = tc.slab(shape)                                                   # (C, frames, nfreq) powers
    tm = tc.templates(shape, K=3)
    tm = tm if log else 10.0**(tm/10.0)
    floor = tc.FLOOR_DB if log else -np.inf
    min_std = tc.MIN_STD_DB if log else tc.MIN_STD_LINEAR
    got = host_template_scores(p.transpose(1, 0, 2), tm, k0, -5, tc.FRAMES + 9, normalize, log, floor, min_std)
    v = host_values(p.astype(np.float64), log, floor).astype(np.float32)
    ref = td.scores(v, td.prepare(tm, normalize)[0], k0, -5, tc.FRAMES + 9, normalize, min_std)
    assert got.dtype == np.float32 and got.shape == ref['value'].shape
    want = ref['value']
    if normalize:
        assert not ref['near'].any() and np.array_equal(np.isnan(got), np.isnan(want))
    else:
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    # float64 sums of float64(float32 v): far inside the float32 bound; what is left is the rounding to float32
    assert np.all(np.abs(got[ok] - want[ok]) <= 2.0**-23*np.abs(want[ok]) + 1e-3*ref['bound'][ok] + 2.0**-149)


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
CHIRPS = (0.8, 2.1, 3.3)                     # onsets of the planted chirps, seconds
CHIRP_LEN, BURST_AT, BURST_LEN = 0.12, 1.5, 0.12


def call_recording(seconds=4.5):
    """Channel 0: three copies of an up-chirp 2000 -> 4000 Hz of 0.12 s and one LOUDER tone burst at 3000 Hz of the
    same length; channel 1: noise only; faint noise everywhere."""
    rng = np.random.default_rng(4)
    n = int(RATE*seconds)
    t = np.arange(n)/RATE
    x = 1e-3*rng.standard_normal((n, 2))
    for on in CHIRPS:
        m = (t >= on) & (t < on + CHIRP_LEN)
        s = t[m] - on
        x[m, 0] += 0.1*np.hanning(m.sum())*np.sin(2*np.pi*(2000.0*s + 0.5*(2000.0/CHIRP_LEN)*s**2))
    m = (t >= BURST_AT) & (t < BURST_AT + BURST_LEN)
    x[m, 0] += 0.3*np.hanning(m.sum())*np.sin(2*np.pi*3000.0*(t[m] - BURST_AT))
    return x


def host_graph(oracle, x, nfft=256, **match):
    g = TraceGraph(10.0, 2.0)
    s = host_spectrogram(oracle)(source='data', nfft=nfft)
    t = BufferedTemplateMatch(**match)
    bp = BufferedBandPower(fmin=1800.0, fmax=4200.0, log=True)
    for tr in (s, t, bp):
        g.add_trace(tr)
    g.setup_traces()
    g.open(x, RATE)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g.update_times(0.0, 4.5)
    return g, s, t


def cut(g):
    return g.cut_template(CHIRPS[0] - 0.01, CHIRPS[0] + CHIRP_LEN + 0.01, 1800.0, 4200.0, 0, floor_db=-100.0, name='chirp')


def test_template_and_cut_template(oracle, tmp_path):
    x = call_recording()
    g, s, t = host_graph(oracle, x)
    tm = cut(g)
    i0, i1 = g.region_frames(s, CHIRPS[0] - 0.01, CHIRPS[0] + CHIRP_LEN + 0.01)
    k0, k1 = ceil(1800.0/s.fresolution), int(4200.0/s.fresolution) + 1
    assert tm.values.shape == (i1 - i0, k1 - k0) and tm.fmin == k0*s.fresolution and tm.first_bin(s) == k0
    assert (tm.fresolution, tm.tresolution, tm.log, tm.floor_db, tm.name) == (s.fresolution, s.tresolution, True, -100.0, 'chirp')
    assert tm.duration == (i1 - i0)*s.tresolution and tm.bandwidth == (k1 - k0)*s.fresolution
    want = host_values(np.asarray(s.buffer)[i0 - s.offset:i1 - s.offset, 0, k0:k1], True, -100.0)
    assert np.array_equal(tm.values, want) and tm.values.min() >= -100.0 and tm.values.max() > -60.0
    lin = g.cut_template(CHIRPS[0], CHIRPS[0] + 0.05, 1800.0, 4200.0, 0, log=False)
    assert not lin.log and lin.floor == -np.inf and np.all(lin.values >= 0)
    path = str(tmp_path/'chirp.npz')
    tm.save(path)
    back = Template.load(path)
    assert np.array_equal(back.values, tm.values) and vars(back).keys() == vars(tm).keys()
    assert all(np.array_equal(getattr(back, k), getattr(tm, k)) for k in vars(tm))
    for bad in (np.zeros((0, 3)), np.zeros(5), np.full((2, 2), np.nan), np.zeros((257, 2)), np.zeros((256, 257))):
        with pytest.raises(ValueError):
            Template(bad, 0.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        g.cut_template(1.0, 1.1, 9000.0, 9500.0, 0)                      # no bin up there
    with pytest.raises(IndexError):
        g.cut_template(1.0, 1.1, 1800.0, 4200.0, 2)


def test_trace_on_a_host_only_graph_recomputes_itself_and_not_its_source(oracle):
    x = call_recording()
    g, s, t = host_graph(oracle, x)
    assert [tr.name for tr in g.traces] == ['data', 'spectrogram', 'match', 'bandpower'] and t._dev is None and s._dev is None
    assert (t.ampl_min, t.ampl_max, t.unit, t.min_std, t.normalize, t.stale) == (-1, 1, '', 0.1, True, False)
    assert np.all(np.isnan(np.asarray(t.buffer))) and len(t.buffer) == len(s.buffer)       # no template yet
    tm = cut(g)

    def check():
        assert (t.rate, t.frames, t.offset, len(t.buffer)) == (s.rate, s.frames, s.offset, len(s.buffer))
        tpl = t.template
        Tt = tpl.values.shape[0]
        slab = np.asarray(s.buffer).transpose(1, 0, 2).astype(np.float32)
        v = host_values(slab.astype(np.float64), tpl.log, tpl.floor).astype(np.float32)
        n = len(s.buffer)
        ref = td.scores(v[:, :, :], td.prepare(tpl.values, t.normalize)[0], t.k0, -(Tt//2), n, t.normalize, t.min_std)
        got = np.asarray(t.buffer).T.copy()
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)       # float32 values
        want = ref['value'][0]
        if t.normalize:
            assert not ref['near'].any() and np.array_equal(np.isnan(got), np.isnan(want))
        ok = np.isfinite(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 2.0**-23*np.abs(want[ok]) + 1e-3*ref['bound'][0][ok] + 2.0**-149)
        return got

    calls, mine = [], []
    real, real_t = s.process, t.process
    s.process = lambda *a: (calls.append(1), real(*a))
    t.process = lambda *a: (mine.append(1), real_t(*a))
    t.set_template(tm)
    r = check()
    assert not calls and len(mine) == 1
    Tt = tm.values.shape[0]
    for on in CHIRPS:                                                    # the planted copies score close to 1 ...
        k = int(on*s.rate) + Tt//2
        assert np.nanmax(r[0, k - 2:k + 3]) > 0.8
    burst = int(BURST_AT*s.rate) + Tt//2
    assert np.nanmax(r[0, burst - 6:burst + 7]) < 0.5 and np.nanmax(r[1]) < 0.5           # ... the burst and the noise do not
    assert np.all(np.isnan(r[:, :Tt//2])) and np.all(np.isnan(r[:, len(s.buffer) - (Tt - Tt//2) + 1:]))
    t.update(min_std=3.0)
    more_nan = check()
    assert np.isnan(more_nan).sum() > np.isnan(r).sum() and t.min_std == 3.0
    t.update(normalize=False)
    check()
    assert t.ampl_min == -t.ampl_max and t.unit == 'dB^2'
    t.update(min_std=0.1, normalize=True)
    assert np.array_equal(check(), r, equal_nan=True) and not calls and len(mine) == 4
    # refusals change nothing and compute nothing
    other = Template(tm.values, tm.fmin, tm.fresolution*1.001, tm.tresolution)
    high = Template(tm.values, 7000.0, tm.fresolution, tm.tresolution)
    flat = Template(np.full((4, 4), -80.0), tm.fmin, tm.fresolution, tm.tresolution)
    for bad in (other, high, flat, tm.values):
        with pytest.raises(ValueError):
            t.set_template(bad)
    with pytest.raises(ValueError):
        t.update(min_std=-1.0)
    assert t.template is tm and t.min_std == 0.1 and not calls and len(mine) == 4
    fresh = BufferedTemplateMatch(template=high)
    with pytest.raises(ValueError):
        fresh.open(s)                                                    # before any launch
    assert fresh not in s.dests
    with pytest.raises(ValueError):
        BufferedTemplateMatch(template=flat)
    with pytest.raises(ValueError):
        BufferedTemplateMatch(min_std=float('nan'))
    # a scroll and a change of the spectrogram's window carry through: the template is stale, nothing raises
    g.update_times(1.0, 4.0)
    check()
    s.update(nfft=512, overlap_frac=0.75)
    assert calls and t.stale and t.rate == RATE/128 and t.frames == ceil(len(x)/128) and len(t.buffer) == len(s.buffer)
    assert np.all(np.isnan(np.asarray(t.buffer)))
    t.set_template(cut(g))
    assert not t.stale
    check()
    t.set_template(None)
    assert np.all(np.isnan(np.asarray(t.buffer))) and not t.stale


def test_detect_calls_finds_the_chirps_and_not_the_louder_burst(oracle):
    x = call_recording()
    g, s, t = host_graph(oracle, x)
    tm = cut(g)
    Tt = tm.values.shape[0]
    short = Template(tm.values[2:-2], tm.fmin, tm.fresolution, tm.tresolution, True, -100.0, 'core')
    scores, i0 = g.match_templates([tm, short])
    assert isinstance(scores, np.ndarray) and scores.dtype == np.float32 and scores.shape == (2, 2, len(s.buffer))
    assert i0 == s.offset
    one = template_scores(s, [tm], s.offset + 10, s.offset + 90)
    assert np.array_equal(one[0], scores[0][:, 10:90], equal_nan=True)
    t.set_template(tm)
    assert np.array_equal(np.asarray(t.buffer).T.astype(np.float32), scores[0], equal_nan=True)
    events, best, best_r = g.detect_calls([tm, short], min_r=0.5)
    assert events.channels == 2 and events.rate == s.rate and events.trace_name == 'spectrogram'
    assert len(events.onsets[1]) == 0 and len(events.onsets[0]) == 3 == len(best[0]) == len(best_r[0])
    for on, a, b in zip(CHIRPS, events.onsets[0], events.offsets[0]):
        assert abs(a - (int((on - 0.01)*s.rate))) <= 1 and b - a >= Tt      # within one frame of where the call was cut
    assert np.all(best_r[0] > 0.8) and set(best[0].tolist()) <= {0, 1}
    burst = int(BURST_AT*s.rate)
    assert not np.any((events.onsets[0] <= burst + 2) & (events.offsets[0] >= burst))
    # a threshold detector on the band power finds all four
    bp = g['bandpower']
    level = np.asarray(bp.buffer)[:, 0]
    found = bp.detect_events(float(np.median(level)) + 15.0, min_gap=0.03)
    assert len(found.onsets[0]) == 4 and len(found.onsets[1]) == 0
    # the events are what the analysis entry points take
    c = g.event_contours(events, fmin=1800.0, fmax=4200.0, min_power=1e-12)
    assert len(c) == 3 and np.all(c.voiced > 0.5) and np.all((c.min_freq >= 1800.0) & (c.max_freq <= 4200.0))
    with pytest.raises(ValueError):
        g.detect_calls([Template(tm.values, tm.fmin, tm.fresolution*2, tm.tresolution)])
    assert len(g.detect_calls([tm], min_r=0.5, t0=1.9, t1=2.6)[0].onsets[0]) == 1


def test_default_pivot_is_the_templates_mean_in_float32():
    v = np.array([[-90.1, -70.3], [-55.5, -81.7]])
    assert default_pivot(v) == float(np.float32(v.mean())) and isinstance(default_pivot(v), float)
