"""hipdsp_spec_adapt through the C ABI against tests/adaptive_spectrogram_definition.py: every element under the
per-element bounds derived there (none left out), the same bits twice, alone and in company, in place, under a captured
graph, with the scratch filled with 0x00 and 0xff, and past 2^32 bytes; then BufferedAdaptiveSpectrogram in a small graph
under the ledger of tests/facade_ledger.py.  Every output lies between sentinel guards; a case's slab is uploaded
once."""

import ctypes

import numpy as np
import pytest

import adaptive_spectrogram_definition as ad
import facade_ledger as fl
import far_placement as fp
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

L = ad.CHUNK
GUARD = 16
SENT = np.float32(-12345.5)
SMOOTH = ad.smooth_for(0.4, 8000.0/128.0)               # the default time constant at 62.5 frames/s: 0.0392
WORST = {}


class Slab(object):
    """A host slab (C, frames, F) on the device at a chosen pitch and element offset."""

    def __init__(self, spec, pitch_extra=0, offset=0, c=None):
        from audian_amd import hipdsp
        self.c = gh.ctx() if c is None else c
        self.spec = np.ascontiguousarray(spec, dtype=np.float32)
        self.C, self.frames, self.F = self.spec.shape
        self.total = self.frames*self.F
        self.pitch = self.total + pitch_extra
        self.offset = offset
        self.host = np.full(offset + max(1, self.C)*self.pitch + 8, SENT, dtype=np.float32)
        for ch in range(self.C):
            a = offset + ch*self.pitch
            self.host[a:a + self.total] = self.spec[ch].ravel()
        self.dev = hipdsp.DeviceArray.from_host(self.c, self.host)
        self.pitch_arg = self.pitch if pitch_extra else 0

    def ptr(self, channel=0, col=0):
        return self.dev.view(self.offset + channel*self.pitch + col, (1,))

    def free(self):
        self.dev.free()


def run(slab, nbefore, mode, smooth=SMOOTH, padded=False, channels=None, channel0=0, refuse=None, **kw):
    """One out-of-place hipdsp_spec_adapt call: (C, frames - nbefore, F) float32.  padded: an out base at an odd 4-byte
    offset and a pitch larger than dense.  The guards around every output row must hold the sentinel afterwards, the
    input must be unchanged.  refuse: the exception class the call must raise; the output must then be untouched."""
    from audian_amd import hipdsp
    C = slab.C if channels is None else channels
    n = max(slab.frames - nbefore, 0)
    total = n*slab.F
    o_off, o_pitch = (GUARD + 1, total + 2*GUARD + 3) if padded else (GUARD, total)
    do = hipdsp.DeviceArray.from_host(slab.c, np.full(o_off + max(C, 1)*max(o_pitch, 1) + GUARD, SENT, dtype=np.float32))
    args = (slab.c, slab.ptr(channel0), slab.pitch_arg, do.view(o_off, (1,)), o_pitch if padded else 0, C, slab.frames,
            slab.F, nbefore, smooth, mode)
    if refuse is not None:
        with pytest.raises(refuse):
            hipdsp.spec_adapt(*args, **kw)
    else:
        hipdsp.spec_adapt(*args, **kw)
    flat = do.to_host()
    do.free()
    if refuse is not None:
        assert np.all(flat == SENT), 'a refused call wrote something'
        return None
    written = np.zeros(flat.size, dtype=bool)
    out = np.empty((C, n, slab.F), dtype=np.float32)
    for ch in range(C):
        a = o_off + ch*o_pitch
        out[ch] = flat[a:a + total].reshape(n, slab.F)
        written[a:a + total] = True
    assert np.all(flat[~written] == SENT), 'written outside the rows'
    return out


def nbefores(frames):
    return sorted(set(n for n in (0, 1, L, frames - 1, frames) if 0 <= n <= frames))


FRAMES = (1, 2, L - 1, L, L + 1, 3*L + 7)
NFREQ = (1, 5, 64, 65, 129, 1025)
SHAPES = [(frames, F) for frames in FRAMES for F in NFREQ if F < 1025 or frames <= L + 1]


@pytest.mark.parametrize('frames, F', SHAPES)
def test_every_element_inside_the_bound(frames, F):
    """x >= 0 over 12 decades per column, a column that drops by 10^9 mid-slab, zero tail frames: every mode, every
    nbefore, dense and padded with an odd out base, one and three channels."""
    i = SHAPES.index((frames, F))
    for C in ((1, 3) if F in (5, 65) else ((1,) if i % 2 else (3,))):
        rng = np.random.default_rng([frames, F, C])
        tail = min(3, frames - 1)
        spec = ad.decades_slab(rng, C, frames, F, zero_tail=tail)
        d = ad.Definition(spec, SMOOTH)
        slab = Slab(spec, pitch_extra=(0 if i % 3 else 7), offset=(0 if i % 3 else 3))
        for mode in ad.MODES:
            for j, nb in enumerate(nbefores(frames)):
                got = run(slab, nb, mode, padded=bool((i + j) % 2))
                ok, worst = d.within(got, nb, mode)
                WORST[mode] = max(WORST.get(mode, 0.0), worst)
                print('frames %d F %d C %d %s nbefore %d: worst |err|/bound %.4f' % (frames, F, C, mode, nb, worst))
                assert ok, (mode, nb, worst)
                if tail and mode != 'background' and frames - nb >= tail:
                    assert np.all(got[:, frames - nb - tail:] == 0), 'the zero tail frames must give exactly 0'
        assert np.array_equal(slab.dev.to_host().view(np.uint32), slab.host.view(np.uint32)), 'the input changed'
        slab.free()


@pytest.mark.parametrize('kw', [dict(smooth=1.0), dict(smooth=0.9), dict(smooth=1e-3), dict(gain=0.0), dict(gain=1.0, bias=0.0),
                                dict(power=2.0, bias=10.0), dict(power=0.25, gain=0.5, eps=1e-6), dict(eps=1e-30)])
def test_other_parameters_inside_the_bound(kw):
    rng = np.random.default_rng(len(repr(kw)))
    spec = ad.decades_slab(rng, 2, 2*L + 9, 65, zero_tail=2)
    kw = dict(kw)
    smooth = kw.pop('smooth', SMOOTH)
    d = ad.Definition(spec, smooth)
    slab = Slab(spec)
    for mode in ad.MODES:
        got = run(slab, 5, mode, smooth=smooth, **kw)
        ok, worst = d.within(got, 5, mode, **kw)
        print('%r %s: worst |err|/bound %.4f' % (kw, mode, worst))
        assert ok, (kw, mode, worst)
    slab.free()


def test_same_bits_twice_alone_and_in_place():
    """The same call twice; a column computed alone (1 channel, 1 bin, its own slab) and inside 3 x 129; in place equals
    out of place."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(21)
    frames, F = 3*L + 7, 129
    spec = ad.decades_slab(rng, 3, frames, F, zero_tail=2)
    slab = Slab(spec, pitch_extra=5, offset=1)
    for mode in ad.MODES:
        full = run(slab, 0, mode)
        assert ad.exact_bits(run(slab, 0, mode, padded=True), full), 'not the same bits twice'
        late = run(slab, L + 3, mode)
        assert ad.exact_bits(late, full[:, L + 3:]), 'nbefore changed a value'
        for ch, k in ((0, 0), (1, 64), (2, 128)):
            alone = Slab(spec[ch:ch + 1, :, k:k + 1])
            assert ad.exact_bits(run(alone, 0, mode)[0, :, 0], full[ch, :, k]), 'the company changed a column'
            alone.free()
        one = run(slab, 0, mode, channels=1, channel0=2)
        assert ad.exact_bits(one[0], full[2])
        # in place: a copy of the slab, out == spec with the same pitch
        copy = Slab(spec, pitch_extra=5, offset=1)
        hipdsp.spec_adapt(copy.c, copy.ptr(), copy.pitch, copy.ptr(), copy.pitch, 3, frames, F, 0, SMOOTH, mode)
        flat = copy.dev.to_host()
        for ch in range(3):
            a = copy.offset + ch*copy.pitch
            assert ad.exact_bits(flat[a:a + copy.total].reshape(frames, F), full[ch]), 'in place differs'
            assert np.all(flat[a + copy.total:a + copy.pitch] == SENT)
        assert np.all(flat[:copy.offset] == SENT)
        copy.free()
    slab.free()


def test_refused_calls_write_nothing():
    from audian_amd import hipdsp
    rng = np.random.default_rng(22)
    spec = ad.decades_slab(rng, 2, 40, 9)
    slab = Slab(spec)
    before = run(slab, 3, 'pcen')
    for mode, kw in (('pcen', dict(smooth=0.0)), ('pcen', dict(smooth=1.5)), ('pcen', dict(smooth=np.nan)),
                     ('divide', dict(eps=0.0)), ('pcen', dict(eps=-1.0)), ('pcen', dict(eps=np.inf)),
                     ('pcen', dict(gain=-0.1)), ('pcen', dict(gain=1.1)), ('pcen', dict(bias=-1.0)),
                     ('pcen', dict(power=0.0)), ('pcen', dict(power=np.nan)), (4, {}), (-1, {})):
        kw = dict(kw)
        run(slab, 3, mode, smooth=kw.pop('smooth', SMOOTH), refuse=ValueError, **kw)
    run(slab, 41, 'divide', refuse=ValueError)                            # nbefore > frames
    run(slab, -1, 'divide', refuse=ValueError)
    assert run(slab, 40, 'divide').size == 0                              # nbefore == frames: nothing (guards checked)
    assert run(slab, 0, 'divide', channels=0).size == 0
    out = hipdsp.DeviceArray.from_host(slab.c, np.full(2*40*9, SENT, dtype=np.float32))
    with pytest.raises(NotImplementedError):               # (refused before anything is written: a small out will do)
        hipdsp.spec_adapt(slab.c, slab.ptr(), 0, out, 0, 65536, 40, 9, 3, SMOOTH, 'divide')
    for raw_mode in (4, -1):                               # past the binding's own check: the C entry's "unknown mode"
        with pytest.raises(ValueError, match='unknown mode'):
            hipdsp.check(hipdsp.lib.hipdsp_spec_adapt(slab.c.handle, hipdsp._p(slab.ptr()), 0, hipdsp._p(out), 0, 2, 40, 9, 3,
                                                      SMOOTH, raw_mode, 0.98, 2.0, 0.5, 1e-20))
    bad = [(slab.ptr(), 40*9 - 1, out, 0, 40, 0), (slab.ptr(), 0, out, 37*9 - 1, 40, 3), (None, 0, out, 0, 40, 0),
           (slab.ptr(), 0, None, 0, 40, 0), (slab.ptr(), 0, slab.ptr(0, 9), 0, 40, 0), (slab.ptr(), 0, slab.ptr(), 0, 40, 3),
           (slab.ptr(), 0, slab.ptr(), 40*9 + 1, 40, 0), (slab.ptr(), 0, out, 0, 2**45, 0), (slab.ptr(), 2**44 + 1, out, 0, 40, 0)]
    for spec_p, spitch, out_p, opitch, frames, nb in bad:
        with pytest.raises(ValueError):
            hipdsp.spec_adapt(slab.c, spec_p, spitch, out_p, opitch, 2, frames, 9, nb, SMOOTH, 'divide')
    assert np.all(out.to_host() == SENT)
    out.free()
    assert np.array_equal(slab.dev.to_host().view(np.uint32), slab.host.view(np.uint32)), 'a refused call wrote into the slab'
    assert ad.exact_bits(run(slab, 3, 'pcen'), before)
    slab.free()


def test_non_finite_samples_follow_the_sequential_float64_pattern():
    """A NaN, a +inf and a finite value after an inf at chosen (c, t0, k), default smooth: from t0 on the column has the
    NaN / +inf / -inf / finite pattern of the sequential float64 evaluation; the other columns keep their bytes."""
    rng = np.random.default_rng(23)
    frames, F = 3*L + 7, 65
    clean = ad.decades_slab(rng, 2, frames, F)
    spec = clean.copy()
    spots = {(0, 5, 3): np.nan, (0, L - 1, 17): np.inf, (1, L, 64): np.inf, (1, 2*L + 3, 0): -np.inf, (0, 0, 30): np.inf,
             (1, frames - 1, 40): np.nan, (0, 40, 50): np.inf, (0, 300, 50): -np.inf, (1, 100, 20): np.inf}
    for (c, t, k), v in spots.items():
        spec[c, t, k] = v
    spec[1, 101, 20] = 0.0                                                 # finite values after an inf
    touched = np.zeros((2, F), dtype=bool)
    first = {}
    for (c, t, k) in spots:
        touched[c, k] = True
        first[c, k] = min(t, first.get((c, k), t))
    a, b = Slab(clean), Slab(spec)
    for mode in ad.MODES:
        for nb in (0, 7):
            got, ref = run(b, nb, mode), run(a, nb, mode)
            want = ad.adapt(spec, nb, SMOOTH, mode, dtype=np.float64)
            assert ad.same_pattern(got, want), mode
            for (c, k), t0 in first.items():                               # in front of t0 the column is the clean one
                assert ad.exact_bits(got[c, :max(t0 - nb, 0), k], ref[c, :max(t0 - nb, 0), k]), (mode, c, k)
            for c in range(2):
                assert ad.exact_bits(got[c][:, ~touched[c]], ref[c][:, ~touched[c]]), 'a neighbouring column changed'
    a.free()
    b.free()


def test_scratch_contents_do_not_matter():
    from audian_amd import hipdsp
    rng = np.random.default_rng(24)
    spec = ad.decades_slab(rng, 3, 3*L + 7, 65)
    c = hipdsp.Context(0)
    slab = Slab(spec, c=c)
    try:
        plain = {mode: run(slab, 9, mode) for mode in ad.MODES}
        for fill in (0x00, 0xff):
            c.set_option('scratch_fill', fill + 1)
            for mode in ad.MODES:
                assert ad.exact_bits(run(slab, 9, mode), plain[mode]), (mode, fill)
    finally:
        c.set_option('scratch_fill', 0)
        slab.free()


def test_one_capture_replayed_twice():
    """A 3 L + 7 frame call captured once after hipdsp_ctx_reserve and replayed twice, on new slab contents the second
    time: the bytes of the direct call.  Without the reserve the capture is refused, and nothing is written."""
    from audian_amd import hipdsp
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    rng = np.random.default_rng(25)
    C, frames, F = 2, 3*L + 7, 65
    specs = [ad.decades_slab(rng, C, frames, F) for _ in range(2)]
    ds = hipdsp.DeviceArray.from_host(c, specs[0])
    do = hipdsp.DeviceArray.from_host(c, np.full((C, frames - 4, F), SENT, dtype=np.float32))
    c.graph_begin()
    with pytest.raises(ValueError):
        hipdsp.spec_adapt(c, ds, 0, do, 0, C, frames, F, 4, SMOOTH, 'pcen')
    c.graph_destroy(c.graph_end())
    c.synchronize()
    assert np.all(do.to_host() == SENT)
    c.reserve(hipdsp.adapt_scratch_bytes(C, frames, F))
    c.graph_begin()
    hipdsp.spec_adapt(c, ds, 0, do, 0, C, frames, F, 4, SMOOTH, 'pcen')
    graph = c.graph_end()
    try:
        for spec in specs:
            ds.copy_from_host(spec)
            do.copy_from_host(np.full((C, frames - 4, F), SENT, dtype=np.float32))
            c.graph_launch(graph)
            c.synchronize()
            got = do.to_host()
            direct = hipdsp.DeviceArray(c, (C, frames - 4, F), np.float32)
            hipdsp.spec_adapt(c, ds, 0, direct, 0, C, frames, F, 4, SMOOTH, 'pcen')
            assert ad.exact_bits(got, direct.to_host())
            direct.free()
            assert ad.Definition(spec, SMOOTH).within(got, 4, 'pcen')[0]
    finally:
        c.graph_destroy(graph)
        c.set_stream(None)
        c.destroy_stream(stream)


def test_far_placement_gives_the_bits_of_the_near_one():
    """Input and output windows of whole frames past 2^31 elements from the pointer (2^33 bytes), which itself lies 2^31
    elements into a NaN-filled block (far_placement.slab_windows): an index or byte offset wrapped to 32 bits stays inside
    the block and reads NaN or misses the output window.  Bit for bit the result of the same slab near the start."""
    from audian_amd import hipdsp
    from audian_amd._lib import check as st, lib
    c = gh.ctx()
    rng = np.random.default_rng(26)
    F, frames, nb = fp.SLAB_F, L + 1, 5
    spec = ad.decades_slab(rng, 1, frames, F)
    windows = {w.name: w for w in fp.slab_windows(rows=frames)}
    near, past, straddle = windows['near'], windows['past'], windows['elem_2_31']
    fp.check_disjoint([near, past, straddle])
    block = hipdsp.DeviceArray(c, (fp.BLOCK,), np.float32)
    try:
        st(lib.hipdsp_memset(c.handle, ctypes.c_void_p(block.ptr), 0xff, block.nbytes))
        results = {}
        for name, src, dst in (('near', near, straddle), ('far', past, straddle), ('far out', near, past)):
            if name == 'far out':
                # (the input moves back to the near window; the past window becomes the output)
                st(lib.hipdsp_memset(c.handle, ctypes.c_void_p(block.ptr), 0xff, block.nbytes))
            block.view(fp.MID + src.start, (frames*F,)).copy_from_host(spec.ravel())
            n_out = (frames - nb)*F
            guard = dst.guard
            block.view(fp.MID + dst.start - guard, (n_out + 2*guard,)).copy_from_host(np.full(n_out + 2*guard, SENT, dtype=np.float32))
            hipdsp.spec_adapt(c, block.view(fp.MID + src.start, (1,)), 0, block.view(fp.MID + dst.start, (1,)), 0, 1, frames, F,
                              nb, SMOOTH, 'pcen')
            got = block.view(fp.MID + dst.start - guard, (n_out + 2*guard,)).to_host()
            assert np.all(got[:guard] == SENT) and np.all(got[guard + n_out:] == SENT), name
            results[name] = got[guard:guard + n_out].reshape(1, frames - nb, F)
            assert ad.exact_bits(block.view(fp.MID + src.start, (frames*F,)).to_host(), spec.ravel()), name
    finally:
        c.synchronize()
        block.free()
    small = Slab(spec)
    want = run(small, nb, 'pcen')
    small.free()
    for name, got in results.items():
        assert not np.any(np.isnan(got)), name
        assert ad.exact_bits(got, want), name


# ---- the facade ------------------------------------------------------------------------------------------------------

def device_db(power, floor):
    """v of the template match's definition: hipdsp_decibel on the same values, clamped on the host."""
    from audian_amd import hipdsp
    c = gh.ctx()
    power = np.ascontiguousarray(power, dtype=np.float32)
    d = hipdsp.DeviceArray.from_host(c, power)
    o = hipdsp.DeviceArray(c, power.shape, np.float32)
    hipdsp.decibel(c, d, o, power.size, 1.0, 0.0)
    v = o.to_host()
    d.free()
    o.free()
    return np.where(v < np.float32(floor), np.float32(floor), v)


def rule_bound(got, want, allow):
    got32 = np.ascontiguousarray(got, dtype=np.float32).astype(ad.LD)
    return ~(np.abs(got32 - want) <= allow)


class Ledger(fl.Ledger):
    """facade_ledger.Ledger with the one definition it lacks: the adaptive trace against the longdouble definition on
    the source slab as the device holds it, with the lead that call used."""

    @staticmethod
    def _step_of(t):
        from audian_amd.bufferedadaptivespectrogram import BufferedAdaptiveSpectrogram
        return 1 if isinstance(t, BufferedAdaptiveSpectrogram) else fl.Ledger._step_of(t)

    def _define(self, t, slab, nbefore, n, first, soffset):
        from audian_amd.bufferedadaptivespectrogram import BufferedAdaptiveSpectrogram
        if not isinstance(t, BufferedAdaptiveSpectrogram):
            return fl.Ledger._define(self, t, slab, nbefore, n, first, soffset)
        self.leads.append(nbefore)
        assert len(slab) == nbefore + n
        assert nbefore == min(t.warmup_frames(), soffset + nbefore), 'the lead is the warm-up, clamped to the source buffer'
        d = ad.Definition(np.ascontiguousarray(slab, dtype=np.float32).transpose(1, 0, 2), t.smooth)
        kw = dict(gain=t.gain, bias=t.bias, power=t.power, eps=t.eps)
        want = d.value(t.mode, **kw)[:, nbefore:].transpose(1, 0, 2)
        allow = d.bound(t.mode, **kw)[:, nbefore:].transpose(1, 0, 2)
        return fl.Segment(first, rule_bound, want=want, allow=allow)


def test_walk_of_the_adaptive_graph(oracle):
    """data -> filtered -> spectrogram (256 / 128) -> adaptive -> bandpower, match: scrolled, jumped and update()d; after
    every action every frame equals the definition on the source slab of the call that wrote it."""
    from audian_amd import hipdsp
    from audian_amd.bufferedadaptivespectrogram import BufferedAdaptiveSpectrogram
    from audian_amd.bufferedbandpower import BufferedBandPower
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
    from audian_amd.tracegraph import TraceGraph
    x = fl.recording(40.0, 78)
    g = TraceGraph(2.5, 0.5)
    for t in (BufferedFilter(name='filtered', source='data'),
              BufferedSpectrogram(name='spectrogram', source='filtered', nfft=256, overlap_frac=0.5),
              BufferedAdaptiveSpectrogram(name='adaptive', source='spectrogram', time_constant=0.2, warmup=5.0),
              BufferedBandPower(name='bandpower', source='adaptive', fmin=1000.0, fmax=3000.0),
              BufferedTemplateMatch(name='match', source='adaptive')):
        g.add_trace(t)
    g.setup_traces()
    g.open(x, fl.RATE)
    for t in g.traces:
        t.plot_items = [fl.Item() for _ in range(t.channels)]
    g.set_need_update()
    f, s, a, bp, m = (g[n] for n in ('filtered', 'spectrogram', 'adaptive', 'bandpower', 'match'))
    ledger = Ledger(g, oracle, db=device_db)
    ledger.leads = []
    before = dict(hipdsp.launches)

    def launched(name):
        return hipdsp.launches.get(name, 0) - before.get(name, 0)

    def done(what):
        for t in (a, bp, m):
            assert (t.rate, t.offset, len(t._hostbuf)) == (s.rate, s.offset, len(s._hostbuf)), (what, t.name)
        assert a.shape == s.shape and (a.nfft, a.hop, a.fresolution) == (s.nfft, s.hop, s.fresolution)
        try:
            ledger.check()
        except AssertionError as err:
            raise AssertionError('%s\n  after: %s' % (err, what))

    g.update_times(0.0, 1.5)
    done('window 0')
    assert a.unit == '' and a.mode == 'pcen' and a.lead == 0 and launched('spec_adapt') >= 1
    assert a._mirror_valid(0, len(a._hostbuf))
    f.highpass_cutoff, f.lowpass_cutoff = 300.0, 3500.0
    f.update()
    done('filter')
    want_lead = a.warmup_frames()
    assert want_lead == int(np.ceil(5.0*0.2*a.rate)) and want_lead > 0
    for t0, t1 in ((0.6, 2.0), (0.9, 2.3), (14.0, 15.5), (15.2, 16.7), (27.0, 28.5), (28.1, 29.6), (3.0, 4.5), (38.6, 40.0)):
        g.update_times(t0, t1)
        done('window %.1f' % t0)
    # a scroll forward that keeps fewer frames of the buffer than the warm-up asks for: the lead is what the source holds.
    # The buffer starts a fixed time in front of the window's start (back time and margins), which the jump shows.
    g.update_times(10.0, 11.5)
    done('jump back to 10.0')
    ahead = 10.0 - a.offset/a.rate
    old_end = a.offset + len(a._hostbuf)
    t0 = (old_end - want_lead//2)/a.rate + ahead
    g.update_times(t0, t0 + 1.5)
    done('forward to %.3f' % t0)
    kept = old_end - a.offset
    assert 0 < kept < want_lead, (kept, want_lead, a.offset, old_end)
    assert ledger.leads[-1] == kept == a.lead, (ledger.leads[-3:], kept)
    assert ledger.stats['adaptive']['partial'] >= 1, (ledger.stats, ledger.leads)
    assert max(ledger.leads) == want_lead and min(ledger.leads) == 0, ledger.leads
    spec_calls = ledger.stats['spectrogram']['calls']
    whole = ledger.stats['adaptive']['whole']
    for kw in (dict(mode='divide'), dict(mode='subtract'), dict(mode='background'), dict(mode='pcen', time_constant=0.4),
               dict(gain=0.5, bias=1.0, power=0.25, eps=1e-12)):
        a.update(**kw)
        done('update %r' % (kw,))
        assert a.unit == ('' if a.mode in ('pcen', 'divide') else s.unit)
    assert ledger.stats['adaptive']['whole'] == whole + 5 and ledger.stats['spectrogram']['calls'] == spec_calls
    n0 = launched('spec_adapt')
    for kw in (dict(mode='multiply'), dict(gain=1.5), dict(eps=0.0), dict(power=0.0), dict(time_constant=0.0), dict(bias=-1.0)):
        with pytest.raises(ValueError):
            a.update(**kw)
    assert launched('spec_adapt') == n0 and (a.mode, a.gain, a.eps, a.power, a.time_constant) == ('pcen', 0.5, 1e-12, 0.25, 0.4)
    g.update_times(37.5, 39.0)
    done('window 37.5')
    # a consumer by name: a template cut from the adaptive image and matched against it
    tm = g.cut_template(38.3, 38.3 + 12/s.rate, 1500.0, 3000.0, 0, spec_name='adaptive', floor_db=-40.0)
    m.set_template(tm)
    done('set_template')
    assert np.nanmax(fl.peek(m)[:, 0]) > 0.9
    events, best, score = g.detect_calls([tm], 0.7, spec_name='adaptive')
    assert len(events.onsets[0]) >= 1
    for t in (a, bp, m):
        assert t._mirror_valid(0, len(t._hostbuf)), t.name
    for name in ('spec_adapt', 'band_power', 'template_match'):
        assert launched(name) > 0, name
    ledger.close()
