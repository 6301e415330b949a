"""A shadow of every load of every derived trace of a TraceGraph, and the walks that are run under it.

``Ledger(graph, oracle)`` wraps ``process`` of every derived trace as an INSTANCE attribute (``type(t).process`` stays the
built-in one, so ``_builtin()`` and the fused launches are unaffected).  At every call it reads where the call sits
(``trace._pending``), lets the real ``process()`` run, reads the source slab as the device holds it WITHOUT touching the
source's ``_stale`` (the mirror, per channel; the loader's host array rounded to float32), applies the trace's definition to
that slab and writes the expected values and their allowances into a table keyed by the absolute frame of the trace.
``check()`` then demands that every frame of every trace's current buffer has an entry -- a frame without one is a frame
nobody computed -- and agrees with it under that trace's rule.  Every definition is one the suite already keeps in tests/ or
the oracle; no host fallback of the package is a comparator (power_envelope_definition.host_power_envelope is what that
module hands out for the power envelope).

The rules (1e-4 is the project's parity tolerance, BASELINE north_star and TOL of the older walks; the kernels' tight bounds
are held by their own tests, a misplaced strip is off by order one):

  rereferenced     common_reference_definition.common_reference                        bit for bit
  filtered, envelope, spectrogram    oracle.filter_process / envelope_process / spectrogram_process
                                     |got - want| < 1e-4 max|want| per channel and call (per frame: spectrogram); an
                                     all-zero reference wants all zeros
  BufferedLowpass  oracle.sosfiltfilt                                                  the same 1e-4
  power-envelope   power_envelope_definition.host_power_envelope                       the same 1e-4
  BufferedKernelFilter   fir_definition.fir_definition(..., with_abs=True)             fir_bound per output; non-finite
                                                                                       samples by the header's rule
  bandpower        float32(scale * sum in float64 over [k0, k1))                       1 float32 ulp; in dB decibel_bound
  peakfreq         spectral_features_definition.slab_features                          its compare()
  match            template_match_definition.prepare / scores on the source's buffer   its bound; NaN pattern exact outside
                                                                                       `near` (at most 1 % of a call)
  eventfiltered    the source, regions inside the buffer replaced by iir_bound.sosfiltfilt (what refine_definition
                   restates scipy's sosfiltfilt with) rounded to float32               copy bit for bit, regions 1e-4

The absolute grid is checked without _load_geometry: dest frame j belongs to source frame j*step of the recording (kernel
filter, power envelope), j*hop (spectrogram), j (everything else)."""

from math import floor

import numpy as np

import common_reference_definition as cd
import decibel_bound as dbb
import iir_bound as ib
import power_envelope_definition as pd
import spectral_features_definition as sd
import template_match_definition as td
from fir_definition import fir_bound, fir_definition

TOL = 1e-4
NEAR_CAP = 0.01


class Item:
    def isVisible(self):
        return True


# ---- reading without flushing --------------------------------------------------------------------------------------------

def mirror_read(t, a, n):
    """Frames [a, a + n) of the device mirror of `t`, channel by channel: (n, channels[, F]) float32."""
    inner = t._inner()
    tail = tuple(t._hostbuf.shape[2:])
    out = np.empty((n, t.channels) + tail, dtype=np.float32)
    for ch in range(t.channels):
        out[:, ch] = t._dev.view(ch*t._pitch() + a*inner, (n*inner,)).to_host().reshape((n,) + tail)
    return out


def peek(t, a=0, n=None):
    """What reading frames [a, a + n) of t.buffer would give, without flushing: the host copy, the stale ranges from the
    mirror.  A stale range without a valid mirror is a broken invariant."""
    n = len(t._hostbuf) - a if n is None else n
    out = np.array(t._hostbuf[a:a + n], dtype=np.float64)
    for r0, r1 in t._stale:
        lo, hi = max(r0, a), min(r1, a + n)
        if hi > lo:
            assert t._mirror_valid(lo, hi), '%s: frames %d-%d are stale on the host and not valid on the mirror' % (
                t.name, t.offset + lo, t.offset + hi)
            out[lo - a:hi - a] = mirror_read(t, lo, hi - lo)
    return out


def source_slab(src, a, n):
    """Frames [a, a + n) of the source's buffer as the device holds them."""
    from audian_amd.buffereddata import BufferedData
    if not isinstance(src, BufferedData):
        return np.asarray(src.buffer[a:a + n]).astype(np.float32)
    if src._mirror_valid(a, a + n):
        return mirror_read(src, a, n)
    return peek(src, a, n)


# ---- the rules ----------------------------------------------------------------------------------------------------------------

def judge(got, want, allow, strict=False, exempt=None, finite_only=False):
    """Mask of the elements of `got` that miss `want`: |got - want| <= allow (< allow with `strict`; allow == 0: equal), NaN
    exactly where `want` has it and infinities equal -- with `finite_only` non-finite exactly where `want` is -- except
    the `exempt` elements."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    allow = np.broadcast_to(np.asarray(allow, dtype=np.float64), want.shape)
    with np.errstate(invalid='ignore'):
        if finite_only:
            bad = np.isfinite(got) != np.isfinite(want)
            fin = np.isfinite(got) & np.isfinite(want)
        else:
            bad = np.isnan(got) != np.isnan(want)
            inf = np.isinf(want)
            bad |= inf & ~(got == want)
            fin = ~np.isnan(want) & ~inf & ~np.isnan(got)
        err = np.abs(np.where(fin, got - want, 0.0))
        over = np.where(allow == 0, err > 0, err >= allow if strict else err > allow)
    bad |= fin & over
    if exempt is not None:
        bad &= ~np.broadcast_to(exempt, bad.shape)
    return bad


def rel_allowance(want, axes):
    """TOL * max|want| over `axes` (the finite elements): rel_err < TOL, element by element."""
    w = np.where(np.isfinite(want), np.abs(want), 0.0)
    return np.broadcast_to(TOL*np.max(w, axis=axes, keepdims=True, initial=0.0), want.shape)


class Segment(object):
    """What one call left for frames [a, a + n) of a trace: arrays with the frames on axis 0, and the rule over them."""

    def __init__(self, a, rule, **arrays):
        self.a, self.rule, self.arrays = int(a), rule, arrays
        self.n = len(next(iter(arrays.values())))

    def cut(self, lo, hi):
        lo, hi = max(lo, self.a), min(hi, self.a + self.n)
        if hi <= lo:
            return None
        return Segment(lo, self.rule, **{k: v[lo - self.a:hi - self.a] for k, v in self.arrays.items()})


def rule_tol(strict=False, finite_only=False):
    def rule(got, want, allow, exempt=None):
        return judge(got, want, allow, strict, exempt, finite_only)
    return rule


def rule_decibel(min_power):
    def rule(got, p32, arg):
        mask = dbb.judge(np.ascontiguousarray(got, dtype=np.float32), p32, 1.0, min_power, extra=1, arg=arg)[2]
        return mask
    return rule


def rule_feature(bit):
    def rule(got, V, T):
        got32 = np.ascontiguousarray(got, dtype=np.float32)[None]
        try:
            sd.compare(got32, V_of(V), T_of(T), 1 << bit)
            return np.zeros(got.shape, bool)
        except AssertionError:
            bad = np.zeros(got.shape, bool)
            for i in range(len(got)):
                try:
                    sd.compare(got32[:, i:i + 1], V_of(V[i:i + 1]), T_of(T[i:i + 1]), 1 << bit)
                except AssertionError:
                    bad[i] = True
            return bad
    return rule


def V_of(v):
    """(frames, channels, 8) as kept in a segment -> (8, frames, channels) as compare() takes it."""
    return np.moveaxis(v, -1, 0)


T_of = V_of


# ---- the ledger --------------------------------------------------------------------------------------------------------------

class Ledger(object):

    def __init__(self, graph, oracle, db=None, only=None):
        """`db(power, floor)`: the dB values of the template match's definition, which takes them as given (the GPU tests
        obtain them from hipdsp_decibel; by default templates.host_values).  `only`: the names of the traces to shadow
        (by default every derived trace)."""
        from audian_amd.bufferedeventfilter import BufferedEventFilter
        self.graph, self.oracle, self.db = graph, oracle, db
        self.traces = [t for t in graph.traces[1:] if only is None or t.name in only]
        self.table = {t.name: [] for t in self.traces}
        self.grid = {t.name: None for t in self.traces}
        self.stats = {t.name: {'partial': 0, 'whole': 0, 'calls': 0} for t in self.traces}
        self.carries = 0
        self.near = [0, 0]
        self.checks = 0
        for t in self.traces:
            if isinstance(t, BufferedEventFilter):
                t.load_buffer = self._wrap_event_filter(t, t.load_buffer)
            else:
                t.process = self._wrap(t, t.process)
            t._adopt_buffer = self._wrap_adopt(t, t._adopt_buffer)

    def close(self):
        """Take the wrappers off again (what the traces had as instance attributes before is not put back)."""
        for t in self.traces:
            for name in ('process', 'load_buffer', '_adopt_buffer'):
                vars(t).pop(name, None)

    def _wrap_adopt(self, t, real):
        def adopt(*args):
            self.carries += bool(t._carry)
            return real(*args)
        return adopt

    def _wrap(self, t, real):
        def process(source, dest, nbefore):
            call = t._pending
            pos = None if call is None else (call.soffset, call.snframes, call.doffset, call.dnframes)
            real(source, dest, nbefore)
            if pos is not None and pos[3] > 0:
                self._record(t, pos, nbefore)
        return process

    def _wrap_event_filter(self, t, real):
        def load_buffer(offset, nframes, buffer):
            real(offset, nframes, buffer)
            n = len(t._hostbuf)
            if n > 0:
                self._count(t, nframes, n)
                self._record_event_filter(t)
        return load_buffer

    def _count(self, t, dn, n):
        s = self.stats[t.name]
        s['calls'] += 1
        s['partial' if 0 < dn < n else 'whole'] += 1

    def _put(self, t, seg):
        """The call's entries replace what the table held for these frames; another grid (rate, shape) drops the table."""
        grid = (t.rate, tuple(t.shape[1:]))
        if self.grid[t.name] != grid:
            self.grid[t.name], self.table[t.name] = grid, []
        rows = []
        for s in self.table[t.name]:
            rows.extend(p for p in (s.cut(s.a, seg.a), s.cut(seg.a + seg.n, s.a + s.n)) if p is not None)
        rows.append(seg)
        self.table[t.name] = rows

    @staticmethod
    def _step_of(t):
        from audian_amd.bufferedkernelfilter import BufferedKernelFilter
        from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
        from audian_amd.bufferedspectrogram import BufferedSpectrogram
        if isinstance(t, BufferedSpectrogram):
            return t.hop
        if isinstance(t, (BufferedKernelFilter, BufferedPowerEnvelope)):
            return t.step
        return 1

    def _record(self, t, pos, nbefore):
        soffset, snframes, doffset, dnframes = pos
        src = t.source
        self._count(t, dnframes, len(t._hostbuf))
        assert doffset >= 0 and doffset + dnframes <= len(t._hostbuf), (t.name, pos)
        assert soffset >= 0 and soffset + snframes <= t._source_len(), (t.name, pos)
        # the absolute grid
        first = t.offset + doffset
        at = src.offset + soffset + nbefore
        ahead = at - first*self._step_of(t)
        assert 0 <= ahead <= max(nbefore, 0), \
            '%s: frame %d belongs to source frame %d, the call starts at %d' % (t.name, first, first*self._step_of(t), at)
        slab = source_slab(src, soffset, snframes)
        self._put(t, self._define(t, slab, nbefore, dnframes, first, soffset))

    # ---- the definitions ------------------------------------------------------------------------------------------------
    def _define(self, t, slab, nbefore, n, first, soffset):
        from audian_amd.bufferedbandpower import BufferedBandPower
        from audian_amd.bufferedcommonreference import BufferedCommonReference
        from audian_amd.bufferedenvelope import BufferedEnvelope
        from audian_amd.bufferedfilter import BufferedFilter
        from audian_amd.bufferedkernelfilter import BufferedKernelFilter
        from audian_amd.bufferedlowpass import BufferedLowpass
        from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
        from audian_amd.bufferedspectralfeature import BufferedSpectralFeature
        from audian_amd.bufferedspectrogram import BufferedSpectrogram
        from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
        oracle = self.oracle
        C = t.channels
        if isinstance(t, BufferedCommonReference):
            x = np.ascontiguousarray(slab.astype(np.float32).T)
            want = cd.common_reference(x, t.group, t.use, t.method).T[nbefore:nbefore + n]
            return Segment(first, rule_tol(), want=want.astype(np.float64), allow=np.zeros(want.shape))
        if isinstance(t, (BufferedFilter, BufferedEnvelope, BufferedLowpass, BufferedPowerEnvelope)):
            x = np.ascontiguousarray(slab, dtype=np.float64)
            want = np.zeros((n, C))
            with np.errstate(all='ignore'):
                if isinstance(t, BufferedFilter):
                    oracle.filter_process(t.sos, x, want, nbefore)
                elif isinstance(t, BufferedEnvelope):
                    oracle.envelope_process(t.sos, x, want, nbefore, t.highpass_cutoff)
                elif isinstance(t, BufferedLowpass):
                    if t.sos is not None:
                        want[:] = oracle.sosfiltfilt(t.sos, x)[nbefore:nbefore + n]
                elif t.sos is not None:
                    want[:] = pd.host_power_envelope(t.sos, x, nbefore, t.step, n, t.gain, t.root)
            return Segment(first, rule_tol(strict=True, finite_only=True), want=want, allow=rel_allowance(want, 0))
        if isinstance(t, BufferedSpectrogram):
            want = np.zeros((n, C, t.nfft//2 + 1))
            with np.errstate(all='ignore'):
                oracle.spectrogram_process(np.ascontiguousarray(slab, dtype=np.float64), want, t.source.rate, t.nfft, t.hop)
            return Segment(first, rule_tol(strict=True, finite_only=True), want=want, allow=rel_allowance(want, 2))
        if isinstance(t, BufferedKernelFilter):
            x = np.ascontiguousarray(np.asarray(slab, dtype=np.float64).T)
            with np.errstate(all='ignore'):
                y, m = fir_definition(x, t.kernel[None, :], nbefore, t.step, n, with_abs=True)
                want = np.maximum(y[0] - t.threshold, 0.0) if t.threshold is not None else y[0]
                allow = fir_bound(m[0], len(t.kernel), t.threshold)
            # non-finite samples by the header's rule (hipdsp_fir_bank): an output whose window holds one is non-finite
            # (rectified: max(-inf, 0) is 0, so anything goes), the taps' zero padding may carry that up to 16 samples
            # further, and 16 samples clear of every such sample the output is what the definition gives
            L, lead = len(t.kernel), (len(t.kernel) - 1)//2
            count = np.concatenate((np.zeros((C, 1), np.int64), np.cumsum(~np.isfinite(x), axis=1)), axis=1)
            hi = nbefore + t.step*np.arange(n) + lead
            lo = hi - (L - 1)

            def holds(margin):
                a = np.clip(lo - margin, 0, x.shape[1])
                b = np.clip(hi + margin + 1, 0, x.shape[1])
                return (count[:, b] - count[:, a]) > 0

            inside, near = holds(0), holds(16)
            must = inside & (t.threshold is None)
            fin = np.isfinite(want) & np.isfinite(allow) & ~must
            return Segment(first, rule_tol(finite_only=True), want=np.where(fin, want, np.nan).T,
                           allow=np.where(fin, allow, 0.0).T, exempt=(near & ~must).T)
        if isinstance(t, BufferedSpectralFeature):
            V, T = sd.slab_features(slab[nbefore:nbefore + n], t.k0, t.k1, t.scale, t.min_power, sd.drop_ratio(t.drop_db))
            bit = sd.NAMES.index(t.feature)
            return Segment(first, rule_feature(bit), V=np.moveaxis(V, 0, -1), T=np.moveaxis(T, 0, -1))
        if isinstance(t, BufferedBandPower):
            spec = np.asarray(slab[nbefore:nbefore + n], dtype=np.float32)
            with np.errstate(all='ignore'):
                if t.log:
                    arg = np.longdouble(t.scale)*np.sum(spec[:, :, t.k0:t.k1].astype(np.longdouble), axis=2)
                    return Segment(first, rule_decibel(t.min_power), p32=arg.astype(np.float32), arg=arg)
                want = (t.scale*np.sum(spec[:, :, t.k0:t.k1], axis=2, dtype=np.float64)).astype(np.float32)
                allow = np.where(np.isfinite(want), np.spacing(np.abs(want)), 0.0).astype(np.float64)
            return Segment(first, rule_tol(), want=want.astype(np.float64), allow=allow)
        if isinstance(t, BufferedTemplateMatch):
            return self._define_match(t, nbefore, n, first, soffset)
        raise AssertionError('%s: no definition for %s' % (t.name, type(t).__name__))

    def _define_match(self, t, nbefore, n, first, soffset):
        """The scores on the span of the source's buffer at call time: exactly NaN where the window leaves it, all NaN while
        the template is stale or there is none."""
        from audian_amd.templates import default_pivot, host_values
        C = t.channels
        nan = np.full((n, C), np.nan)
        if t.template is None or t.stale:
            return Segment(first, rule_tol(), want=nan, allow=np.zeros((n, C)), exempt=np.zeros((n, C), bool))
        tm, src = t.template, t.source
        Tt = tm.values.shape[0]
        s0 = soffset + nbefore
        lo, hi = max(0, s0 - Tt//2), min(t._source_len(), s0 + n - 1 - Tt//2 + Tt)
        power = source_slab(src, lo, hi - lo)
        if not tm.log:
            v = np.asarray(power, dtype=np.float64)
        elif self.db is None:
            v = host_values(np.asarray(power, dtype=np.float64), True, tm.floor)
        else:
            v = self.db(np.ascontiguousarray(power, dtype=np.float32), tm.floor)
        taps = td.prepare(tm.values, t.normalize)[0]
        pivot = default_pivot(tm.values) if t.pivot is None else t.pivot
        ref = td.scores(np.ascontiguousarray(np.moveaxis(v, 1, 0)), taps, t.k0, s0 - Tt//2 - lo, n, t.normalize, t.min_std, pivot)
        near = ref['near'].T if t.normalize else np.zeros((n, C), bool)
        self.near[0] += int(near.sum())
        self.near[1] += near.size
        assert near.mean() <= NEAR_CAP, '%s: %d of %d windows undecided at the mask' % (t.name, near.sum(), near.size)
        want, bound = ref['value'][0].T, ref['bound'][0].T
        outside = (np.arange(n) + s0 - Tt//2 < 0) | (np.arange(n) + s0 - Tt//2 + Tt > t._source_len())
        assert np.all(np.isnan(want[outside]))
        near = near & ~outside[:, None]
        return Segment(first, rule_tol(), want=want, allow=np.where(np.isfinite(bound), bound, 0.0), exempt=near)

    def _record_event_filter(self, t):
        src = t.source
        n, C = len(t._hostbuf), t.channels
        a = t.offset - src.offset
        assert 0 <= a and a + n <= t._source_len(), '%s: frames %d-%d are not in the source buffer' % (
            t.name, t.offset, t.offset + n)
        slab = source_slab(src, a, n)
        want = slab.astype(np.float32).astype(np.float64)
        allow = np.zeros((n, C))
        lo, hi = t.offset, t.offset + n
        cut = []
        for (c, r0, r1), sos in zip(t.regions.tolist(), t.sos):
            if r0 >= lo and r1 <= hi:
                x = want[r0 - lo:r1 - lo, c].copy()
                if np.all(np.isfinite(x)):
                    y = ib.sosfiltfilt(sos, x[:, None], np.float64, gain=1.0, rectify=False, clamp=False)[:, 0]
                    y = y.astype(np.float32).astype(np.float64)
                    if t.clamp:
                        y = np.where(y < 0, 0.0, y)
                else:
                    y = np.full(len(x), np.nan)
                want[r0 - lo:r1 - lo, c] = y
                allow[r0 - lo:r1 - lo, c] = TOL*np.max(np.abs(y), initial=0.0) if np.all(np.isfinite(y)) else 0.0
            elif r0 < hi and r1 > lo:
                cut.append((c, r0, r1))
        assert sorted(t.skipped) == sorted(cut), '%s: skipped %r, the border cuts %r' % (t.name, t.skipped, cut)
        self._put(t, Segment(lo, rule_tol(strict=True), want=want, allow=allow))

    # ---- the check ------------------------------------------------------------------------------------------------------
    def check(self, flush=None):
        """Every frame of every buffer has an entry and agrees with it.  Alternating: through trace.buffer, which flushes,
        and through the mirror, which leaves _stale alone."""
        flush = self.checks % 2 == 1 if flush is None else flush
        self.checks += 1
        for t in self.traces:
            off, n = t.offset, len(t._hostbuf)
            got = np.asarray(t.buffer, dtype=np.float64) if flush else peek(t)
            assert got.shape == t._hostbuf.shape
            rows = [p for p in (s.cut(off, off + n) for s in self.table[t.name]) if p is not None]
            if self.grid[t.name] != (t.rate, tuple(t.shape[1:])):
                rows = []
            self.table[t.name] = rows
            covered = np.zeros(n, bool)
            for s in rows:
                covered[s.a - off:s.a - off + s.n] = True
            if not covered.all():
                i = int(np.argmin(covered))
                raise AssertionError('%s: frame %d (index %d of %d in the buffer) was computed by no call'
                                     % (t.name, off + i, i, n))
            for s in rows:
                bad = s.rule(got[s.a - off:s.a - off + s.n], **s.arrays)
                if bad.any():
                    at = np.argwhere(bad)[0]
                    i = int(at[0])
                    want = s.arrays.get('want')
                    raise AssertionError('%s: frame %d (index %d of %d in the buffer) element %s: got %r%s; %d elements of '
                                         'the entry written for frames %d-%d differ'
                                         % (t.name, s.a + i, s.a + i - off, n, at[1:].tolist(),
                                            got[(s.a - off + i,) + tuple(at[1:])],
                                            '' if want is None else ', want %r' % (want[tuple(at)],), int(bad.sum()),
                                            s.a, s.a + s.n))


# ---- the graph, the recording, the walk ----------------------------------------------------------------------------------------

RATE, CHANNELS = 8000.0, 3
CHIRP_AT, CHIRP_LEN, CHIRP_F = 0.3, 0.1, (1500.0, 3000.0)      # an up-chirp on channel 0 in every second


def recording(seconds, seed, poison=0):
    """Noise floor, an amplitude-modulated carrier, an up-chirp per second on channel 0, a loud last channel; float32-exact."""
    rng = np.random.default_rng(seed)
    n = int(RATE*seconds)
    t = np.arange(n)/RATE
    x = 0.02*rng.standard_normal((n, CHANNELS))
    for c in range(CHANNELS):
        x[:, c] += 0.3*np.sin(2*np.pi*(700.0 + 300*c)*t)*(1 + np.sin(2*np.pi*3*t))/2
    tc = (t % 1.0) - CHIRP_AT
    on = (tc >= 0) & (tc < CHIRP_LEN)
    sweep = CHIRP_F[0]*tc + 0.5*(CHIRP_F[1] - CHIRP_F[0])/CHIRP_LEN*tc**2
    x[:, 0] += np.where(on, 0.5*np.sin(2*np.pi*sweep)*np.sin(np.pi*tc/CHIRP_LEN)**2, 0.0)
    x[:, CHANNELS - 1] *= 4.0
    x = x.astype(np.float32).astype(np.float64)
    for _ in range(poison):
        x[int(rng.integers(0, n)), int(rng.integers(0, CHANNELS))] = rng.choice([np.nan, np.nan, np.inf, -np.inf])
    return x


def device_classes():
    from audian_amd.bufferedcommonreference import BufferedCommonReference
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    return BufferedCommonReference, BufferedFilter, BufferedEnvelope, BufferedSpectrogram


def build_graph(classes, x, buffer_time, back_time, nfft, step, below, swap=None):
    """data -> rereferenced -> filtered -> envelope -> features -> below;  envelope -> eventfiltered;
    filtered -> spectrogram -> bandpower, peakfreq, match;  filtered -> power-envelope -> slow-envelope.
    `swap`: {name: class} takes another class (a subclass) for that trace."""
    from audian_amd.bufferedbandpower import BufferedBandPower
    from audian_amd.bufferedeventfilter import BufferedEventFilter
    from audian_amd.bufferedkernelfilter import BufferedKernelFilter
    from audian_amd.bufferedlowpass import BufferedLowpass
    from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
    from audian_amd.bufferedspectralfeature import BufferedSpectralFeature
    from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
    from audian_amd.tracegraph import TraceGraph
    R, F, E, S = classes
    traces = [(R, 'rereferenced', 'data', {}), (F, 'filtered', 'rereferenced', {}),
              (E, 'envelope', 'filtered', dict(envelope_cutoff=200.0)),
              (BufferedKernelFilter, 'features', 'envelope', dict(kernel=np.hanning(11)[1:-1]/5.0, step=step)),
              (BufferedKernelFilter, 'below', 'features', dict(kernel=np.array([0.25, 0.5, 0.25]), step=2))
              if below == 'kernel' else (BufferedLowpass, 'below', 'features', dict(cutoff=20.0)),
              (BufferedEventFilter, 'eventfiltered', 'envelope', {}),
              (S, 'spectrogram', 'filtered', dict(nfft=nfft, overlap_frac=0.5)),
              (BufferedBandPower, 'bandpower', 'spectrogram', dict(fmin=1000.0, fmax=3000.0)),
              (BufferedSpectralFeature, 'peakfreq', 'spectrogram', dict(fmin=500.0, fmax=3500.0)),
              (BufferedTemplateMatch, 'match', 'spectrogram', {}),
              (BufferedPowerEnvelope, 'power-envelope', 'filtered', dict(envelope_cutoff=100.0)),
              (BufferedLowpass, 'slow-envelope', 'power-envelope', dict(cutoff=5.0))]
    g = TraceGraph(buffer_time, back_time)
    for cls, name, source, kw in traces:
        g.add_trace((swap or {}).get(name, cls)(name=name, source=source, **kw))
    g.setup_traces()
    g.open(x, RATE)
    for t in g.traces:
        t.plot_items = [Item() for _ in range(t.channels)]
    g.set_need_update()
    return g


def below_of(t):
    out = []
    for d in t.dests:
        out.append(d)
        out.extend(below_of(d))
    return out


def assert_on_grid(t):
    """rate, offset and len(buffer) of `t` against its source's, by align_buffer's rule."""
    src = t.source
    step = Ledger._step_of(t)
    assert t.rate == src.rate/step, (t.name, t.rate, src.rate, step)
    first, count = src.offset, t._source_len()
    reaches_end = first + count >= src.frames
    if first > 0:
        margin = floor(t.source_tbefore*src.rate)
        first, count = first + margin, count - margin
    if not reaches_end:
        count -= floor(t.source_tafter*src.rate)
    offset = max(0, -(-first//step))
    n = max(0, min((first + count)//step - offset, t.frames - offset))
    assert (t.offset, len(t._hostbuf)) == (offset, n), \
        '%s sits at %d + %d, its source\'s grid puts it at %d + %d' % (t.name, t.offset, len(t._hostbuf), offset, n)


def new_reached():
    return {'fused': 0, 'carry': 0, 'refitted': 0, 'features step': 0, 'power-envelope step': 0, 'own': {}, 'source': {},
            'partial': {}, 'launches': {}, 'near': [0, 0], 'walks': 0}


class Walk(object):
    """One walk: the graph, its ledger and the actions.  Every action ends with ledger.check()."""

    def __init__(self, classes, oracle, seed, poison, reached=None, db=None, launches=None, swap=None):
        self.rng = rng = np.random.default_rng(31000 + seed)
        self.seconds = float(rng.uniform(28.5, 30.0))
        self.x = recording(self.seconds, seed, int(rng.integers(1, 4)) if poison else 0)
        self.buffer_time = float(rng.uniform(2.0, 3.0))
        step = int(rng.choice([1, 3, 8]))
        self.g = build_graph(classes, self.x, self.buffer_time, float(rng.uniform(0.3, 1.0)), 256, step,
                             'kernel' if seed % 2 == 0 else 'lowpass', swap)
        self.ledger = Ledger(self.g, oracle, db)
        self.reached = reached if reached is not None else new_reached()
        self.launches = launches if launches is not None else (lambda: {})
        self.t0 = 0.0
        self.log = []
        self.end_zone = 2*self.g.tbefore + self.g.back_time + 0.1      # (see prologue)

    # -- helpers
    def done(self, what, changed=None):
        """After an action: the traces below the changed one sit on its grid, and every buffer agrees with the ledger."""
        self.log.append(what)
        if changed is not None:
            for d in below_of(changed):
                assert_on_grid(d)
        try:
            self.ledger.check()
        except AssertionError as e:
            raise AssertionError('%s\n  after: %s' % (e, ' | '.join(self.log[-6:])))

    def counted(self, trace, fn):
        """Run a parameter change of `trace`: whole recomputes of it and of everything below are counted."""
        stats = self.ledger.stats
        before = {n: s['whole'] for n, s in stats.items()}
        carried = self.ledger.carries
        launched = dict(self.launches())
        fn()
        after = self.launches()
        new = {k for k, v in after.items() if v != launched.get(k, 0)}
        r = self.reached
        if new & {'chain_forward', 'sosfilt_envelope:0', 'sosfilt_envelope:2'} and trace.name in ('filtered', 'rereferenced'):
            r['fused'] += 1
        if stats[trace.name]['whole'] > before[trace.name]:
            r['own'][trace.name] = r['own'].get(trace.name, 0) + 1
        for d in below_of(trace):
            if stats[d.name]['whole'] > before[d.name]:
                r['source'][d.name] = r['source'].get(d.name, 0) + 1
        r['carry'] += self.ledger.carries - carried

    def move(self, t0, width=None):
        width = float(self.rng.uniform(0.3, 0.6*self.buffer_time)) if width is None else width
        self.t0 = float(np.clip(t0, 0.0, self.seconds - 0.5))
        carried = self.ledger.carries
        self.g.update_times(self.t0, min(self.t0 + width, self.seconds))
        self.reached['carry'] += self.ledger.carries - carried
        for t in self.ledger.traces:
            assert_on_grid(t)
        self.done('window %.2f + %.2f' % (self.t0, width))

    def set_filter(self, hp, lp):
        f = self.g['filtered']
        f.highpass_cutoff, f.lowpass_cutoff = hp, lp
        self.counted(f, f.update)
        self.done('filter %.0f-%.0f' % (hp, lp), f)

    def cut_template(self):
        """A template around the chirp nearest to the window, at most 32 frames by 64 bins of the current spectrogram."""
        g, s = self.g, self.g['spectrogram']
        frames = int(np.clip(CHIRP_LEN*s.rate, 3, 30))
        fmin = 1500.0
        fmax = min(3000.0, fmin + 60*s.fresolution)
        # a chirp the spectrogram holds and whose window does not send the loader back; else whichever can be cut
        lo = max(s.offset/s.rate, g.tbefore + g.data.offset/RATE if g.data.offset > 0 else 0.0)
        hi = (s.offset + len(s._hostbuf))/s.rate
        inside = [k for k in range(1, int(self.seconds) - 1) if lo + 0.05 < k + CHIRP_AT and k + CHIRP_AT + 2*CHIRP_LEN < hi]
        for second in inside + [k for k in range(1, int(self.seconds) - 1) if k not in inside]:
            t0 = second + CHIRP_AT
            carried = self.ledger.carries
            try:
                tm = g.cut_template(t0, t0 + (frames - 1)/s.rate, fmin, fmax, 0, floor_db=-100.0)
            except (ValueError, IndexError):  # a non-finite sample under the patch, or the buffers do not reach it
                tm = None
            self.reached['carry'] += self.ledger.carries - carried
            for t in self.ledger.traces:
                assert_on_grid(t)
            self.t0 = t0
            self.done('cut_template at %.2f' % t0)
            if tm is not None and np.ptp(tm.values) > 0:           # (a constant patch -- silence at the floor -- is none)
                assert tm.values.shape[0] <= 32 and tm.values.shape[1] <= 64
                return tm
        return None

    def set_template(self, tm):
        m = self.g['match']
        self.counted(m, lambda: m.set_template(tm))
        assert m.stale is (tm is None and m.stale)
        self.done('set_template %s' % (None if tm is None else tm.values.shape,), m)

    def set_events(self):
        """Regions near the buffer's borders: one just inside each end, one across each border, one in the middle."""
        from audian_amd.events import Events
        e = self.g['eventfiltered']
        lo, hi = e.offset, e.offset + len(e._hostbuf)
        width = int(round(2.0*0.02*e.rate))
        L = int(self.rng.integers(1200, 2400))
        spots = [lo + width + 1, lo - L//2, (lo + hi)//2, hi - L - width - 1, hi - L//2]
        pairs = []
        for c in range(e.channels):
            # another choice of the five per channel; events ascending, apart, longer than any pad length after widening
            rows = sorted({(max(a, 0), min(a + L, e.frames)) for a in spots[c::2] + spots[:1 + c]})
            keep = []
            for a, b in rows:
                if b - a > 600 and (not keep or a > keep[-1][1] + 3*width):
                    keep.append((a, b))
            pairs.append(keep)
        freqs = [np.array([float(self.rng.uniform(5.0, 60.0)) for _ in p]) for p in pairs]
        self.counted(e, lambda: e.set_events(Events(pairs, e.rate, 'envelope'), freqs, 0.02, clamp=bool(self.rng.integers(0, 2))))
        self.done('set_events %r' % (pairs,), e)

    def features_step(self, step):
        f = self.g['features']
        if step == 1 and len(f.kernel) > 65:
            self.set_kernel(33)
        old = f.step
        self.counted(f, lambda: f.update(step=step))
        if f.step != old and f.dests:
            self.reached['features step'] += 1
        assert_on_grid(f)
        self.done('features step %d' % step, f)

    def set_kernel(self, L):
        f = self.g['features']
        taps = np.hanning(L + 2)[1:-1]*np.cos(np.arange(L)*0.3)
        self.counted(f, lambda: f.set_kernel(taps/np.sum(np.abs(taps))))
        self.done('set_kernel %d' % L, f)

    def power_step(self, cutoff, step):
        p = self.g['power-envelope']
        old = p.step
        self.counted(p, lambda: p.update(envelope_cutoff=cutoff, step=step))
        if p.step != old and p.dests:
            self.reached['power-envelope step'] += 1
        assert_on_grid(p)
        self.done('power-envelope %.0f Hz step %r' % (cutoff, step), p)

    def spectrogram_update(self, nfft, overlap):
        s, m = self.g['spectrogram'], self.g['match']
        had = m.template is not None
        self.counted(s, lambda: s.update(nfft=nfft, overlap_frac=overlap))
        self.done('spectrogram %d / %.2f' % (nfft, overlap), s)
        if m.stale:
            assert had and np.all(np.isnan(np.asarray(m.buffer)))
            tm = self.cut_template()
            self.set_template(tm)
            self.reached['refitted'] += tm is not None

    # -- the walk
    def prologue(self):
        """The loader keeps tbefore + back_time seconds behind a window and tafter ahead of it, so its buffer sits at the
        start of the recording until a window comes within tafter of the end, follows it from there, and goes back when a
        window starts before what it holds: the walk scrolls forward near the end and jumps back."""
        g = self.g
        self.move(0.0, 1.5)
        self.set_filter(300.0, 3000.0)                  # one plan: the fused launch, the whole graph below it
        self.set_template(self.cut_template())
        self.set_events()
        self.move(self.end_zone, 1.5)
        self.move(self.t0 + 0.7, 1.5)                   # (nothing flushed in between on every other check)
        self.features_step(8 if g['features'].step != 8 else 3)
        self.move(self.t0 + 0.9, 1.5)
        self.power_step(60.0, None)
        self.move(self.seconds - 1.0)
        self.spectrogram_update(512, 0.5)
        self.move(8.0)                                  # back: strips at the front of every buffer

    def action(self):
        rng, g = self.rng, self.g
        kind = int(rng.integers(0, 20))
        if kind <= 4:                                   # scroll on towards the end (from the start: up to the end zone)
            self.move(max(self.t0, self.end_zone - 0.2) + float(rng.uniform(0.05, 1.2)), 1.5)
        elif kind == 5:                                 # jump: the start, the end, back to before what the buffers hold
            self.move(float(rng.choice([0.0, self.seconds - 1.0, rng.uniform(0.0, 12.0)])))
        elif kind == 6:
            hp = float(rng.choice([0.0, rng.uniform(20.0, 0.2*RATE)]))
            lp = float(rng.choice([RATE/2, rng.uniform(max(2*hp, 200.0), 0.45*RATE)]))
            self.set_filter(hp, lp)
        elif kind == 7:
            e = g['envelope']
            cut = float(rng.uniform(5.0, 0.1*RATE))
            e.envelope_cutoff, e.highpass_cutoff = cut, float(rng.choice([0.0, 0.0, rng.uniform(0.5, cut/3)]))
            e.filter_order = int(rng.integers(1, 5))
            self.counted(e, e.update)
            self.done('envelope %.0f Hz' % cut, e)
        elif kind == 8:
            nfft = int(rng.choice([64, 256, 512, 1024]))
            self.spectrogram_update(nfft, float(rng.choice([0.0, 0.5] if nfft == 64 else [0.0, 0.5, 0.75])))
        elif kind == 9:
            b = g['bandpower']
            fmin = float(rng.choice([0.0, rng.uniform(100.0, 2000.0)]))
            fmax = rng.choice([None, fmin + float(rng.uniform(10.0, 1500.0))])
            self.counted(b, lambda: b.set_band(fmin, fmax))
            if rng.integers(0, 3) == 0:
                self.counted(b, lambda: b.update(log=not b.log))
            self.done('set_band %r %r log %r' % (fmin, fmax, b.log), b)
        elif kind == 10:
            p = g['peakfreq']
            feature = str(rng.choice(sd.NAMES))
            self.counted(p, lambda: p.update(feature=feature))
            self.done('peakfreq %s' % feature, p)
        elif kind == 11:
            self.set_kernel(int(rng.choice([1, 5, 33, 65] if g['features'].step == 1 else [9, 65, 257])))
        elif kind == 12:
            f = g['features']
            thr = rng.choice([None, float(rng.uniform(0.0, 0.2))])
            self.counted(f, lambda: f.update(threshold=thr))
            self.done('features threshold %r' % (thr,), f)
        elif kind == 13:
            self.features_step(int(rng.choice([1, 3, 8])))
        elif kind == 14:
            self.power_step(float(rng.uniform(20.0, 400.0)), rng.choice([None, 1, 3, 8]))
        elif kind == 15:
            for name in ('slow-envelope', 'below'):
                t = g[name]
                if hasattr(t, 'cutoff'):
                    cutoff = float(rng.uniform(1.0, 40.0))
                    self.counted(t, lambda: t.update(cutoff=cutoff))
                    self.done('%s %.1f Hz' % (name, cutoff), t)
                else:                                   # (the kernel filter below the kernel filter)
                    thr = rng.choice([None, float(rng.uniform(0.0, 0.05))])
                    self.counted(t, lambda: t.update(threshold=thr))
                    self.done('%s threshold %r' % (name, thr), t)
        elif kind == 16:
            r = g['rereferenced']
            method = str(rng.choice(['mean', 'median']))
            groups = [None, [[0, 1, 2]], [[0, 2]], [[1], [2, 0]]][int(rng.integers(0, 4))]
            exclude = [(), (CHANNELS - 1,), (0,)][int(rng.integers(0, 3))]
            groups = [list(range(CHANNELS))] if groups is None else groups
            if any(all(c in exclude for c in grp) for grp in groups):
                exclude = ()
            self.counted(r, lambda: r.update(method=method, groups=groups, exclude=exclude))
            self.done('rereferenced %s %r %r' % (method, groups, exclude), r)
        elif kind == 17:
            m = g['match']
            if m.template is not None and rng.integers(0, 2) == 0:
                self.set_template(None)
                assert np.all(np.isnan(np.asarray(m.buffer)))
            else:
                self.set_template(self.cut_template())
        elif kind == 18:
            self.set_events()
        else:
            # partial reads: the host copy current there, stale elsewhere
            for name in ('filtered', 'features', 'bandpower', 'slow-envelope', 'spectrogram'):
                t = g[name]
                n = len(t._hostbuf)
                if n > 12:
                    a = int(rng.integers(0, n - 10))
                    ch = int(rng.integers(0, t.channels))
                    want = peek(t, a, 7)[:, ch]
                    assert np.array_equal(np.asarray(t.buffer[a:a + 7, ch]), want, equal_nan=True), name
                    i0 = t.offset + int(rng.integers(0, n - 5))
                    want = peek(t, i0 - t.offset, 4)[:, ch]
                    assert np.array_equal(np.asarray(t[i0:i0 + 4, ch]), want, equal_nan=True), name
            self.done('partial reads')

    def run(self, actions=14):
        self.prologue()
        for _ in range(actions):
            self.action()
        self.ledger.check(flush=True)
        r = self.reached
        r['walks'] += 1
        for name, s in self.ledger.stats.items():
            r['partial'][name] = r['partial'].get(name, 0) + s['partial']
        r['near'][0] += self.ledger.near[0]
        r['near'][1] += self.ledger.near[1]
        return self


def walk(classes, oracle, seed, poison, reached=None, db=None, launches=None, actions=14):
    return Walk(classes, oracle, seed, poison, reached, db, launches).run(actions)
