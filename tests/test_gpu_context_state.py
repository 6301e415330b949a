"""What a context carries from one call to the next must not reach a result: the contents of the scratch block and of
the segment flags (hipdsp_scratch() and hd_seg_flags() hand both out uncleared), the order of the calls, and a call that
returned an error.

Every entry point that works in the scratch is a case below: hipdsp_pcm_minmax, hipdsp_envelope, hipdsp_envelope_multi,
hipdsp_sosfilt (segmented: the flags), hipdsp_sosfilt_envelope (phase 0, phases 1 + 2), hipdsp_chain_forward (+ phase 2,
+ hipdsp_chain_backward, and without an envelope plan), hipdsp_spectrogram on the four-step path through the scratch,
hipdsp_unwrap, hipdsp_mean_spectrum_db, hipdsp_histogram, hipdsp_masked_stats, hipdsp_region_stats, hipdsp_detect_events,
hipdsp_find_peaks, hipdsp_region_spectra, hipdsp_region_filtfilt and hipdsp_region_crossings.

(a) The context option "scratch_fill" (include/hip_dsp.h) fills the scratch and the flags with one byte value right
    before a call is handed them.  Every case runs with 0x00 (zeros), 0x01 (small counts, tiny floats, "not finite" in
    every flag), 0x7f (huge finite floats and doubles) and 0xff (NaN and -1) into outputs prefilled with 0x5a: the bytes
    of the four runs and of a run with the option off on a fresh context are equal, and the 0xff run is judged by the
    unit's own comparator under the unit's own bound (events_definition, peaks_definition, threshold_definition / numpy,
    spectra_definition, refine_definition, iir_bound, spectral_bound, decibel_bound, the oracle) -- never against the
    code under test.
(b) The cases run on ONE context in three seeded orders, plans and FFT tables staying: every output equals the bytes
    of its run alone on a fresh context.
(c) A call that returned an error changes nothing: the next valid call gives the bytes it gave before, and a forward
    sweep that was refused after it had taken the scratch leaves no tile states a backward sweep would accept.

Shapes: three channels; per unit one length of three whole chunks (or tiles, or groups of frames) of the launcher plus
a few samples -- a ragged last chunk, more than one block -- and one shorter than a chunk; one channel, range or region
that yields nothing (a flat channel, start == stop, an empty region table, a short region next to a long one).  The
chunk each length comes from stands next to the case.  The sweeps run iir_bound.T_LONG = 16 tiles + 5 samples under
the "three segments" and "one-tile segments" settings of test_gpu_iir_accuracy.py, which put the flags in play."""

import functools

import numpy as np
import pytest

import decibel_bound as dbb
import events_definition as ed
import iir_bound as ib
import peaks_definition as pd
import refine_definition as rd
import spectral_bound as sb
import threshold_definition as td
from test_gpu_decibel_accuracy import mean_case
from test_gpu_histogram import check_hist, check_masked
from test_gpu_iir_accuracy import SEGMENTATIONS, options
from test_gpu_overview import pcm_bytes, ref_minmax, wrapped_ints
from test_gpu_regioncrossings import Slab as CrossSlab, expect as expect_crossings, same as same_crossings
from test_gpu_regionfilter import SENTINEL as RF_SENTINEL, Slab as FilterSlab
from test_gpu_regionspectra import Slab as SpectraSlab, bound_and_reference, length_for
from test_gpu_regionstats import Slab as StatsSlab, check_contract, numpy_slots

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0x01, 0x7f, 0xff)
PREFILL = 0x5a                                   # every byte of every output buffer before a call
SEGS = {'three segments': SEGMENTATIONS[1][1], 'one-tile segments': SEGMENTATIONS[3][1]}
assert SEGMENTATIONS[1][0] == 'three segments' and SEGMENTATIONS[3][0] == 'one-tile segments'
INF = float('inf')


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == PREFILL))


def orc():
    from oracle import oracle
    oracle.build()
    return oracle


class Run(object):
    """What a case works with: the context, the plans that stay with it, and device arrays that go when the call is over."""

    def __init__(self, c, plans):
        self.c, self.plans, self.keep = c, plans, []

    def upload(self, host, dtype=None):
        from audian_amd import hipdsp
        d = hipdsp.DeviceArray.from_host(self.c, host, dtype)
        self.keep.append(d)
        return d

    def fresh(self, shape, dtype=np.float32):
        """An output: every byte PREFILL."""
        from audian_amd import hipdsp
        d = hipdsp.DeviceArray(self.c, shape, dtype)
        hipdsp.lib.hipdsp_memset(self.c.handle, hipdsp._p(d), PREFILL, d.nbytes)
        self.keep.append(d)
        return d

    def slab(self, cls, x):
        s = cls(x, ctx=self.c)
        self.keep.append(s.dev)
        return s

    def plan(self, key, sos):
        from audian_amd import hipdsp
        if key not in self.plans:
            self.plans[key] = hipdsp.SosPlan(self.c, sos)
        return self.plans[key]

    def free(self):
        for d in self.keep:
            d.free()


class Case(object):
    """body(run) -> [numpy arrays], every output of the call(s); judge(outputs) holds them to the unit's comparator;
    bad(run) is one call the unit's own error test lists: it must raise."""

    def __init__(self, name, body, judge, bad=None):
        self.name, self.body, self.judge, self.bad = name, body, judge, bad

    def run(self, c, plans):
        r = Run(c, plans)
        try:
            return self.body(r)
        finally:
            r.free()

    def run_bad(self, c, plans):
        r = Run(c, plans)
        try:
            with pytest.raises((ValueError, NotImplementedError)):
                self.bad(r)
        finally:
            r.free()


CASES = {}


def case(name, bad=None):
    def add(pair):
        body, judge = pair()
        CASES[name] = Case(name, body, judge, bad)
        return pair
    return add


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            a, b = np.ascontiguousarray(g).view(np.uint8).ravel(), np.ascontiguousarray(w).view(np.uint8).ravel()
            at = int(np.flatnonzero(a != b)[0])//g.dtype.itemsize
            raise AssertionError('%s: output %d differs in %d bytes, first at element %d: %r, %r' % (
                what, i, int(np.count_nonzero(a != b)), at, g.ravel()[at], w.ravel()[at]))


# ---- the sweeps: sos.hip and chain.hip, tiles of 2048 samples ------------------------------------------------------------

BP, ENV = 'bp2 300-3000 Hz @ 96 kHz', 'lp2 20 Hz @ 96 kHz'
LANES = ib.FAMILIES[:3]                         # stepdown, stepup, offset: both case lists carry them
T = ib.T_LONG
MULTI, MULTI_SPLIT = 'lp4 300 Hz @ 48 kHz', (1, 1)       # two plans of one section: the cheapest reference of a hand-over


@functools.lru_cache(maxsize=None)
def sweep_input():
    sos, rate, fams = ib.design(BP)
    esos, erate, efams = ib.design(ENV, ib.ENVELOPES)
    assert rate == erate and all(f in fams and f in efams for f in LANES)
    return sos, esos, rate, ib.families(LANES, T, rate)


def judge_bandpass(yf, what):
    sos, esos, rate, x = sweep_input()
    ref, q = ib.sosfilt_case(sos, x)
    assert np.all(q <= ib.Q_CAP), (what, q)
    ib.assert_within(yf.T, ref, q, what + ', band-pass')


def judge_envelope_of(yf, env, what, between=False):
    """The contract of the fused launches: the envelope of the float32 band-pass output the same launch wrote."""
    sos, esos, rate, x = sweep_input()
    own = np.ascontiguousarray(yf.T)
    ref, q = ib.envelope_case(esos, own)
    assert np.all(q <= ib.Q_CAP), (what, q)
    ib.assert_within(env.T, ref, q, what + ', envelope', term=ib.between_term(esos, own) if between else None)


def judge_psd(yf, psd, rate, nfft, hop, what):
    want = np.zeros((psd.shape[1], psd.shape[0], nfft//2 + 1))
    orc().spectrogram_process(yf.T.astype(np.float64), want, rate, nfft, hop)
    rho, beta = sb.assert_within(psd, want.transpose(1, 0, 2), nfft, what + ', spectrogram')
    print('%s: rho %.3f beta %.2f' % (what, rho, beta))


def refuse_sosfilt(r):
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    dx, dy = r.upload(np.zeros((2, 5000), np.float32)), r.fresh((2, 5000))
    hipdsp.sosfilt(r.c, r.plan('bp', sos), dx, 5000, dy, 5000, 2, 5000, 5001)          # skip > frames


def refuse_envelope(r):
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    dx, dy = r.upload(np.zeros((2, 5000), np.float32)), r.fresh((2, 5000))
    hipdsp.envelope(r.c, r.plan('env', esos), dx, 5000, dy, 5000, 2, 9, 0)              # not longer than padlen


def refuse_sosfilt_envelope(r):
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    dx, dy = r.upload(np.zeros((2, 5000), np.float32)), r.fresh((2, 5000))
    hipdsp.sosfilt_envelope(r.c, r.plan('bp', sos), r.plan('env', esos), dx, 5000, dx, 5000, dy, 5000, 2, 5000)     # yf over x


def refuse_chain(r):
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    dx, dy, ps = r.upload(np.zeros((2, 9000), np.float32)), r.fresh((2, 9000)), r.fresh((2, 3, 2049))
    hipdsp.chain_forward(r.c, r.plan('bp', sos), r.plan('env', esos), dx, 9000, dy, 9000, 2, 9000, 4096, 2048, rate, ps, 3)


def refuse_multi(r):
    from audian_amd import hipdsp
    sos = ib.design(MULTI, ib.ENVELOPES)[0]
    plans = [r.plan(('multi', i), sos[part]) for i, part in enumerate(ib.plan_slices(sos, MULTI_SPLIT))]
    dx, dy = r.upload(np.zeros((2, 5000), np.float32)), r.fresh((2, 5000))
    hipdsp.envelope_multi(r.c, plans*8 + plans[:1], dx, 5000, dy, 5000, 2, 5000, 0)      # 17 plans: 'n_plans'


def add_sweeps(seg):
    opts = SEGS[seg]

    @case('hipdsp_sosfilt, %s' % seg, bad=refuse_sosfilt)
    def _():
        def body(r):
            from audian_amd import hipdsp
            sos, esos, rate, x = sweep_input()
            dx, dy = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T))
            with options(r.c, opts):
                hipdsp.sosfilt(r.c, r.plan('bp', sos), dx, T, dy, T, 3, T, 0)
            return [dy.to_host()]
        return body, lambda o: judge_bandpass(o[0], 'hipdsp_sosfilt, %s' % seg)

    @case('hipdsp_envelope, %s' % seg, bad=refuse_envelope)
    def _():
        def body(r):
            from audian_amd import hipdsp
            sos, esos, rate, x = sweep_input()
            dx, dy = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T))
            with options(r.c, opts):
                hipdsp.envelope(r.c, r.plan('env', esos), dx, T, dy, T, 3, T, 0, clamp=False)
            return [dy.to_host()]

        def judge(o):
            sos, esos, rate, x = sweep_input()
            ref, q = ib.envelope_case(esos, x)
            assert np.all(q <= ib.Q_CAP), q
            ib.assert_within(o[0].T, ref, q, 'hipdsp_envelope, %s' % seg)
        return body, judge

    @case('hipdsp_envelope_multi, %s' % seg, bad=refuse_multi)
    def _():
        @functools.lru_cache(maxsize=None)
        def setup():
            sos, rate, fams = ib.design(MULTI, ib.ENVELOPES)
            assert sum(MULTI_SPLIT) == len(sos) and all(f in fams for f in LANES)
            return sos, ib.families(LANES, T, rate)

        def body(r):
            from audian_amd import hipdsp
            sos, x = setup()
            plans = [r.plan(('multi', i), sos[part]) for i, part in enumerate(ib.plan_slices(sos, MULTI_SPLIT))]
            dx, dy = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T))
            with options(r.c, opts):
                hipdsp.envelope_multi(r.c, plans, dx, T, dy, T, 3, T, 0, clamp=False)
            return [dy.to_host()]

        def judge(o):
            sos, x = setup()
            ref, q = ib.envelope_case(sos, x)
            assert np.all(q <= ib.Q_CAP), q
            ib.assert_within(o[0].T, ref, q, 'hipdsp_envelope_multi, %s' % seg, term=ib.multi_term(sos, MULTI_SPLIT, x))
        return body, judge

    for phases in ((0,), (1, 2)):
        label = 'hipdsp_sosfilt_envelope, phase %s, %s' % (' + '.join(str(p) for p in phases), seg)

        @case(label, bad=refuse_sosfilt_envelope)
        def _(phases=phases, label=label):
            def body(r):
                from audian_amd import hipdsp
                sos, esos, rate, x = sweep_input()
                dx, yf, ye = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T)), r.fresh((3, T))
                with options(r.c, opts):
                    for phase in phases:
                        hipdsp.sosfilt_envelope(r.c, r.plan('bp', sos), r.plan('env', esos), dx, T, yf, T, ye, T, 3, T,
                                                clamp=False, phase=phase)
                return [yf.to_host(), ye.to_host()]

            def judge(o):
                judge_bandpass(o[0], label)
                judge_envelope_of(o[0], o[1], label)
            return body, judge

    # the fused sweep: both ends of its window list, with and without the envelope plan, and the frame-split pair
    for nfft, hop, how in ((2048, 1024, 'phase 2'), (2048, 1024, 'no envelope'), (256, 128, 'phase 2'), (256, 128, 'no envelope'),
                           (2048, 1024, 'hipdsp_chain_backward')):
        label = 'hipdsp_chain_forward %d/%d, %s, %s' % (nfft, hop, how, seg)

        @case(label, bad=refuse_chain)
        def _(nfft=nfft, hop=hop, how=how, label=label):
            nd = (T + hop - 1)//hop
            split = how == 'hipdsp_chain_backward'

            def body(r):
                from audian_amd import hipdsp
                sos, esos, rate, x = sweep_input()
                fplan, eplan = r.plan('bp', sos), (r.plan('env', esos) if how != 'no envelope' else None)
                dx, yf, ps = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T)), r.fresh((3, nd, nfft//2 + 1))
                with options(r.c, opts + ((('chain_split_frames', 1),) if split else ())):
                    hipdsp.chain_forward(r.c, fplan, eplan, dx, T, yf, T, 3, T, nfft, hop, rate, ps, nd)
                    if eplan is None:
                        return [yf.to_host(), ps.to_host()]
                    ye = r.fresh((3, T))
                    if split:
                        hipdsp.chain_backward(r.c, eplan, yf, T, ye, T, 3, T, nfft, hop, rate, ps, nd, clamp=False)
                    else:
                        hipdsp.sosfilt_envelope(r.c, fplan, eplan, dx, T, yf, T, ye, T, 3, T, clamp=False, phase=2)
                return [yf.to_host(), ps.to_host(), ye.to_host()]

            def judge(o):
                rate = sweep_input()[2]
                judge_bandpass(o[0], label)
                judge_psd(o[0], o[1], rate, nfft, hop, label)
                if len(o) > 2:
                    judge_envelope_of(o[0], o[2], label, between=split)
            return body, judge


for _seg in SEGS:
    add_sweeps(_seg)


# ---- hipdsp_spectrogram through the scratch: run_big of spectrogram.hip, the four-step path ------------------------------
# The dispatch sends 65536 ... 524288 there under "spec_kernel" 2 only (by default 65536 takes the frame on chip,
# spec_chip.h, and no scratch: it runs here as the default it is).  Two frames and one past the input; 131072 at hop
# nfft/2 is the largest that stays within 2^18 samples per channel.

RATE = 48000.0
LEVELS3 = sb.LEVELS + (1.0,)


def refuse_spectrogram(r):
    from audian_amd import hipdsp
    dx, out = r.upload(np.zeros((2, 5000), np.float32)), r.fresh((2, 1, 129))
    hipdsp.spectrogram(r.c, dx, 5000, 2, 5000, 1 << 20, 1 << 19, RATE, out, 1)


for _nfft, _kernel in ((65536, 0), (65536, 2), (131072, 2)):
    @case('hipdsp_spectrogram %d, spec_kernel %d' % (_nfft, _kernel), bad=refuse_spectrogram)
    def _(nfft=_nfft, kernel=_kernel):
        hop, frames = nfft//2, 2
        n = (frames - 1)*hop + nfft
        what = 'hipdsp_spectrogram %d, spec_kernel %d' % (nfft, kernel)

        @functools.lru_cache(maxsize=None)
        def signal():
            return sb.family('tones', n, nfft, RATE, seed=nfft + kernel, levels=LEVELS3)

        def body(r):
            from audian_amd import hipdsp
            dx = r.upload(np.ascontiguousarray(signal().T, dtype=np.float32))
            out, db = r.fresh((3, frames + 1, nfft//2 + 1)), r.fresh((3, frames + 1, nfft//2 + 1))
            r.c.set_option('spec_kernel', kernel)
            try:
                hipdsp.spectrogram(r.c, dx, n, 3, n, nfft, hop, RATE, out, frames + 1, db_out=db)
            finally:
                r.c.set_option('spec_kernel', 0)
            return [out.to_host(), db.to_host()]

        def judge(o):
            want = np.zeros((frames + 1, 3, nfft//2 + 1))
            orc().spectrogram_process(signal().astype(np.float64), want, RATE, nfft, hop)
            assert np.all(o[0][:, frames] == 0) and np.all(o[1][:, frames] == -np.inf), what + ': zero tail'
            sb.assert_within(o[0], want.transpose(1, 0, 2), nfft, what, db=o[1])
        return body, judge


# ---- the analysis units ----------------------------------------------------------------------------------------------
# ranges per unit: three chunks + 5 samples, 100 samples, and nothing (start == stop)

def ranges(chunk, start=3):
    return [(start, start + 3*chunk + 5), (start, start + 100), (7, 7)]


def framed(rows, start, n, outside):
    """(C, start + n + 3) float32: `rows` (C, n) with `outside` before start and behind start + n (it must not be looked at)."""
    x = np.full((rows.shape[0], start + n + 3), outside, dtype=np.float32)
    x[:, start:start + n] = rows
    return x


EV_CHUNK, EV_CAP, EV_THR, EV_GAP, EV_LEN = 4096, 4096, [0.25, 0.0, 1.0], 1, 2


def refuse_events(r):
    from audian_amd import hipdsp
    dx, counts = r.upload(np.zeros((3, 200), np.float32)), r.fresh((3,), np.int64)
    hipdsp.detect_events_into(r.c, dx, 200, 3, 10, 9, 0.5, 0, 0, 0, None, counts)       # stop < start


@case('hipdsp_detect_events', bad=refuse_events)
def _():
    """events.hip: EV_CHUNK = 4096 samples per wave.  Channel 2 is flat under its threshold: no event."""
    @functools.lru_cache(maxsize=None)
    def signal():
        rng = np.random.default_rng(11)
        n = 3*EV_CHUNK + 5
        rows = np.stack([np.where(rng.random(n) < 0.04, 2.0, -1.0), rng.standard_normal(n), np.full(n, -1.0)])
        return framed(rows, 3, n, 50.0)

    def body(r):
        from audian_amd import hipdsp
        x = signal()
        dx, thr = r.upload(x), r.upload(np.asarray(EV_THR, dtype=np.float32))
        out = []
        for a, b in ranges(EV_CHUNK):
            ev, counts = r.fresh((3, EV_CAP, 2), np.int64), r.fresh((3,), np.int64)
            hipdsp.detect_events_into(r.c, dx, x.shape[1], 3, a, b, thr, EV_GAP, EV_LEN, EV_CAP, ev, counts)
            out += [ev.to_host(), counts.to_host()]
        return out

    def judge(o):
        x = signal()
        for i, (a, b) in enumerate(ranges(EV_CHUNK)):
            ev, counts = o[2*i], o[2*i + 1]
            for ch in range(3):
                want = ed.detect(x[ch], a, b, EV_THR[ch], EV_GAP, EV_LEN)
                assert counts[ch] == len(want) <= EV_CAP, (a, b, ch, counts[ch], len(want))
                assert ev[ch, :len(want)].tolist() == [list(p) for p in want], (a, b, ch)
                assert untouched(ev[ch, len(want):]), (a, b, ch)
            assert counts[2] == 0 and (counts[0] > 0 or b - a < 1000)
    return body, judge


PK_CHUNK, PK_CAP, OPEN6 = 4096, 6144, [-INF, INF]*3


def refuse_peaks(r):
    from audian_amd import hipdsp
    dx, counts = r.upload(np.zeros((3, 200), np.float32)), r.fresh((3,), np.int64)
    hipdsp.find_peaks_into(r.c, dx, 200, 3, 10, 9, OPEN6, 0, 0, None, None, counts)      # stop < start


@case('hipdsp_find_peaks', bad=refuse_peaks)
def _():
    """peaks.hip: PK_CHUNK = 4096 samples per wave.  Channel 2 is constant: no peak."""
    @functools.lru_cache(maxsize=None)
    def signal():
        from audian_amd import hipdsp
        assert hipdsp.PEAKS_CHUNK == PK_CHUNK
        rng = np.random.default_rng(12)
        n = 3*PK_CHUNK + 5
        rows = rng.integers(-2000, 0, size=(3, n)).astype(np.float64)            # (many levels: the definition's walks stay short)
        rows[1] = np.repeat(rows[1], rng.integers(1, 4, size=n))[:n]                     # runs of equal samples
        rows[2] = -5.0
        return framed(rows, 3, n, np.inf)

    def body(r):
        from audian_amd import hipdsp
        x = signal()
        dx = r.upload(x)
        out = []
        for a, b in ranges(PK_CHUNK):
            pk, pr, counts = r.fresh((3, PK_CAP), np.int64), r.fresh((3, PK_CAP, 4), np.float64), r.fresh((3,), np.int64)
            hipdsp.find_peaks_into(r.c, dx, x.shape[1], 3, a, b, OPEN6, 0, PK_CAP, pk, pr, counts)
            out += [pk.to_host(), pr.to_host(), counts.to_host()]
        return out

    def judge(o):
        x = signal()
        for i, (a, b) in enumerate(ranges(PK_CHUNK)):
            pk, pr, counts = o[3*i:3*i + 3]
            for ch in range(3):
                want = pd.find_peaks(x[ch, a:b], wlen=0, first=a)
                k = len(want[0])
                assert counts[ch] == k <= PK_CAP, (a, b, ch, counts[ch], k)
                assert pd.same(pk[ch, :k], pr[ch, :k], want), (a, b, ch)
                assert untouched(pk[ch, k:]) and untouched(pr[ch, k:]), (a, b, ch)
            assert counts[2] == 0 and (counts[0] > 100 or b - a < 1000)
    return body, judge


HG_CHUNK, HG_BINS = 16384, 49


def refuse_histogram(r):
    from audian_amd import hipdsp
    dx, out = r.upload(np.zeros((3, 100), np.float32)), r.fresh((3, 4), np.int64)
    hipdsp.histogram(r.c, dx, 100, 3, 0, 100, [1.0, 0.0], out=out)                      # edges that decrease


@case('hipdsp_histogram', bad=refuse_histogram)
def _():
    """histogram.hip: HgChunk::CHUNK = 16384 elements per workgroup, whose counts are added into the caller's row."""
    @functools.lru_cache(maxsize=None)
    def signal():
        rng = np.random.default_rng(13)
        n = 3*HG_CHUNK + 5
        return framed(rng.uniform(-1.2, 3.2, size=(3, n)), 3, n, 0.5), np.linspace(-1.0, 3.0, HG_BINS + 1)

    def body(r):
        from audian_amd import hipdsp
        x, e = signal()
        dx = r.upload(x)
        out = []
        for a, b in ranges(HG_CHUNK):
            rows = r.fresh((3, HG_BINS + 3), np.int64)
            hipdsp.histogram(r.c, dx, x.shape[1], 3, a, b, e, out=rows)
            out.append(rows.to_host())
        return out

    def judge(o):
        x, e = signal()
        for (a, b), got in zip(ranges(HG_CHUNK), o):
            check_hist(got, x, a, b, e, 'hipdsp_histogram [%d, %d)' % (a, b))
            for ch in range(3):
                assert got[ch].tolist() == td.histogram_slots(x[ch, a:b], e).tolist()
    return body, judge


MASK_BOUNDS = [(-INF, 0.25, 0.25), (0.5, INF, 0.5), (5.0, 6.0, 5.0)]       # the third selects nothing


def refuse_masked(r):
    from audian_amd import hipdsp
    dx, out = r.upload(np.zeros((3, 100), np.float32)), r.fresh((3, 4), np.float64)
    hipdsp.masked_stats(r.c, dx, 100, 3, 10, 9, np.asarray(MASK_BOUNDS), out=out)        # stop < start


@case('hipdsp_masked_stats', bad=refuse_masked)
def _():
    """histogram.hip: one record per chunk of 16384 elements and channel in the scratch, merged by a second launch."""
    @functools.lru_cache(maxsize=None)
    def signal():
        rng = np.random.default_rng(14)
        n = 3*HG_CHUNK + 5
        return framed(rng.standard_normal((3, n)), 3, n, 0.1)

    def body(r):
        from audian_amd import hipdsp
        x = signal()
        dx, bounds = r.upload(x), r.upload(np.asarray(MASK_BOUNDS, dtype=np.float64))
        out = []
        for a, b in ranges(HG_CHUNK):
            slots = r.fresh((3, 4), np.float64)
            hipdsp.masked_stats(r.c, dx, x.shape[1], 3, a, b, bounds, out=slots)
            out.append(slots.to_host())
        return out

    def judge(o):
        x = signal()
        for (a, b), got in zip(ranges(HG_CHUNK), o):
            for ch, (lo, hi, K) in enumerate(MASK_BOUNDS):
                check_masked(got[ch], x[ch, a:b], lo, hi, K, 'hipdsp_masked_stats [%d, %d) channel %d' % (a, b, ch))
            assert got[2, 0] == 0 and np.isnan(got[2, 1])
    return body, judge


RS_CHUNK = 16384
RS_REGIONS = [(5, 5 + 3*RS_CHUNK + 5), (5, 105), (7, 7), (20000, 20100)]   # long, short inside it, empty, short


def refuse_region_stats(r):
    from audian_amd import hipdsp
    dx, out = r.upload(np.zeros((3, 100), np.float32)), r.fresh((2, 3, 8), np.float64)
    hipdsp.region_stats(r.c, dx, 100, 3, 100, [(0, 10), (10, 9)], out=out)


@case('hipdsp_region_stats', bad=refuse_region_stats)
def _():
    """regionstats.hip: RsChunk::CHUNK = 16384 elements per workgroup, a record per chunk, region and channel."""
    @functools.lru_cache(maxsize=None)
    def signal():
        rng = np.random.default_rng(15)
        return rng.standard_normal((3, 5 + 3*RS_CHUNK + 5 + 9)).astype(np.float32)

    def body(r):
        from audian_amd import hipdsp
        x = signal()
        slab = r.slab(StatsSlab, x)
        out = r.fresh((len(RS_REGIONS), 3, 8), np.float64)
        hipdsp.region_stats(r.c, slab.view, slab.pitch, 3, slab.frames, RS_REGIONS, out=out)
        return [out.to_host()]

    def judge(o):
        x = signal()
        for i, (a, b) in enumerate(RS_REGIONS):
            for ch in range(3):
                if b > a:
                    check_contract(o[0][i, ch], x[ch, a:b], 'hipdsp_region_stats region %d channel %d' % (i, ch))
                else:
                    assert np.array_equal(o[0][i, ch], numpy_slots(x[ch, a:b]), equal_nan=True), (i, ch)
    return body, judge


SP_GROUP, SP_NFFT, SP_HOP = 16, 64, 32


def refuse_spectra(r):
    from audian_amd import hipdsp
    dx, out, info = r.upload(np.zeros((3, 2000), np.float32)), r.fresh((1, 7)), r.fresh((1, 2), np.int64)
    hipdsp.region_spectra_into(r.c, dx, 2000, 3, 2000, [(0, 0, 1000)], 12, 6, 1, RATE, out, info)     # nfft 12


@case('hipdsp_region_spectra', bad=refuse_spectra)
def _():
    """regionspectra.hip: SP_GROUP = 16 frames per work item, a partial row per group in the scratch.  Regions of 3 groups
    + 2 frames, of 15 frames (no whole group), of no frame at all, and an empty one; then an empty table."""
    F = SP_NFFT//2 + 1

    @functools.lru_cache(maxsize=None)
    def setup():
        from audian_amd import hipdsp
        assert hipdsp.SPECTRA_GROUP == SP_GROUP
        x = sb.family('tones', 4000, SP_NFFT, rate=RATE, seed=11, levels=LEVELS3).T
        regions = [(0, 3, 3 + length_for(3*SP_GROUP + 2, SP_NFFT, SP_HOP, 1)), (1, 0, length_for(SP_GROUP - 1, SP_NFFT, SP_HOP, 1)),
                   (2, 5, 5 + SP_NFFT - 1), (1, 9, 9)]
        return np.ascontiguousarray(x, dtype=np.float32), regions

    def body(r):
        from audian_amd import hipdsp
        x, regions = setup()
        slab = r.slab(SpectraSlab, x)
        rows, info = r.fresh((len(regions), F)), r.fresh((len(regions), 2), np.int64)
        hipdsp.region_spectra_into(r.c, slab.view, slab.pitch, 3, slab.frames, regions, SP_NFFT, SP_HOP, 1, RATE, rows, info)
        none, ninfo = r.fresh((1, F)), r.fresh((1, 2), np.int64)
        hipdsp.region_spectra_into(r.c, slab.view, slab.pitch, 3, slab.frames, np.zeros((0, 3), dtype=np.int64), SP_NFFT, SP_HOP,
                                   1, RATE, none, ninfo)
        return [rows.to_host(), info.to_host(), none.to_host(), ninfo.to_host()]

    def judge(o):
        x, regions = setup()
        rows, info = o[0], o[1]
        assert untouched(o[2]) and untouched(o[3]), 'an empty region table wrote something'
        counts = []
        for i, region in enumerate(regions):
            B, ref, n, argmax = bound_and_reference(x[region[0]], region, SP_NFFT, SP_HOP, 1, RATE)
            counts.append(n)
            assert info[i, 0] == n, region
            if n == 0:
                assert np.isnan(rows[i]).all() and info[i, 1] == -1, region
                continue
            err = np.abs(rows[i].astype(np.float64) - ref)
            k = int(np.argmax(err - B))
            assert err[k] <= B[k], '%r: bin %d is %r, reference %r, allowed +-%.3g' % (region, k, rows[i, k], ref[k], B[k])
            assert info[i, 1] == np.argmax(rows[i]), region
        assert counts == [3*SP_GROUP + 2, SP_GROUP - 1, 0, 0]
    return body, judge


RF_TILE, RF_LABEL = 4096, 'lp1 400 Hz @ 5 kHz'


def refuse_filtfilt(r):
    from audian_amd import hipdsp
    sos = rd.case_design(RF_LABEL)[0]
    dx, dy = r.upload(np.zeros((3, 400), np.float32)), r.fresh((3, 400))
    hipdsp.region_filtfilt(r.c, dx, 400, dy, 400, 3, 400, [(0, 10, 200), (0, 199, 300)], np.array([sos, sos]))    # overlap


@case('hipdsp_region_filtfilt', bad=refuse_filtfilt)
def _():
    """regionfilter.hip: tiles of RF_CHUNK * 64 = 4096 samples of the extended sequence per wave, a state per chunk of 64
    and per tile in the scratch.  Extended lengths of 3 tiles + 5, of 1 tile + 1 right behind the shortest legal region,
    and of 65; then an empty table."""
    @functools.lru_cache(maxsize=None)
    def setup():
        from audian_amd import hipdsp
        assert hipdsp.FILTER_TILE == RF_TILE
        sos = rd.case_design(RF_LABEL)[0]
        pad = ib.padlen(sos)
        lengths = [3*RF_TILE + 5 - 2*pad, pad + 1, RF_TILE + 1 - 2*pad, 65 - 2*pad]
        lanes = [0, 1, 2, 3]
        regions = [(0, 3, 3 + lengths[0]), (1, 2, 2 + lengths[1]), (1, 2 + lengths[1], 2 + lengths[1] + lengths[2]),
                   (2, 5, 5 + lengths[3])]
        x = np.zeros((3, 3 + lengths[0] + 5), dtype=np.float32)
        for (ch, a, b), L, lane in zip(regions, lengths, lanes):
            x[ch, a:b] = rd.case_signal(RF_LABEL, L)[:, lane]
        return x, regions, list(zip(lengths, lanes)), np.array([sos]*len(regions))

    def body(r):
        x, regions, what, sos = setup()
        slab = r.slab(FilterSlab, x)
        return [slab.filtfilt(regions, sos), slab.filtfilt(np.zeros((0, 3), dtype=np.int64), np.zeros((0, 1, 6)))]

    def judge(o):
        x, regions, what, sos = setup()
        slab = FilterSlab.__new__(FilterSlab)
        slab.C, slab.frames = x.shape
        slab.pitch = slab.frames + 7
        assert np.all(slab.outside(o[0], regions) == RF_SENTINEL) and np.all(o[1] == RF_SENTINEL)
        got = slab.rows(o[0])
        for (ch, a, b), (L, lane) in zip(regions, what):
            ref, q = rd.filtfilt_case(sos[0], rd.case_signal(RF_LABEL, L))
            assert q[lane] <= ib.Q_CAP
            ib.assert_within(got[ch, a:b, None], ref[:, lane:lane + 1], q[lane],
                             'hipdsp_region_filtfilt, L %d at channel %d start %d' % (L, ch, a), first=0)
    return body, judge


RC_CHUNK = 4096
RC_REGIONS = [(0, 3, 3 + 3*RC_CHUNK + 5), (1, 5, 105), (2, 5, 5), (1, 200, 200 + RC_CHUNK + 1)]
RC_THRESHOLDS = [0.5, 10.0, 0.0, 1.0]          # the second: no sample above


def refuse_crossings(r):
    from audian_amd import hipdsp
    dx, out = r.upload(np.zeros((3, 100), np.float32)), r.fresh((2, 8), np.float64)
    hipdsp.region_crossings(r.c, dx, 100, 3, 100, [(0, 10, 9), (1, 5, 9)], 0.0, out=out)


@case('hipdsp_region_crossings', bad=refuse_crossings)
def _():
    """regionfilter.hip: RC_CHUNK = 4096 samples per workgroup, a record per chunk in the scratch, merged per region."""
    @functools.lru_cache(maxsize=None)
    def signal():
        from audian_amd import hipdsp
        assert hipdsp.CROSSINGS_CHUNK == RC_CHUNK
        return np.random.default_rng(17).standard_normal((3, 3 + 3*RC_CHUNK + 5 + 11)).astype(np.float32)

    def body(r):
        from audian_amd import hipdsp
        x = signal()
        slab = r.slab(CrossSlab, x)
        out, none = r.fresh((len(RC_REGIONS), 8), np.float64), r.fresh((1, 8), np.float64)
        hipdsp.region_crossings(r.c, slab.view, slab.pitch, 3, slab.frames, RC_REGIONS, RC_THRESHOLDS, out=out)
        hipdsp.region_crossings(r.c, slab.view, slab.pitch, 3, slab.frames, [], [], out=none)
        return [out.to_host(), none.to_host()]

    def judge(o):
        assert same_crossings(o[0], expect_crossings(signal(), RC_REGIONS, RC_THRESHOLDS))
        assert o[0][1, 1] == 0 and o[0][2, 0] == 0 and untouched(o[1])
    return body, judge


# ---- hipdsp_pcm_minmax, hipdsp_unwrap, hipdsp_mean_spectrum_db -----------------------------------------------------------

OV_BLOCK, OV_STEP, OV_SCALE = 4096, 7, 1.0/32768


def refuse_overview(r):
    from audian_amd import hipdsp
    raw, out = r.upload(np.zeros(64, np.uint8)), r.fresh((8, 4), np.float64)
    hipdsp.pcm_minmax(r.c, raw, 2, 16, 2, 0, 1.0, out, 4)                               # step 0


@case('hipdsp_pcm_minmax', bad=refuse_overview)
def _():
    """overview.hip: with three 16-bit channels a workgroup takes 64 parts of 64 frames = 4096 frames; the keys of the
    rows and (unwrapping) a count per part and channel live in the scratch -- the grid's last parts lie past the frames."""
    @functools.lru_cache(maxsize=None)
    def signals():
        return [wrapped_ints(n, 3, 2, 11 + n) for n in (3*OV_BLOCK + 5, 100)]

    def body(r):
        from audian_amd import hipdsp
        out = []
        for ints in signals():
            raw = pcm_bytes(ints, 2)
            src = r.upload(np.concatenate((raw, np.zeros(16, np.uint8)))).view(0, (len(raw),))      # (slack, as the unit's tests)
            rows = 2*((len(ints) + OV_STEP - 1)//OV_STEP)
            for thresh in (1.5, 0.0):
                got = r.fresh((rows, 4), np.float64)
                hipdsp.pcm_minmax(r.c, src, 2, len(ints), 3, OV_STEP, OV_SCALE, got, 4, unwrap_thresh=thresh, ampl_max=1.0)
                out.append(got.to_host())
        return out

    def judge(o):
        oracle = orc()
        for i, ints in enumerate(signals()):
            y = oracle.unwrap((ints*OV_SCALE).astype(np.float32), 1.5, 1.0, clips=False, down_scale=False)
            assert np.array_equal(o[2*i][:, :3], oracle.minmax_decimate(y.astype(np.float64), 0, len(y), OV_STEP)), len(ints)
            assert np.array_equal(o[2*i + 1][:, :3], ref_minmax(ints*OV_SCALE, OV_STEP)), len(ints)
            assert untouched(o[2*i][:, 3]) and untouched(o[2*i + 1][:, 3])
    return body, judge


UW_CHUNK = 16384


def refuse_unwrap(r):
    from audian_amd import hipdsp
    dx = r.upload(np.zeros((3, 100), np.float32))
    hipdsp.unwrap(r.c, dx, 100, 3, 100, 0.0, dx, 100)                                   # thresh 0


@case('hipdsp_unwrap', bad=refuse_unwrap)
def _():
    """elementwise.hip: UW_CHUNK = UW_ROW * UW_ROWS = 16384 samples per workgroup, a count per chunk and channel."""
    @functools.lru_cache(maxsize=None)
    def signals():
        out = []
        for n in (3*UW_CHUNK + 5, 100):
            rng = np.random.default_rng(n)
            t = np.arange(n)/48000.0
            true = np.stack([2.6*np.sin(2*np.pi*(400.0 + 130*ch)*t) + 0.05*rng.standard_normal(n) for ch in range(3)], axis=1)
            out.append(((true + 1.0) % 2.0 - 1.0).astype(np.float32))
        return out

    def body(r):
        from audian_amd import hipdsp
        out = []
        for w in signals():
            n = len(w)
            dx, dy = r.upload(np.ascontiguousarray(w.T)), r.fresh((3, n))
            hipdsp.unwrap(r.c, dx, n, 3, n, 1.5, dy, n, clips=False, down_scale=True)
            out.append(dy.to_host())
        return out

    def judge(o):
        for w, got in zip(signals(), o):
            assert np.array_equal(got.T, orc().unwrap(w, 1.5, clips=False, down_scale=True)), len(w)
    return body, judge


MS_SLICES = 64


def refuse_mean_spectrum(r):
    from audian_amd import hipdsp
    ds, out = r.upload(np.ones((40, 129), np.float32)), r.fresh((129,))
    hipdsp.mean_spectrum_db(r.c, ds, 129, 5, 5, out)                                    # empty frame range


@case('hipdsp_mean_spectrum_db', bad=refuse_mean_spectrum)
def _():
    """elementwise.hip: up to 64 slices of the frame range times blocks of 256 bins, a float64 partial sum each in the
    scratch.  3 * 64 + 5 frames of 257 bins, and 63 frames of 129."""
    shapes = [(3*MS_SLICES + 5, 257), (MS_SLICES - 1, 129)]
    ref_power, min_power = dbb.PAIRS[0]

    def body(r):
        from audian_amd import hipdsp
        out = []
        for frames, F in shapes:
            ds = r.upload(mean_case(frames, F))
            for i0 in (0, frames//3):
                got = r.fresh((F + 3,))
                hipdsp.mean_spectrum_db(r.c, ds, F, i0, frames, got, ref_power, min_power, -200.0)
                out.append(got.to_host())
        return out

    def judge(o):
        k = 0
        for frames, F in shapes:
            spec = mean_case(frames, F)
            for i0 in (0, frames//3):
                with np.errstate(all='ignore'):
                    mean = np.sum(spec[i0:frames].astype(np.longdouble), axis=0)/np.longdouble(frames - i0)
                    p32 = mean.astype(np.float32)
                dbb.assert_within(o[k][:F], p32, ref_power, min_power, 'hipdsp_mean_spectrum_db %d x %d from %d' % (frames, F, i0),
                                  extra=1, arg=mean, floor_db=-200.0)
                assert untouched(o[k][F:])
                k += 1
    return body, judge


NAMES = list(CASES)


# ---- the tests -------------------------------------------------------------------------------------------------------

def close(c, plans):
    for p in plans.values():
        p.close()
    c.close()


ALONE = {}


def alone(name):
    """The outputs of a case run once on a context of its own, "scratch_fill" off: computed once, never changed."""
    from audian_amd import hipdsp
    if name not in ALONE:
        c, plans = hipdsp.Context(0), {}
        try:
            ALONE[name] = CASES[name].run(c, plans)
        finally:
            close(c, plans)
    return ALONE[name]


@pytest.mark.parametrize('name', NAMES)
def test_results_do_not_depend_on_scratch_contents(name):
    """(a): four fill bytes and the option off, byte for byte; the 0xff run under the unit's own comparator."""
    from audian_amd import hipdsp
    want = alone(name)
    c, plans = hipdsp.Context(0), {}
    try:
        for fill in FILLS:
            c.set_option('scratch_fill', fill + 1)
            got = CASES[name].run(c, plans)
            same_bytes(got, want, '%s: scratch filled with 0x%02x against the option off' % (name, fill))
        c.synchronize()
    finally:
        close(c, plans)
    CASES[name].judge(got)


@pytest.fixture(scope='module')
def shared():
    """ONE context for all three orders of (b); its plans and FFT tables stay."""
    from audian_amd import hipdsp
    c, plans = hipdsp.Context(0), {}
    yield c, plans
    close(c, plans)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_results_do_not_depend_on_call_order(shared, seed):
    """(b): every case on one context in a seeded order; each output equals its run alone on a fresh context."""
    c, plans = shared
    order = [NAMES[i] for i in np.random.default_rng(seed).permutation(len(NAMES))]
    for k, name in enumerate(order):
        same_bytes(CASES[name].run(c, plans), alone(name),
                   '%s as call %d of order %d (behind %s)' % (name, k, seed, order[k - 1] if k else 'nothing'))
    c.synchronize()


def test_scratch_fill_option():
    """Off by default, 0 ... 256 accepted, anything else refused and the value kept."""
    from audian_amd import hipdsp
    c = hipdsp.Context(0)
    try:
        for bad in (-1, 257):
            with pytest.raises(ValueError, match='scratch_fill'):
                c.set_option('scratch_fill', bad)
        for good in (256, 1, 0):
            c.set_option('scratch_fill', good)
        c.reserve(1 << 16)                        # hipdsp_ctx_reserve with the option off and on
        c.set_option('scratch_fill', 0x100)
        c.reserve(1 << 17)
        c.synchronize()
    finally:
        c.close()


RETIRED_OPTIONS = ('sos_split', 'sos_single_wave_wg', 'sos_no_pin', 'sos_trace', 'sos_trace_rows', 'sos_fair', 'sos_debug',
                   'spec_debug')


def test_retired_options_are_refused_and_change_nothing():
    """The experiment switches of rounds 2-4 are unknown names now: each is refused, none is silently accepted, and the
    envelope behind the refusals has the bytes of the one in front of them."""
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    c, plans = hipdsp.Context(0), {}
    r = Run(c, plans)
    try:
        dx = r.upload(np.ascontiguousarray(x.T))

        def envelope():
            dy = r.fresh((3, T))
            hipdsp.envelope(c, r.plan('env', esos), dx, T, dy, T, 3, T, 0)
            return [dy.to_host()]

        want = envelope()
        for name in RETIRED_OPTIONS:
            with pytest.raises(ValueError, match='unknown option'):
                c.set_option(name, 1)
        same_bytes(envelope(), want, 'hipdsp_envelope behind the refused options')
        c.synchronize()
    finally:
        close(c, plans)


def test_no_fill_is_recorded_into_a_capture():
    """While the stream is capturing, a request for the scratch records no fill: a graph captured around
    hipdsp_ctx_reserve with the option on, replayed between a forward sweep and its backward sweep, leaves the parked
    tile states alone -- the envelope has the bytes of the plain pair."""
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    c, plans = hipdsp.Context(0), {}
    stream = c.create_stream()
    c.set_stream(stream)
    r = Run(c, plans)
    graph = None
    try:
        fplan, eplan = r.plan('bp', sos), r.plan('env', esos)
        dx, yf = r.upload(np.ascontiguousarray(x.T)), r.fresh((3, T))
        small, db = r.upload(np.linspace(0.1, 1.0, 500, dtype=np.float32)), r.fresh((500,))

        def sweep(phase):
            ye = r.fresh((3, T))
            hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T, 3, T, clamp=False, phase=phase)
            return ye

        sweep(1)
        want = sweep(2).to_host()
        c.set_option('scratch_fill', 0x100)
        c.synchronize()
        c.graph_begin()
        try:
            hipdsp.decibel(c, small, db, 500)                     # something to capture
            c.reserve(64)                                         # asks for the scratch: no growth, and no fill either
        finally:
            graph = c.graph_end()
        sweep(1)                                                  # (fills, then parks its states)
        c.graph_launch(graph)
        same_bytes([sweep(2).to_host()], [want], 'phase 2 behind a replayed graph that asked for the scratch')
        c.synchronize()
    finally:
        if graph is not None:
            c.graph_destroy(graph)
        r.free()
        c.set_stream(None)
        c.destroy_stream(stream)
        close(c, plans)


@pytest.mark.parametrize('trigger', ['envelope plan at 1024/512', 'three-section band-pass at 2048/1024'])
def test_a_refused_forward_sweep_leaves_no_tile_states(trigger):
    """(c): with "chain_debug" 4 (workgroup barriers) the launcher of hipdsp_chain_forward has no instantiation for nfft
    1024 nor for a band-pass of three sections: HIPDSP_ERR_UNSUPPORTED on the host, after the call has taken the scratch.
    hipdsp_chain_backward and phase 2 with the sizes of that call must then refuse ("tile states") and leave the
    envelope alone, and the good pair must give its bytes again."""
    from audian_amd import hipdsp
    sos, esos, rate, x = sweep_input()
    nfft, hop = 2048, 1024
    nd = (T + hop - 1)//hop
    c, plans = hipdsp.Context(0), {}
    r = Run(c, plans)
    try:
        fplan, eplan = r.plan('bp', sos), r.plan('env', esos)
        dx = r.upload(np.ascontiguousarray(x.T))
        c.set_option('chain_split_frames', 1)

        def good_pair():
            yf, ye, ps = r.fresh((3, T)), r.fresh((3, T)), r.fresh((3, nd, nfft//2 + 1))
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, 3, T, nfft, hop, rate, ps, nd)
            hipdsp.chain_backward(c, eplan, yf, T, ye, T, 3, T, nfft, hop, rate, ps, nd)
            return yf, [yf.to_host(), ye.to_host(), ps.to_host()]

        yf, kept = good_pair()
        c.set_option('chain_debug', 4)
        try:
            with pytest.raises(NotImplementedError, match='barrier variant'):
                if trigger.startswith('envelope plan'):
                    ps2 = r.fresh((3, (T + 511)//512, 513))
                    hipdsp.chain_forward(c, fplan, eplan, dx, T, r.fresh((3, T)), T, 3, T, 1024, 512, rate, ps2, (T + 511)//512)
                else:
                    three = r.plan('bp3', ib.design('bp3 300-3000 Hz @ 48 kHz')[0])
                    hipdsp.chain_forward(c, three, eplan, dx, T, r.fresh((3, T)), T, 3, T, nfft, hop, rate,
                                         r.fresh((3, nd, nfft//2 + 1)), nd)
            ye, ps = r.fresh((3, T)), r.fresh((3, nd, nfft//2 + 1))
            with pytest.raises(ValueError, match='tile states'):
                hipdsp.chain_backward(c, eplan, yf, T, ye, T, 3, T, nfft, hop, rate, ps, nd)
            with pytest.raises(ValueError, match='tile states'):
                hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T, 3, T, phase=2)
            c.synchronize()
            assert untouched(ye.to_host()) and untouched(ps.to_host()), 'a refused backward sweep wrote something'
        finally:
            c.set_option('chain_debug', 0)
        same_bytes(good_pair()[1], kept, 'the good pair after the refused forward sweep')
        c.synchronize()
    finally:
        r.free()
        close(c, plans)


@pytest.mark.parametrize('name', [n for n in NAMES if CASES[n].bad is not None and 'one-tile' not in n])
def test_an_error_changes_nothing(name):
    """(c), the general rule: one refused call per entry point, with the arguments of the unit's own error test; the
    context synchronises without an error and the next valid call gives the bytes it gave before."""
    from audian_amd import hipdsp
    c, plans = hipdsp.Context(0), {}
    try:
        before = CASES[name].run(c, plans)
        CASES[name].run_bad(c, plans)
        c.synchronize()                           # raises unless hipdsp_ctx_synchronize returns HIPDSP_OK
        same_bytes(CASES[name].run(c, plans), before, '%s after a refused call' % name)
        same_bytes(before, alone(name), '%s on its own context' % name)
    finally:
        close(c, plans)
