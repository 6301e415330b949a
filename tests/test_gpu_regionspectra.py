"""hipdsp_region_spectra, BufferedData.peak_freqs and PeakFrequencyAnalyzer on the GPU.  The comparator is never the
code under test: tests/spectra_definition.py (sequential numpy float64, pinned to scipy.signal.welch by the golden file).

The kernel cuts the frames of a region into groups of G = 16 consecutive frames counted from the region's first frame,
one workgroup per group, which adds its frames' spectra to float64 sums on chip; a second launch adds the groups'
partial rows of a region one after the other, in ascending order.  So of the frame counts used here 0 launches no
group at all (the second launch writes NaN and -1), 1, 2 and G-1 = 15 stay in one group that is not full, G = 16 fills
exactly one, G+1 = 17 opens a second group of one frame (the merge's first step: partial row 1 added to partial row
0), 2G+1 = 33 has three groups and 3G+2 = 50 four: there the merge goes on past its first step.  Inside a workgroup the
256 threads share a frame's nfft/4 butterflies per stage: nfft 8, 16 and 64 leave most threads idle, 512 is the first
size at which a stage gives every thread of the first half one butterfly, 1024 the first at which the butterfly loop runs
twice for a thread, and 8192 the largest, with the most LDS (96 KB) and 17 bins per thread.

Accuracy.  Every bin is held to B_k = mean_j(2 a_jk d_jk + d_jk^2) + 2^-24 ref_k, where a_jk is the amplitude (square
root of the PSD) of bin k in frame j of the definition, r_j the rms of a_j over the bins and d_jk = beta_max(nfft) EPS
(a_jk + log2(nfft) r_j) the per-frame amplitude bound every spectrogram kernel is held to (tests/spectral_bound.py): an
amplitude off by at most d changes the power by at most 2 a d + d^2, the mean over the frames keeps that, and the last
term is the rounding of the row to float32.  No new constant."""

import functools

import numpy as np
import pytest

import gpu_helpers as gh
import spectra_definition as sd
import spectral_bound as sb

pytestmark = pytest.mark.gpu

G = 16                                          # frames per group: hipdsp.SPECTRA_GROUP
COUNTS = [0, 1, 2, G - 1, G, G + 1, 2*G + 1, 3*G + 2]
STARTS = [0, 1, 2, 3, 5]
STEPS = [1, 2, 7]
NFFTS = [8, 16, 64, 512, 1024, 8192]
LEVELS3 = sb.LEVELS + (1.0,)                    # the two levels of the spectrogram tests and one between: three channels
BASE = 3                                        # elements between the allocation and x
RATE = 48000.0


def hops(nfft):
    return [nfft//2, nfft, 3] + ([1] if nfft <= 16 else [])


class Slab(object):
    """A host (C, frames) float32 array on the device with a base offset of 3 elements and pitch = frames + 7 (as
    test_gpu_regionstats.Slab)."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(BASE + self.C*self.pitch, 12345.0, dtype=np.float32)
        for c in range(self.C):
            host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(BASE, (1,))

    def spectra(self, regions, nfft, hop, step=1, fs=RATE, channels=None):
        """(rows (R, F) float32, info (R, 2) int64) through the C ABI."""
        from audian_amd import hipdsp
        return hipdsp.region_spectra(self.ctx, self.view, self.pitch, self.C if channels is None else channels,
                                     self.frames, regions, nfft, hop, step, fs)


def length_for(count, nfft, hop, step, extra=0):
    """A region length (in samples of x) that holds exactly `count` frames: `extra` < hop unused decimated samples behind
    the last frame (count 0: nfft - 1 decimated samples)."""
    decimated = (count - 1)*hop + nfft + extra if count > 0 else nfft - 1
    return (decimated - 1)*step + 1


def total_for(nfft):
    """Samples per channel of the accuracy slabs: every count fits with hop 3 at every step, the larger hops get the
    counts that fit."""
    return 40*nfft + 4000


def layout(nfft, hop, step, shift, total):
    """[(channel, start, stop)]: one region per frame count that fits into `total` samples, starts and channels taking
    turns (every start meets every count over the (hop, step) pairs of a size)."""
    regions = []
    for j, count in enumerate(COUNTS):
        start = STARTS[(shift + j) % len(STARTS)]
        n = length_for(count, nfft, hop, step, extra=(j*5) % hop)
        if start + n <= total:
            regions.append(((shift + j) % 3, start, start + n))
    return regions


def bound_and_reference(x_row, region, nfft, hop, step, fs):
    """(B (F,), ref (F,), n_frames, argmax) of one region from the definition's float64 frames."""
    c, a, b = region
    frames = sd.region_frames(x_row, a, b, nfft, hop, step)
    F = nfft//2 + 1
    if len(frames) == 0:
        return np.zeros(F), np.full(F, np.nan), 0, -1
    P = sd.frame_psds(frames, fs)
    amp = np.sqrt(P)
    r = np.sqrt(np.mean(P, axis=1, keepdims=True))
    delta = sb.beta_max(nfft)*sb.EPS*(amp + np.log2(nfft)*r)
    ref = np.mean(P, axis=0)
    return np.mean(2*amp*delta + delta*delta, axis=0) + 2.0**-24*ref, ref, len(frames), int(np.argmax(ref))


@functools.lru_cache(maxsize=None)
def family_slab(name, nfft):
    x = sb.family(name, total_for(nfft), nfft, rate=RATE, seed=11, levels=LEVELS3).T
    return x, Slab(x)


@pytest.mark.parametrize('name', sb.FAMILIES)
@pytest.mark.parametrize('nfft', NFFTS)
def test_every_bin_within_the_bound(nfft, name):
    """All families at three levels, every hop and step of the size, starts 0, 1, 2, 3 and 5, frame counts 0 ... 3G+2:
    |got - ref| <= B_k for every bin; n_frames exact; argmax is that of the returned row, and the definition's wherever
    the reference's two largest bins differ by more than their bounds."""
    x, slab = family_slab(name, nfft)
    worst, seen, counts, decided = 0.0, 0, set(), 0
    for shift, (hop, step) in enumerate((h, s) for h in hops(nfft) for s in STEPS):
        regions = layout(nfft, hop, step, shift, slab.frames)
        fs = RATE/step
        rows, info = slab.spectra(regions, nfft, hop, step, fs)
        assert rows.shape == (len(regions), nfft//2 + 1) and rows.dtype == np.float32 and info.dtype == np.int64
        for i, region in enumerate(regions):
            B, ref, n, argmax = bound_and_reference(x[region[0]], region, nfft, hop, step, fs)
            what = '%s nfft %d hop %d step %d region %r' % (name, nfft, hop, step, region)
            assert info[i, 0] == n, what
            counts.add(n)
            if n == 0:
                assert np.isnan(rows[i]).all() and info[i, 1] == -1, what
                continue
            assert np.isfinite(rows[i]).all() and (rows[i] >= 0).all(), what
            err = np.abs(rows[i].astype(np.float64) - ref)
            k = int(np.argmax(err - B))
            assert err[k] <= B[k], '%s: bin %d is %r, reference %r, allowed +-%.3g' % (what, k, rows[i, k], ref[k], B[k])
            worst = max(worst, float(np.max(err/B)))
            assert info[i, 1] == np.argmax(rows[i]), what
            order = np.argsort(ref)
            if ref[order[-1]] - ref[order[-2]] > B[order[-1]] + B[order[-2]]:
                assert info[i, 1] == argmax, what
                decided += 1
            seen += 1
    print('%s nfft %d: %d spectra, worst |err|/B %.3g, argmax decided for %d, frame counts %s'
          % (name, nfft, seen, worst, decided, sorted(counts)))
    # (the spectrum of a chirp is symmetric about its centre: its two largest bins are often equal to rounding)
    assert counts == set(COUNTS) and decided > (0 if name == 'chirp' else seen//2)


@pytest.fixture(scope='module')
def exact_slab():
    """Three channels of 150000 samples: noise over a tone and an offset; channel 2 constant from 75000 on."""
    rng = np.random.default_rng(5)
    n = 150000
    x = (0.3*rng.standard_normal((3, n)) + np.sin(2*np.pi*0.11*np.arange(n)) + 2.0).astype(np.float32)
    x[2, 75000:] = np.float32(0.1)
    return x, Slab(x)


def test_constant_regions_are_exactly_zero(exact_slab):
    x, slab = exact_slab
    for nfft, hop, step in [(8, 4, 1), (64, 3, 2), (1024, 512, 7), (8192, 8192, 1)]:
        regions = [(2, 75001, 75001 + length_for(count, nfft, hop, step)) for count in (1, G, 2*G + 1)
                   if length_for(count, nfft, hop, step) < 74999]
        rows, info = slab.spectra(regions, nfft, hop, step)
        assert len(regions) and (rows == 0.0).all() and not np.signbit(rows).any(), (nfft, hop, step)
        assert (info[:, 1] == 0).all() and (info[:, 0] > 0).all()


NONFINITE = [np.nan, np.inf, -np.inf]


@pytest.mark.parametrize('nfft,hop,step', [(16, 8, 1), (512, 3, 7), (1024, 512, 2)])
def test_nonfinite_samples_poison_their_region_only(exact_slab, nfft, hop, step):
    """A NaN, +inf or -inf in a used frame of channel 1 (first, middle and last used sample, the first frame, a middle
    group and the last frame): that region's row is NaN with argmax 0 and n_frames as before; regions that do not
    hold the sample (next to it, overlapping elsewhere, on other channels) keep their bytes; so does the region when
    the sample lies in its unused tail or between the decimated samples."""
    x, slab = exact_slab
    count = 2*G + 1
    n = length_for(count, nfft, hop, step, extra=min(2, hop - 1))
    a = 101
    used_last = a + ((count - 1)*hop + nfft - 1)*step          # the last sample of the last frame
    target = (1, a, a + n)
    regions = [target, (0, a, a + n), (2, a, a + n), (1, a + n, min(a + 2*n, slab.frames)), (1, 0, a),
               (1, a, a + length_for(1, nfft, hop, step))]
    clean_rows, clean_info = slab.spectra(regions, nfft, hop, step)
    assert clean_info[0, 0] == count and np.isfinite(clean_rows[0]).all()
    middle = a + ((G + 3)*hop + nfft//2)*step
    for k, at in enumerate([a, middle, used_last]):
        y = x.copy()
        y[1, at] = NONFINITE[k % 3]
        rows, info = Slab(y).spectra(regions, nfft, hop, step)
        assert np.isnan(rows[0]).all() and info[0].tolist() == [count, 0], (at, NONFINITE[k % 3])
        for i in range(1, len(regions)):
            c, p, q = regions[i]
            holds = c == 1 and p <= at < q and at <= p + ((int(clean_info[i, 0]) - 1)*hop + nfft - 1)*step \
                and (at - p) % step == 0
            if holds:
                assert np.isnan(rows[i]).all() and info[i].tolist() == [clean_info[i, 0], 0]
            else:
                assert rows[i].tobytes() == clean_rows[i].tobytes() and info[i].tolist() == clean_info[i].tolist(), (at, i)
    # the unused tail, and (with a step) a sample between the decimated ones
    harmless = [at for at in (used_last + 1, a + n - 1) if used_last < at < a + n] + ([a + 1] if step > 1 else [])
    assert harmless
    y = x.copy()
    y[1, harmless] = np.nan
    rows, info = Slab(y).spectra(regions[:3], nfft, hop, step)
    assert rows.tobytes() == clean_rows[:3].tobytes() and info.tobytes() == clean_info[:3].tobytes()


def test_bit_identity(exact_slab):
    """Twice the same bytes; a region alone, among 40 others, in reversed order and with channels = 1 instead of 3 gives
    the same row and info; overlapping and duplicate regions are allowed."""
    x, slab = exact_slab
    rng = np.random.default_rng(1)
    for nfft, hop, step in [(64, 32, 1), (1024, 3, 2), (8192, 4096, 1)]:
        mine = [(0, 5, 5 + length_for(2*G + 1, nfft, hop, step, extra=1)), (0, 0, length_for(1, nfft, hop, step)),
                (0, 3, 3 + length_for(G + 1, nfft, hop, step)), (0, 7, 7 + nfft - 1)]
        others = []
        for k in range(40):
            n = int(rng.integers(0, min(slab.frames, length_for(3*G, nfft, hop, step))))
            p = int(rng.integers(0, slab.frames - n))
            others.append((int(rng.integers(0, 3)), p, p + n))
        others[7] = others[3]                                   # a duplicate
        others[9] = mine[0]                                     # and one of mine again, elsewhere in the table
        alone = [slab.spectra([r], nfft, hop, step) for r in mine]
        table = others[:11] + [mine[0]] + others[11:25] + [mine[1], mine[2]] + others[25:] + [mine[3]]
        where = [11, 26, 27, len(table) - 1]
        rows, info = slab.spectra(table, nfft, hop, step)
        again = slab.spectra(table, nfft, hop, step)
        assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == info.tobytes()
        back = slab.spectra(table[::-1], nfft, hop, step)
        assert back[0][::-1].tobytes() == rows.tobytes() and back[1][::-1].tobytes() == info.tobytes()
        for (r, i), at in zip(alone, where):
            assert rows[at].tobytes() == r[0].tobytes() and info[at].tobytes() == i[0].tobytes(), (nfft, at)
        assert rows[9].tobytes() == rows[11].tobytes() and rows[7].tobytes() == rows[3].tobytes()
        one = slab.spectra(mine, nfft, hop, step, channels=1)
        three = slab.spectra(mine, nfft, hop, step, channels=3)
        assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes()
        assert info[where[0], 0] == 2*G + 1 and info[where[3], 0] == 0


def test_errors_are_decided_on_the_host(exact_slab):
    from audian_amd import hipdsp
    x, slab = exact_slab
    ok = dict(nfft=64, hop=32, step=1)
    for bad in (dict(nfft=12), dict(nfft=4), dict(nfft=16384), dict(nfft=0), dict(hop=0), dict(hop=65), dict(hop=-1),
                dict(step=0), dict(step=-3)):
        with pytest.raises(ValueError):
            slab.spectra([(0, 0, 1000)], **dict(ok, **bad))
    with pytest.raises(ValueError, match='fs'):
        slab.spectra([(0, 0, 1000)], fs=0.0, **ok)
    for region, message in [((3, 0, 100), 'channel 3'), ((-1, 0, 100), 'channel -1'), ((0, -1, 100), 'not inside'),
                            ((0, 0, slab.frames + 1), 'not inside'), ((0, 100, 99), r'\[100, 99\)')]:
        with pytest.raises(ValueError, match=message):
            slab.spectra([(0, 0, 1000), region], **ok)
    with pytest.raises(ValueError, match='channel 1'):
        slab.spectra([(1, 0, 1000)], channels=1, **ok)
    out = hipdsp.DeviceArray(slab.ctx, (1, 33), np.float32)
    info = hipdsp.DeviceArray(slab.ctx, (1, 2), np.int64)
    for o, i in ((None, info), (out, None)):
        with pytest.raises(ValueError, match='NULL output'):
            hipdsp.region_spectra_into(slab.ctx, slab.view, slab.pitch, 3, slab.frames, [(0, 0, 1000)], 64, 32, 1, RATE, o, i)
    with pytest.raises(ValueError, match='out_pitch'):
        hipdsp.region_spectra_into(slab.ctx, slab.view, slab.pitch, 3, slab.frames, [(0, 0, 1000)], 64, 32, 1, RATE, out,
                                   info, out_pitch=32)
    # no region: nothing is written, not even with NULL outputs
    sentinel = hipdsp.DeviceArray.from_host(slab.ctx, np.full(33, -7.5, dtype=np.float32))
    hipdsp.region_spectra_into(slab.ctx, slab.view, slab.pitch, 3, slab.frames, np.zeros((0, 3), dtype=np.int64), 64, 32, 1,
                               RATE, sentinel, None)
    assert (sentinel.to_host() == -7.5).all()
    rows, info = slab.spectra([], **ok)
    assert rows.shape == (0, 33) and info.shape == (0, 2)
    rows, info = slab.spectra([(0, 0, 1000)], **ok)             # the context still works
    assert info[0, 0] == 30 and np.isfinite(rows).all()


def test_writes_exactly_its_rows(exact_slab):
    """out_pitch > F: the gaps between the rows and what lies around them stay untouched."""
    from audian_amd import hipdsp
    x, slab = exact_slab
    F, pitch, R, pad = 33, 40, 3, 8
    regions = [(0, 0, 1000), (1, 5, 40), (2, 100, 3000)]
    host = np.full(pad + R*pitch + pad, -7.5, dtype=np.float32)
    dev = hipdsp.DeviceArray.from_host(slab.ctx, host)
    info = hipdsp.DeviceArray(slab.ctx, (R, 2), np.int64)
    hipdsp.region_spectra_into(slab.ctx, slab.view, slab.pitch, 3, slab.frames, regions, 64, 32, 1, RATE, dev.view(pad, (R*pitch,)),
                               info, out_pitch=pitch)
    back = dev.to_host()
    rows, want_info = slab.spectra(regions, 64, 32)
    assert (back[:pad] == -7.5).all() and (back[-pad:] == -7.5).all()
    inner = back[pad:-pad].reshape(R, pitch)
    assert (inner[:, F:] == -7.5).all() and inner[:, :F].tobytes() == rows.tobytes()
    assert info.to_host().tobytes() == want_info.tobytes() and np.isnan(rows[1]).all()


class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def test_facade_peak_freqs_and_analyzer_on_the_mirror():
    """filter + envelope on 3 channels x 10 s of amplitude-modulated tones in bursts: BufferedData.peak_freqs and
    PeakFrequencyAnalyzer.analyze_many run on the device mirror -- one hipdsp_region_spectra call per nfft group, the
    host copy as stale as before -- and give the host version's frequencies exactly and its powers within the bound."""
    from audian_amd import hipdsp
    from audian_amd.analyzer import PeakFrequencyAnalyzer
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.peaks import host_find_peaks
    from audian_amd.spectra import event_nfft, welch_nfft
    from audian_amd.tracegraph import TraceGraph
    rate, seconds, C = 16000.0, 10.0, 3
    rng = np.random.default_rng(31)
    n = int(rate*seconds)
    t = np.arange(n)/rate
    x = 0.002*rng.standard_normal((n, C))
    bursts = {0: [(0.5, 2.0), (3.0, 3.4), (6.0, 9.0)], 1: [(1.0, 1.02), (4.0, 6.5)], 2: [(0.2, 0.26), (2.0, 2.3), (7.0, 9.5)]}
    for c in range(C):
        for t0, t1 in bursts[c]:
            on = (t >= t0) & (t < t1)
            x[on, c] += (1.0 + 0.7*np.sin(2*np.pi*(25.0 + 10*c)*t[on]))*0.3*np.sin(2*np.pi*(1200.0 + 700*c)*t[on])
    g = TraceGraph(30.0, 5.0)
    for tr in (BufferedFilter(), BufferedEnvelope(envelope_cutoff=200.0)):
        g.add_trace(tr)
    g.setup_traces()
    g.open(x.astype(np.float32).astype(np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g['filtered'].highpass_cutoff, g['filtered'].lowpass_cutoff = 300.0, 6000.0
    g['filtered'].update()
    g.update_times(0.0, seconds)
    f, e = g['filtered'], g['envelope']
    ev = g.detect_events('envelope', 0.04, min_gap=0.05, min_duration=0.01)
    assert [len(o) for o in ev.onsets] == [3, 2, 3]
    stale = {tr.name: [list(r) for r in tr._stale] for tr in g.traces[1:]}
    assert stale['filtered'] and stale['envelope']
    thresh = 10.0
    top = welch_nfft(rate, 10.0)
    sizes = sorted({event_nfft(b - a, top) for c in range(C) for a, b in ev.frames(c).tolist()} - {0})
    assert top == 2048 and len(sizes) >= 3
    before = dict(hipdsp.launches)
    hz = f.peak_freqs(ev, 10.0)
    assert hipdsp.launches['region_spectra'] == before.get('region_spectra', 0) + len(sizes)
    assert hipdsp.launches.get('find_peaks', 0) == before.get('find_peaks', 0)
    hz_thresh, power_thresh = f.peak_freqs(ev, 10.0, thresh=thresh, powers=True)
    assert hipdsp.launches['region_spectra'] == before.get('region_spectra', 0) + 2*len(sizes)
    a = PeakFrequencyAnalyzer(g, 'filtered', freq_resolution=10.0, thresh=thresh)
    count = hipdsp.launches['region_spectra']
    g.analyze_events(ev)
    assert hipdsp.launches['region_spectra'] <= count + C*len(sizes)
    rows = a.rows()
    assert len(rows) == len(ev)
    pulse = g.event_peak_freqs(ev, freq_resolution=2.0)                     # the envelope at 16000/8 Hz
    assert {tr.name: [list(r) for r in tr._stale] for tr in g.traces[1:]} == stale      # nothing crossed
    # the host versions last: they read the host copy
    for tr in (f, e):
        tr._spectra_on_mirror = lambda tab: False
    before = dict(hipdsp.launches)
    host = f.peak_freqs(ev, 10.0)
    host_thresh, host_power = f.peak_freqs(ev, 10.0, thresh=thresh, powers=True)
    host_pulse = g.event_peak_freqs(ev, freq_resolution=2.0)
    assert hipdsp.launches.get('region_spectra', 0) == before.get('region_spectra', 0)
    k = 0
    for c in range(C):
        assert np.array_equal(hz[c], host[c], equal_nan=True) and np.array_equal(hz_thresh[c], host_thresh[c], equal_nan=True)
        assert np.array_equal(pulse[c], host_pulse[c], equal_nan=True)
        v = np.asarray(f[:, c]).astype(np.float32)
        for j, (p, q) in enumerate(ev.frames(c).tolist()):
            nfft = event_nfft(q - p, top)
            if nfft == 0:
                assert np.isnan(hz[c][j]) and np.isnan(hz_thresh[c][j]) and np.isnan(rows[k][0])
                k += 1
                continue
            B, ref, frames, argmax = bound_and_reference(v, (c, p, q), nfft, nfft//2, 1, rate)
            want = sd.pick_peak(ref, thresh, rate)
            # the inputs: of the peaks at least as strong as the picked one -- the only ones whose being a candidate
            # or not decides the result -- none has a prominence within 1e-3 dB of the threshold
            with np.errstate(divide='ignore'):
                pos, props = host_find_peaks(10.0*np.log10(ref), prominence=(0.0, None))
            strong = ref[pos] >= ref[int(round(want*nfft/rate))]
            assert strong.any() and np.min(np.abs(props[strong, 1] - thresh)) > 1e-3
            assert hz_thresh[c][j] == want and abs(hz[c][j] - (1200.0 + 700*c)) <= rate/nfft, (c, j)
            bin_ = int(round(want*nfft/rate))
            assert abs(power_thresh[c][j] - ref[bin_]) <= B[bin_] and abs(host_power[c][j] - ref[bin_]) <= 1e-9*ref[bin_]
            assert rows[k][0] == want and rows[k][1] == power_thresh[c][j]
            k += 1
        long = [j for j, (p, q) in enumerate(ev.frames(c).tolist()) if q - p >= 2*rate]
        assert long and all(abs(pulse[c][j] - (25.0 + 10*c)) <= 2000.0/1024 for j in long)
