"""Per-bin spectrogram accuracy on every path hipdsp_spectrogram and hipdsp_chain_forward take
(spectrogram.hip's dispatch, the fused sweep's six windows): each frame against the float64 oracle under the
bound of tests/spectral_bound.py (calibrated on the CPU by tests/test_spectral_bound.py), on signal families that
span 60-120 dB inside a frame, with the dB image held to the same bound.  A failure names the path, nfft, hop,
family and the worst frame; test_zz_worst_per_path prints the worst rho and beta of every path measured.

The non-stationary families (spectral_bound.NONSTATIONARY: a level that falls back, rises, steps, bursts, goes
silent, pulses on the frame borders, a decaying transient) hold a frame's accuracy independent of the frames before
it, on every path and with the event placed by the runs and batches the kernels walk (test_nonstationary_*).
Measured on an MI355X, worst over the cases that pass (rho of 2; beta of its bound 4 log2 nfft):

    default            rho 1.46 (nfft 131072) beta 48.9 of 68 (131072)     spec_kernel=2   1.10 (16384)  25.9 of 60
    spec_fpw=3         rho 1.24 (32768)       beta 21.4 of 60 (32768)      spec_kernel=3   0.63 (256)     2.6 of 48
    spec_fpw=16        rho 1.24 (32768)       beta 27.5 of 60 (32768)      spec_no_half    0.62 (256)     1.9 of 40
    spec_fpw=1         rho 0.80 (8)           beta 0.6 of 12               direct          0.29 (24)      3.9 of 40
    force_generic_fft  rho 1.82 (4096)        beta 2.8 of 48               fused, all six windows, both plans
    fused split frames rho 0.53               beta 1.8 of 44                       rho 0.39-0.56, beta 0.7-2.7 of 32-44

Before the kernels that carry a pivot learnt to find their own: spec_fast_kernel with register reuse
rho 243 (2048 / 512, fall of 1e4 levels) and inf on silence; spec_pack_kernel rho 8.6e4 (128 / 64, fall of 1e6, over
the 8 frames of a batch), 1.1e3 behind 1e4, 8.9 behind 1e2; spec_wgs_kernel rho 3.0e4 (8192 / 4096, 1e6), 477 (4096 /
2048, 1e4), 4.3 behind 1e2; psd_frame_pivot (the odd frames of 2048 / 1024 under "chain_split_frames", walked backwards
with a pivot two hops old) rho 1.1e3 behind a rise of 1e4 in one segment, 6.8 on the staircase of 1e2 -- and, own pivot
or not, 2.07 where a step of 1e6 ended one sample before the frame: its float32 sum of what the detrending left is good
to eps times the frame's largest sample, the filter's ringing there; that sum is float64 in this kernel now.

And one find that the pivot has no part in: 'fall' with the event ONE SAMPLE BEFORE A BORDER, on the kernels that
compute their Hann window in float32 as 0.5 - 0.5 cos (spec_wgs.h 8192-32768, spec_chip.h 65536).  The frame before
the fall ends on a sample S levels under the rest of it, where the window is 1.5e-7 -- and carried an absolute error
of 3e-8 there (the cancellation near cos = 1; a float64 table rounded to float32, as the short windows use, has none).
S times that error is spread over every bin: rho 6.8 / 9.7 (8192, S 1e4 / 1e6), 7.6 and 5.0 (16384), 3.8 (32768 with
"spec_fpw" 16), 3.8 (65536), against 0.3 of the faithful emulation; an emulation of spec_wgs.h's window arithmetic on
the CPU gave the same 6.8.  Both kernels now take the weights next to the window's zeros as 0.5 sin^2 / (1 + cos).
"""

import numpy as np
import pytest

import gpu_helpers as gh
import spectral_bound as sb

pytestmark = pytest.mark.gpu

RATE = 48000.0
WORST = {}


def note(path, nfft, rb):
    old = WORST.get((path, nfft), (0.0, 0.0))
    WORST[(path, nfft)] = (max(old[0], rb[0]), max(old[1], rb[1]))


def frames_for(nfft):
    return 3 if nfft <= 16384 else 2


def reference(oracle, x, nfft, hop, frames_out):
    """float64 PSD of the float32 input laid out (C, frames_out, F) like the kernel's output."""
    want = np.zeros((frames_out, x.shape[1], nfft//2 + 1))
    oracle.spectrogram_process(x.astype(np.float64), want, RATE, nfft, hop)
    return want.transpose(1, 0, 2)


def run_spec(x, nfft, hop, frames_out, options=(), want_db=False):
    """hipdsp_spectrogram with context options set for the call; (C, frames_out, F) PSD and dB image (or None)."""
    from audian_amd import hipdsp
    c = gh.ctx()
    T, C = x.shape
    F = nfft//2 + 1
    for k, v in options:
        c.set_option(k, v)
    try:
        dx = gh.to_planar(c, x)
        out = hipdsp.DeviceArray(c, (C, frames_out, F), np.float32)
        db = hipdsp.DeviceArray(c, (C, frames_out, F), np.float32) if want_db else None
        for arr in (out, db) if want_db else (out,):
            hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(arr), 0x7f, 4*C*frames_out*F)   # every bin must be written
        hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, RATE, out, frames_out, db_out=db)
        return out.to_host(), (db.to_host() if want_db else None)
    finally:
        for k, _ in options:
            c.set_option(k, 0)


def check_case(oracle, path, name, nfft, hop, options=(), want_db=False, frames=None, direct=False, seed=0):
    frames = frames or frames_for(nfft)
    x = sb.family(name, (frames - 1)*hop + nfft, nfft, RATE, seed=seed + nfft + hop)
    got, db = run_spec(x, nfft, hop, frames + 1, options, want_db)          # one frame past the input: zero
    want = reference(oracle, x, nfft, hop, frames + 1)
    assert np.all(got[:, frames] == 0), (path, nfft, hop, name, 'zero tail')
    if want_db:
        assert np.all(db[:, frames] == -np.inf), (path, nfft, hop, name, 'zero tail dB')
    what = '%s nfft %d hop %d family %s%s' % (path, nfft, hop, name, ' +dB' if want_db else '')
    rb = sb.assert_within(got, want, nfft, what, direct=direct, db=db)
    note(path, nfft, rb)


POW2 = [2**k for k in range(3, 20)]


@pytest.mark.parametrize('nfft', POW2)
def test_default_dispatch(oracle, nfft):
    """Every power of two with the default kernel choice, every family, the dB image on every other one."""
    names = sb.FAMILIES if nfft <= 65536 else ('tones', 'edges', 'offset')
    for i, name in enumerate(names):
        check_case(oracle, 'default', name, nfft, nfft//2, want_db=i % 2 == 1)


@pytest.mark.parametrize('nfft', POW2)
def test_spec_kernel_2(oracle, nfft):
    """"spec_kernel" 2: the two-stage kernel / run_wg up to 32768, the four-step path through HBM from 65536."""
    for i, name in enumerate(('tones', 'edges', 'chirp')):
        check_case(oracle, 'spec_kernel=2', name, nfft, nfft//2, options=[('spec_kernel', 2)], want_db=i == 1)


@pytest.mark.parametrize('nfft', [256, 512, 1024, 4096])
def test_spec_kernel_3(oracle, nfft):
    for i, name in enumerate(('tones', 'bandpass', 'edges')):
        for hop in (nfft//2, nfft//4):
            check_case(oracle, 'spec_kernel=3', name, nfft, hop, options=[('spec_kernel', 3)], want_db=i == 2)


@pytest.mark.parametrize('fpw', [1, 3])
@pytest.mark.parametrize('nfft', [8, 32, 128, 256, 1024])
def test_spec_fpw(oracle, nfft, fpw):
    """Frames per wave forced on the short-window kernels, over a run of frames long enough to use it."""
    for name in ('tones', 'edges'):
        check_case(oracle, 'spec_fpw=%d' % fpw, name, nfft, nfft//2, options=[('spec_fpw', fpw)], frames=40)


@pytest.mark.parametrize('nfft', [256, 512, 1024, 2048])
def test_spec_no_half(oracle, nfft):
    for name in ('tones', 'edges', 'offset'):
        check_case(oracle, 'spec_no_half', name, nfft, nfft//2, options=[('spec_no_half', 1)], frames=8)


@pytest.mark.parametrize('nfft', [256, 4096, 16384])
def test_force_generic_fft(oracle, nfft):
    for i, name in enumerate(('tones', 'edges', 'offset')):
        check_case(oracle, 'force_generic_fft', name, nfft, nfft//2, options=[('force_generic_fft', 1)],
                   want_db=i == 1)


def hops(nfft):
    return [nfft, nfft//2, nfft//4, (nfft//3) | 1]


@pytest.mark.parametrize('nfft', [8, 64, 512, 1024, 2048, 4096, 8192, 65536])
def test_hops_with_and_without_db(oracle, nfft):
    """hop nfft, nfft/2, nfft/4 and an odd hop, with and without the dB image (at 512 and 1024 the kernel choice
    depends on both)."""
    for j, hop in enumerate(hops(nfft)):
        for want_db in (False, True):
            name = sb.FAMILIES[(j + 2*want_db) % len(sb.FAMILIES)] if nfft <= 8192 else ('tones', 'edges')[want_db]
            check_case(oracle, 'default', name, nfft, hop, want_db=want_db, frames=6 if nfft <= 8192 else 2)


@pytest.mark.parametrize('nfft', [24, 1000, 3000, 12000])
def test_direct_dft(oracle, nfft):
    """Sizes that are not powers of two: the direct DFT, under its own bound (sqrt(nfft) growth)."""
    names = sb.FAMILIES if nfft <= 3000 else ('tones', 'edges')
    for i, name in enumerate(names):
        check_case(oracle, 'direct', name, nfft, nfft//2 + (i % 2), want_db=i % 2 == 0, direct=True,
                   frames=2 if nfft <= 3000 else 1)


SHAPES = [(2048, 1024), (2048, 512), (1024, 512), (1024, 256), (512, 256), (256, 128)]


@pytest.mark.parametrize('nfft,hop', SHAPES)
def test_fused_sweep(oracle, nfft, hop):
    """hipdsp_chain_forward's spectrogram for all six windows, 2- and 4-section band-passes, with and without the
    envelope plan, with the dB image, spec_first > 0, one segment and many.  The oracle reads the filtered trace
    the same launch wrote, so the bound measures the transform alone."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = gh.ctx()
    C, T = 2, 60001
    F = nfft//2 + 1
    cases = [(1, 'tones', True, True, 0, 0), (2, 'edges', False, True, 300, 1), (1, 'chirp', True, False, 5, 37),
             (2, 'bandpass', False, False, 0, 1)]
    for order, name, with_env, with_db, spec_first, max_segments in cases:
        x = sb.family(name, T, nfft, RATE, seed=nfft + hop + order)
        sos = butter_sos(order, (300.0, 9000.0), 'bandpass', RATE)           # order 1 / 2: one / two sections
        sos = np.concatenate([sos, butter_sos(order, (200.0, 12000.0), 'bandpass', RATE)])
        esos = butter_sos(2, 20.0, 'lowpass', RATE)
        fplan = hipdsp.SosPlan(c, sos)
        eplan = hipdsp.SosPlan(c, esos) if with_env else None
        nsrc = T - spec_first
        nd = (nsrc + hop - 1)//hop + 1
        c.set_max_segments(max_segments)
        try:
            dx = gh.to_planar(c, x)
            yf = hipdsp.DeviceArray(c, (C, T), np.float32)
            ps = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
            db = hipdsp.DeviceArray(c, (C, nd, F), np.float32) if with_db else None
            for arr in (ps, db) if with_db else (ps,):
                hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(arr), 0x7f, 4*C*nd*F)
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, RATE, ps, nd, db_out=db,
                                 spec_first=spec_first)
            gf, gs = yf.to_host(), ps.to_host()
            gdb = db.to_host() if with_db else None
        finally:
            c.set_max_segments(0)
        want = np.zeros((nd, C, F))
        oracle.spectrogram_process(gf.T[spec_first:].astype(np.float64), want, RATE, nfft, hop)
        want = want.transpose(1, 0, 2)
        zero = np.max(want, axis=-1) == 0
        assert zero.any() and not zero.all()
        what = 'fused %d/%d family %s, %d sections%s%s, spec_first %d, max_segments %d' % (
            nfft, hop, name, len(sos), ', envelope' if with_env else '', ' +dB' if with_db else '', spec_first,
            max_segments)
        rb = sb.assert_within(gs, want, nfft, what, db=gdb)
        note('fused %d/%d' % (nfft, hop), nfft, rb)


# ---- non-stationary traces (spectral_bound.NONSTATIONARY): a frame's accuracy must not depend on the frames before it
#
# The kernels that carry the pivot of a frame's mean from frame to frame process frames in RUNS, and the run's first
# frame finds its own pivot.  What the launchers make of the small shapes here (spectrogram.hip, spec_pack.h,
# spec_wgs.h; a batch is the G = 64 / LPF frames a wave transforms side by side):
#
#   run_pack  nfft   8  16  32  64 128 256 512 1024     a run is "spec_fpw" batches (1 unless the call has more than
#             G     64  64  32  16   8   4   2    1     2 x 48 x CUs batches); up to nfft 64 every batch takes two steps
#   run_fast  nfft 256 512 1024 2048 4096               a run is "spec_fpw" batches, 4 by default (frames_per_wave());
#             G      4   2    1    1    1               the pivot is carried at 1024 and 2048 with hop nfft/2, nfft/4
#   run_wgs   nfft 4096 ... 32768, G = 1                a run is "spec_fpw" frames (1 unless frames x channels > 4 OCC CUs)
#
# ns_frames_for() gives 200 frames up to nfft 64 (three full batches of 64 and a ragged one of 8), 40 up to 1024 (at
# G = 8 with "spec_fpw" 3: a run of 24 and a ragged one of 16; at G = 1 with runs of 4 or 16: ten or two and a half
# runs), 12 up to 32768 (three runs of 4; one ragged run of "spec_fpw" 16) and 3 from 65536 (no kernel carries
# anything there).  EVENT_SLOTS places the event by run and batch.

NS_OTHER = tuple(n for n in sb.NONSTATIONARY if n != 'fall')
EVENT_SLOTS = ('first', 'border', 'later', 'last')
PACK_G = {8: 64, 16: 64, 32: 32, 64: 16, 128: 8, 256: 4, 512: 2, 1024: 1}


def ns_frames_for(nfft):
    return 200 if nfft <= 64 else (40 if nfft <= 1024 else (12 if nfft <= 32768 else 3))


def batch_and_run(nfft, options, want_db=False):
    """(G, frames per run) of the kernel that carries a pivot at this size, as the launchers above have it."""
    fpw = dict(options).get('spec_fpw', 0)
    G = PACK_G.get(nfft, 1)
    if nfft <= 512 or (nfft == 1024 and want_db):
        return G, G*(fpw or 1)                                 # run_pack (1024: with the dB image)
    if nfft <= 2048:
        return 1, fpw or 4                                     # run_fast, one frame per wave
    return 1, fpw or 1                                         # run_wgs and the kernels that carry nothing


def event_frame(slot, frames, G, run):
    """The frame of the event: in the first batch of the second run (the first, where there is only one), on that
    run's first batch border, in its third batch, or in the ragged last batch of all the frames."""
    base = run if 2*run <= frames else 0
    f = {'first': base + G//2, 'border': base + G, 'later': base + 2*G + G//2,
         'last': G*((frames - 1)//G) + ((frames - 1) % G)//2}[slot]
    return min(max(f, 1), frames - 2)


def ns_case(path, name, nfft, hop, S, i, options=(), want_db=False, frames=None, direct=False):
    """One case: family `name` with a step of S levels, the event's slot and placement rotated by the index i."""
    frames = frames or ns_frames_for(nfft)
    slot, place = EVENT_SLOTS[i % 4], sb.PLACES[(i//2) % 3]
    frame = event_frame(slot, frames, *batch_and_run(nfft, options, want_db))
    return dict(path=path, name=name, nfft=nfft, hop=hop, S=S, slot=slot, place=place, frame=frame,
                options=tuple(options), want_db=want_db, frames=frames, direct=direct)


def ns_sweep(path, nfft, k, options=(), hop_list=None, frames=None, direct=False, both=True):
    """The cases of one path at one size: every hop with 'fall' (S rotating with the hop) and, where `both`, one
    other family; the dB image on every other case."""
    cases = []
    for h, hop in enumerate(hop_list or hops(nfft)):
        i = 4*k + h
        cases.append(ns_case(path, 'fall', nfft, hop, sb.STEPS[i % 3], i, options, h % 2 == 1, frames, direct))
        if both:
            cases.append(ns_case(path, NS_OTHER[i % 6], nfft, hop, sb.STEPS[(i + 1) % 3], i + 1, options, h % 2 == 0,
                                 frames, direct))
    return cases


def k_of(nfft):
    return POW2.index(nfft)


def default_cases(nfft):
    cases = ns_sweep('default', nfft, k_of(nfft), both=nfft <= 32768)
    if nfft > 32768:                                         # one more family per size there, on one hop
        cases.append(ns_case('default', NS_OTHER[(k_of(nfft) + 1) % 6], nfft, nfft//2, sb.STEPS[k_of(nfft) % 3],
                             k_of(nfft)))
    return cases


def kernel2_cases(nfft):
    return ns_sweep('spec_kernel=2', nfft, k_of(nfft) + 1, [('spec_kernel', 2)], both=nfft <= 32768)


def kernel3_cases(nfft):
    return ns_sweep('spec_kernel=3', nfft, k_of(nfft) + 2, [('spec_kernel', 3)])


def fpw_cases(nfft, fpw):
    return ns_sweep('spec_fpw=%d' % fpw, nfft, k_of(nfft) + fpw, [('spec_fpw', fpw)])


def no_half_cases(nfft):
    return ns_sweep('spec_no_half', nfft, k_of(nfft), [('spec_no_half', 1)])


def generic_cases(nfft):
    return ns_sweep('force_generic_fft', nfft, k_of(nfft) + 1, [('force_generic_fft', 1)])


def direct_cases(nfft):
    return ns_sweep('direct', nfft, nfft % 7, hop_list=[nfft, nfft//2, nfft//4, (nfft//3) | 1], frames=7, direct=True)


FUSED_FRAMES = 72                          # frames of a fused case (256 / 128 needs 64 for the sweep's four tiles); events by runs of 8


def fused_cases(nfft, hop, plan):
    """'fall' at every S, 'silence' and one more family, per window and forward plan; dB and envelope plan alternate."""
    k = SHAPES.index((nfft, hop)) + (plan == 'bandpass')
    todo = [('fall', sb.STEPS[j], 4*k + j) for j in range(3)] + [('silence', 1.0, k),
                                                                    (NS_OTHER[k % 6], sb.STEPS[k % 3], k + 1)]
    cases = []
    for j, (name, S, i) in enumerate(todo):
        slot, place = EVENT_SLOTS[i % 4], sb.PLACES[(i//2) % 3]
        cases.append(dict(path='fused ' + plan, name=name, nfft=nfft, hop=hop, S=S, slot=slot, place=place,
                          frame=event_frame(slot, FUSED_FRAMES, 1, 8), want_db=j % 2 == 1, with_env=j % 3 == 0,
                          max_segments=1 if plan == 'bandpass' else (0, 37, 1)[j % 3]))
    return cases


def check_ns(oracle, case):
    path, name, nfft, hop, frames = case['path'], case['name'], case['nfft'], case['hop'], case['frames']
    x = sb.nonstationary(name, (frames - 1)*hop + nfft, nfft, hop, RATE, seed=nfft + hop, S=case['S'],
                         place=case['place'], frame=case['frame'])
    got, db = run_spec(x, nfft, hop, frames + 1, case['options'], case['want_db'])
    want = reference(oracle, x, nfft, hop, frames + 1)
    what = '%s nfft %d hop %d family %s S %g event %s of frame %d (%s)%s' % (
        path, nfft, hop, name, case['S'], case['place'], case['frame'], case['slot'], ' +dB' if case['want_db'] else '')
    assert np.all(got[:, frames] == 0), (what, 'zero tail')
    if case['want_db']:
        assert np.all(db[:, frames] == -np.inf), (what, 'zero tail dB')
    if name == 'silence':
        assert (want[:, :frames].max(axis=-1) == 0).any(), what
    rb = sb.assert_within(got, want, nfft, what, direct=case['direct'], db=db)
    note('ns ' + path, nfft, rb)


def check_all(oracle, cases):
    """Every case is measured; the first failure is raised after the last one, with all of them in its message."""
    failed = []
    for case in cases:
        try:
            check_ns(oracle, case)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '%d of %d cases:\n%s' % (len(failed), len(cases), '\n'.join(failed))


@pytest.mark.parametrize('nfft', POW2)
def test_nonstationary_default_dispatch(oracle, nfft):
    check_all(oracle, default_cases(nfft))


@pytest.mark.parametrize('nfft', POW2)
def test_nonstationary_spec_kernel_2(oracle, nfft):
    check_all(oracle, kernel2_cases(nfft))


KERNEL3 = [256, 512, 1024, 4096]


@pytest.mark.parametrize('nfft', KERNEL3)
def test_nonstationary_spec_kernel_3(oracle, nfft):
    check_all(oracle, kernel3_cases(nfft))


FPW, FPW_SIZES = [1, 3, 16], [8, 32, 128, 256, 512, 1024]        # (512: spec_pack's G = 2 with a carried pivot)
FPW_LONG, FPW_LONG_SIZES = [3, 16], [4096, 8192, 16384, 32768]


@pytest.mark.parametrize('fpw', FPW)
@pytest.mark.parametrize('nfft', FPW_SIZES)
def test_nonstationary_spec_fpw(oracle, nfft, fpw):
    check_all(oracle, fpw_cases(nfft, fpw))


@pytest.mark.parametrize('fpw', FPW_LONG)
@pytest.mark.parametrize('nfft', FPW_LONG_SIZES)
def test_nonstationary_runs_of_long_windows(oracle, nfft, fpw):
    """spec_wgs.h carries its pivot only inside a run of frames, and small calls get runs of one frame: "spec_fpw"
    makes the runs (3: four of them in 12 frames; 16: one ragged run)."""
    check_all(oracle, fpw_cases(nfft, fpw))


def last_sample_cases(nfft):
    """'fall' with the event on the LAST sample of a frame (hop nfft: 'before' of frame 1; hop nfft/2: of frame 2),
    where the Hann weight is smallest and its absolute error shows: spec_chip.h's two-workgroup form and spec_chipx.h
    take the second half's window as one minus the first's."""
    return [dict(path='default', name='fall', nfft=nfft, hop=hop, S=S, slot='first', place='before', frame=nfft//hop,
                 options=(), want_db=False, frames=4, direct=False) for hop, S in ((nfft, 1e4), (nfft//2, 1e6))]


@pytest.mark.parametrize('nfft', [131072, 262144])
def test_nonstationary_last_sample_of_the_longest_windows(oracle, nfft):
    check_all(oracle, last_sample_cases(nfft))


NO_HALF = [256, 512, 1024, 2048]
GENERIC = [256, 4096, 16384]
DIRECT = [24, 1000]


@pytest.mark.parametrize('nfft', NO_HALF)
def test_nonstationary_spec_no_half(oracle, nfft):
    check_all(oracle, no_half_cases(nfft))


@pytest.mark.parametrize('nfft', GENERIC)
def test_nonstationary_force_generic_fft(oracle, nfft):
    check_all(oracle, generic_cases(nfft))


@pytest.mark.parametrize('nfft', DIRECT)
def test_nonstationary_direct_dft(oracle, nfft):
    check_all(oracle, direct_cases(nfft))


@pytest.mark.parametrize('plan', ['lowpass', 'bandpass'])
@pytest.mark.parametrize('nfft,hop', SHAPES)
def test_nonstationary_fused_sweep(oracle, nfft, hop, plan):
    """hipdsp_chain_forward's six windows behind a wide first-order low-pass (the step survives the filter) and behind
    a band-pass (the step becomes a transient).  The FFT waves of this launch carry no pivot: the IIR wave hands every
    frame's float64 mean over (psd_frame_mean), so these cases hold that hand-over and the transform to the bound; the
    fused sweep's one carried pivot is test_nonstationary_split_frames' business.  The oracle reads the filtered trace of the same launch, as in test_fused_sweep, so that the bound
    measures the transform alone -- which holds inside a segment of the sweep.  A frame that spans a segment border is
    transformed from the later segment's warm-up tiles, and those agree with the stored trace to the IIR warm-up's
    tolerance, which is relative to the INPUT: behind a band-pass that removes an offset of 1e6 levels that is 1e-5 of
    what is left (measured: rho 24 and 29 in the one frame on the border, 2048 / 512, S 1e6; 0.2 everywhere else and
    with one or two segments).  That is the IIR sweep's accuracy (tests/test_gpu_iir_accuracy.py), not the
    transform's, so the band-pass cases run in one segment; the low-pass cases, whose output is the size of their
    input, rotate the segmentation as test_fused_sweep does."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = gh.ctx()
    C, frames = 2, FUSED_FRAMES
    T = (frames - 1)*hop + nfft
    F = nfft//2 + 1
    sos = (butter_sos(1, 0.4*RATE, 'lowpass', RATE) if plan == 'lowpass'
           else butter_sos(1, (300.0, 9000.0), 'bandpass', RATE))
    esos = butter_sos(2, 20.0, 'lowpass', RATE)
    failed = []
    for case in fused_cases(nfft, hop, plan):
        # (silence behind a filter: a floor 180 dB down, not exact zeros -- spectral_bound.nonstationary has the reason)
        x = sb.nonstationary(case['name'], T, nfft, hop, RATE, seed=nfft + hop, S=case['S'], place=case['place'],
                             frame=case['frame'], floor=1e-9)
        with_db = case['want_db']
        fplan = hipdsp.SosPlan(c, sos)
        eplan = hipdsp.SosPlan(c, esos) if case['with_env'] else None
        nd = (T + hop - 1)//hop + 1
        dx = gh.to_planar(c, x)
        yf = hipdsp.DeviceArray(c, (C, T), np.float32)
        ps = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
        db = hipdsp.DeviceArray(c, (C, nd, F), np.float32) if with_db else None
        for arr in (ps, db) if with_db else (ps,):
            hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(arr), 0x7f, 4*C*nd*F)
        c.set_max_segments(case['max_segments'])
        try:
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, RATE, ps, nd, db_out=db)
            gf, gs = yf.to_host(), ps.to_host()
            gdb = db.to_host() if with_db else None
        finally:
            c.set_max_segments(0)
        want = np.zeros((nd, C, F))
        oracle.spectrogram_process(gf.T.astype(np.float64), want, RATE, nfft, hop)
        want = want.transpose(1, 0, 2)
        what = 'fused %d/%d %s family %s S %g event %s of frame %d (%s)%s%s' % (
            nfft, hop, plan, case['name'], case['S'], case['place'], case['frame'], case['slot'],
            ', envelope' if case['with_env'] else '', ' +dB' if with_db else '') + ', max_segments %d' % case['max_segments']
        try:
            rb = sb.assert_within(gs, want, nfft, what, db=gdb)
            note('ns fused %s %d/%d' % (plan, nfft, hop), nfft, rb)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '%d cases:\n%s' % (len(failed), '\n'.join(failed))


def split_cases():
    """'fall', 'rise' and 'staircase' at every S, and 'silence': the events on odd and even frames, every placement,
    the segmentation rotated against the families (the pivot starts anew in every segment, so one segment is the
    hard case)."""
    cases = []
    for j, S in enumerate(sb.STEPS):
        for m, name in enumerate(('fall', 'rise', 'staircase')):
            i = 3*j + m
            cases.append(dict(path='fused split frames', name=name, nfft=2048, hop=1024, S=S, slot=EVENT_SLOTS[i % 4],
                              place=sb.PLACES[i % 3], frame=(9, 30, 12, 37, 22, 51, 16, 45, 64)[i], want_db=False,
                              max_segments=(0, 37, 1)[(j + m) % 3]))
    cases.append(dict(path='fused split frames', name='silence', nfft=2048, hop=1024, S=1.0, slot='later',
                      place='border', frame=21, want_db=False, max_segments=0))
    return cases


def test_nonstationary_split_frames(oracle):
    """"chain_split_frames": hipdsp_chain_forward leaves the odd frames of 2048 / 1024 to hipdsp_chain_backward, whose
    FFT waves walk the filtered trace BACKWARDS and take frame 2t + 1's pivot from frame 2t + 3 (psd_frame_pivot): two
    hops away, no overlap -- the stalest pivot in the project, and a 'rise' in time is its fall.  Behind the wide
    low-pass the steps survive the filter; the oracle reads the filtered trace of the same launches."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = gh.ctx()
    nfft, hop, C, frames = 2048, 1024, 2, FUSED_FRAMES
    T = (frames - 1)*hop + nfft
    F = nfft//2 + 1
    nd = frames + 1
    fplan = hipdsp.SosPlan(c, butter_sos(1, 0.4*RATE, 'lowpass', RATE))
    eplan = hipdsp.SosPlan(c, butter_sos(2, 20.0, 'lowpass', RATE))
    failed = []
    for case in split_cases():
        x = sb.nonstationary(case['name'], T, nfft, hop, RATE, seed=nfft + hop, S=case['S'], place=case['place'],
                             frame=case['frame'], floor=1e-9)
        c.set_max_segments(case['max_segments'])
        c.set_option('chain_split_frames', 1)
        try:
            dx = gh.to_planar(c, x)
            yf = hipdsp.DeviceArray(c, (C, T), np.float32)
            ye = hipdsp.DeviceArray(c, (C, T), np.float32)
            ps = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
            hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(ps), 0x7f, 4*C*nd*F)
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, RATE, ps, nd)
            hipdsp.chain_backward(c, eplan, yf, T, ye, T, C, T, nfft, hop, RATE, ps, nd, clamp=False)
            gf, gs = yf.to_host(), ps.to_host()
        finally:
            c.set_option('chain_split_frames', 0)
            c.set_max_segments(0)
        want = np.zeros((nd, C, F))
        oracle.spectrogram_process(gf.T.astype(np.float64), want, RATE, nfft, hop)
        want = want.transpose(1, 0, 2)
        what = 'fused split frames 2048/1024 family %s S %g event %s of frame %d, max_segments %d' % (
            case['name'], case['S'], case['place'], case['frame'], case['max_segments'])
        try:
            assert np.all(gs[:, frames] == 0), (what, 'zero tail')
            rb = sb.assert_within(gs, want, nfft, what)
            note('ns fused split frames', nfft, rb)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '%d cases:\n%s' % (len(failed), '\n'.join(failed))


def all_ns_cases():
    cases = []
    for nfft in POW2:
        cases += default_cases(nfft) + kernel2_cases(nfft)
    for nfft in KERNEL3:
        cases += kernel3_cases(nfft)
    for nfft in (131072, 262144):
        cases += last_sample_cases(nfft)
    for fpw, sizes in ((FPW, FPW_SIZES), (FPW_LONG, FPW_LONG_SIZES)):
        for nfft in sizes:
            for f in fpw:
                cases += fpw_cases(nfft, f)
    for nfft in NO_HALF:
        cases += no_half_cases(nfft)
    for nfft in GENERIC:
        cases += generic_cases(nfft)
    for nfft in DIRECT:
        cases += direct_cases(nfft)
    for nfft, hop in SHAPES:
        for plan in ('lowpass', 'bandpass'):
            cases += fused_cases(nfft, hop, plan)
    return cases + split_cases()


def test_the_nonstationary_cases_cover_the_lists():
    """Every family, every S, every placement of the event and every slot in a run appears; every path sees 'fall'
    at all three S and 'silence'; every hop kind appears on every spectrogram path; the dB image on half the cases."""
    cases = all_ns_cases()
    assert {c['name'] for c in cases} == set(sb.NONSTATIONARY)
    assert {c['place'] for c in cases} == set(sb.PLACES)
    assert {c['slot'] for c in cases} == set(EVENT_SLOTS)
    paths = {c['path'] for c in cases}
    assert paths == {'default', 'spec_kernel=2', 'spec_kernel=3', 'spec_fpw=1', 'spec_fpw=3', 'spec_fpw=16',
                     'spec_no_half', 'force_generic_fft', 'direct', 'fused lowpass', 'fused bandpass',
                     'fused split frames'}
    for p in sorted(paths):
        mine = [c for c in cases if c['path'] == p]
        assert {('fall', S) for S in sb.STEPS} <= {(c['name'], c['S']) for c in mine}, p
        assert any(c['name'] == 'silence' for c in mine), p
        assert {c['place'] for c in mine} == set(sb.PLACES), p
        assert len({c['frame'] for c in mine}) >= 3, p
        n_db = sum(c['want_db'] for c in mine)
        assert len(mine) <= 3*n_db <= 2*len(mine) or p == 'fused split frames', (p, n_db, len(mine))   # (no dB there)
        if not p.startswith('fused'):
            kinds = {('nfft' if c['hop'] == c['nfft'] else 'half' if 2*c['hop'] == c['nfft'] else
                      'quarter' if 4*c['hop'] == c['nfft'] else 'odd') for c in mine}
            assert kinds == {'nfft', 'half', 'quarter', 'odd'}, (p, kinds)
    for c in cases:                                          # the event and a frame behind it lie inside the trace
        assert 1 <= c['frame'] <= c.get('frames', FUSED_FRAMES) - 2, c


def test_zz_worst_per_path():
    """The worst rho and beta of every path measured above (run with -s to see the table)."""
    if not WORST:
        print('\n(no path measured in this session)')
        return
    lines = ['%-22s %7s %8s %8s %8s' % ('path', 'nfft', 'rho', 'beta', 'beta max')]
    for (path, nfft), (rho, beta) in sorted(WORST.items()):
        lines.append('%-22s %7d %8.3f %8.2f %8.0f' % (path, nfft, rho, beta, sb.beta_max(nfft)))
    print('\n' + '\n'.join(lines))
