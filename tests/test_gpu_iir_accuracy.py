"""Local accuracy of the IIR sweeps: hipdsp_sosfilt, hipdsp_envelope, hipdsp_sosfilt_envelope, hipdsp_chain_forward
+ the backward sweep and the frame-split pair, every 64-sample window against a longdouble restatement of scipy's
sosfilt / sosfiltfilt under the bound of tests/iir_bound.py (calibrated on the CPU by tests/test_iir_bound.py:
e_w <= (1 + 16 q) 2^-24 r_w, q the case's own float64 error, at most 2^-6).  The signal families put a quiet stretch
behind a loud one, a step up, an offset, a burst and 5000 exact zeros in front of the kernels; they ride as the
channels of one call of 16 tiles + 5 samples, cut into one segment, three, the planner's choice and one-tile
segments; every output buffer is filled with a sentinel first.  The band-pass output is judged against the reference
of x, an envelope against the reference of the launch's own float32 band-pass output (the contract).  The clamp is
judged apart from the arithmetic: the clamped result must be the clamp of the unclamped one bit for bit
(iir_bound.envelope_case says why).  Two float32 roundings the reference does not have sit in tile loops and are held to
derived terms on top of the bound, on the paths they reach only: the odd extension of an envelope with a high-pass
(iir_bound.extension_term), and the forward pass handed to the backward pass in the float32 tile by the three- and
four-section envelope sweeps and by the frame-split backward sweep (iir_bound.between_term).

hipdsp_envelope_multi (cascades of more than four sections, run plan by plan) is held to the same bound: its 2P - 1
float32 hand-overs between the P plans take iir_bound.handover_term, both of its float32 extensions extension_term
where the cascade has a high-pass; 8 tiles + 5 samples, the smallest size at which the four segmentations of the
extended trace differ.  Its section also covers what only that call has: pitches with slack and odd base offsets, a
gain other than pi/2, y == x and y over the tail of x (the header's "x and y may overlap"), non-finite samples in one
lane, the pad length's edge and the limit of 16 plans.

Warm-ups that start inside the trace (iir_bound.T_WARM: 64 and 48 tiles + 5 samples, longer than the 26- and 15-tile
warm-ups of the 20 Hz low-pass and the 100 Hz high-pass): hipdsp_sosfilt, hipdsp_envelope and the fused launches in three
segments, the planner's and one-tile segments, each run after asserting that its segmentation does start segments from
zero state in mid-trace, on the far side of a loud passage.

A failure names the path, the filter, the segmentation, the lane (family) and the window; test_zz_worst_per_path
prints the worst ratio e_w / (2^-24 r_w) of every path measured (run with -s).
"""

import contextlib

import numpy as np
import pytest

import gpu_helpers as gh
import iir_bound as ib

pytestmark = pytest.mark.gpu

SEGMENTATIONS = (('one segment', (('max_segments', 1),)),
                 ('three segments', (('max_segments', 3),)),
                 ('the planner\'s segments', ()),
                 ('one-tile segments', (('n_cus', 1024), ('sos_waves_per_cu', 16), ('sos_waves_min', 16))))
DEFAULTS = (('max_segments', 0), ('n_cus', 256), ('sos_waves_per_cu', 0), ('sos_waves_min', 0), ('sos_prefetch', 1),
            ('chain_split_frames', 0))
WORST = {}


def note(path, worst):
    WORST[path] = max(WORST.get(path, 0.0), worst)


@contextlib.contextmanager
def options(c, opts):
    try:
        for k, v in opts:
            c.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS:
            c.set_option(k, v)


def fresh(c, C, n):
    """A (C, n) float32 device array filled with a sentinel (3.4e38): every sample must be written."""
    from audian_amd import hipdsp
    a = hipdsp.DeviceArray(c, (C, n), np.float32)
    hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(a), 0x7f, 4*C*n)
    return a


def capped(q, what):
    assert np.all(q <= ib.Q_CAP), '%s: q %s above the cap on the case list' % (what, q)
    return q


def bandpass(case):
    sos, rate, fams = ib.design(ib.GENERAL if case == 'general' else case)
    return (ib.spread(sos) if case == 'general' else sos), rate, fams


# ---- hipdsp_sosfilt ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', list(ib.BANDPASSES) + ['general'])
def test_sosfilt(case):
    """One to four sections, unit and general numerators, in every segmentation; exact zeros in front of the onset."""
    from audian_amd import hipdsp
    sos, rate, fams = bandpass(case)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, case)
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    for seg, opts in SEGMENTATIONS:
        with options(c, opts):
            dy = fresh(c, C, T)
            hipdsp.sosfilt(c, plan, dx, T, dy, T, C, T, 0)
            got = dy.to_host().T
        what = 'hipdsp_sosfilt, %s, %s' % (case, seg)
        if 'onset' in fams:
            assert np.all(got[:ib.ONSET, fams.index('onset')] == 0), what + ': not zero in front of the onset'
        note('hipdsp_sosfilt', ib.assert_within(got, ref, q, what))


@pytest.mark.parametrize('case', ib.SKIP_BANDPASSES)
def test_sosfilt_skip(case):
    from audian_amd import hipdsp
    sos, rate, fams = bandpass(case)
    T, C = ib.T_SKIP, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, case)
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    for skip in ib.SKIPS:
        for seg, opts in SEGMENTATIONS:
            with options(c, opts):
                dy = fresh(c, C, T - skip)
                hipdsp.sosfilt(c, plan, dx, T, dy, T - skip, C, T, skip)
                got = dy.to_host().T
            what = 'hipdsp_sosfilt, %s, skip %d, %s' % (case, skip, seg)
            note('hipdsp_sosfilt, skip', ib.assert_within(got, ref[skip:], q, what, first=skip))


# ---- hipdsp_envelope ---------------------------------------------------------------------------------------------

def run_envelope(c, plan, dx, T, C, skip=0, rectify=True, clamp=False):
    from audian_amd import hipdsp
    dy = fresh(c, C, T - skip)
    hipdsp.envelope(c, plan, dx, T, dy, T - skip, C, T, skip, rectify=rectify, clamp=clamp)
    return dy.to_host().T


@pytest.mark.parametrize('case', list(ib.ENVELOPES))
def test_envelope(case):
    """One to four sections, with and without a high-pass, with and without the register prefetch, clamp off and on,
    in every segmentation; once without the rectifier (the playback low-pass)."""
    from audian_amd import hipdsp
    sos, rate, fams = ib.design(case, ib.ENVELOPES)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    term = ib.extension_term(sos, x) if ib.has_highpass(sos) else None
    if len(sos) > 2:                                  # the forward pass goes through the float32 tile (env_bwd_kernel, REGW false)
        term = ib.between_term(sos, x) + (0.0 if term is None else term)
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    for seg, opts in SEGMENTATIONS:
        for prefetch in (1, 0):
            with options(c, opts + (('sos_prefetch', prefetch),)):
                got = run_envelope(c, plan, dx, T, C)
                clamped = run_envelope(c, plan, dx, T, C, clamp=True)
            what = 'hipdsp_envelope, %s, %s, sos_prefetch %d' % (case, seg, prefetch)
            note('hipdsp_envelope, %d section%s%s' % (len(sos), 's'[:len(sos) > 1], ', high-pass' if ib.has_highpass(sos) else ''),
                 ib.assert_within(got, ref, q, what, term=term))
            assert np.array_equal(clamped, ib.clamped(got)), what + ': the clamped run is not the clamp of the unclamped one'
    if case == ib.PLAYBACK:
        ref, q = ib.envelope_case(sos, x, rectify=False)
        capped(q, case + ', rectify 0')
        for seg, opts in SEGMENTATIONS:
            with options(c, opts):
                got = run_envelope(c, plan, dx, T, C, rectify=False)
            note('hipdsp_envelope, rectify 0', ib.assert_within(got, ref, q, 'hipdsp_envelope, rectify 0, %s, %s' % (case, seg)))


@pytest.mark.parametrize('case', ib.SKIP_ENVELOPES)
def test_envelope_skip(case):
    from audian_amd import hipdsp
    sos, rate, fams = ib.design(case, ib.ENVELOPES)
    T, C = ib.T_SKIP, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    term = ib.extension_term(sos, x) if ib.has_highpass(sos) else None
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    for skip in ib.SKIPS:
        for seg, opts in SEGMENTATIONS:
            with options(c, opts):
                got = run_envelope(c, plan, dx, T, C, skip=skip)
            what = 'hipdsp_envelope, %s, skip %d, %s' % (case, skip, seg)
            note('hipdsp_envelope, skip' + (', high-pass' if term is not None else ''),
                 ib.assert_within(got, ref[skip:], q, what, first=skip, term=None if term is None else term[skip:]))


# ---- the fused launches ------------------------------------------------------------------------------------------

def judge_envelopes(path, esos, runs, env_first, what, between=False):
    """runs: [(label, yf (T, lanes) float32 as the launch wrote it, env (T - env_first, lanes))]: every envelope against
    the reference of its own yf[env_first:], all of them lanes of ONE reference run.  between: the sweep hands its
    forward pass over in the float32 tile (iir_bound.between_term)."""
    yfs = np.concatenate([yf[env_first:] for _, yf, _ in runs], axis=1)
    envs = np.concatenate([env for _, _, env in runs], axis=1)
    ref, q = ib.envelope_case(esos, yfs)
    capped(q, what)
    term = ib.extension_term(esos, yfs, left=env_first > 0) if ib.has_highpass(esos) else None
    if between:
        term = ib.between_term(esos, yfs) + (0.0 if term is None else term)
    lanes = runs[0][1].shape[1]
    for i, (label, _, _) in enumerate(runs):
        sl = slice(i*lanes, (i + 1)*lanes)
        note(path, ib.assert_within(envs[:, sl], ref[:, sl], q[sl], '%s, %s, envelope from %d' % (what, label, env_first),
                                    first=env_first, term=None if term is None else term[:, sl]))


@pytest.mark.parametrize('bp,env', ib.SOSFILT_ENVELOPE)
def test_sosfilt_envelope(bp, env):
    """Phase 0 and phase 1 followed by phase 2, the envelope from sample 0 and from inside the trace, in every
    segmentation."""
    from audian_amd import hipdsp
    sos, rate, fams = bandpass(bp)
    esos, _, efams = ib.design(env, ib.ENVELOPES)
    lanes = ib.envelope_lanes(fams, efams)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan, eplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos), hipdsp.SosPlan(c, esos)
    for env_first in ib.ENV_FIRST:
        runs = []
        for seg, opts in SEGMENTATIONS:
            for phases in ((0,), (1, 2)):
                with options(c, opts):
                    yf, ye = fresh(c, C, T), fresh(c, C, T - env_first)
                    for phase in phases:
                        hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T - env_first, C, T, clamp=False, phase=phase,
                                                env_first=env_first)
                    gf, ge = yf.to_host().T, ye.to_host().T
                    if phases == (0,):
                        yc = fresh(c, C, T - env_first)
                        hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, yc, T - env_first, C, T, clamp=True,
                                                env_first=env_first)
                        assert np.array_equal(yc.to_host().T, ib.clamped(ge)), (bp, env, seg, 'clamp')
                label = '%s, phase %s' % (seg, '+'.join(str(p) for p in phases))
                note('hipdsp_sosfilt_envelope, band-pass', ib.assert_within(gf, ref, q, 'hipdsp_sosfilt_envelope, %s, %s' % (bp, label)))
                runs.append((label, gf[:, lanes], ge[:, lanes]))
        judge_envelopes('hipdsp_sosfilt_envelope, envelope' + (', high-pass' if ib.has_highpass(esos) else ''), esos, runs,
                        env_first, 'hipdsp_sosfilt_envelope, %s + %s' % (bp, env))


def run_chain(c, fplan, eplan, dx, T, C, nfft, hop, rate, spec_first=0, env_first=0):
    """hipdsp_chain_forward, then the backward sweep: (yf (T, C), env (T - env_first, C) or None)."""
    from audian_amd import hipdsp
    nd = (T - spec_first + hop - 1)//hop
    yf = fresh(c, C, T)
    ps = hipdsp.DeviceArray(c, (C, nd, nfft//2 + 1), np.float32)
    hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, rate, ps, nd, spec_first=spec_first,
                         env_first=env_first)
    if eplan is None:
        return yf.to_host().T, None
    ye = fresh(c, C, T - env_first)
    hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T - env_first, C, T, clamp=False, phase=2, env_first=env_first)
    return yf.to_host().T, ye.to_host().T


@pytest.mark.parametrize('nfft,hop', list(ib.CHAIN))
def test_chain_forward(nfft, hop):
    """The fused forward sweep + phase 2 for all six windows (yf and the envelope; the spectrogram has its own suite);
    at 2048/1024 in every segmentation, on the shifted grid (spec_first, env_first > 0) and without an envelope plan."""
    from audian_amd import hipdsp
    bp, env = ib.CHAIN[nfft, hop]
    sos, rate, fams = bandpass(bp)
    esos, _, efams = ib.design(env, ib.ENVELOPES)
    lanes = ib.envelope_lanes(fams, efams)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan, eplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos), hipdsp.SosPlan(c, esos)
    full = (nfft, hop) == (2048, 1024)
    path = 'hipdsp_chain_forward %d/%d' % (nfft, hop)
    runs = []
    for seg, opts in SEGMENTATIONS if full else SEGMENTATIONS[2:3]:
        with options(c, opts):
            gf, ge = run_chain(c, fplan, eplan, dx, T, C, nfft, hop, rate)
        note(path + ', band-pass', ib.assert_within(gf, ref, q, '%s, %s, %s' % (path, bp, seg)))
        runs.append((seg, gf[:, lanes], ge[:, lanes]))
    judge_envelopes(path + ', envelope', esos, runs, 0, '%s, %s + %s' % (path, bp, env))
    if full:
        spec_first, env_first = 777, ib.ENV_FIRST[1]
        runs = []
        for seg, opts in (SEGMENTATIONS[0], SEGMENTATIONS[3]):
            with options(c, opts):
                gf, ge = run_chain(c, fplan, eplan, dx, T, C, nfft, hop, rate, spec_first, env_first)
            note(path + ', band-pass', ib.assert_within(gf, ref, q, '%s shifted, %s, %s' % (path, bp, seg)))
            runs.append((seg + ', shifted grid', gf[:, lanes], ge[:, lanes]))
        judge_envelopes(path + ', envelope', esos, runs, env_first, '%s, %s + %s' % (path, bp, env))
        for seg, opts in SEGMENTATIONS:
            with options(c, opts):
                gf, _ = run_chain(c, fplan, None, dx, T, C, nfft, hop, rate)
            note(path + ', band-pass', ib.assert_within(gf, ref, q, '%s without an envelope plan, %s, %s' % (path, bp, seg)))


@pytest.mark.parametrize('bp,env', ib.SPLIT_FRAMES)
def test_chain_split_frames(bp, env):
    """"chain_split_frames": hipdsp_chain_forward + hipdsp_chain_backward at 2048/1024, envelopes of one and two sections."""
    from audian_amd import hipdsp
    nfft, hop = 2048, 1024
    sos, rate, fams = bandpass(bp)
    esos, _, efams = ib.design(env, ib.ENVELOPES)
    lanes = ib.envelope_lanes(fams, efams)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan, eplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos), hipdsp.SosPlan(c, esos)
    nd = (T + hop - 1)//hop + 1
    runs = []
    for seg, opts in SEGMENTATIONS:
        with options(c, opts + (('chain_split_frames', 1),)):
            yf, ye = fresh(c, C, T), fresh(c, C, T)
            ps = hipdsp.DeviceArray(c, (C, nd, nfft//2 + 1), np.float32)
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, rate, ps, nd)
            hipdsp.chain_backward(c, eplan, yf, T, ye, T, C, T, nfft, hop, rate, ps, nd, clamp=False)
            gf, ge = yf.to_host().T, ye.to_host().T
        note('chain_split_frames, band-pass', ib.assert_within(gf, ref, q, 'chain_split_frames, %s, %s' % (bp, seg)))
        runs.append((seg, gf[:, lanes], ge[:, lanes]))
    judge_envelopes('chain_split_frames, envelope', esos, runs, 0, 'chain_split_frames, %s + %s' % (bp, env), between=True)


# ---- warm-ups that start inside the trace -----------------------------------------------------------------------------
# At T_LONG every warm-up of the slow filters is clipped at the start of the trace.  Here a segment starts from zero state
# in mid-trace, and a condition on the segmentation that actually runs keeps it so: a test whose planner one day picks a
# single segment fails instead of passing without testing.

WARM_SEGMENTATIONS = SEGMENTATIONS[1:]                   # (one segment has no warm-up)
# forward segments of two to five tiles are where env_fix_kernel once multiplied (A^TILE)^segment out in float64 and lost
# the states behind a loud passage (3e-7, 25 to 35 roundings of the envelope on `stepdown`); of 65 tiles these are 2, 3, 4, 5
SHORT_SEGMENTATIONS = tuple(('at most %d segments' % n, (('max_segments', n),)) for n in (33, 22, 17, 13))
FORWARD_ALONE, FORWARD_FUSED, BACKWARD = -1, -2, 4       # the planner's cost tables (csrc/sos_plan.hip: tile_step_cost)


def planned(opts, model, n_tiles, channels, warm, w_cap=16):
    """Segment length in tiles of a single-wave sweep under the context options `opts` (csrc/sos_device.h:
    plan_segments), through hipdsp_sos_segments_host."""
    import ctypes
    from audian_amd import _lib
    o = dict(DEFAULTS)
    o.update(dict(opts))
    w_max = min(o['sos_waves_per_cu'] or 16, w_cap)
    length, count = ctypes.c_int64(), ctypes.c_int()
    _lib.check(_lib.lib.hipdsp_sos_segments_host(o['n_cus'], w_max, 0 if o['sos_waves_min'] >= w_max else model, o['max_segments'],
                                                 n_tiles*ib.TILE, channels, warm, ctypes.byref(length), ctypes.byref(count)))
    assert length.value % ib.TILE == 0 and count.value == -(-n_tiles//(length.value//ib.TILE))
    return int(length.value)//ib.TILE


def forward_condition(seg_tiles, T, warm, what, need=2):
    """At least `need` segments start from zero state at least one tile inside the trace, one of them behind the loud
    quarter of `stepdown`."""
    assert warm % ib.TILE == 0
    cut = ib.cut_warmups(-(-T//ib.TILE), seg_tiles, warm//ib.TILE)
    assert len(cut) >= need, '%s: %d-tile segments, warm-up %d tiles: %d warm-ups start inside the trace' % (
        what, seg_tiles, warm//ib.TILE, len(cut))
    assert any(t*ib.TILE >= T//4 for t, _ in cut), what + ': no such segment behind the loud quarter of stepdown'


def backward_condition(seg_tiles, n_tiles, T, warm, what, need=2):
    """The same for a backward sweep, whose tiles count from the end of the extended trace: a segment that starts at
    reversed tile t runs downwards from sample (n_tiles - t) 2048, its warm-up from (n_tiles - t + warm) 2048; one of
    them starts in front of the loud half of `stepup`."""
    assert warm % ib.TILE == 0
    cut = ib.cut_warmups(n_tiles, seg_tiles, warm//ib.TILE)
    assert len(cut) >= need, '%s: %d-tile segments, warm-up %d tiles: %d warm-ups start inside the trace' % (
        what, seg_tiles, warm//ib.TILE, len(cut))
    assert any((n_tiles - t)*ib.TILE <= T//2 for t, _ in cut), what + ': no such segment in front of the loud half of stepup'


def backward_need(seg):
    """Three segments of the 65 tiles are 22 tiles each: only the third one (from reversed tile 44, its warm-up from
    tile 18) fits a 26-tile warm-up in front of it.  Every other segmentation has at least two."""
    return 1 if seg == 'three segments' else 2


def warm_opts(opts, more=()):
    return (('n_cus', 256),) + opts + more


def test_warmup_sosfilt():
    """hipdsp_sosfilt, hp3 100 Hz @ 192 kHz (warm-up 15 tiles) over 48 tiles + 5: in three segments of 17 tiles the second
    and the third start from zero state at tiles 2 and 19."""
    from audian_amd import hipdsp
    case = ib.WARM_BANDPASS
    sos, rate, _ = bandpass(case)
    fams = ib.WARM_FAMILIES
    T, C = ib.T_WARM[case], len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, case)
    ib.assert_in_range(ref, case)
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    warm = plan.info()[0]
    assert warm == ib.WARM_TILES[case]*ib.TILE
    for seg, opts in WARM_SEGMENTATIONS:
        what = 'hipdsp_sosfilt, %s, %d frames, %s' % (case, T, seg)
        forward_condition(planned(warm_opts(opts), FORWARD_ALONE, -(-T//ib.TILE), C, warm), T, warm, what)
        with options(c, warm_opts(opts)):
            dy = fresh(c, C, T)
            hipdsp.sosfilt(c, plan, dx, T, dy, T, C, T, 0)
            got = dy.to_host().T
        note('hipdsp_sosfilt, warm-ups inside the trace', ib.assert_within(got, ref, q, what))


def test_warmup_envelope():
    """hipdsp_envelope, lp2 20 Hz @ 96 kHz (warm-up 26 tiles) over 64 tiles + 5, with and without the register prefetch:
    the backward sweep's segments start from zero state with the future cut off, and the forward sweep hands its states
    over sums of up to 27 segments (env_fix_kernel); once more in segments of 2, 3, 4 and 5 tiles."""
    from audian_amd import hipdsp
    case = ib.WARM_ENVELOPE
    sos, rate, _ = ib.design(case, ib.ENVELOPES)
    fams = ib.WARM_FAMILIES
    T, C = ib.T_WARM[case], len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    ib.assert_in_range(ref, case)
    c = gh.ctx()
    dx, plan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    warm, edge = plan.info()
    assert warm == ib.WARM_TILES[case]*ib.TILE and edge == ib.padlen(sos)
    n_tiles = -(-(T + edge)//ib.TILE)
    assert [planned(warm_opts(opts), FORWARD_FUSED, n_tiles, C, 0) for _, opts in SHORT_SEGMENTATIONS] == [2, 3, 4, 5]
    for seg, opts in WARM_SEGMENTATIONS + SHORT_SEGMENTATIONS:
        for prefetch in (1, 0) if (seg, opts) in WARM_SEGMENTATIONS else (1,):
            what = 'hipdsp_envelope, %s, %d frames, %s, sos_prefetch %d' % (case, T, seg, prefetch)
            backward_condition(planned(warm_opts(opts), BACKWARD, n_tiles, C, warm, 8), n_tiles, T, warm, what, backward_need(seg))
            with options(c, warm_opts(opts, (('sos_prefetch', prefetch),))):
                got = run_envelope(c, plan, dx, T, C)
            note('hipdsp_envelope, warm-ups inside the trace', ib.assert_within(got, ref, q, what))


@pytest.mark.parametrize('shifted', [False, True], ids=['from sample 0', 'shifted grid'])
def test_warmup_fused(shifted):
    """bp2 300-3000 Hz in front of the 20 Hz envelope over 64 tiles + 5 through hipdsp_sosfilt_envelope (phase 0, phases 1
    + 2) and hipdsp_chain_forward 2048/1024 + phase 2: the band-pass's short warm-ups and the envelope's exact hand-over
    forward, the envelope's 26-tile warm-ups backward.  Once more on the shifted grid (spec_first 777, env_first
    ENV_FIRST[1]) in one-tile segments.  Every envelope against the reference of its own launch's float32 band-pass
    output, all of them lanes of one reference run."""
    from audian_amd import hipdsp
    bp, env = ib.WARM_FUSED, ib.WARM_ENVELOPE
    nfft, hop = 2048, 1024
    sos, rate, _ = bandpass(bp)
    esos = ib.design(env, ib.ENVELOPES)[0]
    fams = ib.WARM_FAMILIES
    T, C = ib.T_WARM[env], len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan, eplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos), hipdsp.SosPlan(c, esos)
    warm_f, (warm_e, edge) = fplan.info()[0], eplan.info()
    assert warm_e == ib.WARM_TILES[env]*ib.TILE
    spec_first, env_first = (777, ib.ENV_FIRST[1]) if shifted else (0, 0)
    n_tiles = -(-(T + edge)//ib.TILE) if not shifted else (T - env_first + edge)//ib.TILE     # (shifted: a lower bound)
    runs = []
    for seg, opts in WARM_SEGMENTATIONS[2:] if shifted else WARM_SEGMENTATIONS:
        o = warm_opts(opts)
        what = '%s + %s, %d frames, %s%s' % (bp, env, T, seg, ', shifted grid' if shifted else '')
        forward_condition(planned(o, FORWARD_FUSED, -(-T//ib.TILE), C, warm_f), T, warm_f, 'hipdsp_sosfilt_envelope, ' + what)
        backward_condition(planned(o, BACKWARD, n_tiles, C, warm_e, 8), n_tiles, T - env_first, warm_e, what, backward_need(seg))
        for phases in ((0,), (1, 2)):
            with options(c, o):
                yf, ye = fresh(c, C, T), fresh(c, C, T - env_first)
                for phase in phases:
                    hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T - env_first, C, T, clamp=False, phase=phase,
                                            env_first=env_first)
                gf, ge = yf.to_host().T, ye.to_host().T
            label = 'hipdsp_sosfilt_envelope, %s, phase %s' % (seg, '+'.join(str(p) for p in phases))
            note('hipdsp_sosfilt_envelope, warm-ups inside the trace, band-pass', ib.assert_within(gf, ref, q, label + ', ' + what))
            runs.append((label, gf, ge))
        with options(c, o):
            seg_frames, n_seg = hipdsp.chain_plan(c, fplan, eplan, C, T)
            assert seg_frames % ib.TILE == 0 and n_seg >= 2
            forward_condition(seg_frames//ib.TILE, T, warm_f, 'hipdsp_chain_forward, ' + what)
            gf, ge = run_chain(c, fplan, eplan, dx, T, C, nfft, hop, rate, spec_first, env_first)
        label = 'hipdsp_chain_forward %d/%d + phase 2, %s' % (nfft, hop, seg)
        note('hipdsp_chain_forward 2048/1024, warm-ups inside the trace, band-pass', ib.assert_within(gf, ref, q, label + ', ' + what))
        runs.append((label, gf, ge))
    judge_envelopes('fused launches, warm-ups inside the trace, envelope', esos, runs, env_first, '%s + %s, %d frames' % (bp, env, T))


# ---- hipdsp_envelope_multi ---------------------------------------------------------------------------------------

MULTI_SPLITS = [(case, split) for case in ib.MULTI for split in ib.MULTI[case][5]]


def splitname(split):
    return '+'.join(str(n) for n in split)


def multi_plans(c, sos, split):
    from audian_amd import hipdsp
    return [hipdsp.SosPlan(c, sos[part]) for part in ib.plan_slices(sos, split)]


def run_multi(c, plans, dx, T, C, skip=0, rectify=True, gain=ib.GAIN, clamp=False):
    from audian_amd import hipdsp
    dy = fresh(c, C, T - skip)
    hipdsp.envelope_multi(c, plans, dx, T, dy, T - skip, C, T, skip, rectify=rectify, gain=gain, clamp=clamp)
    return dy.to_host().T


def judge_multi(path, got, ref, q, what, term, first=0):
    """assert_within, and next to the worst ratio beyond the term (0 where the term alone covers the error) the share of
    the whole allowance that the run uses."""
    note(path, ib.assert_within(got, ref, q, what, first=first, term=term))
    note(path + ': share of the allowance', float(np.max(ib.allowance_share(got, ref, q, term, first))))


def multi_setup(case, T=ib.T_MULTI):
    sos, rate, fams, splits = ib.multi_design(case)
    x = ib.families(fams, T, rate)
    c = gh.ctx()
    return sos, fams, x, c, gh.to_planar(c, x)


@pytest.mark.parametrize('case,split', MULTI_SPLITS, ids=['%s as %s' % (case, splitname(split)) for case, split in MULTI_SPLITS])
def test_envelope_multi(case, split):
    """Every cascade and split in every segmentation, clamp off under the bound and its terms, clamp on bit for bit the
    clamp of that."""
    sos, fams, x, c, dx = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    term = ib.multi_term(sos, split, x)
    plans = multi_plans(c, sos, split)
    for seg, opts in SEGMENTATIONS:
        with options(c, opts):
            got = run_multi(c, plans, dx, T, C)
            clamped = run_multi(c, plans, dx, T, C, clamp=True)
        what = 'hipdsp_envelope_multi, %s as %s, %s' % (case, splitname(split), seg)
        judge_multi('hipdsp_envelope_multi, %s as %s' % (case.split(' @')[0], splitname(split)), got, ref, q, what, term)
        assert np.array_equal(clamped, ib.clamped(got)), what + ': the clamped run is not the clamp of the unclamped one'


@pytest.mark.parametrize('case', ib.MULTI_SKIP)
def test_envelope_multi_skip(case):
    """`skip` up to, at and behind a tile border; the windows stay on the grid of sample 0."""
    sos, fams, x, c, dx = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    split = ib.MULTI[case][5][0]
    term = ib.multi_term(sos, split, x)
    plans = multi_plans(c, sos, split)
    for skip in ib.SKIPS:
        for seg, opts in SEGMENTATIONS:
            with options(c, opts):
                got = run_multi(c, plans, dx, T, C, skip=skip)
            what = 'hipdsp_envelope_multi, %s as %s, skip %d, %s' % (case, splitname(split), skip, seg)
            judge_multi('hipdsp_envelope_multi, skip', got, ref[skip:], q, what, term[skip:], first=skip)


@pytest.mark.parametrize('case', ib.MULTI_SKIP)
def test_envelope_multi_pitches(case):
    """Rows with slack on both sides and odd base offsets (4-byte alignment only): NaN in the slack of x must not be
    read, the sentinel in the slack of y must stay."""
    from audian_amd import hipdsp
    sos, fams, x, c, _ = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x)
    split = ib.MULTI[case][5][0]
    term = ib.multi_term(sos, split, x)
    plans = multi_plans(c, sos, split)
    x_off, x_pitch, y_off = 3, T + 13, 5
    host = np.full(x_off + C*x_pitch, np.nan, np.float32)
    for ch in range(C):
        host[x_off + ch*x_pitch:x_off + ch*x_pitch + T] = x[:, ch]
    bx = hipdsp.DeviceArray.from_host(c, host)
    dx = bx.view(x_off, (C*x_pitch,))
    for skip in (0, 2047):
        y_pitch = T - skip + 11
        by = fresh(c, 1, y_off + C*y_pitch + 7)
        sentinel = by.to_host()[0, 0]
        dy = by.view(y_off, (C*y_pitch,))
        hipdsp.envelope_multi(c, plans, dx, x_pitch, dy, y_pitch, C, T, skip, clamp=False)
        raw = by.to_host()[0]
        rows = raw[y_off:y_off + C*y_pitch].reshape(C, y_pitch)
        what = 'hipdsp_envelope_multi, %s as %s, pitches %d / %d, skip %d' % (case, splitname(split), x_pitch, y_pitch, skip)
        judge_multi('hipdsp_envelope_multi, pitches', rows[:, :T - skip].T, ref[skip:], q, what, term[skip:], first=skip)
        slack = np.concatenate([raw[:y_off], rows[:, T - skip:].ravel(), raw[y_off + C*y_pitch:]])
        assert np.all(slack.view(np.uint32) == sentinel.view(np.uint32)), what + ': written outside the rows'
    assert np.array_equal(bx.to_host(), host, equal_nan=True)


def test_envelope_multi_without_the_rectifier():
    case = ib.MULTI_PLAIN
    sos, fams, x, c, dx = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x, rectify=False)
    capped(q, case + ', rectify 0')
    split = ib.MULTI[case][5][0]
    term = ib.multi_term(sos, split, x, rectify=False)
    plans = multi_plans(c, sos, split)
    for seg, opts in SEGMENTATIONS:
        with options(c, opts):
            got = run_multi(c, plans, dx, T, C, rectify=False, gain=123.0)         # (the gain belongs to the rectifier)
        judge_multi('hipdsp_envelope_multi, rectify 0', got, ref, q,
                    'hipdsp_envelope_multi, rectify 0, %s as %s, %s' % (case, splitname(split), seg), term)


def test_envelope_multi_with_another_gain():
    case, gain = ib.MULTI_GAIN
    sos, fams, x, c, dx = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x, gain=gain)
    capped(q, case + ', gain %g' % gain)
    split = ib.MULTI[case][5][0]
    term = ib.multi_term(sos, split, x, gain=gain)
    plans = multi_plans(c, sos, split)
    for seg, opts in SEGMENTATIONS:
        with options(c, opts):
            got = run_multi(c, plans, dx, T, C, gain=gain)
        judge_multi('hipdsp_envelope_multi, gain %g' % gain, got, ref, q,
                    'hipdsp_envelope_multi, gain %g, %s as %s, %s' % (gain, case, splitname(split), seg), term)


def test_envelope_multi_and_the_single_plan_call():
    """A four-section cascade as 2 + 2, as 1 + 1 + 1 + 1 and through hipdsp_envelope: one reference, each run with the
    term of its own roundings (the single plan: the float32 tile between the passes)."""
    from audian_amd import hipdsp
    case = ib.MULTI_SINGLE
    sos, fams, x, c, dx = multi_setup(case)
    T, C = x.shape
    ref, q = ib.envelope_case(sos, x)
    capped(q, case)
    for seg, opts in SEGMENTATIONS:
        for split in ib.MULTI[case][5]:
            with options(c, opts):
                got = run_multi(c, multi_plans(c, sos, split), dx, T, C)
            judge_multi('hipdsp_envelope_multi, %s as %s' % (case.split(' @')[0], splitname(split)), got, ref, q,
                        'hipdsp_envelope_multi, %s as %s, %s' % (case, splitname(split), seg), ib.multi_term(sos, split, x))
        with options(c, opts):
            got = run_envelope(c, hipdsp.SosPlan(c, sos), dx, T, C)
        judge_multi('hipdsp_envelope, 4 sections, 8 tiles', got, ref, q, 'hipdsp_envelope, %s, %s' % (case, seg), ib.between_term(sos, x))


@pytest.mark.parametrize('case', ib.MULTI_SKIP)
def test_envelope_multi_in_place(case):
    """"x and y may overlap": y == x (skip 0 and skip > 0) and a y that starts inside the last row of x give the bits of
    the run with separate buffers."""
    from audian_amd import hipdsp
    sos, fams, x, c, _ = multi_setup(case)
    T, C = x.shape
    split = ib.MULTI[case][5][0]
    plans = multi_plans(c, sos, split)
    planar = np.ascontiguousarray(x.T)
    for skip in (0, 2049):
        dx = hipdsp.DeviceArray.from_host(c, planar)
        want = run_multi(c, plans, dx, T, C, skip=skip, clamp=True)
        hipdsp.envelope_multi(c, plans, dx, T, dx, T, C, T, skip, clamp=True)
        assert np.array_equal(dx.to_host()[:, :T - skip].T, want), (case, skip, 'y == x')
        if skip:
            assert np.array_equal(dx.to_host()[:, T - skip:], planar[:, T - skip:]), (case, skip, 'written behind the rows')
        both = hipdsp.DeviceArray(c, (2*C*T,), np.float32)
        dx, dy = both.view(0, (C, T)), both.view((C - 1)*T + 101, (C, T))
        dx.copy_from_host(planar)
        hipdsp.envelope_multi(c, plans, dx, T, dy, T - skip, C, T, skip, clamp=True)
        got = dy.to_host().ravel()[:C*(T - skip)].reshape(C, T - skip).T
        assert np.array_equal(got, want), (case, skip, 'y over the tail of x')


POISON_T = 4*ib.TILE + 5


@pytest.mark.parametrize('case', ib.MULTI_SKIP)
def test_envelope_multi_non_finite_samples_stay_in_their_lane(case):
    """NaN, +inf and -inf at sample 0, at T - 1, at a tile border of the extended trace's sweep, at one of the trace's
    own and inside a tile, in the planner's segmentation and in one-tile segments: that lane is NaN everywhere, every
    other lane keeps the bits of the clean run."""
    from audian_amd import hipdsp
    sos, fams, x, c, dx = multi_setup(case, POISON_T)
    T, C = x.shape
    split = ib.MULTI[case][5][0]
    plans = multi_plans(c, sos, split)
    lane = 1
    others = [ch for ch in range(C) if ch != lane]
    for seg, opts in (SEGMENTATIONS[2], SEGMENTATIONS[3]):
        with options(c, opts):
            clean = run_multi(c, plans, dx, T, C)
            assert np.all(np.isfinite(clean))
            for pos in (0, T - 1, ib.TILE - ib.padlen(sos), 2*ib.TILE, 5000):
                for value in (np.nan, np.inf, -np.inf):
                    bad = x.copy()
                    bad[pos, lane] = value
                    got = run_multi(c, plans, gh.to_planar(c, bad), T, C)
                    what = (case, seg, pos, value)
                    assert np.all(np.isnan(got[:, lane])), what
                    assert np.array_equal(got[:, others], clean[:, others]), what


def test_envelope_multi_edges():
    """Eight sections, pad length 51: 51 frames raise like scipy, 52 run under the bound; skip == frames writes nothing."""
    from audian_amd import hipdsp
    case = ib.MULTI_EDGE
    sos, rate, fams, splits = ib.multi_design(case)
    split = splits[0]
    edge = ib.padlen(sos)
    assert len(sos) == 8 and edge == 51
    c = gh.ctx()
    plans = multi_plans(c, sos, split)
    x = ib.families(fams, edge, rate)
    dy = fresh(c, len(fams), edge)
    with pytest.raises(ValueError, match='padlen'):
        hipdsp.envelope_multi(c, plans, gh.to_planar(c, x), edge, dy, edge, len(fams), edge, 0)
    T, C = edge + 1, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.envelope_case(sos, x)
    capped(q, case + ', %d frames' % T)
    ib.assert_in_range(ref, case + ', %d frames' % T)
    dx = gh.to_planar(c, x)
    for seg, opts in SEGMENTATIONS:
        with options(c, opts):
            got = run_multi(c, plans, dx, T, C)
        judge_multi('hipdsp_envelope_multi, padlen + 1 frames', got, ref, q,
                    'hipdsp_envelope_multi, %s, %d frames, %s' % (case, T, seg), ib.multi_term(sos, split, x))
    dy = fresh(c, C, 8)
    before = dy.to_host()
    hipdsp.envelope_multi(c, plans, dx, T, dy, 8, C, T, T)
    assert np.array_equal(dy.to_host().view(np.uint32), before.view(np.uint32)), 'skip == frames wrote something'


def test_envelope_multi_sixteen_plans():
    """The limit of the call: sixteen one-section plans (a band-pass of order 16 at its pad length + 1) run under the
    bound, seventeen are refused."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    rate, fams, split = 48000.0, ib.HP_FAMILIES, (1,)*16
    sos = butter_sos(16, (50.0, 4000.0), 'bandpass', rate)
    assert len(sos) == 16
    T, C = ib.padlen(sos) + 1, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.envelope_case(sos, x)
    capped(q, 'bp16')
    ib.assert_in_range(ref, 'bp16')
    c = gh.ctx()
    dx = gh.to_planar(c, x)
    plans = multi_plans(c, sos, split)
    got = run_multi(c, plans, dx, T, C)
    judge_multi('hipdsp_envelope_multi, 16 plans', got, ref, q, 'hipdsp_envelope_multi, 16 plans', ib.multi_term(sos, split, x))
    dy = fresh(c, C, T)
    with pytest.raises(ValueError, match='n_plans'):
        hipdsp.envelope_multi(c, plans + plans[:1], dx, T, dy, T, C, T, 0)
    assert np.all(dy.to_host().view(np.uint32) == 0x7f7f7f7f)


def test_zz_worst_per_path():
    """The worst ratio e_w / (2^-24 r_w) of every path measured above (run with -s to see the table); with a term: of
    what is left beyond it, and for hipdsp_envelope_multi also the share of the whole allowance used."""
    if not WORST:
        print('\n(no path measured in this session)')
        return
    lines = ['%-72s %s' % ('path', 'worst e_w / (2^-24 r_w)')]
    for path, worst in sorted(WORST.items()):
        lines.append('%-72s %.4f' % (path, worst))
    print('\n' + '\n'.join(lines))
