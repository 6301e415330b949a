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

Out of scope: hipdsp_envelope_multi, which hands over in float32 between its plans by design and keeps that term in
its own test (test_envelope_cascades_longer_than_one_plan).

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


def test_zz_worst_per_path():
    """The worst ratio e_w / (2^-24 r_w) of every path measured above (run with -s to see the table); with a
    high-pass: of what is left beyond the extension term."""
    if not WORST:
        print('\n(no path measured in this session)')
        return
    lines = ['%-50s %s' % ('path', 'worst e_w / (2^-24 r_w)')]
    for path, worst in sorted(WORST.items()):
        lines.append('%-50s %.4f' % (path, worst))
    print('\n' + '\n'.join(lines))
