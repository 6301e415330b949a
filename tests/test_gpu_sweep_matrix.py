"""Every instantiation of the fused sweeps under the local bounds: chain_fwd_kernel<SF, SE, 8, FLAGS, DB, NFFT, HOP> for
the six window shapes x band-passes of one to four sections x no envelope or one of one or two sections x PSD only or
PSD + dB image (144 code objects), the 8 barrier variants at 2048/1024, and sos_ckpt_kernel<SF, SE, PREFETCH> for the 16
(band-pass, envelope) pairs of hipdsp_sosfilt_envelope with the second, prefetching build of the pairs of at most two
sections each (and, behind both, phase 2 through env_bwd_kernel<1 .. 4> from that sweep's tile states).

fused_rows() and ckpt_rows() ARE the matrix: the tests below walk them and nothing else, and
tests/test_sweep_matrix_host.py holds them to the launch tables in csrc/chain_shape.inc, csrc/Makefile and csrc/sos.hip,
both ways.  The rows of sos_ckpt_kernel<0, SE, *> (no band-pass: hipdsp_envelope) belong to
test_gpu_iir_accuracy.py::test_envelope (envelope_rows()).

What is judged, with the filters of iir_bound.MATRIX_BANDPASS / MATRIX_ENVELOPE at T_LONG, a sentinel in every output:
* yf of every launch against the longdouble reference of x (iir_bound.assert_within);
* every envelope against the reference of its own launch's yf (judge_envelopes; iir_bound.between_term where the plan has
  three or four sections);
* the PSD of 16 stationary lanes (iir_bound.matrix_spectral_lanes) per bin against the oracle's spectrogram of the
  launch's own yf[spec_first:], and the dB image next to it (spectral_bound.assert_within);
* bit for bit, within one (shape, band-pass, segmentation, grid): yf and the PSD are the same for every SE and with or
  without db_out, the envelope is the same with or without db_out, the dB image the same for every SE -- so one
  judgement of each covers six kernels.  Nothing is asserted across shapes, segmentations or the two hand-over variants.
The fused sweep runs in the planner's segments, in one-tile segments and once on the shifted grid (spec_first 777, env_first
ENV_FIRST[1], one-tile segments); sos_ckpt_kernel as phase 0 and as phases 1 + 2 in all four segmentations, its clamped
run bit for bit the clamp of the unclamped one.  test_zz_worst_per_path prints the worst ratios (run with -s).
"""

import numpy as np
import pytest

import gpu_helpers as gh
import iir_bound as ib
import spectral_bound as sb
from test_gpu_iir_accuracy import SEGMENTATIONS, WORST, bandpass, capped, fresh, judge_envelopes, note, options

pytestmark = pytest.mark.gpu

SHAPES = ((2048, 1024), (2048, 512), (1024, 512), (1024, 256), (512, 256), (256, 128))
BARRIER_SHAPE = (2048, 1024)                 # "chain_debug" 4: workgroup barriers in place of the pairwise flags
SPECTRAL_WORST = {}


def fused_rows():
    """(nfft, hop, SF, SE, db_out present, barrier variant) of every chain_fwd_kernel launch of the matrix."""
    rows = [(nfft, hop, sf, se, db, False) for nfft, hop in SHAPES for sf in (1, 2, 3, 4) for se in (0, 1, 2) for db in (False, True)]
    rows += [BARRIER_SHAPE + (sf, se, db, True) for sf in (1, 2) for se in (1, 2) for db in (False, True)]
    return rows


def ckpt_rows():
    """(SF, SE, "sos_prefetch") of every sos_ckpt_kernel launch of the matrix: the option is switched off too where a
    second, prefetching build exists (SF, SE <= 2)."""
    rows = [(sf, se, 1) for sf in (1, 2, 3, 4) for se in (1, 2, 3, 4)]
    rows += [(sf, se, 0) for sf in (1, 2) for se in (1, 2)]
    return rows


def envelope_rows():
    """The same for SF = 0: what test_gpu_iir_accuracy.py::test_envelope runs (every case of iir_bound.ENVELOPES with
    "sos_prefetch" 1 and 0)."""
    return sorted({(0, len(ib.design(case, ib.ENVELOPES)[0]), prefetch) for case in ib.ENVELOPES for prefetch in (1, 0)})


def ckpt_instantiation(sf, se, prefetch):
    """(SF, SE, PREFETCH) of the sos_ckpt_kernel that launch_env_ckpt picks at T_LONG (at least four tiles)."""
    return sf, se, bool(prefetch) and sf <= 2 and se <= 2


FUSED_ROWS, CKPT_ROWS = fused_rows(), ckpt_rows()
# (segmentation, spec_first, env_first) of the three launches of every instantiation
LAUNCHES = ((SEGMENTATIONS[2], 0, 0), (SEGMENTATIONS[3], 0, 0), (SEGMENTATIONS[3], 777, ib.ENV_FIRST[1]))


def spectral_note(path, rb):
    old = SPECTRAL_WORST.get(path, (0.0, 0.0))
    SPECTRAL_WORST[path] = (max(old[0], rb[0]), max(old[1], rb[1]))


def run_fused(c, fplan, eplan, dx, T, C, nfft, hop, rate, want_db, spec_first, env_first):
    """hipdsp_chain_forward into sentinel-filled buffers, one frame more than the trace holds (zero), then phase 2 where
    there is an envelope plan: (yf (T, C), env (T - env_first, C) or None, PSD (C, nd, F), dB image or None)."""
    from audian_amd import hipdsp
    F = nfft//2 + 1
    nd = (T - spec_first + hop - 1)//hop + 1
    yf, ps = fresh(c, C, T), fresh(c, C, nd*F)
    db = fresh(c, C, nd*F) if want_db else None
    hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, rate, ps, nd, db_out=db, spec_first=spec_first,
                         env_first=env_first)
    env = None
    if eplan is not None:
        ye = fresh(c, C, T - env_first)
        hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T - env_first, C, T, clamp=False, phase=2, env_first=env_first)
        env = ye.to_host().T
    return yf.to_host().T, env, ps.to_host().reshape(C, nd, F), (db.to_host().reshape(C, nd, F) if want_db else None)


@pytest.mark.parametrize('sf', (1, 2, 3, 4))
@pytest.mark.parametrize('nfft,hop', SHAPES)
def test_chain_fwd_kernel(oracle, nfft, hop, sf):
    """The rows of fused_rows() for one shape and band-pass: 6 instantiations (10 at 2048/1024 with one or two sections:
    the barrier variants) x 3 launches."""
    from audian_amd import hipdsp
    rows = [r for r in FUSED_ROWS if r[:3] == (nfft, hop, sf)]
    assert len(rows) == (10 if (nfft, hop) == BARRIER_SHAPE and sf <= 2 else 6)
    bp = ib.MATRIX_BANDPASS[sf]
    sos, rate, fams = bandpass(bp)
    T, n_fam = ib.T_LONG, len(fams)
    x = np.concatenate([ib.families(fams, T, rate), ib.matrix_spectral_lanes(T, rate)], axis=1)
    C = x.shape[1]
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos)
    envelopes = {se: ib.design(ib.matrix_pair(sf, se)[1], ib.ENVELOPES) for se in (1, 2)}
    eplans = {se: hipdsp.SosPlan(c, envelopes[se][0]) for se in envelopes}
    eplans[0] = None
    lanes = {se: ib.envelope_lanes(fams, envelopes[se][2]) for se in envelopes}
    runs = {}                                    # (barrier, se, env_first): the launches whose envelope is judged
    for barrier in (False, True):
        variant = [r for r in rows if r[5] == barrier]
        if not variant:
            continue
        path = 'sweep matrix, chain_fwd_kernel %d/%d%s' % (nfft, hop, ', barriers' if barrier else '')
        for (seg, opts), spec_first, env_first in LAUNCHES:
            grid = '%s%s' % (seg, ', shifted grid' if spec_first else '')
            base = {}
            for _, _, _, se, want_db, _ in variant:
                what = '%s, %s, SE %d%s, %s' % (path, bp, se, ' +dB' if want_db else '', grid)
                c.set_option('chain_debug', 4 if barrier else 0)
                try:
                    with options(c, opts):
                        gf, ge, gs, gd = run_fused(c, fplan, eplans[se], dx, T, C, nfft, hop, rate, want_db, spec_first, env_first)
                finally:
                    c.set_option('chain_debug', 0)
                if 'yf' not in base:
                    base['yf'], base['psd'] = gf, gs
                    note(path + ', band-pass', ib.assert_within(gf, ref, q, what))
                    want = np.zeros((gs.shape[1], C - n_fam, gs.shape[2]))
                    oracle.spectrogram_process(gf[spec_first:, n_fam:].astype(np.float64), want, rate, nfft, hop)
                    want = want.transpose(1, 0, 2)
                    zero = np.max(want, axis=-1) == 0
                    assert zero.any() and not zero.all(), what
                    spectral_note(path, sb.assert_within(gs[n_fam:], want, nfft, what))
                else:
                    assert np.array_equal(gf, base['yf']), what + ': yf depends on SE or db_out'
                    assert np.array_equal(gs, base['psd']), what + ': the PSD depends on SE or db_out'
                if want_db and 'db' not in base:
                    base['db'] = gd
                    spectral_note(path, sb.assert_within(gs[n_fam:], want, nfft, what, db=gd[n_fam:]))
                elif want_db:
                    assert np.array_equal(gd, base['db']), what + ': the dB image depends on SE'
                if se and ('env', se) not in base:
                    base['env', se] = ge
                    runs.setdefault((barrier, se, env_first), []).append((grid, gf[:, lanes[se]], ge[:, lanes[se]]))
                elif se:
                    assert np.array_equal(ge, base['env', se]), what + ': the envelope depends on db_out'
    for (barrier, se, env_first), group in sorted(runs.items()):
        path = 'sweep matrix, chain_fwd_kernel %d/%d%s' % (nfft, hop, ', barriers' if barrier else '')
        judge_envelopes(path + ', envelope', envelopes[se][0], group, env_first,
                        '%s, %s + %s' % (path, bp, ib.matrix_pair(sf, se)[1]))


@pytest.mark.parametrize('sf,se', sorted({r[:2] for r in CKPT_ROWS}))
def test_sos_ckpt_kernel(sf, se):
    """The rows of ckpt_rows() for one pair: phase 0 and phases 1 + 2 from sample 0 in every segmentation, with
    "sos_prefetch" 0 too where the pair has a prefetching build."""
    from audian_amd import hipdsp
    rows = [r for r in CKPT_ROWS if r[:2] == (sf, se)]
    assert len(rows) == (2 if sf <= 2 and se <= 2 else 1)
    bp, env = ib.matrix_pair(sf, se)
    sos, rate, fams = bandpass(bp)
    esos, _, efams = ib.design(env, ib.ENVELOPES)
    assert (len(sos), len(esos)) == (sf, se)
    lanes = ib.envelope_lanes(fams, efams)
    T, C = ib.T_LONG, len(fams)
    x = ib.families(fams, T, rate)
    ref, q = ib.sosfilt_case(sos, x)
    capped(q, bp)
    c = gh.ctx()
    dx, fplan, eplan = gh.to_planar(c, x), hipdsp.SosPlan(c, sos), hipdsp.SosPlan(c, esos)
    between = len(esos) > 2
    runs = []
    for _, _, prefetch in rows:
        for seg, opts in SEGMENTATIONS:
            for phases in ((0,), (1, 2)):
                label = '%s, phase %s, sos_prefetch %d' % (seg, '+'.join(str(p) for p in phases), prefetch)
                what = 'sweep matrix, sos_ckpt_kernel, %s + %s, %s' % (bp, env, label)
                with options(c, opts + (('sos_prefetch', prefetch),)):
                    yf, ye, yc = fresh(c, C, T), fresh(c, C, T), fresh(c, C, T)
                    for phase in phases:
                        hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, ye, T, C, T, clamp=False, phase=phase)
                    gf, ge = yf.to_host().T, ye.to_host().T
                    hipdsp.sosfilt_envelope(c, fplan, eplan, dx, T, yf, T, yc, T, C, T, clamp=True, phase=phases[-1])
                assert np.array_equal(yc.to_host().T, ib.clamped(ge)), what + ': the clamped run is not the clamp of the unclamped one'
                assert np.array_equal(yf.to_host().T, gf), what + ': yf changed with the clamp'
                note('sweep matrix, sos_ckpt_kernel, band-pass', ib.assert_within(gf, ref, q, what))
                runs.append((label, gf[:, lanes], ge[:, lanes]))
    judge_envelopes('sweep matrix, sos_ckpt_kernel, envelope of %d section%s%s%s' % (
        se, 's'[:se > 1], ', high-pass' if ib.has_highpass(esos) else '', ' (beyond between_term)' if between else ''),
        esos, runs, 0, 'sweep matrix, sos_ckpt_kernel, %s + %s' % (bp, env), between=between)


def test_zz_worst_per_path():
    """The worst ratio e_w / (2^-24 r_w) of every path of the matrix (with a term: of what is left beyond it), and the
    worst rho (of 2) and beta of the PSDs (run with -s to see the table)."""
    mine = {path: worst for path, worst in WORST.items() if path.startswith('sweep matrix')}
    if not mine and not SPECTRAL_WORST:
        print('\n(no path measured in this session)')
        return
    lines = ['%-72s %s' % ('path', 'worst e_w / (2^-24 r_w)')]
    for path, worst in sorted(mine.items()):
        lines.append('%-72s %.4f' % (path, worst))
    lines.append('%-72s %s' % ('path', 'worst rho, worst beta'))
    for path, (rho, beta) in sorted(SPECTRAL_WORST.items()):
        lines.append('%-72s %.3f  %.2f' % (path + ', PSD', rho, beta))
    print('\n' + '\n'.join(lines))
