"""Calibration of the local IIR bound (tests/iir_bound.py) on the CPU, before any kernel is held to it.

1. The restatement of sosfilt / sosfiltfilt / sosfilt_zi / the pad length agrees in float64 with the C oracle to
   1e-10 of the channel's peak, the figure test_oracle_golden.py holds the oracle to.
2. Every (filter, family) pair the GPU tests use meets q <= 2^-6 (a cap on the case list, not a measurement), and
   its reference stays in float32's normal range.
3. The correct model -- the sequential float64 run rounded once to float32 -- meets the bound with the factor 16
   replaced by 1; so does the same run with the odd extensions formed in float32 as the kernels form them, for every
   low-pass envelope.  An envelope with a high-pass does NOT (the rounding of the extension shows against an answer
   far under the rectified trace's level): it meets the bound with iir_bound.extension_term, again with 1 for 16.
   A sweep that hands its forward pass to the backward pass through a float32 tile does not either; it meets the
   bound with iir_bound.between_term.
4. Two wrong versions violate the bound: the cascade's state rounded to float32 at every tile border -- while still
   passing rel_err < 1e-4 on the same data, the gap this bound closes -- and eight-tile segments warmed up over one
   tile only, on the filter with the longest memory.
   Rows long enough for a warm-up to start in mid-trace (iir_bound.T_WARM): the model cut into three segments passes
   with the plan's own warm-up and misses the bound with half of it, forward (the past cut off, `stepdown`) and in the
   envelope's backward pass (the future cut off, `stepup`); the shortest warm-up that still passes is recorded.
5. hipdsp_envelope_multi (a cascade over several plans, float32 between them): every case of iir_bound.MULTI meets the
   cap and the range at T_MULTI; the restatement of a five- and an eight-section cascade is the oracle's; the model of
   the call with its 2P - 1 roundings lies inside the bound with iir_bound.handover_term (1 for 16); five wrong
   versions of that model each fall outside it on at least one case, several of them under rel_err < 1e-4
   (test_zz_multi_table prints the figures, run with -s).
"""

import numpy as np
import pytest

from conftest import rel_err
import iir_bound as ib


def peak_err(a, b):
    return max(rel_err(np.asarray(a, dtype=np.float64)[:, c], b[:, c]) for c in range(b.shape[1]))


@pytest.mark.parametrize('case', ['lp1 4000 Hz @ 48 kHz', 'hp3 100 Hz @ 192 kHz', 'bp4 300-3000 Hz @ 48 kHz'])
def test_sosfilt_restatement_is_the_oracles(oracle, case):
    sos, rate, fams = ib.design(case)
    x = ib.families(fams, 4096, rate)
    assert peak_err(ib.sosfilt(sos, x, np.float64), oracle.sosfilt(sos, x.astype(np.float64))) <= 1e-10
    assert peak_err(ib.sosfilt(sos, x, ib.LD), oracle.sosfilt(sos, x.astype(np.float64))) <= 1e-10


@pytest.mark.parametrize('case', list(ib.ENVELOPES))
def test_sosfiltfilt_restatement_is_the_oracles(oracle, case):
    sos, rate, fams = ib.design(case, ib.ENVELOPES)
    assert ib.padlen(sos) == oracle.sosfiltfilt_edge(sos)
    zi = oracle.sosfilt_zi(sos)
    assert np.max(np.abs(ib.sosfilt_zi(sos, np.float64) - zi)) <= 1e-10*np.max(np.abs(zi))
    x = ib.families(fams, 4096, rate)
    want = oracle.sosfiltfilt(sos, (np.pi/2)*np.abs(x.astype(np.float64)))
    assert peak_err(ib.sosfiltfilt(sos, x, np.float64, clamp=False), want) <= 1e-10
    want[want < 0] = 0
    assert peak_err(ib.sosfiltfilt(sos, x, np.float64), want) <= 1e-10
    assert np.array_equal(ib.sosfiltfilt(sos, x, np.float64), ib.clamped(ib.sosfiltfilt(sos, x, np.float64, clamp=False)))
    plain = oracle.sosfiltfilt(sos, x.astype(np.float64))                   # rectify 0: the trace itself, no gain
    assert peak_err(ib.sosfiltfilt(sos, x, np.float64, gain=1.0, rectify=False, clamp=False), plain) <= 1e-10


def test_pad_length_with_first_order_sections(oracle):
    for case in ib.BANDPASSES:
        sos = ib.design(case)[0]
        assert ib.padlen(sos) == oracle.sosfiltfilt_edge(sos), case


def test_windows_sit_on_the_grid_of_the_calls_first_sample():
    ref = np.ones((200, 1))
    got = ref.copy()
    got[70, 0] += 3*ib.ULP                                    # sample 75 of the call: window 1
    rho = ib.ratios(got, ref, first=5)
    assert rho.shape == (4, 1) and rho[1, 0] == pytest.approx(3.0) and np.all(np.delete(rho[:, 0], 1) == 0)
    zero = np.zeros((130, 1))
    assert ib.assert_within(zero, zero, 0.0, 'zeros') == 0.0
    with pytest.raises(AssertionError):
        ib.assert_within(zero + 1e-40, zero, 0.0, 'not exactly zero')
    with pytest.raises(AssertionError):
        ib.assert_within(np.full((130, 1), np.nan), ref[:130], 0.0, 'NaN')


def check_case(ref, run, what):
    """q under the cap, the reference in range, the rounded float64 run inside the bound with 1 for 16."""
    q = ib.allowance(run, ref)
    print('%s: q %s' % (what, ' '.join('%.2g' % v for v in q)))
    assert np.all(q <= ib.Q_CAP), (what, q)
    ib.assert_in_range(ref, what)
    ib.assert_within(run.astype(np.float32), ref, q, what + ', float64 rounded once', margin=1.0)
    return q


@pytest.mark.parametrize('case', list(ib.BANDPASSES) + ['general'])
def test_bandpass_cases(case):
    sos, rate, fams = ib.design(ib.GENERAL if case == 'general' else case)
    if case == 'general':
        sos = ib.spread(sos)
    for T in (ib.T_LONG, ib.T_SKIP) if case in ib.SKIP_BANDPASSES else (ib.T_LONG,):
        x = ib.families(fams, T, rate)
        ref, run = ib.sosfilt_runs(sos, x)
        check_case(ref, run, '%s, T %d' % (case, T))
        if 'onset' in fams:
            assert np.all(ref[:ib.ONSET, fams.index('onset')] == 0)


@pytest.mark.parametrize('case', list(ib.ENVELOPES))
def test_envelope_cases(case):
    sos, rate, fams = ib.design(case, ib.ENVELOPES)
    hp = ib.has_highpass(sos)
    assert hp == (fams is ib.HP_FAMILIES)
    for T in (ib.T_LONG, ib.T_SKIP) if case in ib.SKIP_ENVELOPES else (ib.T_LONG,):
        x = ib.families(fams, T, rate)
        what = '%s, T %d' % (case, T)
        ref, run = ib.envelope_runs(sos, x)
        q = check_case(ref, run, what)
        model = ib.sosfiltfilt(sos, x, np.float64, clamp=False, right_ext_f32=True).astype(np.float32)
        if hp:
            with pytest.raises(AssertionError):
                ib.assert_within(model, ref, q, what)                       # the whole bound, 16 and all
            ib.assert_within(model, ref, q, what + ', float32 right extension', margin=1.0, term=ib.extension_term(sos, x))
        else:
            worst = ib.assert_within(model, ref, q, what + ', float32 right extension', margin=1.0)
            print('%s: float32 right extension %.3f' % (what, worst))
    if case == ib.PLAYBACK:
        x = ib.families(fams, ib.T_LONG, rate)
        ref, run = ib.envelope_runs(sos, x, rectify=False)
        q = check_case(ref, run, case + ', rectify 0')
        model = ib.sosfiltfilt(sos, x, np.float64, gain=1.0, rectify=False, clamp=False, right_ext_f32=True)
        ib.assert_within(model.astype(np.float32), ref, q, case + ', rectify 0, float32 right extension', margin=1.0)


@pytest.mark.parametrize('case', ['lp8 60 Hz @ 48 kHz', 'bp3 20-300 Hz @ 48 kHz', 'lp4 300 Hz @ 48 kHz'])
def test_a_float32_tile_between_the_passes_needs_its_term(case):
    """The sweeps that hand the forward pass to the backward pass through the float32 tile (three- and four-section
    plans, the frame-split backward sweep): that model misses the bound as it stands and meets it, with 1 for 16, with
    between_term (and extension_term where the envelope has a high-pass)."""
    sos, rate, fams = ib.design(case, ib.ENVELOPES)
    x = ib.families(fams, ib.T_LONG, rate)
    ref, run = ib.envelope_runs(sos, x)
    q = ib.allowance(run, ref)
    model = ib.sosfiltfilt(sos, x, np.float64, clamp=False, right_ext_f32=True, between_f32=True).astype(np.float32)
    with pytest.raises(AssertionError):
        ib.assert_within(model, ref, q, case)
    term = ib.between_term(sos, x)
    if ib.has_highpass(sos):
        term = term + ib.extension_term(sos, x)
    worst = ib.assert_within(model, ref, q, case + ', float32 between the passes', margin=1.0, term=term)
    plain = np.max(ib.ratios(model, ref))
    print('%s: float32 between the passes %.3f roundings, %.3f beyond the term' % (case, plain, worst))


PAIRS = sorted(set(ib.SOSFILT_ENVELOPE) | set(ib.CHAIN.values()) | set(ib.SPLIT_FRAMES) | set(ib.MATRIX_PAIRS))


@pytest.mark.parametrize('bp,env', PAIRS)
def test_fused_pairs(bp, env):
    """The envelope of a band-pass output rounded to float32 (the float64 run stands in for the launch's own), from
    sample 0 and from ENV_FIRST[1], where the kernels form the left extension in float32 too.  An envelope of three or
    four sections runs behind a band-pass through env_bwd_kernel without the register window: that model, with the
    forward pass rounded to float32 between the passes, misses the bound as it stands and meets it with between_term."""
    sos, rate, fams = ib.design(bp)
    esos, _, efams = ib.design(env, ib.ENVELOPES)
    hp = ib.has_highpass(esos)
    x = ib.families(fams, ib.T_LONG, rate)
    yf = ib.sosfilt_runs(sos, x)[1].astype(np.float32)[:, ib.envelope_lanes(fams, efams)]
    shifted = (bp, env) in ib.SOSFILT_ENVELOPE or (bp, env) == ib.CHAIN[2048, 1024] or (bp, env) in ib.MATRIX_SHIFTED
    for first in ib.ENV_FIRST if shifted else ib.ENV_FIRST[:1]:
        what = '%s + %s from %d' % (bp, env, first)
        ref, run = ib.envelope_runs(esos, yf[first:])
        q = check_case(ref, run, what)
        model = ib.sosfiltfilt(esos, yf[first:], np.float64, clamp=False, right_ext_f32=True, left_ext_f32=first > 0)
        term = ib.extension_term(esos, yf[first:], left=first > 0) if hp else None
        ib.assert_within(model.astype(np.float32), ref, q, what + ', float32 extensions', margin=1.0, term=term)
        if len(esos) > 2:
            model = ib.sosfiltfilt(esos, yf[first:], np.float64, clamp=False, right_ext_f32=True, left_ext_f32=first > 0,
                                   between_f32=True).astype(np.float32)
            with pytest.raises(AssertionError):
                ib.assert_within(model, ref, q, what)
            term = ib.between_term(esos, yf[first:]) + (0.0 if term is None else term)
            ib.assert_within(model, ref, q, what + ', float32 between the passes', margin=1.0, term=term)


def test_matrix_tables():
    """One band-pass and one envelope of every section count, every envelope's families among every band-pass's, and
    the fused forward sweep's shifted-grid pairs are those with envelopes of at most two sections."""
    for table, names in ((ib.BANDPASSES, ib.MATRIX_BANDPASS), (ib.ENVELOPES, ib.MATRIX_ENVELOPE)):
        assert sorted(names) == [1, 2, 3, 4]
        assert all(len(ib.design(names[n], table)[0]) == n for n in names)
    for (sf, se), env in ib.MATRIX_ENVELOPE_BEHIND.items():
        assert sf in ib.MATRIX_BANDPASS and len(ib.design(env, ib.ENVELOPES)[0]) == se
    assert len(set(ib.MATRIX_PAIRS)) == 16 and set(ib.MATRIX_PAIRS) <= set(PAIRS)
    assert set(ib.MATRIX_SHIFTED) == {(bp, env) for bp, env in ib.MATRIX_PAIRS if len(ib.design(env, ib.ENVELOPES)[0]) <= 2}
    for bp, env in ib.MATRIX_PAIRS:
        assert len(ib.envelope_lanes(ib.design(bp)[2], ib.design(env, ib.ENVELOPES)[2])) >= 4


@pytest.mark.parametrize('sections', sorted(ib.MATRIX_BANDPASS))
def test_matrix_spectral_lanes_meet_the_cap(sections):
    """The stationary lanes whose PSD the sweep matrix judges ride through the band-pass too, and their yf is judged like
    every other lane's: q under the cap, the reference in range, the rounded float64 run inside the bound."""
    bp = ib.MATRIX_BANDPASS[sections]
    sos, rate, _ = ib.design(bp)
    x = ib.matrix_spectral_lanes(ib.T_LONG, rate)
    assert x.shape == (ib.T_LONG, 16)
    ref, run = ib.sosfilt_runs(sos, x)
    check_case(ref, run, '%s, spectral lanes' % bp)


@pytest.mark.parametrize('case,table', [('bp2 300-3000 Hz @ 96 kHz', 'BANDPASSES'), ('bp4 300-3000 Hz @ 48 kHz', 'BANDPASSES'),
                                        ('lp2 20 Hz @ 96 kHz', 'ENVELOPES'), ('lp2 500 Hz @ 48 kHz', 'ENVELOPES')])
def test_a_float32_hand_over_is_caught_and_passes_the_old_metric(case, table):
    sos, rate, _ = ib.design(case, getattr(ib, table))
    x = ib.families(ib.FAMILIES, ib.T_LONG, rate)
    ref, q = ib.sosfilt_case(sos, x)
    assert np.all(q <= ib.Q_CAP)
    wrong = ib.wrong_f32_handover(sos, x).astype(np.float32)
    rho = np.max(ib.ratios(wrong, ref), axis=0)
    old = [rel_err(wrong[:, c], np.asarray(ref[:, c], dtype=np.float64)) for c in range(x.shape[1])]
    print('%s: local %s, rel_err %s' % (case, ' '.join('%.3g' % v for v in rho), ' '.join('%.2g' % v for v in old)))
    assert max(old) < 1e-4                                     # the old metric lets it through in every family
    assert np.any(rho > 1.0 + ib.MARGIN*q)
    with pytest.raises(AssertionError):
        ib.assert_within(wrong, ref, q, case)


def test_a_one_tile_warm_up_is_caught():
    case = 'lp2 20 Hz @ 96 kHz'                                # the longest memory of the list: 26 tiles
    sos, rate, _ = ib.design(case, ib.ENVELOPES)
    x = ib.families(ib.FAMILIES, ib.T_LONG, rate)
    ref, q = ib.sosfilt_case(sos, x)
    wrong = ib.wrong_one_tile_warmup(sos, x).astype(np.float32)
    rho = np.max(ib.ratios(wrong, ref), axis=0)
    print('%s: local %s' % (case, ' '.join('%.3g' % v for v in rho)))
    assert np.any(rho > 1.0 + ib.MARGIN*q)
    with pytest.raises(AssertionError):
        ib.assert_within(wrong, ref, q, case)


# ---- warm-ups that start inside the trace -----------------------------------------------------------------------------

def plan_warm_tiles(sos):
    """The warm-up of a plan in tiles (hipdsp_sos_plan_host, no GPU)."""
    import ctypes
    from audian_amd import _lib
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    warm = ctypes.c_int64()
    _lib.check(_lib.lib.hipdsp_sos_plan_host(ctypes.c_void_p(sos.ctypes.data), len(sos), ctypes.byref(warm), None, None))
    assert warm.value % ib.TILE == 0
    return int(warm.value)//ib.TILE


# the shortest warm-up (tiles) with which the three-segment model still meets the bound on the four families at their
# levels, of the plan's 15 / 26 / 26; steps of 120 dB in place of 80 (q within the cap) move it to 9 / 16 / 16 tiles and
# no further: no admissible level makes three quarters of a warm-up (11 / 19 tiles) fail
SHORTEST = {(ib.WARM_BANDPASS, 'forward'): 8, (ib.WARM_ENVELOPE, 'forward'): 16, (ib.WARM_ENVELOPE, 'backward'): 14}


def check_warmups(model, ref, q, what, warm, shortest, lane):
    """The plan's own warm-up and the shortest recorded one pass, one tile less and half the plan's fail, the latter on
    `lane`, the family that has quiet windows on the far side of a loud passage."""
    assert shortest <= 3*warm//4 and warm//2 < shortest
    for w in (warm, shortest):
        worst = ib.assert_within(model(w).astype(np.float32), ref, q, '%s, warm-up %d tiles' % (what, w))
        print('%s: warm-up %d tiles, worst %.3f' % (what, w, worst))
    for w in sorted({shortest - 1, warm//2}, reverse=True):
        got = model(w).astype(np.float32)
        share = ib.allowance_share(got, ref, q)
        print('%s: warm-up %d tiles misses by %s' % (what, w, ' '.join('%.3g' % v for v in share)))
        with pytest.raises(AssertionError):
            ib.assert_within(got, ref, q, '%s, warm-up %d tiles' % (what, w))
        if w == warm//2:
            assert share[lane] > 1.0, (what, w, share)


def test_warmup_inside_the_trace_forward():
    """hp3 100 Hz @ 192 kHz at 48 tiles + 5 (the longdouble reference takes 3.8 s here): three segments of 17 tiles, the
    second and third start from zero state in mid-trace.  Warm-ups of 15 (the plan's) and 8 tiles pass, 7 tiles miss
    the bound (1.2), as does half the plan's warm-up."""
    case = ib.WARM_BANDPASS
    sos, rate, _ = ib.design(case)
    warm = plan_warm_tiles(sos)
    assert warm == ib.WARM_TILES[case] == 15
    T = ib.T_WARM[case]
    assert len(ib.cut_warmups(-(-T//ib.TILE), 17, warm)) == 2
    x = ib.families(ib.WARM_FAMILIES, T, rate)
    ref, run = ib.sosfilt_runs(sos, x)
    q = check_case(ref, run, '%s, T %d' % (case, T))
    check_warmups(lambda w: ib.segmented_sosfilt(sos, x, w), ref, q, case, warm, SHORTEST[case, 'forward'],
                  ib.WARM_FAMILIES.index('stepdown'))


def test_warmup_inside_the_trace_envelope():
    """lp2 20 Hz @ 96 kHz at 64 tiles + 5 (the longdouble references take 2.1 s for the forward pass and 4.3 s for the
    envelope here): three segments of 22 tiles, the third starts at tile 44 from zero state at tile 18.  As a forward
    sweep (a band-pass with this memory; `stepdown` shows the past that is cut off) warm-ups of 26 and 16 tiles pass,
    15 (1.7) and 13 (11) miss the bound.  As the envelope's backward pass (`stepup` shows the future that is cut off) 26
    and 14 tiles pass, 13 tiles miss it (2.4)."""
    case = ib.WARM_ENVELOPE
    sos, rate, _ = ib.design(case, ib.ENVELOPES)
    warm = plan_warm_tiles(sos)
    assert warm == ib.WARM_TILES[case] == 26
    T = ib.T_WARM[case]
    assert ib.cut_warmups(-(-T//ib.TILE), 22, warm) == [(44, 18)]
    assert ib.cut_warmups(-(-(T + ib.padlen(sos))//ib.TILE), 22, warm) == [(44, 18)]
    x = ib.families(ib.WARM_FAMILIES, T, rate)
    ref, run = ib.sosfilt_runs(sos, x)
    q = check_case(ref, run, '%s, T %d, forward' % (case, T))
    check_warmups(lambda w: ib.segmented_sosfilt(sos, x, w), ref, q, case + ', forward', warm, SHORTEST[case, 'forward'],
                  ib.WARM_FAMILIES.index('stepdown'))
    ref, run = ib.envelope_runs(sos, x)
    q = check_case(ref, run, '%s, T %d, envelope' % (case, T))
    check_warmups(lambda w: ib.segmented_envelope(sos, x, w), ref, q, case + ', backward', warm, SHORTEST[case, 'backward'],
                  ib.WARM_FAMILIES.index('stepup'))


def test_warmup_fused_pair_meets_the_cap():
    """The fused launches' long case: the 20 Hz envelope of the 300-3000 Hz band-pass output (the float64 run rounded to
    float32 stands in for the launch's own), from sample 0 and from ENV_FIRST[1]: the cap, the range, and the model with
    the sweeps' float32 extensions inside the bound with 1 for 16."""
    sos, rate, _ = ib.design(ib.WARM_FUSED)
    esos = ib.design(ib.WARM_ENVELOPE, ib.ENVELOPES)[0]
    assert plan_warm_tiles(sos) <= 2
    x = ib.families(ib.WARM_FAMILIES, ib.T_WARM[ib.WARM_ENVELOPE], rate)
    ref, run = ib.sosfilt_runs(sos, x)
    check_case(ref, run, ib.WARM_FUSED + ', T %d' % len(x))
    yf = run.astype(np.float32)
    for first in ib.ENV_FIRST:
        what = '%s + %s from %d, T %d' % (ib.WARM_FUSED, ib.WARM_ENVELOPE, first, len(x))
        ref, run = ib.envelope_runs(esos, yf[first:])
        q = check_case(ref, run, what)
        model = ib.sosfiltfilt(esos, yf[first:], np.float64, clamp=False, right_ext_f32=True, left_ext_f32=first > 0)
        ib.assert_within(model.astype(np.float32), ref, q, what + ', float32 extensions', margin=1.0)


# ---- hipdsp_envelope_multi ---------------------------------------------------------------------------------------------

def multi_case(case):
    sos, rate, fams, splits = ib.multi_design(case)
    x = ib.families(fams, ib.T_MULTI, rate)
    ref, run = ib.envelope_runs(sos, x)
    return sos, fams, splits, x, ref, run


@pytest.mark.parametrize('case', list(ib.MULTI))
def test_multi_cases_meet_the_cap_and_the_range(case):
    sos, fams, splits, x, ref, run = multi_case(case)
    q = check_case(ref, run, '%s, T %d' % (case, ib.T_MULTI))
    assert ib.has_highpass(sos) == (fams is ib.HP_FAMILIES)
    assert all(sum(split) == len(sos) and max(split) <= 4 for split in splits)
    if case == ib.MULTI_PLAIN:
        ref, run = ib.envelope_runs(sos, x, rectify=False)
        check_case(ref, run, case + ', rectify 0')
    if case == ib.MULTI_GAIN[0]:
        ref, run = ib.envelope_runs(sos, x, gain=ib.MULTI_GAIN[1])
        check_case(ref, run, case + ', gain %g' % ib.MULTI_GAIN[1])
    if case in ib.MULTI_SKIP:
        assert ib.T_MULTI - max(ib.SKIPS) > ib.padlen(sos)


@pytest.mark.parametrize('case', ['lp10 800 Hz @ 48 kHz', 'bp8 50-4000 Hz @ 48 kHz'])
def test_multi_restatement_is_the_oracles(oracle, case):
    """Five and eight sections: pad length, zi and sosfiltfilt of the whole cascade."""
    sos, rate, fams, _ = ib.multi_design(case)
    assert len(sos) == (5 if case.startswith('lp10') else 8)
    assert ib.padlen(sos) == oracle.sosfiltfilt_edge(sos)
    zi = oracle.sosfilt_zi(sos)
    assert np.max(np.abs(ib.sosfilt_zi(sos, np.float64) - zi)) <= 1e-10*np.max(np.abs(zi))
    x = ib.families(fams, 4096, rate)
    want = oracle.sosfiltfilt(sos, (np.pi/2)*np.abs(x.astype(np.float64)))
    assert peak_err(ib.sosfiltfilt(sos, x, np.float64, clamp=False), want) <= 1e-10
    assert peak_err(ib.sosfiltfilt(sos, x, ib.LD, clamp=False), want) <= 1e-10


def model_figures(case, _memo={}):
    """{split: (the model's worst e_w / (2^-24 r_w), share of the allowance used, median and largest term / (2^-24 r_w))},
    after asserting the model inside (1 + q) 2^-24 r_w + term for every split and lane."""
    if case not in _memo:
        sos, fams, splits, x, ref, run = multi_case(case)
        q = ib.allowance(run, ref)
        _, r = ib.window_stats(ref, ref)
        ok = r > 0
        rows = {'q': float(np.max(q))}
        for split in splits:
            what = '%s as %s' % (case, '+'.join(str(n) for n in split))
            model = ib.multi_model(sos, split, x)
            term = ib.multi_term(sos, split, x)
            ib.assert_within(model, ref, q, what + ', the model', margin=1.0, term=term)
            _, t = ib.window_stats(term, term)
            size = np.asarray(t[ok]/(ib.ULP*r[ok]), dtype=np.float64)
            rows[split] = (float(np.max(ib.ratios(model, ref))), float(np.max(ib.allowance_share(model, ref, q, term))),
                           float(np.median(size)), float(np.max(size)))
        _memo[case] = rows
    return _memo[case]


def figure_lines(case):
    rows = model_figures(case)
    return ['%-24s %-8s q %.1e  model %5.2f roundings, %3.0f %% of the allowance; term median %6.1f, largest %6.0f' % (
        (case, '+'.join(str(n) for n in split), rows['q'], figures[0], 100*figures[1]) + figures[2:])
        for split, figures in rows.items() if split != 'q']


@pytest.mark.parametrize('case', list(ib.MULTI))
def test_multi_model_lies_inside_the_bound(case):
    """The call restated with its roundings, every split and lane: inside (1 + q) 2^-24 r_w + term (1 for 16); also
    without the rectifier and with another gain."""
    sos, fams, splits, x, ref, run = multi_case(case)
    print('\n'.join(figure_lines(case)))
    assert all(figures[1] <= 1.0 for split, figures in model_figures(case).items() if split != 'q')
    split = splits[0]
    if case == ib.MULTI_PLAIN:
        ref, run = ib.envelope_runs(sos, x, rectify=False)
        ib.assert_within(ib.multi_model(sos, split, x, rectify=False), ref, ib.allowance(run, ref), case + ', rectify 0',
                         margin=1.0, term=ib.multi_term(sos, split, x, rectify=False))
    if case == ib.MULTI_GAIN[0]:
        gain = ib.MULTI_GAIN[1]
        ref, run = ib.envelope_runs(sos, x, gain=gain)
        ib.assert_within(ib.multi_model(sos, split, x, gain=gain), ref, ib.allowance(run, ref), case + ', gain %g' % gain,
                         margin=1.0, term=ib.multi_term(sos, split, x, gain=gain))


WRONG_CASES = [c for c in ib.MULTI if c != ib.MULTI_SINGLE]


def wrong_figures(case, _memo={}):
    """{wrong version: (per lane e_w / allowed under the bound the GPU tests apply, 16 and all; per lane rel_err)} on the
    case's first split, after checking that assert_within says the same."""
    if case not in _memo:
        sos, fams, splits, x, ref, run = multi_case(case)
        q = ib.allowance(run, ref)
        split = splits[0]
        term = ib.multi_term(sos, split, x)
        ref64 = np.asarray(ref, dtype=np.float64)
        rows = {}
        for wrong in ib.MULTI_WRONG:
            got = ib.multi_model(sos, split, x, wrong=wrong)
            miss = ib.allowance_share(got, ref, q, term)
            old = np.array([rel_err(got[:, c].astype(np.float64), ref64[:, c]) for c in range(x.shape[1])])
            if np.max(miss) > 1.0:
                with pytest.raises(AssertionError):
                    ib.assert_within(got, ref, q, case, term=term)
            else:
                ib.assert_within(got, ref, q, case, term=term)
            rows[wrong] = (miss, old)
        _memo[case] = rows
    return _memo[case]


@pytest.mark.parametrize('case', WRONG_CASES)
def test_multi_wrong_versions(case):
    """Every wrong version of the model, per lane: by how much it misses the bound, and what rel_err makes of it.
    Judged over all cases by test_zz_multi_table."""
    for wrong, (miss, old) in wrong_figures(case).items():
        print('%s, %s: e_w / allowed %s, rel_err %s' % (case, wrong, ' '.join('%.3g' % v for v in miss),
                                                         ' '.join('%.2g' % v for v in old)))


def test_zz_multi_table():
    """The teeth of the multi-plan bound and the calibration's table (run with -s): every wrong version falls outside
    the bound on at least one case, at least two of them on a lane that rel_err < 1e-4 lets through meanwhile; the
    float32 state is caught on the 10-500 Hz band-pass and stays inside on the 800 Hz low-pass, where the designed
    hand-over dominates."""
    lines = [line for case in ib.MULTI for line in figure_lines(case)]
    quiet = 0
    worst = {}
    for wrong in ib.MULTI_WRONG:
        seen = {case: wrong_figures(case)[wrong] for case in WRONG_CASES}
        worst[wrong] = {case: float(np.max(miss)) for case, (miss, _) in seen.items()}
        caught = {c: m for c, m in worst[wrong].items() if m > 1.0}
        inside = {c: m for c, m in worst[wrong].items() if m <= 1.0}
        through = any(np.any((miss > 1.0) & (old < 1e-4)) for miss, old in seen.values())
        quiet += through
        lines.append('%s: caught on %s; inside on %s%s' % (
            wrong, ', '.join('%s (%.3g)' % (c.split(' @')[0], m) for c, m in caught.items()) or 'nothing',
            ', '.join('%s (%.2f)' % (c.split(' @')[0], m) for c, m in inside.items()) or 'nothing',
            '; under rel_err < 1e-4 meanwhile' if through else ''))
        assert caught, wrong
    print('\n' + '\n'.join(lines))
    assert quiet >= 2
    assert worst['float32 state at tile borders']['lp10 800 Hz @ 48 kHz'] <= 1.0
    assert worst['float32 state at tile borders']['bp5 10-500 Hz @ 48 kHz'] > 1.0
