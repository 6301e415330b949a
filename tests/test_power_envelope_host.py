"""The power envelope without a GPU: the definition (power_envelope_definition.py) against what the reference's own
functions recorded (tests/golden/power_envelope.npz), the calibration of the per-window bound the GPU tests apply, the
facade's host fallback, the step rule, the absolute grid of BufferedPowerEnvelope, a host-only walk of detect_songs and the
calibration of the rows longer than the filter's memory (power_envelope_definition.carry_emulation and its mutations)."""

from math import ceil

import numpy as np
import pytest

import iir_bound as ib
import power_envelope_definition as pd
from conftest import load_golden, rel_err
from audian_amd.bufferedlowpass import BufferedLowpass
from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope, power_envelope_host, power_envelope_step
from audian_amd.tracegraph import TraceGraph

CASES = ('a_', 'b_')


class Item:
    def isVisible(self):
        return True


@pytest.fixture(scope='module')
def golden():
    return load_golden('power_envelope')


# ---- the definition and the golden -------------------------------------------------------------------------------------

@pytest.mark.parametrize('prefix', CASES)
def test_definition_restates_the_reference(golden, prefix):
    x, rate, freq = golden[prefix + 'x'], float(golden[prefix + 'rate']), float(golden[prefix + 'freq'])
    step = pd.reference_step(rate, freq)
    assert step == int(golden[prefix + 'step']) and float(golden[prefix + 'envrate']) == rate/step
    assert (prefix, step) in (('a_', 19), ('b_', 1))
    env = golden[prefix + 'envelope']
    assert env.shape == (pd.grid_size(len(x), 0, step), x.shape[1])
    sos = pd.first_order_sos(freq, rate)
    assert sos.shape == (1, 6) and sos[0, 2] == 0 and sos[0, 5] == 0 and ib.padlen(sos) == 6
    f = pd.filtered_squares(sos, x, np.float64)[::step]
    own = 2.0*np.sqrt(np.maximum(f, 0.0))                      # sqrt(2 f) sqrt(2) of the reference
    for c in range(x.shape[1]):
        assert rel_err(own[:, c], env[:, c]) <= 1e-12
    # the float32 result of the definition: one rounding of the power, one of the root
    got = pd.power_envelope(sos, x, 0, step, None, 4.0, True)
    assert got.dtype == np.float32 and got.shape == env.shape
    for c in range(x.shape[1]):
        assert rel_err(got[:, c], env[:, c]) < 2e-7
    # edata[::step] of the reference is root = 0, gain = 2: its root times sqrt(2) is the envelope
    power = pd.power_envelope(sos, x, 0, step, None, 2.0, False)
    for c in range(x.shape[1]):
        assert rel_err(np.sqrt(power[:, c].astype(np.float64))*np.sqrt(2.0), env[:, c]) < 2e-7
    # the slow envelope: lowpass_filter(env, envrate, 2 Hz)
    slow_sos = pd.first_order_sos(float(golden['slow_cutoff']), rate/step)
    slow = ib.sosfiltfilt(slow_sos, env, np.float64, gain=1.0, rectify=False, clamp=False)
    for c in range(x.shape[1]):
        assert rel_err(slow[:, c], golden[prefix + 'slow'][:, c]) <= 1e-12


def test_root_in_float32_is_the_float64_root_rounded_once():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(0, 1, 4000)**8, [0.0, 1e-45, 1.2e-38, 3e-39, 3.4e38]]).astype(np.float32)
    assert np.array_equal(np.sqrt(p), np.sqrt(p.astype(np.float64)).astype(np.float32))


# ---- the host fallback ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('prefix', CASES)
def test_host_fallback_against_the_golden(golden, prefix):
    x, rate, freq = golden[prefix + 'x'], float(golden[prefix + 'rate']), float(golden[prefix + 'freq'])
    step = power_envelope_step(rate, freq)
    assert step == int(golden[prefix + 'step'])
    sos = pd.first_order_sos(freq, rate)
    got = power_envelope_host(sos, x, 0, step)
    env = golden[prefix + 'envelope']
    assert got.dtype == np.float32 and got.shape == env.shape
    for c in range(x.shape[1]):
        assert rel_err(got[:, c], env[:, c]) < 1e-4
    assert np.array_equal(got, pd.power_envelope(sos, x, 0, step, None, 4.0, True, np.float64))


@pytest.mark.parametrize('prefix', CASES)
def test_facade_process_on_host_arrays(golden, prefix):
    from audian_amd.bufferedarray import ArrayLoader
    x, rate, freq = golden[prefix + 'x'], float(golden[prefix + 'rate']), float(golden[prefix + 'freq'])
    env = golden[prefix + 'envelope']
    src = ArrayLoader(x.astype(np.float64), rate, buffer_time=1.0, back_time=0.0, unit='V', ampl_max=2.0)
    t = BufferedPowerEnvelope(source='data', envelope_cutoff=freq)
    t.open(src)
    assert t.step == int(golden[prefix + 'step']) and t.rate == float(golden[prefix + 'envrate'])
    assert t.frames == len(env) and t.shape == env.shape and (t.ampl_min, t.ampl_max) == (0, 4.0)
    assert (t.name, t.source_name, t.source_tbefore) == ('power-envelope', 'data', 1)
    dest = np.full(env.shape, np.nan)
    t.process(x, dest, 0)
    for c in range(x.shape[1]):
        assert rel_err(dest[:, c], env[:, c]) < 1e-4
    with pytest.raises(ValueError):
        t.process(x, np.zeros((len(env) + 1, x.shape[1])), 0)
    # the slow envelope through BufferedLowpass, of the recorded envelope
    low = BufferedLowpass(source='data', cutoff=float(golden['slow_cutoff']))
    low.open(ArrayLoader(env, t.rate, buffer_time=1.0, back_time=0.0))
    slow = np.full(env.shape, np.nan)
    low.process(env.astype(np.float32), slow, 0)
    for c in range(x.shape[1]):
        assert rel_err(slow[:, c], golden[prefix + 'slow'][:, c]) < 1e-4


def test_short_slab_raises_like_scipy():
    sos = pd.first_order_sos(500.0, 96000.0)
    x = np.ones((6, 2), dtype=np.float32)
    with pytest.raises(ValueError, match='padlen'):
        power_envelope_host(sos, x)
    with pytest.raises(ValueError, match='padlen'):
        pd.power_envelope(sos, x)
    assert power_envelope_host(sos, np.ones((7, 2), dtype=np.float32)).shape == (7, 2)
    from audian_amd.bufferedarray import ArrayLoader
    t = BufferedPowerEnvelope(source='data', envelope_cutoff=500.0, step=1)
    t.open(ArrayLoader(np.ones((100, 2)), 96000.0, buffer_time=1.0, back_time=0.0))
    with pytest.raises(ValueError, match='padlen'):
        t.process(np.ones((6, 2)), np.zeros((6, 2)), 0)
    low = BufferedLowpass(source='data', cutoff=2.0)
    low.open(ArrayLoader(np.ones((100, 2)), 5000.0, buffer_time=1.0, back_time=0.0))
    with pytest.raises(ValueError, match='padlen'):
        low.process(np.ones((6, 2)), np.zeros((6, 2)), 0)


def test_rejected_design_gives_zeros():
    from audian_amd.bufferedarray import ArrayLoader
    t = BufferedPowerEnvelope(source='data', envelope_cutoff=60000.0)       # above Nyquist
    t.open(ArrayLoader(np.ones((100, 2)), 96000.0, buffer_time=1.0, back_time=0.0))
    assert t.sos is None and t.step == 1
    dest = np.full((100, 2), np.nan)
    t.process(np.ones((100, 2)), dest, 0)
    assert np.all(dest == 0)


def test_non_finite_channel_is_nan_others_keep_their_bits():
    sos = pd.first_order_sos(500.0, 96000.0)
    x = ib.families(['burst', 'offset'], 700, 96000.0)
    clean = power_envelope_host(sos, x, 0, 19)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[333, 0] = bad
        got = power_envelope_host(sos, y, 0, 19)
        assert np.all(np.isnan(got[:, 0])) and np.array_equal(got[:, 1], clean[:, 1])


# ---- the step rule and the grid ---------------------------------------------------------------------------------------

def test_step_rule():
    for rate, freq, want in ((96000.0, 500.0, 19), (48000.0, 100.0, 48), (44100.0, 6000.0, 1), (48000.0, 500.0, 10),
                             (44100.0, 500.0, 9), (96000.0, 9600.0, 1), (96000.0, 20.0, 480)):
        assert pd.reference_step(rate, freq) == want == power_envelope_step(rate, freq)


@pytest.mark.parametrize('step', [1, 2, 19, 48])
def test_grid_arithmetic(step):
    sos = pd.first_order_sos(500.0, 96000.0)
    frames = 4*48 + 7
    x = ib.families(['burst'], frames, 96000.0)
    full = power_envelope_host(sos, x, 0, 1)
    for first in sorted({0, 1, step - 1}):
        n_max = pd.grid_size(frames, first, step)
        assert n_max == len(range(first, frames, step)) == ceil((frames - first)/step)
        assert first + (n_max - 1)*step < frames <= first + n_max*step
        for n_out in (n_max, n_max - 1):
            got = power_envelope_host(sos, x, first, step, n_out)
            assert np.array_equal(got, full[first::step][:n_out])
            assert np.array_equal(got, pd.power_envelope(sos, x, first, step, n_out, 4.0, True, np.float64))
        with pytest.raises(ValueError):
            power_envelope_host(sos, x, first, step, n_max + 1)
    with pytest.raises(ValueError):
        power_envelope_host(sos, x, -1, step, 1)
    with pytest.raises(ValueError):
        power_envelope_host(sos, x, 0, 0, 1)


# ---- the facade in a host-only graph ----------------------------------------------------------------------------------

def planted(rate, seconds, songs, rng, floor=0.01, carrier=4000.0):
    """(frames, 2) float64: a noise floor and, per (channel, t0, t1), a carrier modulated at 40 Hz, 30 dB over it."""
    n = int(seconds*rate)
    t = np.arange(n)/rate
    x = floor*rng.standard_normal((n, 2))
    song = floor*10**1.5*np.sqrt(2.0)*(1.0 + np.cos(2*np.pi*40.0*t))*np.sin(2*np.pi*carrier*t)
    for c, t0, t1 in songs:
        i0, i1 = int(t0*rate), int(t1*rate)
        x[i0:i1, c] += song[i0:i1]*np.hanning(i1 - i0)**0.25
    return x


def host_graph(x, rate, buffer_time, back_time, **kwargs):
    g = TraceGraph(buffer_time, back_time)
    env = BufferedPowerEnvelope(source='data', **kwargs)
    slow = BufferedLowpass(source='power-envelope', cutoff=2.0)
    g.add_trace(env)
    g.add_trace(slow)
    g.setup_traces()
    g.open(x, rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    return g, env, slow


def test_absolute_grid_survives_a_scroll():
    rate = 8000.0
    rng = np.random.default_rng(3)
    x = rng.standard_normal((int(12*rate) + 5, 2))
    g, env, slow = host_graph(x, rate, 3.0, 0.5, envelope_cutoff=100.0)
    assert env.step == 8 and env.rate == 1000.0 and env.frames == ceil(len(x)/8) and slow.rate == 1000.0
    assert g.tbefore == 2                                     # a second for each of the two levels
    src = env.source
    g.update_times(0.0, 1.0)
    assert env.offset == 0 and len(env.buffer) > 0
    seen = {}
    for t0, t1 in [(0.0, 1.0), (1.2503, 2.2), (2.0, 3.1), (1.0, 2.0), (6.0001, 7.0), (6.7, 7.9)]:
        g.update_times(t0, t1)
        buf = np.asarray(env.buffer).copy()
        assert env.offset == ceil((src.offset + (int(rate) if src.offset > 0 else 0))/env.step)
        # frame j of the trace is frame j*step of the recording: a value that stayed in the buffer kept its bits
        kept = 0
        for j in range(env.offset, env.offset + len(buf)):
            if j in seen:
                assert np.array_equal(seen[j], buf[j - env.offset])
                kept += 1
        seen = {env.offset + i: buf[i] for i in range(len(buf))}
    assert kept > 0

    def check_whole():
        # a recompute of the whole buffer: away from the slab's ends the values are those of the definition on ANY slab
        # around them, at the frames j*step of the recording
        buf = np.asarray(env.buffer)
        lo, hi = env.offset + 200, env.offset + len(buf) - 200
        a, b = max(0, lo*env.step - 4000), min(len(x), hi*env.step + 4000)
        want = power_envelope_host(env.sos, x[a:b], lo*env.step - a, env.step, hi - lo)
        for c in range(2):
            assert rel_err(buf[lo - env.offset:hi - env.offset, c], want[:, c]) < 1e-4

    # a new cut-off and a new step recompute this trace (and the slow envelope below it) alone
    env.update()
    check_whole()
    before = np.asarray(env.buffer).copy()
    env.update(envelope_cutoff=200.0)
    check_whole()
    assert env.step == 4 and env.rate == 2000.0
    assert slow.rate == 2000.0 and len(slow.buffer) > 0 and slow.frames == env.frames      # the trace below follows
    assert len(env.buffer) >= 2*len(before) - 2
    env.update(step=8)
    assert env.step == 8 and env.rate == 1000.0 and len(env.buffer) == len(before)
    check_whole()
    assert not np.array_equal(np.asarray(env.buffer), before)              # the 200 Hz filter
    env.update(envelope_cutoff=100.0, step=None)
    assert env.step == 8 and np.array_equal(np.asarray(env.buffer), before)


def test_detect_songs_is_the_step_by_step_calls_on_the_host():
    rate = 8000.0
    rng = np.random.default_rng(17)
    songs = [(0, 2.0, 4.0), (1, 3.0, 5.0), (0, 7.0, 9.0)]
    x = planted(rate, 12.0, songs, rng, carrier=1000.0)
    x[int(5.5*rate):, 1] = 0.0                               # silence behind channel 1's song
    g, env, slow = host_graph(x, rate, 20.0, 0.0, envelope_cutoff=100.0)
    g.update_times(0.0, 12.0)
    events, freqs, thresholds = g.detect_songs('power-envelope', 'slow-envelope', min_duration=0.5, peak_thresh=10.0)
    thr = g.event_thresholds('slow-envelope', 0.0, method='histogram')
    ev = g.detect_events('slow-envelope', thr, min_gap=0.5, min_duration=0.5)
    fr = g.event_peak_freqs(ev, 'power-envelope', thresh=10.0)
    ev, fr = g.clean_event_freqs(ev, fr)
    ev = g.refine_events(ev, fr, thr, trace_name='power-envelope', min_duration=0.5, min_thresh_fac=1.0)
    assert np.array_equal(thresholds, thr)
    for c in range(2):
        assert np.array_equal(events.frames(c), ev.frames(c)) and np.array_equal(freqs[c], fr[c], equal_nan=True)
    assert events.rate == env.rate
    for c in range(2):
        mine = [(t0, t1) for ch, t0, t1 in songs if ch == c]
        found = events.frames(c)/events.rate
        assert len(found) == len(mine)
        for (t0, t1), (a, b) in zip(mine, found):
            assert a < t1 and b > t0 and abs(a - t0) < 0.5 and abs(b - t1) < 0.5
        assert np.all(np.abs(freqs[c][~np.isnan(freqs[c])] - 40.0) <= 1.0)


# ---- the calibration of the bound the GPU tests apply -----------------------------------------------------------------------

@pytest.mark.parametrize('name', list(pd.FILTERS))
def test_bound_calibration(name):
    """The cases meet the cap, the float64 sequential run rounded once is inside (1 + 16 q) 2^-24 r_w, and four wrong
    versions that pass the project's rel_err < 1e-4 by one to three decades all miss it."""
    sos, rate, fams = pd.design(name)
    assert len(sos) <= 2 and ib.padlen(sos) == {'lp1': 6, 'lp2': 9, 'lp3': 12, 'lp4': 15}[name[:3]]
    x = ib.families(list(fams), pd.T_CASE, rate)
    ref, q = pd.case(sos, x)
    ib.assert_in_range(ref, name)
    assert np.all(q <= ib.Q_CAP), (name, q)
    assert np.max(q) <= 1e-4, (name, q)                      # 3.9e-5 at most when this was written
    run = pd.runs(sos, x)[1]
    worst = ib.assert_within(run.astype(np.float32), ref, q, name + ', the float64 run rounded once')
    assert worst <= 1.0 + 16*np.max(q)
    for which in pd.WRONG:
        got = pd.wrong(sos, x, which).astype(np.float32)
        share = ib.allowance_share(got, ref, q)
        rel = np.array([rel_err(got[:, c], ref[:, c]) for c in range(x.shape[1])])
        print('%s, %s: misses by %s, rel_err %s' % (name, which, np.round(share, 3), ['%.1e' % r for r in rel]))
        with pytest.raises(AssertionError):
            ib.assert_within(got, ref, q, name + ', ' + which)
        # on at least one lane the project's metric passes by a decade or more (1e-6 at worst, 4e-8 typically) while the bound is missed
        assert np.any((share > 1.0) & (rel < 1e-5)), (name, which, share, rel)
        if which != 'extension of the samples':             # (that one is gross where the trace's ends are loud)
            assert np.all(rel < 1e-5), (name, which, rel)


# ---- rows longer than the filter's memory: every power of the ladder, every step of the carry --------------------------------

LONG_ROWS = [(name, frames) for name in pd.LONG_FILTERS for frames in pd.long_rows(name)]


def test_carry_emulation_is_the_sequential_run():
    """The emulation restates the same recurrence: on the short cases it is the sequential float64 run to float64 round-off
    (of the row's largest value: the non-normal powers of a two-section cascade reach 7e5)."""
    for name in pd.FILTERS:
        sos, rate, fams = pd.design(name)
        x = ib.families(list(fams), pd.T_CASE, rate)
        run = pd.runs(sos, x)[1]
        emu = pd.carry_emulation(sos, x)
        assert np.max(np.abs(emu - run)/np.max(np.abs(run), axis=0)) < 1e-12, name
    assert pd.powers_reached(4) == list(range(8)) and pd.powers_reached(5) == list(range(8))
    assert pd.powers_reached(6) == list(range(9)) and pd.powers_reached(18) == list(range(11))
    assert pd.powers_reached(128) == list(range(12)) and pd.powers_reached(129) == list(range(13))


@pytest.mark.parametrize('name,frames', LONG_ROWS)
def test_carry_calibration(name, frames):
    """Rows of 6, 10, 18 (two sections) and 131 tiles (one section): the case meets the cap and the range, the float64
    emulation of csrc/powerenv.hip's three-level hand-over lies inside the bound the GPU test applies, and every mutation of
    it that the row claims to reach misses the bound: P[b] = 0 and P[b] = P[b - 1] for every b of powers_reached(tiles), and on
    the 131-tile row the step hand-over without its P[12] s term and the downward carry's blocks of 64 taken from the wrong
    end of the ragged row.  A mutation the row does NOT reach leaves the emulation's bits alone, so the list of what a row
    reaches is not wishful.  Out of reach of the two-section rows: P[11] (max |.| 3.3e-24) and P[12] (4.5e-54) of lp3 8 Hz,
    which only the one-section 131-tile row shows (there 1.9e-4 and 3.5e-8).

    Measured when written, shares of the allowance (1 + 16 q) 2^-24 r_w: emulation 0.94 / 0.88 / 0.93 / 0.996; weakest
    mutants P[10] = 0 at 18 tiles 8.7, P[12] = 0 and the missing P[12] s at 131 tiles 8.5e3 (first in tile 88 of stepdown
    through the backward carry, 1.1e7 on stepup), every other one above 1e5.  The 131-tile case takes 15 s here for its
    longdouble reference and float64 run (two passes over 532497 samples each), the others 1 to 5 s."""
    sos, rate, fams = pd.long_design(name)
    tiles = pd.tiles_of(sos, frames)
    E = frames + 2*ib.padlen(sos)
    assert len(sos) == (1 if name == pd.LONG else 2)
    if name == pd.LONG:
        assert tiles == 131 and tiles > 2*pd.BLOCK and tiles % pd.BLOCK != 0 and E % pd.TILE != 0
    else:
        assert E in pd.MIDDLE_E and min(abs(E % pd.TILE - v) for v in (0, 1, pd.TILE - 1)) == 0
    x = ib.families(list(fams), frames, rate)
    ref, q = pd.case(sos, x)
    what = '%s, %d frames' % (name, frames)
    print('%s: %d tiles, q %s' % (what, tiles, ' '.join('%.2g' % v for v in q)))
    ib.assert_in_range(ref, what)
    assert np.all(q <= ib.Q_CAP), (what, q)
    clean = pd.carry_emulation(sos, x)
    worst = ib.assert_within(clean.astype(np.float32), ref, q, what + ', the emulation')
    print('%s: the emulation %.3f' % (what, worst))
    reached = pd.powers_reached(tiles)
    assert max(reached) == {6: 8, 10: 9, 18: 10, 131: 12}[tiles]
    for mutation in pd.MUTATIONS:
        if mutation.startswith('P['):
            claimed = int(mutation[2:mutation.index(']')]) in reached
        else:
            claimed = name == pd.LONG
        got = pd.carry_emulation(sos, x, mutation)
        if not claimed:
            assert got.tobytes() == clean.tobytes(), (what, mutation)
            continue
        share = ib.allowance_share(got.astype(np.float32), ref, q)
        print('%s, %s: misses by %s' % (what, mutation, ' '.join('%.3g' % v for v in share)))
        with pytest.raises(AssertionError):
            ib.assert_within(got.astype(np.float32), ref, q, what + ', ' + mutation)
