"""hipdsp_power_envelope on the device: every 64-sample window against the longdouble definition under the bound that
tests/test_power_envelope_host.py calibrates, the lengths around every chunk and tile border, the decimation grid and the
root bit for bit, the reference's own results (tests/golden/power_envelope.npz), determinism, isolation, non-finite rows,
context state, rows past element 2^31, and the facade: BufferedPowerEnvelope, BufferedLowpass, TraceGraph.detect_songs.

Every call goes through run(): the rows sit in a larger input with pitch slack and an odd base offset, the output is
prefilled with a sentinel and EVERYTHING outside y[c*y_pitch + j], j < n_out, must still hold it afterwards."""

import functools

import numpy as np
import pytest

import gpu_helpers as gh
import iir_bound as ib
import power_envelope_definition as pd
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0xa5
CHUNK, TILE = 64, 4096                          # hipdsp.POWER_ENVELOPE_CHUNK / _TILE: samples per lane and per wave
T_CASE = pd.T_CASE                              # three tiles and five samples
NOTES = {}


def note(key, value):
    NOTES[key] = max(NOTES.get(key, 0.0), float(value))
    print('%s: %.6g' % (key, value))


@functools.lru_cache(maxsize=None)
def plan_for(name):
    from audian_amd import hipdsp
    return hipdsp.SosPlan(gh.ctx(), (pd.design if name in pd.FILTERS else pd.long_design)(name)[0])


def run(plan, x, first=0, step=1, n_out=None, gain=1.0, root=False, c=None, x_slack=3, y_slack=5, x_base=1, y_base=3,
        expect=None):
    """hipdsp_power_envelope of the (T, lanes) float32 array x: (n_out, lanes) float32.  `expect`: the exception the call
    must raise; the whole output must then be untouched and None is returned."""
    from audian_amd import hipdsp
    c = gh.ctx() if c is None else c
    x = np.ascontiguousarray(x, dtype=np.float32)
    T, C = x.shape
    if n_out is None:
        n_out = pd.grid_size(T, first, step)
    x_pitch, y_pitch = T + x_slack, max(n_out, 0) + y_slack
    hx = np.full(x_base + C*x_pitch + 1, 1.0e6, dtype=np.float32)
    for k in range(C):
        hx[x_base + k*x_pitch:x_base + k*x_pitch + T] = x[:, k]
    dx = hipdsp.DeviceArray.from_host(c, hx)
    guard = 64
    ny = guard + y_base + C*y_pitch + guard
    dy = hipdsp.DeviceArray(c, (ny,), np.float32)
    hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(dy), SENTINEL_BYTE, dy.nbytes)
    try:
        if expect is not None:
            with pytest.raises(expect):
                hipdsp.power_envelope(c, plan, dx.view(x_base, (1,)), x_pitch, C, T, dy.view(guard + y_base, (1,)), y_pitch,
                                      first, step, n_out, gain, root)
        else:
            hipdsp.power_envelope(c, plan, dx.view(x_base, (1,)), x_pitch, C, T, dy.view(guard + y_base, (1,)), y_pitch,
                                  first, step, n_out, gain, root)
        raw = dy.to_host()
    finally:
        dx.free()
        dy.free()
    written = np.zeros(ny, dtype=bool)
    if expect is None:
        for k in range(C):
            a = guard + y_base + k*y_pitch
            written[a:a + n_out] = True
    assert np.all(raw[~written].view(np.uint8) == SENTINEL_BYTE), 'an element outside the output rows was written'
    if expect is not None:
        return None
    rows = raw[guard + y_base:guard + y_base + C*y_pitch].reshape(C, y_pitch)[:, :n_out]
    return np.ascontiguousarray(rows.T)


def judge(got, ref, q, what):
    """The call clamps; the bound is the unclamped reference's.  A positive result must lie within its window's allowance
    of the reference; a zero is the clamp of SOME value within the allowance of the reference (exact zeros wherever the
    reference is negative by more than that; no zero where it is positive by more).  Returns the worst ratio."""
    assert got.dtype == np.float32 and got.shape == ref.shape and np.all(got >= 0), what
    unclamped = np.where(got > 0, got.astype(ib.LD), np.minimum(ref, ib.LD(0)))
    return ib.assert_within(unclamped, ref, q, what)


# ---- accuracy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(pd.FILTERS))
def test_every_window_within_the_bound(name):
    sos, rate, fams = pd.design(name)
    x = ib.families(list(fams), T_CASE, rate)
    ref, q = pd.case(sos, x)
    ib.assert_in_range(ref, name)
    assert np.all(q <= ib.Q_CAP)
    got = run(plan_for(name), x)
    note('worst window ratio, ' + name, judge(got, ref, q, name))
    negative = ref < -(1.0 + ib.MARGIN*np.max(q))*ib.ULP*np.max(np.abs(ref))
    assert np.all(got[negative] == 0)


# ---- rows longer than the filter's memory -------------------------------------------------------------------------------

@pytest.mark.parametrize('name,frames', [(name, frames) for name in pd.LONG_FILTERS for frames in pd.long_rows(name)])
def test_long_rows_within_the_bound(name, frames):
    """Rows whose tiles' entering states come through every power of pe_carry's ladder: 6, 10 and 18 tiles of a two-section
    plan (P[8], P[9], P[10]; E one before, on and one behind a multiple of 4096) and 131 tiles of a one-section plan (P[6] ...
    P[12], three steps of pe_carry's loop, the last one ragged), which tests/test_power_envelope_host.py shows to catch each
    of them.  Every window under the same bound.  The device takes milliseconds; the 131-tile case takes 15 s on the CPU for
    its longdouble reference and float64 run (shared with the grid test below), the others 1 to 5 s."""
    sos, rate, fams = pd.long_design(name)
    x = ib.families(list(fams), frames, rate)
    ref, q = pd.case(sos, x)
    what = '%s, %d frames' % (name, frames)
    ib.assert_in_range(ref, what)
    assert np.all(q <= ib.Q_CAP)
    assert frames in pd.long_rows(name) and pd.tiles_of(sos, frames) in (6, 10, 18, 131)
    got = run(plan_for(name), x)
    note('worst window ratio, %s, %d tiles' % (name, pd.tiles_of(sos, frames)), judge(got, ref, q, what))


def test_long_grid_is_exact():
    """The 131-tile row on a grid (step > 1, first > 0, root = 1): the full-rate result picked on the grid, byte for byte,
    and that full-rate result is the root of the power that test_long_rows_within_the_bound judges."""
    sos, rate, fams = pd.long_design(pd.LONG)
    x = ib.families(list(fams), pd.T_ROW, rate)
    plan = plan_for(pd.LONG)
    full = run(plan, x, gain=1.0, root=True)
    assert full.shape == x.shape
    assert full.tobytes() == np.sqrt(run(plan, x)).tobytes()
    for step, first in ((19, 7), (4097, 4099)):
        n_max = pd.grid_size(pd.T_ROW, first, step)
        for n_out in (n_max, n_max - 1):
            got = run(plan, x, first, step, n_out, gain=1.0, root=True)
            assert got.tobytes() == np.ascontiguousarray(full[first::step][:n_out]).tobytes(), (step, first, n_out)


# ---- lengths ----------------------------------------------------------------------------------------------------------

def lengths(edge):
    out = {edge + 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, T_CASE}
    out |= set(range(4096 - edge - 1, 4096 + 2))
    # the kernel's own borders: the EXTENDED sequence (frames + 2 padlen) is cut every 64 and every 4096 samples
    for border in (CHUNK, 2*CHUNK, TILE, 2*TILE):
        out |= {border - 2*edge + d for d in (-1, 0, 1)}
    return sorted(n for n in out if n > edge)


@pytest.mark.parametrize('name', ['lp1 500 Hz @ 96 kHz', 'lp4 300 Hz @ 48 kHz'])
def test_lengths(name):
    from audian_amd import hipdsp
    assert (CHUNK, TILE) == (hipdsp.POWER_ENVELOPE_CHUNK, hipdsp.POWER_ENVELOPE_TILE)
    sos, rate, fams = pd.design(name)
    edge = ib.padlen(sos)
    plan = plan_for(name)
    for T in lengths(edge):
        x = ib.families(['burst', 'offset'], T, rate)
        ref, q = pd.case(sos, x)
        got = run(plan, x)
        note('worst window ratio over the lengths, ' + name, judge(got, ref, q, '%s, %d frames' % (name, T)))
    x = ib.families(['burst', 'offset'], edge, rate)
    run(plan, x, expect=ValueError)
    from audian_amd import _lib
    assert 'padlen' in _lib.last_error()


# ---- the grid and the root, exact -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['lp1 500 Hz @ 96 kHz', 'lp3 200 Hz @ 44.1 kHz'])
def test_grid_is_exact(name):
    sos, rate, fams = pd.design(name)
    x = ib.families(['burst', 'stepup'], T_CASE, rate)
    plan = plan_for(name)
    full = run(plan, x, gain=4.0, root=True)
    assert full.shape == x.shape
    for step in (2, 19, 48, 4097):
        for first in (0, 1, step - 1, 4099):
            n_max = pd.grid_size(T_CASE, first, step)
            assert n_max >= 2
            for n_out in (n_max, n_max - 1):
                got = run(plan, x, first, step, n_out, gain=4.0, root=True)
                assert got.tobytes() == np.ascontiguousarray(full[first::step][:n_out]).tobytes(), (step, first, n_out)
            run(plan, x, first, step, n_max + 1, gain=4.0, root=True, expect=ValueError)
    assert run(plan, x, 0, 1, 0).shape == (0, 2)                               # n_out == 0: a valid call that writes nothing
    assert run(plan, x, T_CASE - 1, 5, 1, gain=4.0, root=True).tobytes() == full[-1:].tobytes()


def test_root_is_exact():
    name = 'lp1 500 Hz @ 96 kHz'
    sos, rate, fams = pd.design(name)
    rng = np.random.default_rng(9)
    x = ib.families(['burst', 'stepdown', 'offset', 'offset', 'offset'], T_CASE, rate)
    x[:, 2] = 0.0                                                             # zero powers
    x[:, 3] = (1e-20*rng.standard_normal(T_CASE)).astype(np.float32)          # powers of 1e-40: float32 denormals
    x[:, 4] = (6e-23*rng.standard_normal(T_CASE)).astype(np.float32)          # powers around the smallest denormal
    plan = plan_for(name)
    for gain in (4.0, 0.37):
        power = run(plan, x, 0, 19, None, gain, False)
        root = run(plan, x, 0, 19, None, gain, True)
        assert root.tobytes() == np.sqrt(power).tobytes(), gain
        assert np.all(power[:, 2] == 0) and np.all(root[:, 2] == 0)
        tiny = np.float32(2.0**-126)
        assert np.any((power[:, 3] > 0) & (power[:, 3] < tiny)) and np.all(power[:, 4] < tiny)
        # and the definition's bits where it has no tie to break: one rounding of the float64 product, then the root
        want = pd.power_envelope(sos, x, 0, 19, None, gain, False, np.float64)
        assert np.mean(power == want) > 0.999


# ---- against the reference --------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden():
    return load_golden('power_envelope')


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_the_reference_through_the_call(golden, prefix):
    from audian_amd import hipdsp
    x, rate, freq = golden[prefix + 'x'], float(golden[prefix + 'rate']), float(golden[prefix + 'freq'])
    step = pd.reference_step(rate, freq)
    assert step == int(golden[prefix + 'step'])
    plan = hipdsp.SosPlan(gh.ctx(), pd.first_order_sos(freq, rate))
    got = run(plan, x, 0, step, None, 4.0, True)
    env = golden[prefix + 'envelope']
    assert got.shape == env.shape
    for k in range(x.shape[1]):
        note('golden %s rel_err, hipdsp_power_envelope' % prefix, rel_err(got[:, k], env[:, k]))
        assert rel_err(got[:, k], env[:, k]) < 1e-4
    power = run(plan, x, 0, step, None, 2.0, False)                            # the reference's edata[::step]
    for k in range(x.shape[1]):
        assert rel_err(np.sqrt(power[:, k].astype(np.float64))*np.sqrt(2.0), env[:, k]) < 1e-4


class Item:
    def isVisible(self):
        return True


def graph(x, rate, buffer_time, back_time, traces, filter_preroll=True):
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(buffer_time, back_time)
    filt = BufferedFilter()                               # wide open: the filtered trace is the recording, on the device
    if not filter_preroll:
        filt.source_tbefore = 0                           # (a pass-through needs none of its ten seconds: the buffers scroll)
    g.add_trace(filt)
    for t in traces:
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    return g


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_the_reference_through_the_facade(golden, prefix):
    from audian_amd import hipdsp
    from audian_amd.bufferedlowpass import BufferedLowpass
    from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
    x, rate, freq = golden[prefix + 'x'], float(golden[prefix + 'rate']), float(golden[prefix + 'freq'])
    env, slow = BufferedPowerEnvelope(envelope_cutoff=freq), BufferedLowpass(cutoff=float(golden['slow_cutoff']))
    g = graph(x.astype(np.float64), rate, 10.0, 0.0, [env, slow])
    before = dict(hipdsp.launches)
    g.update_times(0.0, len(x)/rate)
    assert hipdsp.launches.get('power_envelope', 0) > before.get('power_envelope', 0)           # the device path ran
    assert env.step == int(golden[prefix + 'step']) and env.rate == float(golden[prefix + 'envrate'])
    want, want_slow = golden[prefix + 'envelope'], golden[prefix + 'slow']
    got = np.asarray(env.buffer)
    # align_buffer keeps whole frames only: floor(frames / step) of them, computed from the slab that ends there -- 6
    # samples short of the recording in case a_, which the last frames see through the filter's memory (30 samples)
    assert len(got) == len(x)//env.step and len(want) - len(got) == (1 if prefix == 'a_' else 0)
    n = len(got) - (40 if len(got) < len(want) else 0)
    for k in range(x.shape[1]):
        note('golden %s rel_err, BufferedPowerEnvelope' % prefix, rel_err(got[:n, k], want[:n, k]))
        assert rel_err(got[:n, k], want[:n, k]) < 1e-4
    # the slow envelope: BufferedLowpass below the power envelope (whole where the lengths agree), and of the
    # reference's own envelope as a recording
    got_slow = np.asarray(slow.buffer)
    assert got_slow.shape == got.shape
    if len(got) == len(want):
        for k in range(x.shape[1]):
            note('golden %s rel_err, BufferedLowpass below BufferedPowerEnvelope' % prefix, rel_err(got_slow[:, k], want_slow[:, k]))
            assert rel_err(got_slow[:, k], want_slow[:, k]) < 1e-4
    low = BufferedLowpass(source='filtered', cutoff=float(golden['slow_cutoff']))
    g = graph(want, env.rate, 10.0, 0.0, [low])
    before = hipdsp.launches.get('envelope', 0)
    g.update_times(0.0, len(want)/env.rate)
    assert hipdsp.launches.get('envelope', 0) > before
    got_slow = np.asarray(low.buffer)
    assert got_slow.shape == want_slow.shape
    for k in range(x.shape[1]):
        note('golden %s rel_err, BufferedLowpass' % prefix, rel_err(got_slow[:, k], want_slow[:, k]))
        assert rel_err(got_slow[:, k], want_slow[:, k]) < 1e-4


# ---- determinism and isolation ------------------------------------------------------------------------------------------

def test_a_row_depends_on_itself_alone():
    name = 'lp4 300 Hz @ 48 kHz'
    sos, rate, fams = pd.design(name)
    x = ib.families(['burst', 'stepdown', 'offset', 'stepup', 'burst'], T_CASE, rate)
    x[:, 4] *= np.float32(0.37)
    plan = plan_for(name)
    args = dict(first=1, step=19, gain=4.0, root=True)
    among = run(plan, x, x_slack=77, y_slack=13, x_base=3, y_base=1, **args)
    assert run(plan, x, x_slack=77, y_slack=13, x_base=3, y_base=1, **args).tobytes() == among.tobytes()
    for k in range(5):
        alone = run(plan, x[:, k:k + 1], x_slack=0, y_slack=0, x_base=0, y_base=0, **args)
        assert alone[:, 0].tobytes() == among[:, k].tobytes(), k
    # a NaN or an infinity turns its row NaN throughout and leaves the other rows' bits alone
    edge = ib.padlen(sos)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, T_CASE - 1, TILE - edge, TILE - edge - 1, 2*TILE + 1234):       # (TILE - edge: first sample of tile 1)
            y = x.copy()
            y[at, 1] = bad
            got = run(plan, y, **args)
            assert np.all(np.isnan(got[:, 1])), (bad, at)
            keep = [0, 2, 3, 4]
            assert got[:, keep].tobytes() == among[:, keep].tobytes(), (bad, at)


def test_context_state_does_not_reach_the_result():
    from audian_amd import hipdsp
    name = 'lp3 200 Hz @ 44.1 kHz'
    sos, rate, fams = pd.design(name)
    x = ib.families(['burst', 'stepdown', 'offset'], T_CASE, rate)
    ref, q = pd.case(sos, x)
    outs = []
    for fill in (0x00, 0xff, None):
        c = hipdsp.Context(0)
        plan = hipdsp.SosPlan(c, sos)
        if fill is not None:
            c.set_option('scratch_fill', fill + 1)
        outs.append(run(plan, x, c=c))
        judge(outs[-1], ref, q, '%s, scratch_fill %r' % (name, fill))
        # a refused call changes nothing
        run(plan, x, 0, 7, pd.grid_size(T_CASE, 0, 7) + 1, c=c, expect=ValueError)
        run(plan, x, 0, 0, 1, c=c, expect=ValueError)
        run(plan, x, 0, 1, None, -1.0, c=c, expect=ValueError)
        assert run(plan, x, c=c).tobytes() == outs[-1].tobytes()
        c.set_option('scratch_fill', 0)
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_refusals():
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = gh.ctx()
    name = 'lp1 500 Hz @ 96 kHz'
    x = ib.families(['burst'], 300, 96000.0)
    plan = plan_for(name)
    for kwargs in (dict(step=0, n_out=1), dict(first=-1, n_out=1), dict(first=300, n_out=1), dict(gain=0.0), dict(gain=np.inf),
                   dict(gain=np.nan), dict(y_slack=-1)):
        run(plan, x, expect=ValueError, **kwargs)
    run(None, x, expect=ValueError)
    run(hipdsp.SosPlan(c, butter_sos(6, 500.0, 'lowpass', 96000.0)), x, expect=NotImplementedError)
    dx = hipdsp.DeviceArray.from_host(c, np.zeros(1000, dtype=np.float32))
    with pytest.raises(ValueError):                                          # y overlapping x
        hipdsp.power_envelope(c, plan, dx, 300, 1, 300, dx.view(100, (1,)), 300)
    with pytest.raises(ValueError):                                          # misaligned
        hipdsp.power_envelope(c, plan, hipdsp.DeviceArray(c, (1,), np.float32, ptr=dx.ptr + 2), 300, 1, 300,
                              dx.view(500, (1,)), 300)
    with pytest.raises(ValueError):                                          # pitch smaller than the row
        hipdsp.power_envelope(c, plan, dx, 299, 2, 300, dx.view(700, (1,)), 300, 0, 19)
    assert np.all(dx.to_host() == 0)
    dx.free()


# ---- rows past element 2^31 -------------------------------------------------------------------------------------------

def test_far_rows():
    """Five rows 2^29 + 2^19 elements apart in x and in y, the pointers in the middle of a NaN-filled and a sentinel-filled
    block (tests/test_gpu_far_indices.py): every row equals the near placement bit for bit."""
    import far_placement as fp
    from test_gpu_far_indices import Far, placed
    name = 'lp4 300 Hz @ 48 kHz'
    sos, rate, fams = pd.design(name)
    v = ib.families(['burst'], T_CASE, rate)
    near = run(plan_for(name), v, 1, 3, None, 4.0, True)[:, 0]
    n_out = len(near)
    guard = 64
    windows = fp.by_row(T_CASE, guard)
    far = Far()
    try:
        from audian_amd import hipdsp
        A = fp.IN_ROW + fp.PHASE
        with placed(far, windows, v[:, 0]):
            y = far.out_rows(np.float32, fp.ROW_PITCH, fp.ROWS, n_out, A)
            hipdsp.power_envelope(far.ctx, plan_for(name), far.X(A), fp.ROW_PITCH, fp.ROWS, T_CASE, y, fp.ROW_PITCH,
                                  1, 3, n_out, 4.0, True)
            got = far.rows(np.float32, fp.ROW_PITCH, fp.ROWS, n_out, base=A)
        for k in range(fp.ROWS):
            assert got[k].tobytes() == near.tobytes(), 'row %d differs from the near placement' % k
    finally:
        far.free()


# ---- the facade -------------------------------------------------------------------------------------------------------

def test_facade_random_walk_against_the_host_twin():
    from audian_amd import hipdsp
    from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope, power_envelope_host

    class HostTwin(BufferedPowerEnvelope):
        def process(self, source, dest, nbefore):
            self._pending = None
            dest[...] = power_envelope_host(self.sos, np.asarray(source[:]), nbefore, self.step, len(dest), self.gain, self.root)

    rate = 4000.0
    rng = np.random.default_rng(23)
    n = int(20*rate) + 3
    x = rng.standard_normal((n, 2))*(1.0 + np.sin(2*np.pi*0.7*np.arange(n)/rate))[:, None]
    dev, twin = BufferedPowerEnvelope(envelope_cutoff=50.0), HostTwin(name='twin', envelope_cutoff=50.0)
    g = graph(x, rate, 3.0, 1.0, [dev, twin], filter_preroll=False)
    assert dev.step == 8 and g.tbefore == 1
    launches = hipdsp.launches.get('power_envelope', 0)

    def compare():
        a, b = np.asarray(dev.buffer), np.asarray(twin.buffer)
        assert a.shape == b.shape and dev.offset == twin.offset and dev.rate == twin.rate and len(a) > 0
        for k in range(2):
            assert rel_err(a[:, k], b[:, k]) < 1e-4
        return a.copy()

    seen, moves = {}, []
    t = 0.0
    for move in range(8):
        t = float(np.clip(t + rng.uniform(-2.0, 6.0), 0.0, 17.0))
        g.update_times(t, t + 2.5)
        buf = compare()
        kept = [j for j in range(dev.offset, dev.offset + len(buf)) if j in seen]
        for j in kept:
            assert np.array_equal(seen[j], buf[j - dev.offset]), (move, j)
        seen = {dev.offset + i: buf[i] for i in range(len(buf))}
        moves.append((dev.offset, len(kept), hipdsp.launches['power_envelope']))
        if move in (2, 5):
            cutoff, step = ((100.0, None), (50.0, 5))[move == 5]
            dev.update(envelope_cutoff=cutoff, step=step)
            twin.update(envelope_cutoff=cutoff, step=step)
            assert dev.step == (4 if move == 2 else 5)
            compare()
            seen = {}
    print(moves)
    assert len({m[0] for m in moves}) >= 4 and sum(m[1] > 0 for m in moves) >= 2        # the buffer scrolled, frames stayed
    assert hipdsp.launches.get('power_envelope', 0) >= launches + 6                    # and the device computed the strips


def planted(rate, seconds, songs, rng, floor=0.01):
    """(frames, 2) float64: a noise floor and, per (channel, t0, t1), a 4 kHz carrier modulated at 40 Hz, 30 dB over it."""
    n = int(seconds*rate)
    t = np.arange(n)/rate
    x = floor*rng.standard_normal((n, 2))
    song = floor*10**1.5*np.sqrt(2.0)*(1.0 + np.cos(2*np.pi*40.0*t))*np.sin(2*np.pi*4000.0*t)
    for k, t0, t1 in songs:
        i0, i1 = int(t0*rate), int(t1*rate)
        x[i0:i1, k] += song[i0:i1]
    return x


def test_detect_songs():
    from audian_amd.bufferedlowpass import BufferedLowpass
    from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
    from audian_amd.spectra import event_nfft, welch_nfft
    rate = 48000.0
    rng = np.random.default_rng(31)
    songs = [(0, 4.0, 6.0), (1, 11.0, 13.0), (0, 20.0, 22.0)]
    x = planted(rate, 30.0, songs, rng)
    x[int(14.0*rate):, 1] = 0.0                                  # silence in channel 1 behind its song
    env, slow = BufferedPowerEnvelope(envelope_cutoff=500.0), BufferedLowpass(cutoff=2.0)
    g = graph(x, rate, 60.0, 0.0, [env, slow])
    g.update_times(0.0, 30.0)
    assert env.step == 10 and env.rate == 4800.0 and slow.rate == 4800.0 and len(slow.buffer) == env.frames
    events, freqs, thresholds = g.detect_songs('power-envelope', 'slow-envelope', min_duration=0.5, peak_thresh=10.0)
    thr = g.event_thresholds('slow-envelope', 0.0, method='histogram')
    ev = g.detect_events('slow-envelope', thr, min_gap=0.5, min_duration=0.5)
    fr = g.event_peak_freqs(ev, 'power-envelope', thresh=10.0)
    ev, fr = g.clean_event_freqs(ev, fr)
    kept = [ev.frames(k) for k in range(2)]
    ev = g.refine_events(ev, fr, thr, trace_name='power-envelope', min_duration=0.5, min_thresh_fac=1.0)
    assert np.asarray(thresholds).tobytes() == np.asarray(thr).tobytes()
    for k in range(2):
        assert np.array_equal(events.frames(k), ev.frames(k))
        assert np.asarray(freqs[k]).tobytes() == np.asarray(fr[k]).tobytes()
    full = welch_nfft(env.rate, 1.0)
    for k in range(2):
        mine = [(t0, t1) for ch, t0, t1 in songs if ch == k]
        found = events.frames(k)/events.rate
        assert len(found) == len(mine), (k, found)
        for (t0, t1), (a, b) in zip(mine, found):                # one event per planted song, none elsewhere
            assert a < t1 and b > t0, (k, found)
        assert len(freqs[k]) == len(kept[k]) == len(mine) and not np.any(np.isnan(freqs[k]))
        for f, (a, b) in zip(freqs[k], kept[k]):
            nfft = event_nfft(b - a, full)
            assert abs(f - 40.0) <= env.rate/nfft, (k, f, nfft)


def test_zz_figures():
    """The figures DESIGN 5.3j quotes, printed once (python -m pytest -s)."""
    for key in sorted(NOTES):
        print('%-70s %.6g' % (key, NOTES[key]))
