"""hipdsp_fir_bank, FirPlan and BufferedKernelFilter on the GPU.  The comparator is the definition written out in numpy
(fir_definition.py: int64 where the contract promises exactness, float64 under the header's bound elsewhere) -- never
the code under test."""

import numpy as np
import pytest

import gpu_helpers as gh
from fir_definition import fir_bound, fir_definition

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-123456.75)    # no exact case reaches it (|sum| <= 64*4097 + 8), no bounded case comes near


def run(x, plan, first, step, n_out, rectify=False, strided=True):
    """hipdsp_fir_bank on a host slab x (C, frames) under `plan`: returns (K, C, n_out) float32.  The output block is
    filled with a sentinel first: every value must be written and nothing else touched.  strided: odd base offsets and
    non-compact x_pitch, out_pitch, out_kernel_pitch."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, frames = x.shape
    K = plan.n_kernels
    x_off, x_pitch = (3, frames + 7) if strided else (0, frames)
    o_off, o_pitch = (5, n_out + 5) if strided else (0, n_out)
    o_kernel = C*o_pitch + (11 if strided else 0)
    host = np.full(x_off + C*x_pitch + 1, 1e30, dtype=np.float32)        # what lies between the rows must not be read
    for ch in range(C):
        host[x_off + ch*x_pitch:x_off + ch*x_pitch + frames] = x[ch]
    dx = hipdsp.DeviceArray.from_host(c, host)
    total = o_off + K*o_kernel + 3
    dout = hipdsp.DeviceArray.from_host(c, np.full(total, SENTINEL, dtype=np.float32))
    hipdsp.fir_bank(c, plan, dx.view(x_off, (1,)), x_pitch if strided else 0, C, frames, first, step, n_out,
                    dout.view(o_off, (1,)), rectify=rectify, out_pitch=o_pitch if strided else 0,
                    out_kernel_pitch=o_kernel if strided else 0)
    flat = dout.to_host()
    dx.free()
    dout.free()
    written = np.zeros(total, dtype=bool)
    out = np.empty((K, C, n_out), dtype=np.float32)
    for k in range(K):
        for ch in range(C):
            a = o_off + k*o_kernel + ch*o_pitch
            out[k, ch] = flat[a:a + n_out]
            written[a:a + n_out] = True
    assert np.all(flat[~written] == SENTINEL), 'written outside the rows'
    assert not np.any(out == SENTINEL), 'values left unwritten'
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. exact ------------------------------------------------------------------------------------------------------

TAPS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097]
KERNELS = [1, 2, 15, 16]
STEPS = [1, 2, 3, 7, 96, 1000]
CHANNELS = [1, 3, 64]
MACS = 3e7                           # int64 multiply-adds of the comparator per case: keeps a case well under a second


def frames_of(L):
    return sorted({f for f in (1, 2, L - 1, L, L + 1, 1023, 1024, 1025, 12305) if f >= 1})


def firsts_of(frames):
    return sorted({0, 1, 5, frames - 1, frames + 3})


def n_out_of(L, K, step, frames, first, C, cap=True):
    """Outputs up to three past the end of the trace, at least two, as many as the comparator's budget allows.
    The budget cuts the sampled cases with large L*K*C to a handful of outputs (L 4097, K 16, C 64: 7), so several
    tiles of a long kernel are covered by the C = 1 corners; in the window layout a second tile never holds real
    samples within 20 000 frames (256 outputs x 212 samples at least): its tiles past the first see zeros only."""
    n = max(2, -(-(frames + 3 - first)//step))
    return max(1, min(n, int(MACS/(C*L*K)))) if cap else n


# (L, K, step, frames, first, C, n_out or None): ends of every range, all tiles of a long trace per layout, both sides of
# the sizes at which the launch changes its tile (255*68 + L4, 63*275 + L4 against 17408 floats) or its layout
CORNERS = [
    (1, 1, 1, 1, 0, 1, 1), (1, 16, 1, 1, 4, 1, 3), (2, 1, 1, 1, 0, 1, 2), (4097, 16, 1, 1, 0, 1, 5),
    (4097, 16, 1, 12305, 0, 1, 2300), (4097, 1, 1, 12305, 11000, 3, 700), (4096, 15, 1, 4095, 0, 1, 1200),
    (1025, 16, 1, 12305, 0, 1, None), (257, 16, 1, 12305, 5, 3, None), (65, 16, 1, 12305, 0, 3, None),
    (9, 16, 1, 12305, 1, 64, 3000), (3, 2, 1, 12305, 12304, 3, 9), (16, 15, 1, 1025, 1028, 3, 4),
    (257, 16, 2, 12305, 1, 3, None), (257, 16, 3, 12305, 0, 1, None), (63, 2, 7, 12305, 5, 3, None),
    (257, 16, 96, 12305, 0, 3, None), (4097, 16, 96, 12305, 5, 1, None), (1024, 15, 96, 12305, 1, 3, None),
    (257, 16, 1000, 12305, 0, 3, None), (4097, 2, 1000, 12305, 1, 1, None), (5, 1, 1000, 12305, 12308, 64, 2),
    (65, 16, 68, 20000, 0, 1, None), (69, 16, 68, 20000, 0, 1, None),
    (80, 16, 275, 20000, 0, 1, None), (84, 16, 275, 20000, 0, 1, None), (84, 3, 276, 20000, 7, 3, None),
    (257, 16, 1000, 12305, 0, 1, 600), (9, 2, 300, 20000, 3, 1, 300),
    (17, 16, 200, 20000, 0, 3, None), (4097, 16, 200, 20000, 0, 1, None), (4097, 16, 210, 20000, 3, 1, None),
]


def sampled_cases():
    rng = np.random.default_rng(20260)
    cases = []
    while len(cases) < 240:
        L, K = int(rng.choice(TAPS)), int(rng.choice(KERNELS))
        step, C = int(rng.choice(STEPS)), int(rng.choice(CHANNELS))
        frames = int(rng.choice(frames_of(L)))
        first = int(rng.choice(firsts_of(frames)))
        cases.append((L, K, step, frames, first, C, None))
    return cases


EXACT = CORNERS + sampled_cases()
PER_TEST = 27


def exact_case(case, rectify):
    from audian_amd import hipdsp
    L, K, step, frames, first, C, n_out = case
    rng = np.random.default_rng(list(case[:6]) + [int(rectify)])
    if n_out is None:
        n_out = n_out_of(L, K, step, frames, first, C)
    x = rng.integers(-8, 9, (C, frames))
    taps = rng.integers(-8, 9, (K, L))
    taps[:, 0] = rng.choice([-8, -3, 5, 8], K)            # the first and the last tap are never zero:
    taps[:, -1] = rng.choice([-7, -1, 2, 8], K)           # a dropped end tap shows
    thr = rng.integers(-40, 41, K) if rectify else None
    want = fir_definition(x, taps, first, step, n_out)
    assert want.dtype == np.int64 and np.max(np.abs(want), initial=0) < 1 << 24
    if rectify:
        want = np.maximum(want - thr[:, None, None], 0)
    plan = hipdsp.FirPlan(gh.ctx(), taps, thr)
    got = run(x.astype(np.float32), plan, first, step, n_out, rectify=rectify)
    plan.close()
    bad = np.argwhere(got != want.astype(np.float32))
    assert bad.size == 0, 'L %d K %d step %d frames %d first %d C %d n_out %d rectify %d: %d wrong, first at %s got %r want %r' % (
        L, K, step, frames, first, C, n_out, rectify, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('rectify', [False, True])
@pytest.mark.parametrize('part', range(-(-len(EXACT)//PER_TEST)))
def test_integers_are_exact(part, rectify):
    """Integer samples and taps in [-8, 8]: |sum| <= 64*4097 < 2^24, every output equals the int64 definition bit for
    bit, linear and rectified with integer thresholds."""
    assert len(EXACT) >= 200 + len(CORNERS)
    for case in EXACT[part*PER_TEST:(part + 1)*PER_TEST]:
        exact_case(case, rectify)


def test_the_cases_cover_the_lists():
    for j, values in enumerate((TAPS, KERNELS, STEPS)):
        assert {c[j] for c in EXACT} >= set(values)
    assert {c[5] for c in EXACT} >= set(CHANNELS)
    kinds_f, kinds_0 = set(), set()
    for L, K, step, frames, first, C, n_out in EXACT:
        kinds_f |= {name for name, f in (('1', 1), ('2', 2), ('L-1', L - 1), ('L', L), ('L+1', L + 1), ('1023', 1023),
                                         ('1024', 1024), ('1025', 1025), ('12305', 12305)) if f == frames}
        kinds_0 |= {name for name, f in (('0', 0), ('1', 1), ('5', 5), ('frames-1', frames - 1),
                                         ('frames+3', frames + 3)) if f == first}
    assert len(kinds_f) == 9 and len(kinds_0) == 5


# ---- 2. tap rounding ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L, step', [(1, 1), (6, 1), (64, 1), (257, 1), (257, 3), (4097, 1)])
def test_taps_are_rounded_to_float32_once(L, step):
    """Unit impulses: the output is exactly float32(h) laid around each impulse."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(L)
    frames, C, K = min(5*L + 3000, 20000), 2, 3
    x = np.zeros((C, frames), dtype=np.float32)
    room = (frames - 2*L - 100)//(L + 7)                                # interior places more than L apart
    inner = L + 50 + np.sort(rng.choice(room, min(3, room), replace=False))*(L + 7)
    assert len(inner) >= 2
    for ch in range(C):
        x[ch, [0, frames - 1]] = 1.0
        x[ch, inner + ch] = 1.0
    taps = rng.standard_normal((K, L))*np.exp(rng.uniform(-20, 20, (K, L)))
    n_out = -(-frames//step)
    plan = hipdsp.FirPlan(gh.ctx(), taps)
    got = run(x, plan, 0, step, n_out)
    plan.close()
    # one non-zero product per output: float64 holds float32(h) * 1 exactly
    want = fir_definition(x.astype(np.float64), taps.astype(np.float32).astype(np.float64), 0, step, n_out)
    assert np.count_nonzero(want) > 0
    assert np.array_equal(got, want.astype(np.float32))


# ---- 3. the bound ---------------------------------------------------------------------------------------------------------

def bound_taps(L, K, rng):
    from audian_amd.design import gabor_kernels
    sigma = {65: 0.008, 257: 0.032, 4097: 0.512}.get(L)
    if sigma is None:
        return rng.standard_normal((K, L))
    taps = gabor_kernels(1000.0, sigma, np.linspace(5.0, 400.0, K), phase=0.3)
    assert taps.shape == (K, L)
    return taps


@pytest.mark.parametrize('step', [1, 5])
@pytest.mark.parametrize('L, K', [(3, 1), (65, 5), (257, 16), (1025, 3), (4097, 16)])
def test_every_output_is_within_the_bound(L, K, step):
    """Uniform [-1, 1) samples, Gabor and random taps: |out - y_float64| <= n u / (1 - n u) * sum |h| |x| per output,
    n = L + 2; rectified: (n + 1) u / (1 - (n + 1) u) * (sum |h| |x| + |threshold|)."""
    from audian_amd import hipdsp
    rng = np.random.default_rng([L, K, step])
    C, frames = 2, 12000
    x = rng.uniform(-1.0, 1.0, (C, frames)).astype(np.float32)
    taps = bound_taps(L, K, rng)
    n_out = -(-frames//step)
    y, m = fir_definition(x.astype(np.float64), taps, 0, step, n_out, with_abs=True)
    thr = 0.1*rng.uniform(-1.0, 1.0, K)*np.sqrt(np.sum(taps**2, axis=1))
    plan = hipdsp.FirPlan(gh.ctx(), taps, thr)
    for rectify in (False, True):
        got = run(x, plan, 0, step, n_out, rectify=rectify).astype(np.float64)
        want = np.maximum(y - thr[:, None, None], 0.0) if rectify else y
        bound = fir_bound(m, L, thr[:, None, None] if rectify else None)
        err = np.abs(got - want)
        worst = np.max(err/np.maximum(bound, 1e-300))
        print('L %d K %d step %d rectify %d: worst error %.3g of the bound' % (L, K, step, rectify, worst))
        assert np.all(err <= bound), (rectify, worst)
        if rectify:
            assert np.any(got == 0) and np.any(got > 0) and np.all(got >= 0)
    plan.close()


# ---- 4. independence and determinism --------------------------------------------------------------------------------------

@pytest.mark.parametrize('L, step', [(9, 1), (257, 1), (4097, 1), (257, 7), (257, 96), (63, 200), (257, 1000)])
def test_kernels_do_not_depend_on_their_neighbours(L, step):
    from audian_amd import hipdsp
    rng = np.random.default_rng([L, step])
    C, frames = 3, 12000 if step < 96 else 20000
    x = rng.uniform(-1.0, 1.0, (C, frames)).astype(np.float32)
    taps = rng.standard_normal((16, L))
    thr = rng.uniform(-0.5, 0.5, 16)
    n_out = -(-frames//step)
    plan = hipdsp.FirPlan(gh.ctx(), taps, thr)
    for rectify in (False, True):
        bank = run(x, plan, 2, step, n_out, rectify=rectify)
        again = run(x, plan, 2, step, n_out, rectify=rectify, strided=False)
        assert np.array_equal(bits(bank), bits(again))                  # the same bits twice, whatever the layout
        one = hipdsp.FirPlan(gh.ctx())
        for k in range(16):
            one.set(taps[k:k + 1], thr[k:k + 1])                        # a new set between two calls takes effect
            single = run(x, one, 2, step, n_out, rectify=rectify)
            assert np.array_equal(bits(single[0]), bits(bank[k])), k
        one.close()
    assert len({bank[k].tobytes() for k in range(16)}) == 16
    plan.close()


def test_a_plan_that_shrinks_and_grows_is_a_fresh_plan():
    """One FirPlan set to the largest bank, the smallest and one in between, thresholds on the first and the last only:
    after each set the traces, linear and rectified, at step 1 and at step 96, have the bits a newly created plan
    gives -- no tap or threshold of the bank before is left in the staged block (the host block is cleared up to
    the larger of the old and new sizes, the upload copies the new prefix over a device block that began as zeros)."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(20261021)
    C, frames = 2, 700
    x = rng.uniform(-1.0, 1.0, (C, frames)).astype(np.float32)
    plan = hipdsp.FirPlan(gh.ctx())
    for K, L, thresholds in ((16, 4097, True), (1, 3, False), (5, 257, True)):
        taps = rng.standard_normal((K, L))
        thr = rng.uniform(-0.5, 0.5, K) if thresholds else None
        plan.set(taps, thr)
        fresh = hipdsp.FirPlan(gh.ctx(), taps, thr)
        for step in (1, 96):
            n_out = -(-frames//step)
            for rectify in (False, True):
                got = run(x, plan, 0, step, n_out, rectify=rectify)
                want = run(x, fresh, 0, step, n_out, rectify=rectify)
                assert np.array_equal(bits(got), bits(want)), (K, L, step, rectify)
        fresh.close()
    plan.close()


# ---- 5. non-finite samples --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L, step', [(9, 1), (258, 1), (257, 3), (63, 1000)])
@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_non_finite_samples_stay_local(L, step, value):
    from audian_amd import hipdsp
    rng = np.random.default_rng(L)
    C, frames = 3, 6000
    x = rng.uniform(-1.0, 1.0, (C, frames)).astype(np.float32)
    taps = rng.standard_normal((4, L))
    taps[np.abs(taps) < 0.05] = 0.05                                    # no tap rounds a product with inf away
    n_out = -(-frames//step)
    plan = hipdsp.FirPlan(gh.ctx(), taps)
    clean = run(x, plan, 0, step, n_out)
    t = step*np.arange(n_out)
    lead = (L - 1)//2
    for p in (0, frames//2 + 1, frames - 1):
        bad = x.copy()
        bad[1, p] = value
        got = run(bad, plan, 0, step, n_out)
        assert np.array_equal(bits(got[:, 0]), bits(clean[:, 0])) and np.array_equal(bits(got[:, 2]), bits(clean[:, 2]))
        lo, hi = t + lead - (L - 1), t + lead                           # the window of output t
        inside = (lo <= p) & (p <= hi)
        clear = (p < lo - 16) | (p > hi + 16)
        assert np.all(~np.isfinite(got[:, 1, inside]))
        assert np.array_equal(bits(got[:, 1, clear]), bits(clean[:, 1, clear]))
        assert np.any(clear) and (np.any(inside) or step > 1)
    plan.close()


# ---- 6. errors and empties ------------------------------------------------------------------------------------------------

def test_errors_and_empties():
    from audian_amd import hipdsp, _lib
    c = gh.ctx()
    plan = hipdsp.FirPlan(c)
    d = hipdsp.DeviceArray.from_host(c, np.arange(64, dtype=np.float32))
    o = hipdsp.DeviceArray.from_host(c, np.full(256, SENTINEL, dtype=np.float32))
    with pytest.raises(ValueError):                                     # no taps yet
        hipdsp.fir_bank(c, plan, d, 0, 1, 64, 0, 1, 64, o)
    with pytest.raises(ValueError):
        plan.upload()
    with pytest.raises(NotImplementedError):
        plan.set(np.ones((17, 3)))
    with pytest.raises(NotImplementedError):
        plan.set(np.ones((1, 4098)))
    with pytest.raises(ValueError):
        plan.set(np.ones((0, 3)))
    with pytest.raises(ValueError):
        plan.set(np.ones((2, 0)))
    plan.set(np.ones((16, 4097)))                                       # the largest plan
    plan.set([[1.0, 2.0, 3.0]], [0.5])
    assert (plan.n_kernels, plan.n_taps) == (1, 3)
    plan.set_host(np.ones((2, 5)))                                      # new counts that were never uploaded
    with pytest.raises(ValueError):
        hipdsp.fir_bank(c, plan, d, 0, 1, 64, 0, 1, 64, o)
    plan.upload()
    hipdsp.fir_bank(c, plan, d, 0, 1, 64, 0, 1, 64, o)
    assert np.all(o.to_host()[:128] != SENTINEL)
    o.copy_from_host(np.full(256, SENTINEL, dtype=np.float32))
    plan.set([[1.0, 2.0, 3.0]], [0.5])
    rc = _lib.lib.hipdsp_fir_bank(c.handle, None, hipdsp._p(d), 0, 1, 64, 0, 1, 64, 0, hipdsp._p(o), 0, 0)
    assert rc == _lib.ERR_INVALID                                       # plan == NULL
    for kwargs in (dict(first=-1), dict(step=0), dict(step=-2), dict(frames=-1), dict(n_out=-1), dict(channels=-1)):
        a = dict(channels=1, frames=64, first=0, step=1, n_out=64)
        a.update(kwargs)
        with pytest.raises(ValueError):
            hipdsp.fir_bank(c, plan, d, 0, a['channels'], a['frames'], a['first'], a['step'], a['n_out'], o)
    with pytest.raises(ValueError):                                     # x and out overlap
        hipdsp.fir_bank(c, plan, d, 0, 1, 64, 0, 1, 32, d.view(40, (1,)))
    with pytest.raises(ValueError):
        hipdsp.fir_bank(c, plan, d, 0, 2, 32, 0, 1, 16, o, out_pitch=8)      # out_pitch < n_out
    assert np.all(o.to_host() == SENTINEL)
    hipdsp.fir_bank(c, plan, d, 0, 1, 64, 0, 1, 0, o)                   # n_out == 0, channels == 0: nothing written
    hipdsp.fir_bank(c, plan, d, 0, 0, 64, 0, 1, 64, o)
    assert np.all(o.to_host() == SENTINEL)
    hipdsp.fir_bank(c, plan, None, 0, 2, 0, 3, 2, 50, o)                # frames == 0: zeros ...
    got = o.to_host()
    assert np.all(got[:100] == 0) and np.all(got[100:] == SENTINEL)
    plan.set([[1.0, 2.0, 3.0]], [-0.5])
    hipdsp.fir_bank(c, plan, None, 0, 2, 0, 3, 2, 50, o, rectify=True)  # ... or rectified zeros
    got = o.to_host()
    assert np.all(got[:100] == 0.5) and np.all(got[100:] == SENTINEL)
    hipdsp.fir_bank(c, plan, d, 0, 1, 64, 1 << 40, 1 << 30, 3, o)       # far outside the trace, 64-bit indices
    assert np.all(o.to_host()[:3] == 0)
    plan.close()


# ---- 7. graph ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L, step', [(257, 1), (65, 96)])
def test_graph_replays_under_new_kernels(L, step):
    from audian_amd import hipdsp
    ctx = hipdsp.Context(0)
    stream = ctx.create_stream()
    ctx.set_stream(stream)
    rng = np.random.default_rng(L)
    C, frames, K = 3, 9000, 4
    x = rng.uniform(-1.0, 1.0, (C, frames)).astype(np.float32)
    n_out = -(-frames//step)
    dx = hipdsp.DeviceArray.from_host(ctx, x)
    dout = hipdsp.DeviceArray(ctx, (K, C, n_out), np.float32)
    eager = hipdsp.DeviceArray(ctx, (K, C, n_out), np.float32)
    plan = hipdsp.FirPlan(ctx, rng.standard_normal((K, L)), np.zeros(K))

    def chain():
        plan.upload()
        hipdsp.fir_bank(ctx, plan, dx, 0, C, frames, 0, step, n_out, dout, rectify=True)

    chain()                                                             # once outside the capture
    ctx.synchronize()
    ctx.graph_begin()
    chain()
    graph = ctx.graph_end()
    other = hipdsp.FirPlan(ctx)
    seen = set()
    for _ in range(3):
        taps, thr = rng.standard_normal((K, L)), rng.uniform(-0.3, 0.3, K)
        plan.set_host(taps, thr)                                        # host only: the captured upload carries it over
        dout.zero_()
        ctx.graph_launch(graph)
        ctx.synchronize()
        got = dout.to_host()
        other.set(taps, thr)
        hipdsp.fir_bank(ctx, other, dx, 0, C, frames, 0, step, n_out, eager, rectify=True)
        assert np.array_equal(bits(got), bits(eager.to_host()))
        assert np.any(got > 0)
        seen.add(got.tobytes())
    assert len(seen) == 3
    ctx.graph_destroy(graph)
    plan.close()
    other.close()
    ctx.set_stream(None)
    ctx.destroy_stream(stream)


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True


@pytest.mark.parametrize('step', [1, 48])
def test_kernel_filter_trace_below_the_envelope(oracle, step):
    from audian_amd import hipdsp
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedkernelfilter import BufferedKernelFilter, kernel_bank
    from audian_amd.design import gabor_kernels
    from audian_amd.tracegraph import TraceGraph
    rate, C = 48000.0, 3
    n = int(30*rate)                     # (long enough for the loader's buffer to leave the start of the recording)
    rng = np.random.default_rng(step)
    tt = np.arange(n)/rate
    x = (0.5 + 0.4*np.sin(2*np.pi*7.0*tt))[:, None]*np.sin(2*np.pi*3000.0*tt)[:, None]*np.array([1.0, 0.5, 0.1]) + \
        0.05*rng.standard_normal((n, C))
    bank = gabor_kernels(rate, 0.00125, np.linspace(0.0, 900.0, 16))
    L = bank.shape[1]
    assert L == 481
    g = TraceGraph(4.0, 1.0)
    filt, env = BufferedFilter(), BufferedEnvelope(envelope_cutoff=200.0)
    feat = BufferedKernelFilter(kernel=bank[3], step=step)
    for t in (filt, env, feat):
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for t in g.traces:
        t.plot_items = [Item() for _ in range(t.channels)]
    g.set_need_update()
    counts = {'filter': 0, 'envelope': 0}
    real_f, real_e = filt.process, env.process
    filt.process = lambda *a: (counts.__setitem__('filter', counts['filter'] + 1), real_f(*a))[1]
    env.process = lambda *a: (counts.__setitem__('envelope', counts['envelope'] + 1), real_e(*a))[1]

    def compare():
        """The whole buffer after a whole-buffer recompute: the definition on the envelope as the device holds it."""
        assert feat.rate == rate/step and feat.offset == -(-env.offset//step)
        nb = len(feat.buffer)
        assert nb == min((env.offset + len(env.buffer))//step, feat.frames) - feat.offset and nb > 0
        first = feat.offset*step - env.offset
        slab = np.asarray(env.buffer)[first:first + nb*step].astype(np.float32)
        y, m = fir_definition(slab.T.astype(np.float64), feat.kernel[None, :], 0, step, nb, with_abs=True)
        thr = feat.threshold
        want = np.maximum(y - thr, 0.0) if thr is not None else y
        err = np.abs(np.asarray(feat.buffer).T - want[0])
        assert np.all(err <= fir_bound(m[0], len(feat.kernel), thr))
        assert np.max(np.abs(want)) > 0.01

    started = hipdsp.launches.get('fir_bank', 0)
    from facade_ledger import Ledger
    ledger = Ledger(g, oracle, only=('features',))
    for t0, t1 in [(0.0, 2.0), (1.0, 3.0), (9.0, 11.0), (17.5, 19.9)]:
        g.update_times(t0, t1)
    # a scrolled state: the overlap recycled on the device, the new strip computed from a zero-extended slab at `step`
    kept = (feat.offset, len(feat.buffer))
    g.update_times(24.5, 26.5)
    assert feat.offset > kept[0] and feat.offset < kept[0] + kept[1] and ledger.stats['features']['partial'] >= 1
    ledger.check(flush=False)            # (read from the mirror: the host copy stays stale for what follows)
    ledger.close()
    assert hipdsp.launches.get('fir_bank', 0) > started and feat._stale      # the device path, not the host fallback
    seen = dict(counts)
    before = dict(hipdsp.launches)
    feat.set_kernel(bank[5])
    compare()
    feat.update(threshold=0.01)
    compare()
    assert feat.ampl_min == 0 and np.all(np.asarray(feat.buffer) >= 0)
    feat.update(threshold=None)
    # moving the kernel launched nothing for the filter or the envelope
    assert counts == seen
    after = {k: v - before.get(k, 0) for k, v in hipdsp.launches.items() if v != before.get(k, 0)}
    assert after == {'fir_bank': 3}, after
    # the whole bank in one pass equals the single-kernel traces bit for bit, where both see the same samples: at the
    # start of the recording the buffers start together, and the trace's slab ends at most step - 1 samples earlier
    g.update_times(0.0, 2.0)
    assert env.offset == 0 and feat.offset == 0
    seen = dict(counts)
    launched = hipdsp.launches['fir_bank']
    out = kernel_bank(env, bank, step=step)
    assert out.shape == (16, C, -(-len(env.buffer)//step))
    got = out.to_host()
    assert hipdsp.launches['fir_bank'] == launched + 1
    for k in range(16):
        feat.set_kernel(bank[k])
        nb = len(feat.buffer)
        keep = nb - (L//step + 2)                                       # windows that end inside the shorter slab
        assert keep > 100
        mine = feat._dev.to_host()[:, :keep]
        assert np.array_equal(bits(mine), bits(got[k][:, :keep])), k
        assert np.any(mine != 0)
    assert counts == seen
    out.free()
