"""hipdsp_template_match and TmplPlan on the GPU.  The comparator is the definition written out in np.longdouble
(template_match_definition.py) with the header's bound, derived there -- never the code under test.  The inputs are
template_match_cases.py's: 300 frames, three channels with a pitch above compact and the base one float off alignment.

Worst measured |out - definition| / bound on the MI355X over all cases of test_bound_and_nan_pattern: 0.095 for the
normalised score (shape (33, 3, 27, 7), linear), 0.986 for the raw sum (the one-tap template, dB)."""

import functools

import numpy as np
import pytest

import gpu_helpers as gh
import template_match_cases as tc
import template_match_definition as td

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-123456.75)     # no score comes near it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(spec, plan, k0, first, n_out, db=False, floor=-np.inf, pivot=0.0, min_std=0.0, strided=True):
    """hipdsp_template_match on a host slab (C, frames, nfreq) under `plan`: returns (K, C, n_out) float32.  The output
    block is filled with a sentinel first: every value must be written and nothing else touched.  strided: odd base
    offsets, NaN between the channels of the slab, non-compact pitches."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, frames, nfreq = spec.shape
    K = plan.n_templates
    per = frames*nfreq
    x_off, x_pitch = (1, per + 7) if strided else (0, per)
    o_off, o_pitch = (5, n_out + 5) if strided else (0, n_out)
    o_tmpl = C*o_pitch + (11 if strided else 0)
    host = np.full(x_off + C*x_pitch + 1, np.nan, dtype=np.float32)      # what lies between the channels must not be read
    for ch in range(C):
        host[x_off + ch*x_pitch:x_off + ch*x_pitch + per] = spec[ch].reshape(-1)
    dx = hipdsp.DeviceArray.from_host(c, host)
    total = o_off + K*o_tmpl + 3
    dout = hipdsp.DeviceArray.from_host(c, np.full(total, SENTINEL, dtype=np.float32))
    hipdsp.template_match(c, plan, dx.view(x_off, (1,)), x_pitch if strided else 0, C, frames, nfreq, k0, first, n_out,
                          dout.view(o_off, (1,)), db=db, ref_power=1.0, min_power=0.0, floor=floor, pivot=pivot,
                          min_std=min_std, out_pitch=o_pitch if strided else 0,
                          out_template_pitch=o_tmpl if strided else 0)
    flat = dout.to_host()
    dx.free()
    dout.free()
    written = np.zeros(total, dtype=bool)
    out = np.empty((K, C, n_out), dtype=np.float32)
    for k in range(K):
        for ch in range(C):
            a = o_off + k*o_tmpl + ch*o_pitch
            out[k, ch] = flat[a:a + n_out]
            written[a:a + n_out] = True
    assert np.all(flat[~written] == SENTINEL), 'written outside the rows'
    assert not np.any(out == SENTINEL), 'values left unwritten'
    return out


def device_db(spec, floor):
    """v of the dB cases: hipdsp_decibel on the same slab (ref_power 1, min_power 0), clamped on the host."""
    from audian_amd import hipdsp
    c = gh.ctx()
    d = hipdsp.DeviceArray.from_host(c, spec)
    o = hipdsp.DeviceArray(c, spec.shape, np.float32)
    hipdsp.decibel(c, d, o, spec.size, 1.0, 0.0)
    v = o.to_host()
    d.free()
    o.free()
    return np.where(v < np.float32(floor), np.float32(floor), v)


PIVOTS = {True: (-90.0, -60.0), False: (0.0, 1e-9)}           # dB: the noise level and 30 dB off it; linear: none, the floor


@functools.lru_cache(maxsize=None)
def reference(index, normalize, db):
    """The definition on case `index` for all 16 templates, computed once and shared: (slab, templates, result)."""
    shape = tc.SHAPES[index]
    nfreq, k0, Fb, Tt = shape
    spec = tc.slab(shape)
    tm = tc.templates(shape)
    if not db:
        tm = 10.0**(tm/10.0)
    v = device_db(spec, tc.FLOOR_DB) if db else spec
    taps = td.prepare(tm, normalize)[0]
    ref = td.scores(v, taps, k0, 0, tc.FRAMES - Tt + 1, normalize, tc.MIN_STD_DB if db else tc.MIN_STD_LINEAR, PIVOTS[db])
    for a in ref.values():
        a.setflags(write=False)
    return spec, tm, ref


# ---- 1. the bound and the NaN pattern -------------------------------------------------------------------------------

@pytest.mark.parametrize('db', [True, False], ids=['db', 'linear'])
@pytest.mark.parametrize('normalize', [True, False], ids=['normalised', 'raw'])
@pytest.mark.parametrize('index', range(len(tc.SHAPES)))
def test_bound_and_nan_pattern(index, normalize, db):
    """Every element inside the header's bound, the NaN pattern exactly the definition's, for K = 16, 3 and 1 and at
    two pivots.  Worst measured |out - definition| / bound (printed per case): normalised 0.002 ... 0.095, raw 0.012
    ... 0.986 -- the raw one-tap template sits at its three roundings, the long sums average far below the bound."""
    from audian_amd import hipdsp
    nfreq, k0, Fb, Tt = tc.SHAPES[index]
    if normalize and Tt*Fb == 1:
        with pytest.raises(ValueError):                                  # one tap has no variance
            hipdsp.TmplPlan(gh.ctx(), np.ones((1, 1, 1)), True)
        return
    spec, tm, ref = reference(index, normalize, db)
    n_out = tc.FRAMES - Tt + 1
    min_std = tc.MIN_STD_DB if db else tc.MIN_STD_LINEAR
    assert ref['near'].mean() <= 0.01
    worst = 0.0
    for K in (16, 3, 1):
        plan = hipdsp.TmplPlan(gh.ctx(), tm[:K], normalize)
        for j, pivot in enumerate(PIVOTS[db]):
            got = run(spec, plan, k0, 0, n_out, db=db, floor=tc.FLOOR_DB if db else -np.inf, pivot=pivot, min_std=min_std)
            want, bound = ref['value'][:K], ref['bound'][j, :K]
            decided = np.broadcast_to(~ref['near'], want.shape)
            if normalize:
                assert np.array_equal(np.isnan(got)[decided], np.isnan(want)[decided]), (K, pivot)
                ok = decided & ~np.isnan(want) & ~np.isnan(got)
                assert np.any(np.isnan(want)) and ok.sum() > want.size//3
            else:
                assert np.array_equal(np.isnan(got), np.isnan(want)), (K, pivot)
                inf = np.isinf(want)
                assert np.array_equal(got[inf], want[inf].astype(np.float32))
                ok = np.isfinite(want)
            err = np.abs(got.astype(np.float64)[ok] - want[ok])
            frac = err/np.maximum(bound[ok], 1e-300)
            worst = max(worst, float(frac.max()))
            assert np.all(err <= bound[ok]), (K, pivot, float(frac.max()))
        plan.close()
    print(f'template_match {tc.SHAPES[index]} normalize={normalize} db={db}: worst |err|/bound {worst:.3f}')


def test_floor_none_makes_silence_infinite():
    """Without a floor the zero frames are -inf dB: normalised windows over them are NaN, all others are what they are
    with the floor (no value is below it elsewhere)."""
    from audian_amd import hipdsp
    index = 0
    nfreq, k0, Fb, Tt = tc.SHAPES[index]
    spec, tm, ref = reference(index, True, True)
    plan = hipdsp.TmplPlan(gh.ctx(), tm[:3], True)
    n_out = tc.FRAMES - Tt + 1
    got = run(spec, plan, k0, 0, n_out, db=True, floor=-np.inf, pivot=-90.0, min_std=tc.MIN_STD_DB)
    with_floor = run(spec, plan, k0, 0, n_out, db=True, floor=tc.FLOOR_DB, pivot=-90.0, min_std=tc.MIN_STD_DB)
    t = np.arange(n_out)
    over = (t + Tt > tc.ZEROS.start) & (t < tc.ZEROS.stop)
    assert np.all(np.isnan(got[:, :, over]))
    assert np.array_equal(bits(got[:, :, ~over]), bits(with_floor[:, :, ~over]))
    plan.close()


# ---- 2. exact ---------------------------------------------------------------------------------------------------------

def integer_case(index):
    shape = tc.SHAPES[index]
    nfreq, k0, Fb, Tt = shape
    rng = np.random.default_rng(index)
    spec = rng.integers(-8, 9, (tc.CHANNELS, tc.FRAMES, nfreq)).astype(np.float32)
    tm = tc.templates(shape, integer=True)
    win = np.lib.stride_tricks.sliding_window_view(spec[:, :, k0:k0 + Fb].astype(np.int64), Tt, axis=1)   # (C, n, Fb, Tt)
    want = np.einsum('cnba,kab->kcn', win, tm.astype(np.int64))
    return spec, tm, want


@pytest.mark.parametrize('index', range(len(tc.SHAPES)))
def test_raw_integers_are_exact(index):
    from audian_amd import hipdsp
    nfreq, k0, Fb, Tt = tc.SHAPES[index]
    spec, tm, want = integer_case(index)
    for K in (16, 3, 1):
        plan = hipdsp.TmplPlan(gh.ctx(), tm[:K], False)
        got = run(spec, plan, k0, 0, tc.FRAMES - Tt + 1)
        assert np.array_equal(got.astype(np.int64), want[:K]) and np.all(np.isfinite(got))
        plan.close()


@pytest.mark.parametrize('index', [0, 2])
def test_full_band_equals_fir_bank(index):
    """The full band with Tt*nfreq <= 4097 taps is a FIR kernel over the flattened slab at step = nfreq."""
    from audian_amd import hipdsp
    nfreq, _, _, Tt = tc.SHAPES[index]
    spec, _, _ = integer_case(index)
    tm = np.random.default_rng(3).integers(-4, 5, (5, Tt, nfreq)).astype(np.float64)
    L = Tt*nfreq
    assert L <= 4097
    n_out = tc.FRAMES - Tt + 1
    plan = hipdsp.TmplPlan(gh.ctx(), tm, False)
    got = run(spec, plan, 0, 0, n_out)
    c = gh.ctx()
    fir = hipdsp.FirPlan(c, tm.reshape(5, L)[:, ::-1])
    dx = hipdsp.DeviceArray.from_host(c, spec)
    do = hipdsp.DeviceArray(c, (5, tc.CHANNELS, n_out), np.float32)
    hipdsp.fir_bank(c, fir, dx, 0, tc.CHANNELS, tc.FRAMES*nfreq, (L - 1) - (L - 1)//2, nfreq, n_out, do)
    assert np.array_equal(bits(got), bits(do.to_host()))
    for a in (plan, fir):
        a.close()
    dx.free()
    do.free()


# ---- 3. determinism and placement -----------------------------------------------------------------------------------

@pytest.mark.parametrize('normalize, db', [(True, True), (False, False)], ids=['normalised-db', 'raw-linear'])
def test_determinism(normalize, db):
    """The same bits twice; 16 templates at once are 16 one-template calls; a window alone, at any first, with other
    pitches and without the other channels, is the window inside the long call."""
    from audian_amd import hipdsp
    index = 1
    nfreq, k0, Fb, Tt = tc.SHAPES[index]
    spec, tm, _ = reference(index, normalize, db)
    kw = dict(db=db, floor=tc.FLOOR_DB if db else -np.inf, pivot=PIVOTS[db][0],
              min_std=tc.MIN_STD_DB if db else tc.MIN_STD_LINEAR)
    n_out = tc.FRAMES - Tt + 1
    plan = hipdsp.TmplPlan(gh.ctx(), tm, normalize)
    full = run(spec, plan, k0, 0, n_out, **kw)
    assert np.array_equal(bits(full), bits(run(spec, plan, k0, 0, n_out, **kw)))
    assert np.array_equal(bits(full), bits(run(spec, plan, k0, 0, n_out, strided=False, **kw)))
    one = hipdsp.TmplPlan(gh.ctx())
    for k in range(16):
        one.set(tm[k], normalize)
        assert np.array_equal(bits(run(spec, one, k0, 0, n_out, **kw)[0]), bits(full[k])), k
    one.close()
    for t in (0, 1, 63, 255, 256, 257, n_out - 1):
        alone = run(spec, plan, k0, t, 1, **kw)
        assert np.array_equal(bits(alone[:, :, 0]), bits(full[:, :, t])), t
    part = run(spec[1:2], plan, k0, 100, 77, **kw)                        # one channel, another tile grid
    assert np.array_equal(bits(part[:, 0]), bits(full[:, 1, 100:177]))
    # windows that leave the slab are NaN, the others do not move
    wide = run(spec, plan, k0, -10, tc.FRAMES + 30, **kw)
    assert np.all(np.isnan(wide[:, :, :10])) and np.all(np.isnan(wide[:, :, 10 + n_out:]))
    assert np.array_equal(bits(wide[:, :, 10:10 + n_out]), bits(full))
    assert np.all(np.isnan(run(spec, plan, k0, tc.FRAMES, 5, **kw)))
    assert np.all(np.isnan(run(spec, plan, k0, -(1 << 40), 5, **kw)))
    assert np.all(np.isnan(run(spec, plan, k0, 1 << 40, 5, **kw)))
    plan.close()


@pytest.mark.parametrize('normalize', [True, False], ids=['normalised', 'raw'])
def test_a_plan_that_shrinks_and_grows_is_a_fresh_plan(normalize):
    """One TmplPlan set to a large shape, a tiny one and one in between: after each set the scores have the bits a
    newly created plan gives -- nothing of the shape before is left in the staged block (the host block is cleared up
    to the larger of the old and new sizes, the upload copies the new prefix over a device block that began as zeros)."""
    from audian_amd import hipdsp
    rng = np.random.default_rng(20261021)
    C, frames, nfreq = 2, 300, 129
    spec = rng.uniform(0.1, 1.0, (C, frames, nfreq)).astype(np.float32)
    plan = hipdsp.TmplPlan(gh.ctx())
    for K, Tt, Fb in ((16, 32, 128), (1, 3, 5), (4, 100, 20)):
        tm = rng.standard_normal((K, Tt, Fb))
        plan.set(tm, normalize)
        fresh = hipdsp.TmplPlan(gh.ctx(), tm, normalize)
        got = run(spec, plan, 1, 0, frames - Tt + 1, pivot=0.5)
        want = run(spec, fresh, 1, 0, frames - Tt + 1, pivot=0.5)
        assert np.array_equal(bits(got), bits(want)), (K, Tt, Fb)
        assert np.all(np.isfinite(want)) and len({want[k].tobytes() for k in range(K)}) == K
        fresh.close()
    plan.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------

def test_refusals_leave_out_untouched():
    from audian_amd import hipdsp, _lib
    c = gh.ctx()
    C, frames, nfreq = 2, 40, 33
    rng = np.random.default_rng(5)
    spec = rng.uniform(1.0, 2.0, (C, frames, nfreq)).astype(np.float32)
    d = hipdsp.DeviceArray.from_host(c, spec)
    o = hipdsp.DeviceArray.from_host(c, np.full(4096, SENTINEL, dtype=np.float32))
    plan = hipdsp.TmplPlan(c)
    call = dict(spec_pitch=0, channels=C, frames=frames, nfreq=nfreq, k0=3, first=0, n_out=30)

    def match(plan=plan, spec=d, out=o, min_std=0.0, **kwargs):
        a = dict(call)
        a.update(kwargs)
        hipdsp.template_match(c, plan, spec, a['spec_pitch'], a['channels'], a['frames'], a['nfreq'], a['k0'], a['first'],
                              a['n_out'], out, min_std=min_std)

    with pytest.raises(ValueError):                                     # no templates yet
        match()
    with pytest.raises(ValueError):
        plan.upload()
    for shape in ((17, 3, 3), (1, 257, 2), (1, 256, 257)):
        with pytest.raises(NotImplementedError):
            plan.set(rng.standard_normal(shape))
    with pytest.raises(ValueError):
        plan.set(np.zeros((1, 0, 3)))
    bad = rng.standard_normal((2, 5, 7))
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError):
        plan.set(bad)
    with pytest.raises(ValueError):
        plan.set(np.full((1, 5, 7), 3.0))                               # constant: no coefficient
    plan.set(np.full((1, 5, 7), 3.0), normalize=False)                  # ... but a raw sum
    tm = rng.standard_normal((2, 5, 7))
    plan.set(tm)
    plan.set_host(rng.standard_normal((2, 6, 7)))                       # a new shape that was never uploaded
    with pytest.raises(ValueError):
        match()
    plan.set_host(tm, normalize=False)                                  # the other mode, not uploaded either
    with pytest.raises(ValueError):
        match()
    plan.set(tm)
    rc = _lib.lib.hipdsp_template_match(c.handle, None, hipdsp._p(d), 0, C, frames, nfreq, 3, 0, 30, 0, 1.0, 0.0,
                                        -np.inf, 0.0, 0.0, hipdsp._p(o), 0, 0)
    assert rc == _lib.ERR_INVALID                                       # plan == NULL
    with pytest.raises(ValueError):
        match(spec=None)
    with pytest.raises(ValueError):
        match(out=None)
    for kwargs in (dict(k0=-1), dict(k0=27), dict(nfreq=9), dict(frames=-1), dict(n_out=-1), dict(channels=-1),
                   dict(min_std=-0.5), dict(min_std=np.nan), dict(spec_pitch=frames*nfreq - 1)):
        with pytest.raises(ValueError):
            match(**kwargs)
    with pytest.raises(ValueError):                                     # spec and out overlap
        match(out=d.view(100, (1,)), channels=1, n_out=8)
    with pytest.raises(ValueError):
        hipdsp.template_match(c, plan, d, 0, C, frames, nfreq, 3, 0, 30, o, pivot=np.inf)
    with pytest.raises(ValueError):
        hipdsp.template_match(c, plan, d, 0, C, frames, nfreq, 3, 0, 30, o, out_pitch=8)
    match(n_out=0)                                                      # nothing to do: nothing written
    match(channels=0)
    assert np.all(o.to_host() == SENTINEL)
    match()                                                             # and the next valid call is intact
    got = o.to_host()
    taps = td.prepare(tm, True)[0]
    ref = td.scores(spec, taps, 3, 0, 30, True)
    assert np.all(np.abs(got[:120].reshape(2, 2, 30) - ref['value']) <= ref['bound']) and np.all(got[120:] == SENTINEL)
    plan.close()
    d.free()
    o.free()


# ---- 5. graph -------------------------------------------------------------------------------------------------------

def test_graph_replays_under_new_templates():
    from audian_amd import hipdsp
    ctx = hipdsp.Context(0)
    stream = ctx.create_stream()
    ctx.set_stream(stream)
    rng = np.random.default_rng(9)
    C, frames, nfreq, k0, Tt, Fb, K = 3, 700, 129, 5, 32, 97, 4
    spec = (10.0**rng.uniform(-10.0, -6.0, (C, frames, nfreq))).astype(np.float32)
    n_out = frames - Tt + 1
    dx = hipdsp.DeviceArray.from_host(ctx, spec)
    dout = hipdsp.DeviceArray(ctx, (K, C, n_out), np.float32)
    eager = hipdsp.DeviceArray(ctx, (K, C, n_out), np.float32)
    plan = hipdsp.TmplPlan(ctx, rng.standard_normal((K, Tt, Fb)))

    def chain():
        plan.upload()
        hipdsp.template_match(ctx, plan, dx, 0, C, frames, nfreq, k0, 0, n_out, dout, db=True, pivot=-80.0, min_std=0.1)

    chain()                                                             # once outside the capture
    ctx.synchronize()
    ctx.graph_begin()
    chain()
    graph = ctx.graph_end()
    other = hipdsp.TmplPlan(ctx)
    seen = set()
    for _ in range(3):
        tm = rng.standard_normal((K, Tt, Fb))
        plan.set_host(tm)                                               # host only: the captured upload carries it over
        dout.zero_()
        ctx.graph_launch(graph)
        ctx.synchronize()
        got = dout.to_host()
        other.set(tm)
        hipdsp.template_match(ctx, other, dx, 0, C, frames, nfreq, k0, 0, n_out, eager, db=True, pivot=-80.0, min_std=0.1)
        assert np.array_equal(bits(got), bits(eager.to_host()))
        assert np.all(np.abs(got) <= 1) and np.any(got != 0)
        seen.add(got.tobytes())
    assert len(seen) == 3
    ctx.graph_destroy(graph)
    plan.close()
    other.close()
    for a in (dx, dout, eager):
        a.free()
    ctx.set_stream(None)
    ctx.destroy_stream(stream)


# ---- 6. past element 2^31 -------------------------------------------------------------------------------------------

from test_gpu_far_indices import far, placed            # noqa: E402,F401  (the fixture and its context manager)
import far_placement as fp                              # noqa: E402


def test_far_placement(far):
    """The slab in the middle of a NaN-filled block of 2^32 elements, around every boundary and past element 2^31 (the
    way test_gpu_far_indices.py places hipdsp_band_power): the windows' scores are bit for bit those of the same slab
    near the start, and those are inside the bound."""
    from audian_amd import hipdsp
    F, R = fp.SLAB_F, fp.SLAB_ROWS
    k0, Fb, Tt, K = 5, 97, 32, 2
    rng = np.random.default_rng(21)
    spec = (10.0**rng.uniform(-9.0, -3.0, (R, F))).astype(np.float32)
    tm = rng.uniform(-90.0, -30.0, (K, Tt, Fb))
    n_out = R - Tt + 1
    pitch = n_out + 2*fp.OUT_GUARD
    plan = hipdsp.TmplPlan(far.ctx, tm, True)
    near = None
    for w in fp.slab_windows():
        i0 = w.start//F
        with placed(far, [w], spec.reshape(-1), guard_value=1e30):
            hipdsp.template_match(far.ctx, plan, far.X(), 0, 1, i0 + R, F, k0, i0, n_out,
                                  far.out_rows(np.float32, pitch, K, n_out), db=True, ref_power=1.0, min_power=0.0,
                                  floor=-120.0, pivot=-60.0, min_std=0.1, out_pitch=n_out, out_template_pitch=pitch)
            got = far.rows(np.float32, pitch, K, n_out)
        near = got if near is None else near
        assert np.array_equal(bits(got), bits(near)), w.name
    v = device_db(spec[None], -120.0)
    ref = td.scores(v, td.prepare(tm, True)[0], k0, 0, n_out, True, 0.1, -60.0)
    assert np.all(np.abs(near[:, None, :] - ref['value']) <= ref['bound']) and not np.isnan(near).any()
    plan.close()


# ---- 7. the facade --------------------------------------------------------------------------------------------------

def test_facade_equals_the_kernel_and_its_host_path():
    """BufferedTemplateMatch on the spectrogram's device mirror is hipdsp.template_match bit for bit; detect_calls on
    the device finds what its numpy path finds on the same buffer."""
    from audian_amd import hipdsp
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
    from audian_amd.templates import Template, default_pivot, host_values, template_scores
    from audian_amd.tracegraph import TraceGraph
    from test_template_match_host import CHIRPS, Item, RATE, call_recording, cut
    x = call_recording()
    g = TraceGraph(10.0, 2.0)
    s, t = BufferedSpectrogram(source='data', nfft=256), BufferedTemplateMatch()
    g.add_trace(s)
    g.add_trace(t)
    g.setup_traces()
    g.open(x, RATE)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g.update_times(0.0, 4.5)
    n, F, C = len(s._hostbuf), 129, 2
    assert s._mirror_valid(0, n)
    tm = cut(g)                                                          # only the patch crosses
    Tt = tm.values.shape[0]
    a, k0 = g.region_frames(s, CHIRPS[0] - 0.01, CHIRPS[0])[0], tm.first_bin(s)
    assert np.array_equal(tm.values, host_values(np.asarray(s.buffer)[a:a + Tt, 0, k0:k0 + tm.values.shape[1]], True, -100.0))
    launched = hipdsp.launches.get('template_match', 0)
    t.set_template(tm)
    assert hipdsp.launches['template_match'] == launched + 1 and t._stale     # the device path, one launch
    plan = hipdsp.TmplPlan(s.ctx, tm.values, True)
    out = hipdsp.DeviceArray(s.ctx, (1, C, n), np.float32)
    hipdsp.template_match(s.ctx, plan, s._dev, s._pitch(), C, n, F, k0, -(Tt//2), n, out, db=True, ref_power=1.0,
                          min_power=0.0, floor=-100.0, pivot=default_pivot(tm.values), min_std=0.1)
    direct = out.to_host()[0]
    assert np.array_equal(bits(np.asarray(t.buffer).T), bits(direct))
    for on in CHIRPS:
        k = int(on*s.rate) + Tt//2
        assert np.nanmax(direct[0, k - 2:k + 3]) > 0.8
    short = Template(tm.values[2:-2], tm.fmin, tm.fresolution, tm.tresolution, True, -100.0, 'core')
    lin = g.cut_template(CHIRPS[1], CHIRPS[1] + 0.1, 1800.0, 4200.0, 0, log=False)
    both = [tm, lin, short]                                              # three groups, the middle one of another kind
    scores, i0 = g.match_templates(both)
    assert isinstance(scores, hipdsp.DeviceArray) and scores.shape == (3, C, n) and i0 == s.offset
    dev_scores = scores.to_host()
    assert np.array_equal(bits(dev_scores[0]), bits(direct))
    events, best, best_r = g.detect_calls(both, min_r=0.5)
    assert len(events.onsets[0]) == 3 and len(events.onsets[1]) == 0
    np.asarray(s.buffer)                                                 # the host copy, then the numpy path on it
    valid, s._dev_valid = s._dev_valid, []
    try:
        host_scores = template_scores(s, both)
        h_events, h_best, h_best_r = g.detect_calls(both, min_r=0.5)
    finally:
        s._dev_valid = valid
    assert isinstance(host_scores, np.ndarray)
    assert np.array_equal(np.isnan(host_scores), np.isnan(dev_scores))
    assert np.nanmax(np.abs(host_scores - dev_scores)) < 1e-3
    for c in range(C):
        assert np.array_equal(events.frames(c), h_events.frames(c))
        assert np.all(np.abs(best_r[c] - h_best_r[c]) < 1e-3)
        # (the call the template was cut from scores 1 under the template and under its core: the float32 and the
        # float64 path may break that tie differently, and only such a tie)
        assert np.all((best[c] == h_best[c]) | (best_r[c] > 1.0 - 1e-3))
    plan.close()
    out.free()
    scores.free()
