"""hipdsp_bin_quantiles and hipdsp_spec_equalize through the C ABI, bit for bit against tests/noise_profile_definition.py
(no tolerance anywhere: the two order statistics are elements of the input, the equalised values are numpy's float32
arithmetic).  Every output lies between sentinel guards; a call's slab is uploaded once and serves all its calls."""

import ctypes

import numpy as np
import pytest

import gpu_helpers as gh
import noise_profile_definition as nd

pytestmark = pytest.mark.gpu

GUARD = 16
SENT_F = np.float32(-12345.5)
SENT_I = np.int32(-77)
BUF_FRAMES = 3100             # frames of every select slab: first = 7, step 3, 1000 frames fit


class Slab(object):
    """A host slab (C, frames, F) on the device at a chosen pitch and element offset (1: a 4-byte, not 16-byte base)."""

    def __init__(self, spec, pitch_extra=0, offset=0):
        from audian_amd import hipdsp
        self.c = gh.ctx()
        self.spec = np.ascontiguousarray(spec, dtype=np.float32)
        self.C, self.frames, self.F = self.spec.shape
        self.pitch = self.frames*self.F + pitch_extra
        host = np.full(offset + max(1, self.C)*self.pitch + 8, np.nan, dtype=np.float32)
        for ch in range(self.C):
            a = offset + ch*self.pitch
            host[a:a + self.frames*self.F] = self.spec[ch].ravel()
        self.dev = hipdsp.DeviceArray.from_host(self.c, host)
        self.offset, self.pitch_arg = offset, (self.pitch if pitch_extra else 0)

    def ptr(self, channel=0):
        return self.dev.view(self.offset + channel*self.pitch, (1,))

    def free(self):
        self.dev.free()


def quantiles(slab, first, n_frames, step, k0, k1, q, count=True, channels=None, channel0=0, status=False):
    """One hipdsp_bin_quantiles call: (lo_hi (C, W, 2), count (C, W) or None); the guards around both outputs must hold
    the sentinel afterwards.  status: return the exception of a refused call (the outputs must then be untouched)."""
    from audian_amd import hipdsp
    C = slab.C if channels is None else channels
    W = max(k1 - k0, 0)
    n = C*W
    out = hipdsp.DeviceArray.from_host(slab.c, np.full(2*n + 2*GUARD, SENT_F, dtype=np.float32))
    cnt = hipdsp.DeviceArray.from_host(slab.c, np.full(n + 2*GUARD, SENT_I, dtype=np.int32))
    err = None
    try:
        hipdsp.bin_quantiles(slab.c, slab.ptr(channel0), slab.pitch_arg, C, slab.frames, slab.F, first, n_frames, step,
                             k0, k1, q, out.view(GUARD, (1,)), cnt.view(GUARD, (1,)) if count else None)
    except (ValueError, NotImplementedError) as e:
        if not status:
            raise
        err = e
    o, k = out.to_host(), cnt.to_host()
    out.free()
    cnt.free()
    assert np.all(o[:GUARD] == SENT_F) and np.all(o[GUARD + 2*n:] == SENT_F), 'written outside the lo/hi rows'
    assert np.all(k[:GUARD] == SENT_I) and np.all(k[GUARD + n:] == SENT_I), 'written outside the count rows'
    if status:
        assert err is not None, 'the call was not refused'
        assert np.all(o == SENT_F) and np.all(k == SENT_I), 'a refused call wrote something'
        return err
    if not count:
        assert np.all(k == SENT_I), 'out_count NULL, yet counts were written'
    if n_frames >= 0 and n > 0:
        assert not np.any(o[GUARD:GUARD + 2*n] == SENT_F), 'values left unwritten'
    return o[GUARD:GUARD + 2*n].reshape(C, W, 2), (k[GUARD:GUARD + n].reshape(C, W) if count else None)


def check(slab, first, n_frames, step, k0, k1, q, what):
    got, cnt = quantiles(slab, first, n_frames, step, k0, k1, q)
    want, wcnt = nd.bin_quantiles(slab.spec, first, n_frames, step, k0, k1, q)
    assert np.array_equal(cnt, wcnt), what
    assert nd.same_bits(got, want), what
    return got, cnt


N_FRAMES = (0, 1, 2, 3, 255, 256, 257, 1000)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('F', [1, 5, 64, 65, 129])
def test_select_is_the_definition(F, C):
    """Every shape, value kind and q of the contract: full band, first > 0, both frame steps."""
    rots = range(len(nd.KINDS)) if C*F < len(nd.KINDS) else (0,)
    for rot in rots:
        rng = np.random.default_rng([F, C, rot])
        slab = Slab(nd.mixed_slab(rng, C, BUF_FRAMES, F, rot))
        for n_frames in N_FRAMES:
            for step in (1, 3):
                qs = list(nd.QS)
                # a q whose pos is an exact integer in the columns without NaN (n = n_frames)
                if nd.exact_q(n_frames) is not None:
                    qs.append(nd.exact_q(n_frames))
                for q in dict.fromkeys(qs):
                    check(slab, 7, n_frames, step, 0, F, q, 'F %d C %d rot %d frames %d step %d q %g' % (F, C, rot, n_frames, step, q))
        slab.free()


def test_exact_integer_position():
    """257 values, q = 0.25: pos = 64 exactly, frac = 0, and the host takes lo itself."""
    rng = np.random.default_rng(5)
    spec = nd._noise(rng, 3*300*65).reshape(3, 300, 65)
    slab = Slab(spec)
    got, cnt = check(slab, 0, 257, 1, 0, 65, 0.25, 'exact')
    assert np.all(cnt == 257)
    assert np.array_equal(got[:, :, 0], np.sort(spec[:, :257], axis=1)[:, 64])
    slab.free()


def test_nan_in_one_column_only():
    rng = np.random.default_rng(6)
    spec = nd._noise(rng, 3*300*129).reshape(3, 300, 129)
    spec[1, rng.random(300) < 0.4, 77] = np.nan
    slab = Slab(spec)
    for q in nd.QS:
        got, cnt = check(slab, 0, 300, 1, 0, 129, q, 'one NaN column q %g' % q)
    assert np.all(np.delete(cnt.ravel(), 129 + 77) == 300) and cnt[1, 77] < 300
    slab.free()


@pytest.mark.parametrize('F', [65, 129])
def test_subband_pitch_misaligned_base_and_isolation(F):
    """A sub-band, a one-channel call, a padded pitch and a base that is 4-byte but not 16-byte aligned give the columns
    of the full call; the same call twice gives the same bits; out_count NULL works."""
    rng = np.random.default_rng(F)
    spec = nd.mixed_slab(rng, 3, 700, F)
    plain, padded = Slab(spec), Slab(spec, pitch_extra=13, offset=1)
    assert padded.ptr().ptr % 16 == 4 and (padded.pitch*4) % 16 != 0
    for q in (0.05, 0.5, 1.0):
        for first, n_frames, step in ((0, 700, 1), (5, 231, 3)):
            full, fcnt = check(plain, first, n_frames, step, 0, F, q, 'full')
            again, acnt = quantiles(plain, first, n_frames, step, 0, F, q)
            assert nd.exact_bits(again, full) and np.array_equal(acnt, fcnt), 'not the same bits twice'
            far, pcnt = check(padded, first, n_frames, step, 0, F, q, 'padded')
            assert nd.exact_bits(far, full) and np.array_equal(pcnt, fcnt), 'the pitch or the base address changed a column'
            k0, k1 = 3, F - 2
            sub, scnt = check(padded, first, n_frames, step, k0, k1, q, 'sub-band')
            assert nd.exact_bits(sub, full[:, k0:k1]) and np.array_equal(scnt, fcnt[:, k0:k1]), 'k0/k1 changed a column'
            one, ocnt = quantiles(padded, first, n_frames, step, 0, F, q, channels=1, channel0=2)
            assert nd.exact_bits(one[0], full[2]) and np.array_equal(ocnt[0], fcnt[2]), 'the other channels changed a column'
            nocount, none = quantiles(plain, first, n_frames, step, k0, k1, q, count=False)
            assert none is None and nd.exact_bits(nocount, full[:, k0:k1])
    plain.free()
    padded.free()


def test_empty_calls_write_nothing_or_nan():
    rng = np.random.default_rng(8)
    slab = Slab(nd._noise(rng, 2*10*5).reshape(2, 10, 5))
    got, cnt = quantiles(slab, 3, 0, 1, 0, 5, 0.5)                       # n_frames == 0: NaN, NaN, 0 everywhere
    assert np.all(np.isnan(got)) and np.all(cnt == 0)
    got, cnt = quantiles(slab, 0, 10, 1, 2, 2, 0.5)                      # k1 == k0: nothing (the guards are checked)
    assert got.size == 0
    got, cnt = quantiles(slab, 0, 10, 1, 0, 5, 0.5, channels=0)          # channels == 0
    assert got.size == 0
    slab.free()


def test_refused_calls_write_nothing_and_leave_no_trace():
    from audian_amd import hipdsp
    rng = np.random.default_rng(9)
    spec = nd.mixed_slab(rng, 2, 40, 9)
    slab = Slab(spec)
    before, bcnt = check(slab, 1, 30, 1, 0, 9, 0.5, 'before')
    refused = [dict(q=-0.01), dict(q=1.5), dict(q=np.nan), dict(k0=-1), dict(k1=10), dict(k0=5, k1=4), dict(step=0),
               dict(first=-1), dict(first=11), dict(first=0, n_frames=41), dict(n_frames=14, step=3)]
    for kw in refused:
        a = dict(first=1, n_frames=30, step=1, k0=0, k1=9, q=0.5)
        a.update(kw)
        err = quantiles(slab, a['first'], a['n_frames'], a['step'], a['k0'], a['k1'], a['q'], status=True)
        assert isinstance(err, ValueError), kw
    for kw in (dict(n_frames=2**31), dict(channels=65536)):
        a = dict(n_frames=30, channels=None)
        a.update(kw)
        if a['channels']:
            # (the outputs of 65536 channels are never written: the refusal comes first; one column keeps them small)
            out = hipdsp.DeviceArray.from_host(slab.c, np.full(4, SENT_F, dtype=np.float32))
            with pytest.raises(NotImplementedError):
                hipdsp.bin_quantiles(slab.c, slab.ptr(), 0, a['channels'], slab.frames, slab.F, 1, 30, 1, 0, 1, 0.5, out, None)
            assert np.all(out.to_host() == SENT_F)
            out.free()
        else:
            err = quantiles(slab, 1, a['n_frames'], 1, 0, 9, 0.5, status=True)
            assert isinstance(err, NotImplementedError), kw
    # a pitch too small, NULL pointers with work to do, an output inside the slab
    out = hipdsp.DeviceArray.from_host(slab.c, np.full(2*2*9, SENT_F, dtype=np.float32))
    for args in ((slab.ptr(), 40*9 - 1, out), (None, 0, out), (slab.ptr(), 0, None), (slab.ptr(), 0, slab.ptr())):
        with pytest.raises(ValueError):
            hipdsp.bin_quantiles(slab.c, args[0], args[1], 2, 40, 9, 1, 30, 1, 0, 9, 0.5, args[2], None)
    for frames, pitch in ((2**45, 0), (40, 2**44 + 1)):                    # sizes whose byte offsets would leave int64
        with pytest.raises(ValueError):
            hipdsp.bin_quantiles(slab.c, slab.ptr(), pitch, 2, frames, 9, 1, 30, 1, 0, 9, 0.5, out, None)
    assert np.all(out.to_host() == SENT_F)
    assert nd.exact_bits(slab.dev.to_host()[:2*40*9], spec.ravel()), 'a refused call wrote into the slab'
    out.free()
    after, acnt = check(slab, 1, 30, 1, 0, 9, 0.5, 'after')
    assert nd.exact_bits(after, before) and np.array_equal(acnt, bcnt)
    slab.free()


def test_far_base_gives_the_bits_of_the_near_one():
    """Two channels 2^31 + 64 elements apart inside a NaN-filled block, the pointer 2^31 elements into it: an index or a
    byte offset wrapped to 32 bits stays inside the block and reads NaN or the other channel -- a wrong value or count."""
    from audian_amd import hipdsp
    from audian_amd._lib import check as st, lib
    c = gh.ctx()
    rng = np.random.default_rng(10)
    frames, F = 70, 129
    spec = nd.mixed_slab(rng, 2, frames, F)
    spec[1] = spec[1, ::-1] + np.float32(1.0)
    near = Slab(spec)
    want, wcnt = check(near, 2, 22, 3, 1, F, 0.5, 'near')
    near.free()
    pitch, mid = 2**31 + 64, 2**31
    block = hipdsp.DeviceArray(c, (2**32 + 2**22,), np.float32)
    try:
        st(lib.hipdsp_memset(c.handle, ctypes.c_void_p(block.ptr), 0xff, block.nbytes))
        for ch in range(2):
            block.view(mid + ch*pitch, (frames*F,)).copy_from_host(spec[ch].ravel())
        out = hipdsp.DeviceArray.from_host(c, np.full(2*2*(F - 1), SENT_F, dtype=np.float32))
        cnt = hipdsp.DeviceArray.from_host(c, np.full(2*(F - 1), SENT_I, dtype=np.int32))
        hipdsp.bin_quantiles(c, block.view(mid, (1,)), pitch, 2, frames, F, 2, 22, 3, 1, F, 0.5, out, cnt)
        got, gcnt = out.to_host().reshape(2, F - 1, 2), cnt.to_host().reshape(2, F - 1)
        out.free()
        cnt.free()
    finally:
        c.synchronize()
        block.free()
    assert np.array_equal(gcnt, wcnt)
    assert nd.exact_bits(got, want)


# ---- hipdsp_spec_equalize ------------------------------------------------------------------------------------------

def equalize_case(rng, C, frames, F):
    """A slab and a profile that hold the contract's special values: denormal quotients and differences, N = inf, N = 0,
    P = 0, NaN in P and in N, negative differences."""
    spec = nd._noise(rng, C*frames*F).reshape(C, frames, F)
    prof = nd._noise(rng, C*F).reshape(C, F)
    flat = spec.reshape(-1)
    idx = rng.permutation(flat.size)
    special = np.concatenate((np.array([0.0, -0.0, np.nan, np.inf, 1e-38, 3e-39, 1e-45], dtype=np.float32),
                              nd._bits([0x00000001, 0x007fffff, 0x00800000])))
    for j, v in enumerate(special):
        flat[idx[j::len(special)][:max(1, flat.size//40)]] = v
    if F >= 5:
        prof[:, 1] = np.inf
        prof[:, 2] = np.float32(3e38)                  # quotients of small P are denormal
        prof[0, 3] = 0.0
        prof[-1, 4] = np.nan
        prof[:, 0] = np.float32(1.5e-39)               # a denormal divisor
    return spec, prof


def run_equalize(spec, prof, mode, in_place, padded):
    """hipdsp_spec_equalize on host arrays: the (C, frames, F) result; guards around every output row are checked."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, frames, F = spec.shape
    total = frames*F
    s_off, s_pitch = (1, total + 5) if padded else (0, total)
    o_off, o_pitch = (GUARD + 1, total + 2*GUARD + 1) if padded else (GUARD, total)
    p_off, p_pitch = (3, F + 2) if padded else (0, F)
    if in_place:
        o_off, o_pitch = s_off, s_pitch
    hs = np.full(s_off + C*s_pitch + GUARD, SENT_F, dtype=np.float32)
    hp = np.full(p_off + C*p_pitch, SENT_F, dtype=np.float32)
    for ch in range(C):
        hs[s_off + ch*s_pitch:s_off + ch*s_pitch + total] = spec[ch].ravel()
        hp[p_off + ch*p_pitch:p_off + ch*p_pitch + F] = prof[ch]
    ds, dp = hipdsp.DeviceArray.from_host(c, hs), hipdsp.DeviceArray.from_host(c, hp)
    do = ds if in_place else hipdsp.DeviceArray.from_host(c, np.full(o_off + C*o_pitch + GUARD, SENT_F, dtype=np.float32))
    hipdsp.spec_equalize(c, ds.view(s_off, (1,)), s_pitch if padded else 0, do.view(o_off, (1,)),
                         o_pitch if (padded or in_place) and o_pitch != total else 0, C, frames, F, dp.view(p_off, (1,)),
                         p_pitch if padded else 0, mode)
    flat = do.to_host()
    if not in_place:
        assert nd.exact_bits(ds.to_host(), hs), 'the input changed'
        do.free()
    assert nd.exact_bits(dp.to_host(), hp), 'the profile changed'
    ds.free()
    dp.free()
    written = np.zeros(flat.size, dtype=bool)
    out = np.empty((C, frames, F), dtype=np.float32)
    for ch in range(C):
        a = o_off + ch*o_pitch
        out[ch] = flat[a:a + total].reshape(frames, F)
        written[a:a + total] = True
    assert np.all(flat[~written] == SENT_F), 'written outside the rows'
    return out


def assert_numpy_bits(got, want, what):
    """NaN where numpy has NaN (a NaN's sign and payload are the processor's), the same bits everywhere else -- the sign
    of a zero included."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), what


@pytest.mark.parametrize('mode', ['divide', 'subtract'])
@pytest.mark.parametrize('C, frames, F', [(3, 37, 129), (1, 7, 5), (2, 9001, 1), (3, 3, 1), (2, 41, 4099), (1, 1, 2)])
def test_equalize_is_numpy_float32(C, frames, F, mode):
    """Both modes, out of place and in place, compact and padded (a 4-byte base, head and tail of every row misaligned
    and differently so for input and output), the profile in LDS (F <= 4096) and read through the cache."""
    assert (frames*F) % 4 != 0 or frames*F < 4
    rng = np.random.default_rng([C, frames, F])
    spec, prof = equalize_case(rng, C, frames, F)
    want = nd.equalize(spec, prof, mode)
    with np.errstate(all='ignore'):
        if mode == 'divide':                 # the header's formula is the same thing: the correctly rounded quotient
            assert nd.exact_bits((spec.astype(np.float64)/prof.astype(np.float64)[:, None, :]).astype(np.float32), want)
    for in_place in (False, True):
        for padded in (False, True):
            got = run_equalize(spec, prof, mode, in_place, padded)
            assert_numpy_bits(got, want, '%s in_place %d padded %d' % (mode, in_place, padded))


def test_equalize_aligned_pair_takes_vectors_and_matches():
    """Input and output rows that reach 16-byte alignment at the same element (offset 1 both): the float4 body with a
    three-element head; the same bits as the compact call."""
    from audian_amd import hipdsp
    c = gh.ctx()
    rng = np.random.default_rng(12)
    C, frames, F = 2, 33, 129
    spec, prof = equalize_case(rng, C, frames, F)
    total = frames*F
    pitch = total + 3                                   # 4260: rows of both arrays keep the phase
    assert pitch % 4 == 0
    hs = np.full(1 + C*pitch + 3, SENT_F, dtype=np.float32)
    for ch in range(C):
        hs[1 + ch*pitch:1 + ch*pitch + total] = spec[ch].ravel()
    ds = hipdsp.DeviceArray.from_host(c, hs)
    do = hipdsp.DeviceArray.from_host(c, np.full(hs.size, SENT_F, dtype=np.float32))
    dp = hipdsp.DeviceArray.from_host(c, prof)
    for mode in ('divide', 'subtract'):
        hipdsp.spec_equalize(c, ds.view(1, (1,)), pitch, do.view(1, (1,)), pitch, C, frames, F, dp, 0, mode)
        flat = do.to_host()
        want = nd.equalize(spec, prof, mode)
        for ch in range(C):
            got = flat[1 + ch*pitch:1 + ch*pitch + total].reshape(frames, F)
            assert_numpy_bits(got, want[ch], mode)
            assert np.all(flat[1 + ch*pitch + total:1 + (ch + 1)*pitch] == SENT_F)
        assert flat[0] == SENT_F
    for d in (ds, do, dp):
        d.free()


def test_equalize_refusals_write_nothing():
    from audian_amd import hipdsp
    c = gh.ctx()
    rng = np.random.default_rng(13)
    C, frames, F = 2, 6, 5
    spec, prof = equalize_case(rng, C, frames, F)
    total = frames*F
    ds = hipdsp.DeviceArray.from_host(c, spec)
    dp = hipdsp.DeviceArray.from_host(c, prof)
    do = hipdsp.DeviceArray.from_host(c, np.full(C*total + 8, SENT_F, dtype=np.float32))
    bad = [dict(mode=2), dict(spitch=total - 1), dict(opitch=total - 1), dict(ppitch=F - 1), dict(spec=None),
           dict(out=None), dict(prof=None), dict(out=ds.view(4, (1,))), dict(out=ds, opitch=total + 1),
           dict(out=dp), dict(frames=-1), dict(frames=2**45), dict(spitch=2**44 + 1), dict(opitch=2**44 + 1)]
    for kw in bad:
        a = dict(spec=ds, spitch=0, out=do, opitch=0, C=C, frames=frames, F=F, prof=dp, ppitch=0, mode=0)
        a.update(kw)
        with pytest.raises(ValueError):
            hipdsp.spec_equalize(c, a['spec'], a['spitch'], a['out'], a['opitch'], a['C'], a['frames'], a['F'], a['prof'],
                                 a['ppitch'], a['mode'])
    with pytest.raises(NotImplementedError):
        hipdsp.spec_equalize(c, ds, 0, do, 0, 65536, frames, F, dp, 0, 0)
    assert np.all(do.to_host() == SENT_F)
    assert nd.exact_bits(ds.to_host(), spec) and nd.exact_bits(dp.to_host(), prof)
    hipdsp.spec_equalize(c, ds, 0, do, 0, C, frames, F, dp, 0, 'subtract')
    got = do.to_host()
    assert_numpy_bits(got[:C*total].reshape(C, frames, F), nd.equalize(spec, prof, 'subtract'), 'after the refusals')
    assert np.all(got[C*total:] == SENT_F)
    for d in (ds, dp, do):
        d.free()


def test_both_calls_replay_inside_one_graph():
    """hipdsp_bin_quantiles and hipdsp_spec_equalize captured in one graph: replayed on new slab contents they give the
    new definition (every argument travelled by value, nothing was uploaded or synchronised)."""
    from audian_amd import hipdsp
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    rng = np.random.default_rng(14)
    C, frames, F = 2, 300, 65
    specs = [nd.mixed_slab(rng, C, frames, F, rot) for rot in (0, 4)]
    prof = nd._noise(rng, C*F).reshape(C, F)
    ds = hipdsp.DeviceArray.from_host(c, specs[0])
    dp = hipdsp.DeviceArray.from_host(c, prof)
    dq = hipdsp.DeviceArray(c, (C, F, 2), np.float32)
    dn = hipdsp.DeviceArray(c, (C, F), np.int32)
    de = hipdsp.DeviceArray(c, (C, frames, F), np.float32)

    def chain():
        hipdsp.bin_quantiles(c, ds, 0, C, frames, F, 1, 99, 3, 0, F, 0.5, dq, dn)
        hipdsp.spec_equalize(c, ds, 0, de, 0, C, frames, F, dp, 0, 'divide')

    chain()                                                             # once outside the capture
    c.synchronize()
    c.graph_begin()
    chain()
    graph = c.graph_end()
    try:
        for spec in specs:
            ds.copy_from_host(spec)
            dq.zero_()
            c.graph_launch(graph)
            c.synchronize()
            want, wcnt = nd.bin_quantiles(spec, 1, 99, 3, 0, F, 0.5)
            assert nd.same_bits(dq.to_host(), want) and np.array_equal(dn.to_host(), wcnt)
            assert_numpy_bits(de.to_host(), nd.equalize(spec, prof, 'divide'), 'replayed')
    finally:
        c.graph_destroy(graph)
        c.set_stream(None)
        c.destroy_stream(stream)
