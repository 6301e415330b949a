"""hipdsp_region_xcorr, BufferedData.region_xcorr and TraceGraph.attribute_events on the GPU.  The comparator is never the
code under test: tests/xcorr_definition.py (plain loops over the lags in long double, pinned to np.corrcoef by the golden
file), and every input comes from its table GPU_CASES, for which tests/test_xcorr_host.py asserts T < 2^-30 -- so every
value here is held to one float32 rounding of the exact coefficient plus that.

The kernel cuts a window into chunks of 65536 samples counted from its start (one workgroup per region, partner and
chunk) and takes a chunk in tiles of 2048 samples staged in LDS; a thread owns 9 consecutive lags and walks its segment of
the tile in steps of 8 samples; the segments of a tile, the tiles of a chunk and the chunks of a window are added in
ascending order.  So of the lengths used here 0 launches nothing (the second launch writes NaN and -1), 1 has no
variance, 2 is the first with a coefficient, 7, 8, 9 sit around a thread's step, 63 ... 65 around a wave, 2047 ... 2049
around the tile (2049: the first hand-over into the partial row), 4097 three tiles, 65535 ... 65537 around the chunk and
131073 three chunks; the lags 4 and 5 (9 and 11 of them) sit around a thread's nine, 13 (27) fills three threads, and
the split of the tile among the threads changes with them: 128 segments up to 4, 64 up to 13, 4 at 255, 1 at 1024."""

import ctypes
import functools

import numpy as np
import pytest

import far_placement as fp
import gpu_helpers as gh
import xcorr_definition as xd

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


class Slab(object):
    """A host (C, frames) float32 array on the device, x_pitch == frames by default: the rows lie back to back, so a read
    past a row's end finds the next row's samples (a wrong value, not a fault); with pitch_extra and base the rows start
    at 4-byte addresses that are no multiple of 16."""

    def __init__(self, x, pitch_extra=0, base=0, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(base + self.C*self.pitch, SENTINEL, dtype=np.float32)
        for c in range(self.C):
            host[base + c*self.pitch:base + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(base, (1,))

    def xcorr(self, regions, partners, L, channels=None):
        from audian_amd import hipdsp
        return hipdsp.region_xcorr(self.ctx, self.view, self.pitch, self.C if channels is None else channels, self.frames,
                                   regions, partners, L)

    def free(self):
        self.dev.free()


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's results of a case, computed once: {(region index, partner index): dict}."""
    x, regions, partners, L = xd.case(name)
    return {(i, j): xd.region_xcorr(x, c, a, b, p, L) for i, (c, a, b) in enumerate(regions.tolist())
            for j, p in enumerate(partners)}


@functools.lru_cache(maxsize=None)
def computed(name):
    """(rows, info) of a case through the C ABI, computed once and left unchanged."""
    x, regions, partners, L = xd.case(name)
    slab = Slab(x)
    try:
        rows, info = slab.xcorr(regions, partners, L)
    finally:
        slab.free()
    rows.setflags(write=False)
    info.setflags(write=False)
    return rows, info


def judge(name, rows, info, what=''):
    worst = 0.0
    for (i, j), q in expected(name).items():
        worst = max(worst, xd.compare(q, rows[i, j], info[i, j], '%s %s region %d partner %d' % (name, what, i, j)))
    print('%s %s: largest error %.3f of its allowance' % (name, what, worst))
    return worst


@pytest.mark.parametrize('name', sorted(xd.GPU_CASES))
def test_against_the_definition(name):
    """Every case of the shared table: the exact NaN pattern, info[0] and [1] exactly, the standard deviations to their
    bound, every coefficient to 2^-24 |r| + T."""
    rows, info = computed(name)
    judge(name, rows, info)


def test_row_edges_give_the_exact_nan_pattern():
    x, regions, partners, L = xd.case('edges')
    rows, info = computed('edges')
    for i, (c, a, b) in enumerate(regions.tolist()):
        lo, nl = xd.valid_lags(a, b, x.shape[1], L)
        want = np.ones(2*L + 1, dtype=bool)
        want[L + lo:L + lo + nl] = False
        for j, p in enumerate(partners):
            if b - a >= 2:
                assert np.array_equal(np.isnan(rows[i, j]), want), (i, j)
                assert info[i, j, 0] == nl
    assert xd.valid_lags(0, 100, x.shape[1], L) == (0, 9) and xd.valid_lags(3, 203, x.shape[1], L) == (-3, 12)
    assert np.isnan(rows[5]).all() and np.isnan(rows[6]).all()         # one sample: no variance
    assert info[4, :, 0].tolist() == [1.0]*5                            # the whole row: lag 0 alone


def test_own_channel_and_known_delay_are_exactly_one():
    x, regions, partners, L = xd.case('lengths')
    rows, info = computed('lengths')
    for i, (c, a, b) in enumerate(regions.tolist()):
        if b - a < 2:
            assert np.isnan(rows[i]).all() and (info[i, :, 1] == -1).all()
            continue
        assert rows[i, partners.index(0), L] == np.float32(1.0), (i, 'own channel, lag 0')
        j = partners.index(1)                                           # channel 0, DELAY samples later
        assert rows[i, j, L + xd.DELAY] == np.float32(1.0), (i, 'delayed copy')
        if b - a >= 63:
            assert info[i, j, 1] == L + xd.DELAY and info[i, partners.index(0), 1] == L, i
            assert abs(info[i, j, 3] - info[i, j, 2]) <= 1e-12*info[i, j, 2]    # the same samples, another pivot


def test_constant_windows_give_nan():
    rows, info = computed('const')
    assert np.isnan(rows[0]).all() and (info[0, :, 0] == 0).all() and (info[0, :, 2] == 0).all()
    assert np.isfinite(rows[1, 1]).all() and info[1, 1, 0] == 121      # one more sample: a variance
    assert np.isnan(rows[2, 1]).all() and info[2, 1, 1] == -1 and np.isnan(info[2, 1, 3]) and info[2, 1, 2] > 0
    assert np.isfinite(rows[2, 0]).all() and np.isfinite(rows[2, 2]).all()
    assert np.isnan(rows[3]).all()


def test_non_finite_samples():
    """NaN, +inf, -inf in the event window: the row is NaN.  In the partner: exactly the lags whose window holds the
    sample; other partners and regions keep the bytes they have without it."""
    x, regions, partners, L = xd.case('nonfinite')
    clean = xd.slab('main')
    rows, info = computed('nonfinite')
    slab = Slab(clean)
    try:
        ref, ref_info = slab.xcorr(regions, partners, L)
    finally:
        slab.free()
    for i in (0, 1, 2, 4):
        assert np.isnan(rows[i]).all() and (info[i, :, :2] == [0, -1]).all() and np.isnan(info[i, :, 2:]).all(), i
    # region 3 = (1, 9100, 9160): x[2, 9100] is NaN -- the pivot of partner 2 -- and x[3, 9130], x[3, 9190] are infinite
    i, (c, a, b) = 3, regions[3].tolist()
    lags = np.arange(-L, L + 1)
    for j, bad in ((partners.index(2), [9100]), (partners.index(3), [9130, 9190])):
        want = np.zeros(2*L + 1, dtype=bool)
        for pos in bad:
            want |= (a + lags <= pos) & (pos < b + lags)
        assert np.array_equal(np.isnan(rows[i, j]), want), j
        assert 0 < want.sum() < 2*L + 1
    assert np.isnan(rows[3, partners.index(2), :L + 1]).all() and np.isfinite(rows[3, partners.index(2), L + 1:]).all()
    for j in (partners.index(4), partners.index(1)):
        assert rows[3, j].tobytes() == ref[3, j].tobytes() and info[3, j].tobytes() == ref_info[3, j].tobytes()
    assert rows[5].tobytes() == ref[5].tobytes() and info[5].tobytes() == ref_info[5].tobytes()
    # where the pivot is finite, the lags clear of the sample keep their bytes too
    j = partners.index(3)
    keep = ~np.isnan(rows[3, j])
    assert rows[3, j][keep].tobytes() == ref[3, j][keep].tobytes()


def test_bit_identity_whatever_rides_in_the_call():
    """Twice; regions and partners permuted; a region alone and with 40 others; partners repeated; more channels."""
    x = xd.slab('main')
    slab = Slab(x)
    regions = [(0, 5001, 5001 + n) for n in (2, 65, xd.TILE + 1)] + [(2, xd.MAIN_FRAMES - 205, xd.MAIN_FRAMES - 5),
                                                                      (3, 3, 203), (1, 1001, 1001 + xd.CHUNK + 1)]
    partners = [0, 1, 2, 3, 4]
    try:
        for L in (0, 8, 255):
            rows, info = slab.xcorr(regions, partners, L)
            again = slab.xcorr(regions, partners, L)
            assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == info.tobytes()
            r2, i2 = slab.xcorr(regions[::-1], [3, 3, 0, 4, 2, 1, 3], L)
            order = [2, 5, 4, 0, 3]                                     # where partners 0 ... 4 are in that list
            assert r2[::-1][:, order].tobytes() == rows.tobytes() and i2[::-1][:, order].tobytes() == info.tobytes()
            assert r2[:, 0].tobytes() == r2[:, 1].tobytes() == r2[:, 6].tobytes()
        L = 8
        rows, info = slab.xcorr(regions, partners, L)
        others = [(k % 5, 100 + 37*k, 100 + 37*k + 50 + 61*k) for k in range(40)]
        for i in (1, 2, 5):
            alone = slab.xcorr([regions[i]], [2], L)
            crowd = slab.xcorr(others[:20] + [regions[i]] + others[20:], [4, 2], L)
            assert alone[0][0, 0].tobytes() == rows[i, 2].tobytes() == crowd[0][20, 1].tobytes()
            assert alone[1][0, 0].tobytes() == info[i, 2].tobytes() == crowd[1][20, 1].tobytes()
        wide = Slab(np.concatenate((x, np.ones((3, x.shape[1]), dtype=np.float32))))
        try:
            assert wide.xcorr(regions, partners, L)[0].tobytes() == rows.tobytes()
        finally:
            wide.free()
        # rows at 4-byte addresses that are no multiple of 16, an odd pitch: the same bytes
        odd = Slab(x, pitch_extra=7, base=3)
        try:
            assert (odd.view.ptr % 16, odd.pitch % 2) == (12, 1)
            r3, i3 = odd.xcorr(regions, partners, L)
            assert r3.tobytes() == rows.tobytes() and i3.tobytes() == info.tobytes()
        finally:
            odd.free()
    finally:
        slab.free()


def test_scratch_contents_do_not_reach_the_result():
    from audian_amd import hipdsp
    outs = []
    for fill in (0x00, 0xff):
        c = hipdsp.Context(0)
        c.set_option('scratch_fill', fill + 1)
        for name in ('lengths', 'lag255', 'chunks'):
            x, regions, partners, L = xd.case(name)
            slab = Slab(x, ctx=c)
            try:
                rows, info = slab.xcorr(regions, partners, L)
            finally:
                slab.free()
            outs.append((rows.tobytes(), info.tobytes()))
            assert outs[-1] == (computed(name)[0].tobytes(), computed(name)[1].tobytes()), (name, fill)
        c.set_option('scratch_fill', 0)
    assert outs[:3] == outs[3:]


def test_refusals_leave_the_outputs_alone():
    """One refused call per error class with out and info pre-filled: both untouched, and the next valid call gives its
    bytes again."""
    from audian_amd import _lib, hipdsp
    x, regions, partners, L = xd.case('lag8')
    slab = Slab(x)
    R, P, W = len(regions), len(partners), 2*L + 1
    out = hipdsp.DeviceArray.from_host(slab.ctx, np.full((R, P, W), SENTINEL, dtype=np.float32))
    info = hipdsp.DeviceArray.from_host(slab.ctx, np.full((R, P, 4), SENTINEL))
    par = np.array(partners, dtype=np.intc)

    def call(regs=regions, x_ptr=None, frames=None, pitch=None, tab=True, partner_list=par, n_partners=None, lag=L,
             out_ptr=None, out_pitch=0, info_ptr=None, n=None, ctx=True):
        t = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 3)
        p = np.ascontiguousarray([] if partner_list is None else partner_list, dtype=np.intc)
        st = _lib.lib.hipdsp_region_xcorr(
            slab.ctx.handle if ctx else None, ctypes.c_void_p(slab.view.ptr if x_ptr is None else x_ptr),
            slab.pitch if pitch is None else pitch, slab.C, slab.frames if frames is None else frames,
            t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if tab else None, len(t) if n is None else n,
            p.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if partner_list is not None else None,
            len(p) if n_partners is None else n_partners, lag, ctypes.c_void_p(out.ptr if out_ptr is None else out_ptr),
            out_pitch, ctypes.c_void_p(info.ptr if info_ptr is None else info_ptr))
        slab.ctx.synchronize()
        assert np.all(out.to_host() == SENTINEL) and np.all(info.to_host() == SENTINEL)
        return st

    bad = regions.copy()
    try:
        assert call(ctx=False) == _lib.ERR_INVALID                      # a NULL argument, one of each
        assert call(x_ptr=0) == _lib.ERR_INVALID
        assert call(tab=False) == _lib.ERR_INVALID
        assert call(partner_list=None, n_partners=2) == _lib.ERR_INVALID
        assert call(out_ptr=0) == _lib.ERR_INVALID
        assert call(info_ptr=0) == _lib.ERR_INVALID
        assert call(n=-1) == _lib.ERR_INVALID                           # negative sizes
        assert call(n_partners=-1) == _lib.ERR_INVALID
        assert call(frames=-1) == _lib.ERR_INVALID
        assert call(frames=slab.pitch + 1) == _lib.ERR_INVALID          # x_pitch < frames
        assert call(out_pitch=W - 1) == _lib.ERR_INVALID
        for row in ((5, 0, 10), (-1, 0, 10), (0, -1, 10), (0, 0, slab.frames + 1), (0, 20, 10)):
            bad[1] = row
            assert call(regs=bad) == _lib.ERR_INVALID, row
        assert call(partner_list=[1, 5]) == _lib.ERR_INVALID
        assert call(partner_list=[-1]) == _lib.ERR_INVALID
        assert call(lag=-1) == _lib.ERR_INVALID
        assert call(x_ptr=slab.view.ptr + 2) == _lib.ERR_INVALID        # misaligned pointers
        assert call(out_ptr=out.ptr + 2) == _lib.ERR_INVALID
        assert call(info_ptr=info.ptr + 4) == _lib.ERR_INVALID
        assert call(lag=1025) == _lib.ERR_UNSUPPORTED
        assert call(n=0) == _lib.OK and call(n_partners=0) == _lib.OK   # nothing to do: nothing written
        hipdsp.region_xcorr_into(slab.ctx, slab.view, slab.pitch, slab.C, slab.frames, regions, partners, L, out, info)
        assert out.to_host().tobytes() == computed('lag8')[0].tobytes()
        assert info.to_host().tobytes() == computed('lag8')[1].tobytes()
    finally:
        out.free()
        info.free()
        slab.free()


def test_out_pitch_and_untouched_padding():
    from audian_amd import hipdsp
    x, regions, partners, L = xd.case('lag4')
    slab = Slab(x)
    R, P, W = len(regions), len(partners), 2*L + 1
    pitch = W + 5
    pad = hipdsp.DeviceArray.from_host(slab.ctx, np.full(R*P*pitch, SENTINEL, dtype=np.float32))
    info = hipdsp.DeviceArray(slab.ctx, (R, P, 4), np.float64)
    try:
        hipdsp.region_xcorr_into(slab.ctx, slab.view, slab.pitch, slab.C, slab.frames, regions, partners, L, pad, info,
                                 out_pitch=pitch)
        got = pad.to_host().reshape(R, P, pitch)
        assert np.all(got[:, :, W:] == SENTINEL)
        assert np.ascontiguousarray(got[:, :, :W]).tobytes() == computed('lag4')[0].tobytes()
        assert info.to_host().tobytes() == computed('lag4')[1].tobytes()
    finally:
        pad.free()
        info.free()
        slab.free()


def test_refused_inside_a_graph_capture():
    from audian_amd import hipdsp
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    x = xd.slab('small')
    dx = hipdsp.DeviceArray.from_host(c, x)
    dz = hipdsp.DeviceArray.from_host(c, np.zeros((1, 500), dtype=np.float32))
    out = hipdsp.DeviceArray.from_host(c, np.full((1, 1, 5), SENTINEL, dtype=np.float32))
    info = hipdsp.DeviceArray.from_host(c, np.full((1, 1, 4), SENTINEL))
    c.graph_begin()
    try:
        hipdsp.decibel(c, dz, dz, 500)                                  # something legal to capture
        with pytest.raises(ValueError, match='capture'):
            hipdsp.region_xcorr_into(c, dx, 700, 3, 700, [(0, 10, 310)], [1], 2, out, info)
    finally:
        graph = c.graph_end()
    c.graph_launch(graph)
    c.synchronize()
    assert np.all(out.to_host() == SENTINEL) and np.all(info.to_host() == SENTINEL)
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)


def test_far_row_base():
    """The event's row starts past element 2^31 (row 4 of far_placement's by-row plan, its partner in row 3): bit for bit
    what the same windows give in rows 1 and 0, near the start, and within the contract."""
    from audian_amd import hipdsp
    from test_gpu_far_indices import Far, placed
    chunk = xd.TILE
    n = fp.window_length(chunk)
    rng = np.random.default_rng(17)
    va = rng.uniform(-1, 1, n).astype(np.float32)
    vb = (0.5*np.roll(va, 2) + rng.uniform(-1, 1, n)).astype(np.float32)
    L, margin = 8, 16
    a = fp.IN_ROW + fp.PHASE
    frames = fp.row_frames(n, chunk)
    windows = fp.by_row(n, chunk)
    assert windows[4].start - a == 4*fp.ROW_PITCH > 2**31 and fp.ROWS == 5
    regions = [(1, a + margin, a + n - margin), (4, a + margin, a + n - margin)]
    far = Far()
    try:
        with placed(far, windows, [vb, va, va, vb, va]):
            rows, info = hipdsp.region_xcorr(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, frames, regions, [0, 3], L)
    finally:
        far.free()
    assert rows[1, 1].tobytes() == rows[0, 0].tobytes() and info[1, 1].tobytes() == info[0, 0].tobytes()
    host = np.zeros((2, frames), dtype=np.float32)
    host[0, a:a + n], host[1, a:a + n] = va, vb
    q = xd.region_xcorr(host, 0, a + margin, a + n - margin, 1, L)
    assert np.nanmax(xd.bound_T(q)) < xd.T_LIMIT
    xd.compare(q, rows[1, 1], info[1, 1], 'far', limit=xd.T_LIMIT)
    assert np.isfinite(rows[1, 1]).all() and info[1, 1, 1] == L + 2


# ---- the facade ----------------------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True

    def setVisible(self, show):
        pass


def crosstalk_graph(shift=5, gain=0.3):
    """A filter on four channels x 60 s x 16 kHz of weak noise with three songs of one second: one on channel 1 that
    channel 2 carries `shift` samples later at `gain` times the amplitude, one of its own on channel 3, one on channel 0
    that channel 1 carries.  Buffers as in tests/test_gpu_events.py: 30 s, which hold a window and the filter's margins."""
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.tracegraph import TraceGraph
    rate, seconds = 16000.0, 60.0
    rng = np.random.default_rng(21)
    n = int(rate*seconds)
    x = 0.01*rng.standard_normal((n, 4))
    songs = []
    for t0, src, dst in [(53.0, 1, 2), (54.5, 3, None), (56.0, 0, 1)]:
        a = int(t0*rate)
        song = rng.standard_normal(int(rate))
        x[a:a + len(song), src] += song
        if dst is not None:
            x[a + shift:a + shift + len(song), dst] += gain*song
        songs.append((a, a + len(song), src, dst))
    g = TraceGraph(30.0, 2.0)
    g.add_trace(BufferedFilter())
    g.setup_traces()
    g.open(x.astype(np.float32).astype(np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    g['filtered'].highpass_cutoff, g['filtered'].lowpass_cutoff = 300.0, 3000.0
    g['filtered'].update()
    return g, songs


def test_facade_on_the_mirror_and_after_a_scroll():
    """BufferedData.region_xcorr on the device mirror is BufferedArray.region_xcorr under the comparator, in ONE call and
    with nothing read back, before and after scrolls.  A host write next to a window takes its frames out of the valid
    mirror while the device still holds the old samples there: a region whose shifted windows reach into them is served
    by numpy on the host buffer (the definition on the true samples tells), one whose reach ends at the seam stays on
    the device.  Every input meets T < 2^-30."""
    from audian_amd import hipdsp
    g, songs = crosstalk_graph()
    f = g['filtered']
    g.update_times(0.0, 5.0)
    assert f._dev is not None and f._dev_valid and f._stale
    lo, hi = f._dev_valid[0]
    L = 8

    def table(lo):
        tab = [(c, f.offset + lo + 100 + 900*c, f.offset + lo + 100 + 900*c + n)
               for c, n in ((0, 300), (1, 2049), (2, 65), (3, 700))]
        return tab + [(1, f.offset + lo, f.offset + lo + 64)]           # at the mirror's first valid frame

    def count():
        return hipdsp.launches.get('region_xcorr', 0)

    stale = [list(r) for r in f._stale]
    before = count()
    xc = f.region_xcorr(table(lo), max_lag=L)
    assert count() == before + 1 and [list(r) for r in f._stale] == stale
    split = f.region_xcorr(iter(table(lo)), max_lag=L, max_bytes=1)    # one call per region: the same bytes
    assert count() == before + 1 + len(xc)
    assert split.r.tobytes() == xc.r.tobytes() and split.info.tobytes() == xc.info.tobytes()
    g.update_times(40.0, 45.0)
    g.update_times(52.0, 58.0)                                          # the scrolls: the buffers move
    assert f.offset > 0 and f._dev_valid
    lo, hi = f._dev_valid[0]
    n = len(f._hostbuf)
    assert hi - lo >= 20000
    stale = [list(r) for r in f._stale]
    before = count()
    mirror = f.region_xcorr(table(lo), max_lag=L)
    assert count() == before + 1 and [list(r) for r in f._stale] == stale
    # the host write: 40 frames, 5000 behind the mirror's first valid frame, clear of every region above
    p, q = lo + 5000, lo + 5040
    f.buffer[p:q] = 0.25*np.random.default_rng(3).standard_normal((q - p, 4)).astype(np.float32)
    assert not f._mirror_valid(p, q) and f._mirror_valid(lo, p) and f._mirror_valid(q, hi)
    o = f.offset
    crossing = [(0, o + p - 303, o + p - 3), (1, o + q + L - 1, o + q + L + 199), (3, o + p - 200, o + p)]
    at_seam = [(2, o + q + L, o + q + L + 200), (1, o + p - L - 200, o + p - L)]
    results = [('mirror', mirror)]
    before = count()
    for k, region in enumerate(crossing):                              # valid windows whose lags reach the written frames
        assert f._mirror_valid(region[1] - o, region[2] - o)
        results.append(('crossing %d' % k, f.region_xcorr(iter([region]), max_lag=L)))
        assert count() == before
    results.append(('mixed', f.region_xcorr(at_seam + crossing[:1], max_lag=L)))
    assert count() == before
    results.append(('at the seam', f.region_xcorr(at_seam, max_lag=L)))
    assert count() == before + 1
    results.append(('lag 0', f.region_xcorr(crossing[2:], max_lag=0)))   # no lag: the window alone is read
    assert count() == before + 2
    f._regions_on_mirror = lambda tab: False                            # the host version last: it reads the host copy
    results.append(('host', f.region_xcorr(table(lo), max_lag=L)))
    assert count() == before + 2
    x = np.ascontiguousarray(np.asarray(f[f.offset:f.offset + n]).T, dtype=np.float32)
    for what, res in results:
        rel = [(c, a - f.offset, b - f.offset) for c, a, b in res.table.tolist()]
        assert xd.compare_call(x, rel, [0, 1, 2, 3], res.max_lag, res.r, res.info, what, limit=xd.T_LIMIT) <= 1.0
    host = results[-1][1]
    assert np.array_equal(np.isnan(host.r), np.isnan(mirror.r)) and np.nanmax(np.abs(host.r - mirror.r)) <= 2.0**-23


def test_attribute_events_on_a_four_channel_graph():
    """One source copied to a neighbour at 0.3 of the amplitude, 5 samples later: the neighbour's event is attributed to
    the source with a delay of -5 samples; the result is the definition's rule over the definition's numbers."""
    from audian_amd import hipdsp
    from audian_amd.events import Events
    shift = 5
    g, songs = crosstalk_graph(shift=shift)
    f = g['filtered']
    g.update_times(52.0, 58.0)
    rate = f.rate
    pairs = [[] for _ in range(4)]
    for a, b, src, dst in songs:
        pairs[src].append((a, b))
        if dst is not None:
            pairs[dst].append((a + shift - 3, b + shift + 4))           # the neighbour's event as a detector would cut it
    ev = Events([sorted(p) for p in pairs], rate, 'filtered')
    before = hipdsp.launches.get('region_xcorr', 0)
    own, sources, delays = g.attribute_events(ev, max_delay=0.001)
    assert hipdsp.launches['region_xcorr'] == before + 1               # one call for all events and partners
    assert [s.tolist() for s in sources] == [[0], [1, 0], [1], [3]]
    assert delays[2].tolist() == [-shift/rate] and delays[1].tolist() == [0.0, -shift/rate] and delays[3].tolist() == [0.0]
    assert [len(o) for o in own.onsets] == [1, 1, 0, 1]
    n = len(f._hostbuf)
    x = np.ascontiguousarray(np.asarray(f[f.offset:f.offset + n]).T, dtype=np.float32)
    L = int(round(0.001*rate))
    for c in range(4):
        for k, (a, b) in enumerate(ev.frames(c).tolist()):
            qs = [xd.region_xcorr(x, c, a - f.offset, b - f.offset, p, L) for p in range(4)]
            assert all(np.nanmax(xd.bound_T(q)) < xd.T_LIMIT for q in qs), (c, k)
            s, lag = xd.attribute(c, [0, 1, 2, 3], [float(q['r'][int(q['info'][1])]) for q in qs],
                                  [q['info'][1] - L for q in qs], [q['info'][2] for q in qs], [q['info'][3] for q in qs])
            assert (s, lag/rate) == (sources[c][k], delays[c][k]), (c, k)
