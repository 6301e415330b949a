"""hipdsp_common_reference on the device against the definition in common_reference_definition.py -- equal NaN pattern,
equal float32 bits, no tolerance in either mode: the frame counts around every kernel's time tile, the channel counts
around every slot count of the register kernel and the LDS kernel beyond, grouped, excluded and pass-through channels,
every kind of value, in place, determinism, isolation of the groups, every refusal, a captured graph, rows past 2^32
bytes, and BufferedCommonReference between the recording and the filter.

Every call goes through run(): odd pitches (frames + 5 in, frames + 3 out), base pointers one float into their
allocations, the output prefilled with a sentinel: EVERYTHING the call must not write -- 64 floats before the first and
after the last row, the pitch gap of every row, the rows of pass-through channels in place -- must hold it afterwards."""

import ctypes

import numpy as np
import pytest

import common_reference_definition as cd
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0xa5
GUARD = 64
TILES = (32, 512, 1024)                       # hipdsp.CREF_TILES: frames per workgroup of the three kernels
FRAMES = sorted({1, 63, 64, 65} | {f for L in TILES for f in (L - 1, L, L + 1, 3*L + 17)})
FRAMES_LDS = [1, 31, 32, 33, 63, 64, 65, 113, 1025]          # beyond 64 reference channels the tile is 32 frames
CHANNELS = {cd.MEDIAN: [1, 2, 3, 7, 8, 9, 31, 33, 63, 64], cd.MEAN: [1, 2, 3, 9, 64, 65, 200, 1024]}
LAYOUTS = ['one group', 'interleaved', 'use']


def test_the_tiles_are_the_library_s():
    from audian_amd import hipdsp
    assert hipdsp.CREF_TILES == TILES and hipdsp.CREF_TILE == max(TILES)


def make_data(C, T, seed):
    """(C, T) float32.  The samples are independent, so every column draws its kind: normal floats with row scales from
    1e-6 to 1e6, integers in [-3, 3] (ties), denormals, zeros of either sign, a planted NaN, one infinity of either
    sign, +inf and -inf at one sample."""
    rng = np.random.default_rng(seed)
    scales = 10.0**np.linspace(-6, 6, C)[rng.permutation(C)]
    x = (rng.standard_normal((C, T))*scales[:, None]).astype(np.float32)
    kind = rng.integers(0, 7, size=T)
    kind[:min(T, 7)] = rng.permutation(7)[:min(T, 7)]            # short rows: still one column of each kind they hold
    for t in range(T):
        k = kind[t]
        if k == 1:
            x[:, t] = rng.integers(-3, 4, size=C)
        elif k == 2:
            x[:, t] = (rng.integers(-2000, 2001, size=C).astype(np.float64)*2.0**-149).astype(np.float32)
        elif k == 3:
            x[:, t] = np.where(rng.integers(0, 2, size=C) > 0, np.float32(0.0), np.float32(-0.0))
        elif k == 4:
            x[rng.integers(0, C), t] = np.nan
        elif k == 5:
            x[rng.integers(0, C), t] = np.inf if rng.integers(0, 2) else -np.inf
        elif k == 6:
            x[rng.integers(0, C), t] = np.inf
            x[rng.integers(0, C), t] = -np.inf                   # both at one sample (in the same row the second stays)
    return x


def layout(kind, C):
    """(group, use) of a call whose largest group has C members."""
    if kind == 'one group':
        return np.zeros(C, dtype=np.int32), None
    if kind == 'use':                                            # the first, the last and a middle member do not contribute
        use = np.ones(C, dtype=np.uint8)
        for c in ([], [0], [0, 2], [0, C//2, C - 1])[min(C, 4) - 1]:
            use[c] = 0
        return np.full(C, C - 1, dtype=np.int32), use
    # even and odd channels in two groups, three pass-through channels in the middle of them
    n = C + 3 if C + 3 <= 1024 else C
    group = np.full(n, -1, dtype=np.int32)
    members = [c for c in range(n) if not n//2 - 1 <= c < n//2 + 2]
    group[members[0::2]] = 1 % n
    group[members[1::2]] = n - 1
    return group, None


def place(c, x, pitch, base, guard):
    """The rows of x at `pitch` in a sentinel-filled allocation, the first `guard + base` floats in: (array, host image)."""
    from audian_amd import hipdsp
    C, T = x.shape
    host = np.frombuffer(bytes([SENTINEL_BYTE])*(4*(2*guard + base + C*pitch)), dtype=np.float32).copy()
    for k in range(C):
        a = guard + base + k*pitch
        host[a:a + T] = x[k]
    return hipdsp.DeviceArray.from_host(c, host), host


def run(x, group, use, mode, in_place=False, c=None):
    """hipdsp_common_reference of the (C, T) float32 array x: (C, T) float32 (in place: rows of group -1 as they were)."""
    from audian_amd import hipdsp
    c = gh.ctx() if c is None else c
    C, T = x.shape
    group = np.asarray(group)
    if in_place:
        pitch = T + 5
        dy, before = place(c, x, pitch, 1, GUARD)
        hipdsp.common_reference(c, dy.view(GUARD + 1, (1,)), pitch, dy.view(GUARD + 1, (1,)), pitch, C, T, group, use, mode)
        raw = dy.to_host()
        dy.free()
    else:
        pitch = T + 3
        dx, image = place(c, x, T + 5, 1, 0)
        dy, before = place(c, np.zeros((0, T), dtype=np.float32), pitch, 1 + C*pitch, GUARD)
        hipdsp.common_reference(c, dx.view(1, (1,)), T + 5, dy.view(GUARD + 1, (1,)), pitch, C, T, group, use, mode)
        raw = dy.to_host()
        assert dx.to_host().tobytes() == image.tobytes(), 'the input was written'
        dx.free()
        dy.free()
    written = np.zeros(len(raw), dtype=bool)
    for k in range(C):
        if not in_place or group[k] >= 0:
            a = GUARD + 1 + k*pitch
            written[a:a + T] = True
    assert raw[~written].tobytes() == before[~written].tobytes(), 'an element outside the output rows was written'
    return np.ascontiguousarray(raw[GUARD + 1:GUARD + 1 + C*pitch].reshape(C, pitch)[:, :T])


MODES = [cd.MEAN, cd.MEDIAN]


@pytest.mark.parametrize('kind', LAYOUTS)
@pytest.mark.parametrize('mode', MODES)
def test_against_the_definition(mode, kind):
    for C in CHANNELS[mode]:
        group, use = layout(kind, C)
        used = np.ones(len(group), dtype=bool) if use is None else use.astype(bool)
        refs = max(np.sum((group == g) & used) for g in set(group[group >= 0].tolist()))
        for T in (FRAMES if refs <= 64 else FRAMES_LDS):
            x = make_data(len(group), T, 1000*C + T)
            what = '%s, %s, %d channels, %d frames' % (mode, kind, len(group), T)
            want = cd.common_reference(x, group, use, mode)
            got = run(x, group, use, mode)
            cd.assert_same(got, want, what)
            passing = group < 0
            assert got[passing].tobytes() == x[passing].tobytes(), what + ': a pass-through row is not a copy'
            again = run(x, group, use, mode)
            assert again.tobytes() == got.tobytes(), what + ': two runs differ'
            there = run(x, group, use, mode, in_place=True)
            assert there.tobytes() == got.tobytes(), what + ': in place differs'


@pytest.mark.parametrize('mode', MODES)
def test_a_group_depends_on_its_rows_alone(mode):
    """Group A's rows are byte-equal whether group B rides in the call or B's channels pass through -- also when the
    larger B moves the call to another kernel (more row slots, the LDS tile)."""
    for nb in (3, 20, 70 if mode == cd.MEAN else 64):
        T = 1500
        na = 5
        x = make_data(na + nb, T, 77 + nb)
        group = np.array([0 if c % 2 == 0 and c < 2*na else 1 for c in range(na + nb)], dtype=np.int32)
        use = np.ones(na + nb, dtype=np.uint8)
        use[2] = 0
        rows = group == 0
        both = run(x, group, use, mode)
        alone = run(x, np.where(rows, 0, -1), use, mode)
        assert both[rows].tobytes() == alone[rows].tobytes()
        apart = run(np.ascontiguousarray(x[rows]), np.zeros(int(rows.sum()), dtype=np.int32), use[rows], mode)
        assert both[rows].tobytes() == apart.tobytes()
        cd.assert_same(both, cd.common_reference(x, group, use, mode))


# ---- refusals ---------------------------------------------------------------------------------------------------------

INVALID, UNSUPPORTED = 1, 3


def refused(status, C, T, group, use=None, mode=0, x_pitch=None, y_pitch=None, y_in_x=None):
    """The call is refused with `status` and a message and writes nothing; the next valid call gives the bytes of a run
    of its own.  y_in_x = k: y lies k floats behind x in x's own allocation."""
    from audian_amd import _lib, hipdsp
    c = gh.ctx()
    xp, yp = T + 5, T + 3
    dx, image = place(c, make_data(min(C, 1024) + 2, T, 5), xp, 1, GUARD)        # (two rows more: room for a shifted y)
    dy, blank = place(c, np.zeros((0, T), dtype=np.float32), yp, 1 + (C + 1)*yp, GUARD)
    garr = (ctypes.c_int*len(group))(*[int(g) for g in group])
    uarr = None if use is None else (ctypes.c_ubyte*len(use))(*[int(u) for u in use])
    xptr = dx.ptr + 4*(GUARD + 1)
    yptr = dy.ptr + 4*(GUARD + 1) if y_in_x is None else xptr + 4*y_in_x
    if y_in_x is not None and y_pitch is None:
        y_pitch = xp
    rc = _lib.lib.hipdsp_common_reference(c.handle, ctypes.c_void_p(xptr), int(xp if x_pitch is None else x_pitch),
                                          ctypes.c_void_p(yptr), int(yp if y_pitch is None else y_pitch), int(C), int(T), garr,
                                          uarr, int(mode))
    msg = _lib.last_error()
    assert rc == status and msg, (rc, msg)
    with pytest.raises(ValueError if status == INVALID else NotImplementedError):
        hipdsp.check(rc)
    c.synchronize()
    assert dx.to_host().tobytes() == image.tobytes() and dy.to_host().tobytes() == blank.tobytes()
    dx.free()
    dy.free()
    g, u = layout('use', 9)
    for m in MODES:
        assert run(make_data(9, 600, 6), g, u, m).tobytes() == VALID[m].tobytes()


class _Valid(dict):
    """The stand-alone runs the refusal tests compare with, computed once."""

    def __missing__(self, m):
        g, u = layout('use', 9)
        v = make_data(9, 600, 6)
        self[m] = run(v, g, u, m)
        cd.assert_same(self[m], cd.common_reference(v, g, u, m))
        return self[m]


VALID = _Valid()


def test_refuses_a_group_id_out_of_range():
    refused(INVALID, 4, 100, [0, 4, 0, 0])
    refused(INVALID, 4, 100, [0, -2, 0, 0], mode=1)


def test_refuses_a_group_without_reference_channels():
    refused(INVALID, 4, 100, [0, 2, 0, 2], use=[1, 0, 1, 0])


def test_refuses_an_unknown_mode():
    refused(INVALID, 4, 100, [0, 0, 0, 0], mode=2)
    refused(INVALID, 4, 100, [0, 0, 0, 0], mode=-1)


def test_refuses_a_partial_overlap():
    refused(INVALID, 4, 100, [0, 0, 0, 0], y_in_x=1)                    # y one float behind x
    refused(INVALID, 4, 100, [0, 0, 0, 0], y_in_x=50, mode=1)
    refused(INVALID, 4, 100, [0, 0, 0, 0], y_in_x=0, y_pitch=104)       # y == x, another pitch
    refused(INVALID, 4, 100, [0, -1, -1, 0], y_in_x=105)                # y one row behind x
    refused(INVALID, 4, 100, [0, 0, 0, 0], y_in_x=-3, y_pitch=103)


def test_refuses_a_pitch_below_the_rows():
    refused(INVALID, 4, 100, [0, 0, 0, 0], x_pitch=99)
    refused(INVALID, 4, 100, [0, 0, 0, 0], y_pitch=99)


def test_refuses_more_than_1024_channels():
    refused(UNSUPPORTED, 1025, 8, [0]*1025)


def test_refuses_a_median_over_more_than_64_reference_channels():
    refused(UNSUPPORTED, 65, 100, [0]*65, mode=1)
    use = [1]*66
    use[3] = 0
    refused(UNSUPPORTED, 66, 100, [0]*66, use=use, mode=1)
    # 64 of 66 members is served
    use[60] = 0
    x = make_data(66, 100, 8)
    cd.assert_same(run(x, [0]*66, use, cd.MEDIAN), cd.common_reference(x, [0]*66, use, cd.MEDIAN))


# ---- a captured graph -------------------------------------------------------------------------------------------------

def graph_shape(graph):
    """(nodes, edges) of a captured hipdsp_graph (its first member is the hipGraph_t, audian_amd/csrc/common.h)."""
    from audian_amd import _lib
    hip = ctypes.CDLL(_lib.hip_runtime_path()[0])
    g = ctypes.c_void_p.from_address(graph.value).value
    nodes, edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g), None, ctypes.byref(nodes)) == 0
    assert hip.hipGraphGetEdges(ctypes.c_void_p(g), None, None, ctypes.byref(edges)) == 0
    return nodes.value, edges.value


@pytest.mark.parametrize('mode', MODES)
def test_inside_a_captured_graph(mode):
    """Nothing is uploaded, allocated or synchronised: one call is one kernel node, and a replay reads the x of its time."""
    from audian_amd import hipdsp
    C, T = 12, 2100
    group, use = layout('interleaved', C)
    n = len(group)
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    xs = [make_data(n, T, 31), make_data(n, T, 32)]
    dx = hipdsp.DeviceArray.from_host(c, xs[0])
    dy = hipdsp.DeviceArray(c, (n, T), np.float32)
    c.synchronize()
    c.graph_begin()
    hipdsp.common_reference(c, dx, 0, dy, 0, n, T, group, use, mode)           # (pitch 0: frames)
    graph = c.graph_end()
    assert graph_shape(graph) == (1, 0)
    for x in xs:
        dx.copy_from_host(x)
        hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(dy), SENTINEL_BYTE, dy.nbytes)
        c.graph_launch(graph)
        c.synchronize()
        cd.assert_same(dy.to_host(), cd.common_reference(x, group, use, mode), mode)
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)
    dx.free()
    dy.free()
    c.pool_trim()


# ---- rows past 2^32 bytes ---------------------------------------------------------------------------------------------

def test_far_rows():
    """Three rows 2^30 + 3 floats apart in x and in y: rows 1 and 2 start past 2^32 bytes.  Both modes against the
    definition and bit for bit against the same data at pitch `frames`; 64 sentinel floats around every output row hold."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, T, pitch = 3, 4096, 2**30 + 3
    x = make_data(C, T, 99)
    total = 2*GUARD + (C - 1)*pitch + T
    dx = hipdsp.DeviceArray(c, (total,), np.float32)
    dy = hipdsp.DeviceArray(c, (total,), np.float32)
    sentinel = np.frombuffer(bytes([SENTINEL_BYTE])*(4*(T + 2*GUARD)), dtype=np.float32)
    try:
        for k in range(C):
            dx.view(GUARD + k*pitch, (T,)).copy_from_host(x[k])
        for mode in MODES:
            for k in range(C):
                dy.view(k*pitch, (T + 2*GUARD,)).copy_from_host(sentinel)
            hipdsp.common_reference(c, dx.view(GUARD, (1,)), pitch, dy.view(GUARD, (1,)), pitch, C, T, [0]*C, None, mode)
            got = np.empty((C, T), dtype=np.float32)
            for k in range(C):
                row = dy.view(k*pitch, (T + 2*GUARD,)).to_host()
                assert row[:GUARD].tobytes() == sentinel[:GUARD].tobytes() == row[GUARD + T:].tobytes(), (mode, k)
                got[k] = row[GUARD:GUARD + T]
            cd.assert_same(got, cd.common_reference(x, [0]*C, None, mode), mode)
            assert got.tobytes() == run(x, [0]*C, None, mode).tobytes(), mode
            for k in range(C):                                   # the input rows were not written
                assert dx.view(GUARD + k*pitch, (T,)).to_host().tobytes() == x[k].tobytes()
    finally:
        dx.free()
        dy.free()
        c.pool_trim()


# ---- the facade -------------------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True


def test_facade_between_the_recording_and_the_filter():
    """data -> rereferenced -> filtered on the device: the mirror of `rereferenced` is the definition, `filtered` is
    hipdsp_sosfilt of it; update(method='median') changes both and neither uploads the recording again nor launches
    anything for it."""
    from audian_amd import hipdsp
    from audian_amd.bufferedcommonreference import BufferedCommonReference
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.tracegraph import TraceGraph
    rate, C, n = 20000.0, 8, 20000
    rng = np.random.default_rng(17)
    hum = np.sin(2*np.pi*50.0*np.arange(n)/rate)
    x = (0.1*rng.standard_normal((n, C)) + hum[:, None]).astype(np.float32)
    x[:, 5] *= 40.0                                              # one loud channel
    groups, exclude = [[0, 1, 2, 5, 6], [3, 7]], (6,)            # channel 4 passes through
    ref = BufferedCommonReference(groups=groups, exclude=exclude)
    filt = BufferedFilter(source='rereferenced')
    filt.source_tbefore = 0
    g = TraceGraph(10.0, 0.0)
    g.add_trace(ref)
    g.add_trace(filt)
    g.setup_traces()
    g.open(x.astype(np.float64), rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    filt.highpass_cutoff, filt.lowpass_cutoff = 500.0, 5000.0
    filt.update()
    g.update_times(0.0, n/rate)
    assert ref.source is g.data and filt.source is ref and len(ref.buffer) == n == len(filt.buffer)
    group, use = ref.group, ref.use
    assert group.tolist() == [0, 0, 0, 1, -1, 0, 0, 1] and use.tolist() == [1, 1, 1, 1, 1, 1, 0, 1]

    def check(method):
        assert ref._dev is not None and ref._dev_valid == [[0, n]]
        mirror = ref._dev.to_host()[:C, :n]
        want = cd.common_reference(np.ascontiguousarray(x.T), group, use, method)
        cd.assert_same(np.ascontiguousarray(mirror), want, method)
        cd.assert_same(np.ascontiguousarray(np.asarray(ref.buffer).T).astype(np.float32), want, method + ', read back')
        dw = hipdsp.DeviceArray.from_host(ref.ctx, want)
        dout = hipdsp.DeviceArray(ref.ctx, (C, n), np.float32)
        hipdsp.sosfilt(ref.ctx, filt._plans[0], dw, n, dout, n, C, n, 0)
        assert len(filt._plans) == 1
        assert filt._dev.to_host()[:C, :n].tobytes() == dout.to_host().tobytes()
        return want, dout.to_host()

    mean, mean_filtered = check('mean')
    raw_copy = ref._raw_cache
    before = dict(hipdsp.launches)
    ref.update(method='median')
    assert hipdsp.launches['common_reference'] == before['common_reference'] + 1
    assert hipdsp.launches['sosfilt'] == before['sosfilt'] + 1
    assert {k: v for k, v in hipdsp.launches.items() if k not in ('common_reference', 'sosfilt')} == \
        {k: v for k, v in before.items() if k not in ('common_reference', 'sosfilt')}
    assert ref._raw_cache is raw_copy and raw_copy is not None              # the recording's device copy was reused
    median, median_filtered = check('median')
    assert not np.array_equal(mean, median) and not np.array_equal(mean_filtered, median_filtered)
    # the loud channel leaks into the mean's group with opposite sign, not into the median's
    assert np.std(median[0].astype(np.float64)) < 0.5*np.std(mean[0].astype(np.float64))
    with pytest.raises(ValueError):
        ref.update(groups=[[0, 8]])
    assert hipdsp.launches['common_reference'] == before['common_reference'] + 1
