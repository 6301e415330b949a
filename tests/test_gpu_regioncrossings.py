"""hipdsp_region_crossings on the GPU, exact against tests/refine_definition.region_crossings (a sequential loop over
the samples).

The kernel cuts a region into chunks of K = hipdsp.CROSSINGS_CHUNK = 4096 samples counted from the region's start, one
256-thread workgroup per chunk, and one thread per region merges the chunks in ascending order.  So of the lengths used
here 0 launches no chunk at all, 1, 2, 63, 64, 65 stay inside one wave's first pass over the chunk, K-1, K, K+1 lie
around one chunk (K+1: a second chunk of one sample, the merge's first step) and 3K+5 takes the merge past its first
step."""

import ctypes
import functools

import numpy as np
import pytest

import gpu_helpers as gh
import refine_definition as rd

pytestmark = pytest.mark.gpu

K = 4096                                        # hipdsp.CROSSINGS_CHUNK
LENGTHS = [0, 1, 2, 63, 64, 65, K - 1, K, K + 1, 3*K + 5]
STARTS = [0, 1, 2, 3, 5]
BASE = 3
FRAMES = 3*K + 5 + 5 + 11


def test_constant():
    from audian_amd import hipdsp
    assert hipdsp.CROSSINGS_CHUNK == K


class Slab(object):
    """As test_gpu_regionspectra.Slab: base offset 3 elements, pitch = frames + 7."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        host = np.full(BASE + self.C*self.pitch, 12345.0, dtype=np.float32)
        for c in range(self.C):
            host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, host)
        self.view = self.dev.view(BASE, (1,))

    def crossings(self, regions, thresholds, channels=None):
        from audian_amd import hipdsp
        return hipdsp.region_crossings(self.ctx, self.view, self.pitch, self.C if channels is None else channels,
                                       self.frames, regions, thresholds)


def expect(x, regions, thresholds):
    thresholds = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(regions),))
    return np.array([rd.region_crossings(x[c], a, b, t) for (c, a, b), t in zip(regions, thresholds)]).reshape(-1, 8)


def same(got, want):
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


@functools.lru_cache(maxsize=None)
def noise():
    rng = np.random.default_rng(17)
    x = rng.standard_normal((3, FRAMES)).astype(np.float32)
    return x, Slab(x)


def all_regions():
    return [((i + j) % 3, s, s + n) for i, n in enumerate(LENGTHS) for j, s in enumerate(STARTS)]


def test_lengths_starts_and_thresholds():
    """Every length at every start, thresholds below every sample, above every sample, equal to the region's largest
    sample (not above), NaN and +inf, and two in the middle -- one call per threshold kind, and one with a different
    threshold for every region."""
    x, slab = noise()
    regions = all_regions()
    top = np.array([x[c, a:b].max() if b > a else 0.0 for c, a, b in regions], dtype=np.float64)
    for thr in (-10.0, 10.0, top, np.nan, np.inf, -np.inf, 0.0, 1.5, np.nextafter(top.astype(np.float32), np.float32(-9)).astype(np.float64),
                np.linspace(-2.0, 2.0, len(regions))):
        got = slab.crossings(regions, thr)
        want = expect(x, regions, thr)
        assert same(got, want), thr
    got = slab.crossings(regions, top)
    assert np.all(got[:, 1] == 0) and np.all(got[:, 2:4] == -1)                 # equal to the threshold is not above
    got = slab.crossings(regions, np.nan)
    assert np.all(got[:, 1] == 0) and same(got[:, 4:6], expect(x, regions, 0.0)[:, 4:6])      # the maxima alone


def test_single_samples_above():
    """Only the first sample, only the last, only the first sample of the second chunk."""
    x = np.zeros((2, FRAMES), dtype=np.float32)
    slab_regions = []
    for j, n in enumerate([1, 2, 64, 65, K, K + 1, 3*K + 5]):
        s = STARTS[j % len(STARTS)]
        slab_regions.append((j % 2, s, s + n))
    for which in ('first', 'last', 'second chunk'):
        for c, a, b in slab_regions:
            y = x.copy()
            pos = a if which == 'first' else b - 1 if which == 'last' else a + K
            if pos >= b:
                continue
            y[c, pos] = 2.0
            got = Slab(y).crossings([(c, a, b)], 1.0)
            assert same(got, expect(y, [(c, a, b)], 1.0)), (which, a, b)
            assert got[0, 1:6].tolist() == [1.0, pos, pos + 1, 2.0, pos]


def test_plateau_and_special_samples():
    x, _ = noise()
    x = x.copy()
    regions = [(0, 3, 3 + 3*K + 5), (1, 0, K + 1), (2, 5, 70), (1, K - 10, K + 10)]
    x[0, [100, K + 3, 2*K + 3 + 7]] = 9.0                  # a plateau at the maximum over three chunks: the first one
    x[1, [K - 1, K]] = 7.0                                 # ... on both sides of a chunk border
    x[2, 40] = np.inf
    x[2, 50] = -np.inf
    slab = Slab(x)
    for thr in (0.0, 8.0, np.inf):
        got = slab.crossings(regions, thr)
        assert same(got, expect(x, regions, thr)), thr
    assert slab.crossings(regions, 0.0)[:, 5].tolist() == [100.0, K - 1, 40.0, K - 1]
    x[0, [2*K + 50, K + 90]] = np.nan                      # the first NaN wins over everything, NaN is not above
    x[2, 60] = np.nan
    slab = Slab(x)
    got = slab.crossings(regions, 0.0)
    assert same(got, expect(x, regions, 0.0))
    assert np.isnan(got[0, 4]) and got[0, 5] == K + 90 and np.isnan(got[2, 4]) and got[2, 5] == 60 and got[1, 4] == 7.0


def test_overlapping_and_repeated_regions_and_independence():
    """Regions may overlap or repeat; a region's row does not depend on the call: alone, all together, reversed,
    `channels` raised with unused rows, twice."""
    x, slab = noise()
    regions = [(0, 0, 3*K + 5), (0, 0, 3*K + 5), (0, 100, K + 200), (1, 5, 5), (0, K, 2*K), (2, 7, 7 + K + 1), (0, 100, K + 200)]
    thr = np.array([0.5, 1.0, 0.5, 0.0, 3.9, -5.0, 0.6])
    full = slab.crossings(regions, thr)
    assert same(full, expect(x, regions, thr))
    assert slab.crossings(regions, thr).tobytes() == full.tobytes()
    assert slab.crossings(regions[::-1], thr[::-1])[::-1].tobytes() == full.tobytes()
    wide = Slab(np.concatenate((x, np.ones((2, FRAMES), dtype=np.float32))))
    assert wide.crossings(regions, thr).tobytes() == full.tobytes()
    for i in range(len(regions)):
        assert slab.crossings([regions[i]], thr[i:i + 1]).tobytes() == full[i:i + 1].tobytes()
    assert slab.crossings([], []).shape == (0, 8)


def test_errors_leave_the_output_alone():
    from audian_amd import _lib, hipdsp
    x, slab = noise()
    out = hipdsp.DeviceArray.from_host(slab.ctx, np.full((2, 8), 12345.0))

    def call(regs, x_ptr=None, frames=None, thr=True, out_ptr=None, n=None):
        tab = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 3)
        t = np.zeros(max(1, len(tab)))
        st = _lib.lib.hipdsp_region_crossings(
            slab.ctx.handle, ctypes.c_void_p(slab.view.ptr if x_ptr is None else x_ptr), slab.pitch, slab.C,
            slab.frames if frames is None else frames, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if thr else None, len(tab) if n is None else n,
            ctypes.c_void_p(out.ptr if out_ptr is None else out_ptr))
        slab.ctx.synchronize()
        assert np.all(out.to_host() == 12345.0)
        return st

    good = [(0, 0, 10), (1, 5, 9)]
    assert call([(0, 0, FRAMES + 1), (1, 5, 9)]) == _lib.ERR_INVALID
    assert call([(0, 10, 9), (1, 5, 9)]) == _lib.ERR_INVALID
    assert call([(0, -1, 9), (1, 5, 9)]) == _lib.ERR_INVALID
    assert call([(3, 0, 10), (1, 5, 9)]) == _lib.ERR_INVALID
    assert call([(-1, 0, 10), (1, 5, 9)]) == _lib.ERR_INVALID
    assert call(good, x_ptr=slab.view.ptr + 2) == _lib.ERR_INVALID
    assert call(good, x_ptr=0) == _lib.ERR_INVALID
    assert call(good, thr=False) == _lib.ERR_INVALID
    assert call(good, out_ptr=out.ptr + 4) == _lib.ERR_INVALID
    assert call(good, frames=slab.pitch + 1) == _lib.ERR_INVALID
    assert call(good, n=-1) == _lib.ERR_INVALID
    assert call([], n=0) == _lib.OK
    out.free()


def test_refused_inside_a_graph_capture():
    from audian_amd import hipdsp
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    dx = hipdsp.DeviceArray.from_host(c, np.linspace(0.0, 1.0, 500, dtype=np.float32)[None, :])
    dz = hipdsp.DeviceArray.from_host(c, np.zeros((1, 500), dtype=np.float32))
    out = hipdsp.DeviceArray.from_host(c, np.full((1, 8), 12345.0))
    assert hipdsp.region_crossings(c, dx, 500, 1, 500, [(0, 0, 500)], 0.5)[0, 1] == 250
    c.graph_begin()
    try:
        hipdsp.decibel(c, dx, dz, 500)                                          # something legal to capture
        with pytest.raises(ValueError, match='capture'):
            hipdsp.region_crossings(c, dx, 500, 1, 500, [(0, 0, 500)], 0.5, out=out)
    finally:
        graph = c.graph_end()
    c.graph_launch(graph)
    c.synchronize()
    assert np.all(out.to_host() == 12345.0)
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)
