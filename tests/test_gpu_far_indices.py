"""The analysis, screen and layout entry points at indices, byte offsets and row bases past 2^31 and 2^32.

Two module-scoped device blocks of far_placement.BLOCK float32 elements (17.2 GB each): the input block filled once with
0xff bytes (NaN), the output block with 0xa5 bytes (the sentinel, whatever the element type).  Every call gets block base
+ far_placement.MID elements as its pointer, so an index a kernel has wrapped to 32 bits lands in memory the test owns
and reads NaN or misses its output row: a wrong value, never a fault (tests/far_placement.py, checked on the CPU by
tests/test_far_placement.py).  Only windows of a few chunks with a guard band on each side are written -- the guard
holds values that change the result if read -- and they are set back to the fill afterwards.

By index: one row of 2^31 + 2^22 frames, the window near the start, straddling element 2^29 (byte 2^31), 2^30 (byte
2^32) and 2^31, and past 2^31, one placement in memory at a time.  By row: five rows 2^29 + 2^19 elements apart with the
same in-row window, so c * pitch crosses the same boundaries; output pitches put the output rows across them in the
output block.  Every placement is judged against the entry point's own definition and bound on the host copy of the
window (positions shifted), and equals the near placement bit for bit: the samples and the 4 KB phase are the same and
every one of these kernels anchors its chunk grid at `start` or at the region.

hipdsp_unwrap, the pack/unpack calls and hipdsp_pcm_unpack have no start argument: by index they would have to touch
every element of the row (out of scope here), so they have by-row cases only.  No planned case passes a documented
size limit of its entry point."""

import contextlib
import ctypes
import functools
import math

import numpy as np
import pytest

import decibel_bound as dbb
import events_definition as ed
import far_placement as fp
import gpu_helpers as gh
import iir_bound as ib
import peaks_definition as pd
import refine_definition as rd
from fir_definition import fir_definition

pytestmark = pytest.mark.gpu

NAN_BYTE, SENTINEL_BYTE = 0xff, 0xa5
BIG = np.float32(1.0e6)                        # guard value of the traces: above every threshold, a larger maximum
OUT_GUARD = fp.OUT_GUARD                       # elements checked on each side of every written output row
A = fp.IN_ROW + fp.PHASE                       # by row: the window's start inside its row


class Far(object):
    """The two blocks and the pointers into their middle."""

    def __init__(self):
        from audian_amd import hipdsp
        from audian_amd._lib import check, lib
        self.ctx = gh.ctx()
        self.check, self.lib = check, lib
        self.inp = self.out = None
        try:
            self.inp = hipdsp.DeviceArray(self.ctx, (fp.BLOCK,), np.float32)
            self.out = hipdsp.DeviceArray(self.ctx, (fp.BLOCK,), np.float32)
            self._memset(self.inp.ptr, NAN_BYTE, self.inp.nbytes)
            self._memset(self.out.ptr, SENTINEL_BYTE, self.out.nbytes)
            self.ctx.synchronize()
        except BaseException:
            self.free()                                         # nothing this large stays live behind a failure
            raise
        self.x = self.inp.ptr + 4*fp.MID
        self.y = self.out.ptr + 4*fp.MID

    def free(self):
        try:
            self.ctx.synchronize()
        finally:
            for block in (self.inp, self.out):
                if block is not None:
                    block.free()
            self.inp = self.out = None

    def _memset(self, ptr, value, nbytes):
        self.check(self.lib.hipdsp_memset(self.ctx.handle, ctypes.c_void_p(ptr), value, nbytes))

    def _inside(self, block, ptr, nbytes):
        assert block.ptr <= ptr and ptr + nbytes <= block.ptr + block.nbytes, 'outside the block'

    def X(self, index=0, dtype=np.float32):
        """A device pointer `index` elements of `dtype` behind the input pointer."""
        from audian_amd import hipdsp
        return hipdsp.DeviceArray(self.ctx, (1,), dtype, ptr=self.x + index*np.dtype(dtype).itemsize)

    def Y0(self):
        """The output pointer itself, for a call that places its rows by its own arguments (behind out_rows' check)."""
        from audian_amd import hipdsp
        return hipdsp.DeviceArray(self.ctx, (1,), np.float32, ptr=self.y)

    def out_rows(self, dtype, pitch, rows, n, base=0, guard=OUT_GUARD):
        """The device pointer of `rows` output rows of n elements of `dtype`, pitch elements apart from `base` elements
        behind the output pointer -- after checking that every row and the guard elements beside it lie inside the
        block: no call is made with an output the test does not own."""
        from audian_amd import hipdsp
        size = np.dtype(dtype).itemsize
        assert rows >= 1 and n >= 1 and (rows == 1 or pitch >= n + 2*guard)
        self._inside(self.out, self.y + (base - guard)*size, ((rows - 1)*pitch + n + 2*guard)*size)
        return hipdsp.DeviceArray(self.ctx, (1,), dtype, ptr=self.y + base*size)

    def write(self, index, host):
        """host (float32) to elements [index, index + len) of the input."""
        host = np.ascontiguousarray(host, dtype=np.float32)
        self._inside(self.inp, self.x + 4*index, host.nbytes)
        self.check(self.lib.hipdsp_memcpy_h2d(self.ctx.handle, ctypes.c_void_p(self.x + 4*index),
                                              ctypes.c_void_p(host.ctypes.data), host.nbytes))

    def read(self, base, index, n, dtype):
        out = np.empty(n, dtype=dtype)
        ptr = base + index*out.itemsize
        self._inside(self.inp if base == self.x else self.out, ptr, out.nbytes)
        self.check(self.lib.hipdsp_memcpy_d2h(self.ctx.handle, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                                              out.nbytes))
        return out

    def refill(self, index, n):
        """Elements [index, index + n) of the input back to NaN."""
        self._memset(self.x + 4*index, NAN_BYTE, 4*n)

    def rows(self, dtype, pitch, rows, n, base=0, guard=OUT_GUARD):
        """The (rows, n) elements of `dtype` at base + c * pitch of the output, after checking that the `guard` elements
        on each side of every row still hold the sentinel; the rows are set back to the sentinel."""
        size = np.dtype(dtype).itemsize
        self.out_rows(dtype, pitch, rows, n, base, guard)
        got = np.empty((rows, n), dtype=dtype)
        for c in range(rows):
            at = base + c*pitch - guard
            raw = self.read(self.y, at, n + 2*guard, dtype)
            edge = np.concatenate((raw[:guard], raw[guard + n:])).view(np.uint8)
            assert (edge == SENTINEL_BYTE).all(), 'an element beside output row %d was written' % c
            got[c] = raw[guard:guard + n]
            self._memset(self.y + (at + guard)*size, SENTINEL_BYTE, n*size)
        return got


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL_BYTE).all())


@pytest.fixture(scope='module')
def far():
    f = Far()
    yield f
    f.free()


@contextlib.contextmanager
def placed(far, windows, samples, guard_value=BIG):
    """The windows (each with its guard bands) in the input block while the body runs; `samples` is one array for all
    windows or one per window."""
    per = samples if isinstance(samples, (list, tuple)) else [samples]*len(windows)
    try:
        for w, v in zip(windows, per):
            assert len(v) == w.stop - w.start
            host = np.full(len(v) + 2*w.guard, guard_value, dtype=np.float32)
            host[w.guard:w.guard + len(v)] = v
            far.write(w.start - w.guard, host)
        yield
    finally:
        far.ctx.synchronize()
        for w in windows:
            far.refill(w.start - w.guard, w.stop - w.start + 2*w.guard)


def noise(n, seed, scale=1.0):
    return (scale*np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def same_bits(got, near, what):
    assert np.asarray(got).tobytes() == np.asarray(near).tobytes(), '%s differs from the near placement' % what


def test_the_fill_is_what_a_wrapped_index_finds(far):
    """NaN in front of the input pointer and behind it, the sentinel in the output: at the block's ends and middle."""
    for index in (-fp.MID, -5, 0, 2**29, 2**30, fp.ROW_FRAMES - 8):
        assert np.isnan(far.read(far.x, index, 8, np.float32)).all()
        assert untouched(far.read(far.y, index, 8, np.float32))


# ---- trace analysis ----------------------------------------------------------------------------------------------

def test_region_stats(far):
    from audian_amd import hipdsp
    from test_gpu_regionstats import check_contract
    chunk = 16384
    L = fp.window_length(chunk)
    v = noise(L, 1) + np.float32(0.25)
    near = None
    for w in fp.by_index(chunk):                                # the region straddles the boundary
        with placed(far, [w], v):
            got = hipdsp.region_stats(far.ctx, far.X(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, [(w.start, w.stop)])
        check_contract(got[0, 0], v, 'by index, ' + w.name)
        near = got[0, 0] if near is None else near
        same_bits(got[0, 0], near, w.name)
    rows = fp.by_row(L, chunk)
    with placed(far, rows, v):
        got = hipdsp.region_stats(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, fp.row_frames(L, chunk), [(A, A + L)])
    for c in range(fp.ROWS):
        check_contract(got[0, c], v, 'by row, row %d' % c)
        same_bits(got[0, c], near, 'row %d' % c)


@functools.lru_cache(maxsize=None)
def event_case():
    """Samples with many short runs above 0.5 and one long run over the middle chunk, where the boundary lies; the
    definition's events at start 0."""
    chunk = 4096
    L = fp.window_length(chunk)
    v = noise(L, 2, 0.4)
    v[chunk + chunk//2 - 700:chunk + chunk//2 + 700] = 0.9
    want = ed.detect(v, 0, L, 0.5, 3, 2, sparse=True)
    assert len(want) > 100 and any(b - a >= 1400 for a, b in want)
    return chunk, L, v, np.array(want, dtype=np.int64)


def test_detect_events(far):
    from audian_amd import hipdsp
    chunk, L, v, want = event_case()
    K, cap = len(want), fp.EVENTS_CAP
    counts = hipdsp.DeviceArray(far.ctx, (fp.ROWS,), np.int64)
    for w in fp.by_index(chunk):
        with placed(far, [w], v):
            hipdsp.detect_events_into(far.ctx, far.X(), fp.ROW_FRAMES, 1, w.start, w.stop, 0.5, 3, 2, cap,
                                      far.out_rows(np.int64, 2*cap, 1, 2*cap), counts)
            got = far.rows(np.int64, 2*cap, 1, 2*cap)[0]
        assert counts.to_host()[0] == K, w.name
        assert got[:2*K].reshape(K, 2).tolist() == (want + w.start).tolist(), w.name
        assert untouched(got[2*K:]), w.name
        if w.boundary is not None:                              # a run crosses the boundary
            assert any(a < w.boundary < b for a, b in got[:2*K].reshape(K, 2).tolist()), w.name
        if w.name in ('elem_2_31', 'past'):
            assert got[2*K - 1] > 2**31
    pitch = fp.ROW_PITCH//2                                     # int64 elements: the byte offsets of the float rows
    rows = fp.by_row(L, chunk)
    with placed(far, rows, v):
        hipdsp.detect_events_into(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, A, A + L, 0.5, 3, 2, cap,
                                  far.out_rows(np.int64, pitch, fp.ROWS, 2*cap), counts, events_pitch=pitch)
        got = far.rows(np.int64, pitch, fp.ROWS, 2*cap)
    assert counts.to_host().tolist() == [K]*fp.ROWS
    for c in range(fp.ROWS):
        assert got[c, :2*K].reshape(K, 2).tolist() == (want + A).tolist(), c
        assert untouched(got[c, 2*K:]), c
    counts.free()


@functools.lru_cache(maxsize=None)
def peak_case():
    chunk = 4096
    L = fp.window_length(chunk)
    v = np.random.default_rng(3).integers(-8, 9, L).astype(np.float32)       # plateaus and ties
    borders = [-math.inf, math.inf, -math.inf, math.inf, 2.0, math.inf]
    wlen = 1001
    positions, properties = pd.find_peaks(v, prominence=(2.0, math.inf), wlen=wlen, first=0)
    assert len(positions) > 100
    return chunk, L, v, borders, wlen, np.array(positions, dtype=np.int64), np.array(properties, dtype=np.float64)


def shifted(positions, properties, by):
    return (positions + by).tolist(), (properties + np.array([0.0, 0.0, by, by])).tolist()


def test_find_peaks(far):
    """A closed prominence border and a finite wlen: the min/max table and the walk are used."""
    from audian_amd import hipdsp
    chunk, L, v, borders, wlen, positions, properties = peak_case()
    K, cap = len(positions), fp.PEAKS_CAP
    assert K <= cap
    props_at = fp.PROPS_AT                                          # float64 elements behind the output pointer
    counts = hipdsp.DeviceArray(far.ctx, (fp.ROWS,), np.int64)
    for w in fp.by_index(chunk):
        with placed(far, [w], v):
            hipdsp.find_peaks_into(far.ctx, far.X(), fp.ROW_FRAMES, 1, w.start, w.stop, borders, wlen, cap,
                                   far.out_rows(np.int64, cap, 1, cap), far.out_rows(np.float64, 4*cap, 1, 4*cap, props_at),
                                   counts)
            got = far.rows(np.int64, cap, 1, cap)[0]
            props = far.rows(np.float64, 4*cap, 1, 4*cap, base=props_at)[0]
        assert counts.to_host()[0] == K, w.name
        assert pd.same(got[:K], props[:4*K], shifted(positions, properties, w.start)), w.name
        assert untouched(got[K:]) and untouched(props[4*K:]), w.name
    pitch = fp.ROW_PITCH//2
    rows = fp.by_row(L, chunk)
    with placed(far, rows, v):
        hipdsp.find_peaks_into(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, A, A + L, borders, wlen, cap,
                               far.out_rows(np.int64, pitch, fp.ROWS, cap), far.out_rows(np.float64, pitch, fp.ROWS, 4*cap, props_at),
                               counts, peaks_pitch=pitch, props_pitch=pitch)
        got = far.rows(np.int64, pitch, fp.ROWS, cap)
        props = far.rows(np.float64, pitch, fp.ROWS, 4*cap, base=props_at)
    assert counts.to_host().tolist() == [K]*fp.ROWS
    for c in range(fp.ROWS):
        assert pd.same(got[c, :K], props[c, :4*K], shifted(positions, properties, A)), c
        assert untouched(got[c, K:]) and untouched(props[c, 4*K:]), c
    counts.free()


def test_histogram_and_masked_stats(far):
    """By index (tests/test_gpu_histogram.py has a row placement).  A guard sample read would be counted."""
    from audian_amd import hipdsp
    from test_gpu_histogram import check_hist, check_masked
    chunk = 16384       # HG_CHUNK, what csrc/histogram.hip cuts [start, stop) into (a 4096 grid holds the boundary too:
    #                     the window starts at 37 modulo 1024, so no boundary is a multiple of 4096 from it)
    L = fp.window_length(chunk)
    v = np.random.default_rng(4).uniform(0.0, 1.0, L).astype(np.float32)
    e = np.linspace(0.0, 1.0, 50)
    near = None
    for w in fp.by_index(chunk):
        with placed(far, [w], v, guard_value=0.5):
            hist = hipdsp.histogram(far.ctx, far.X(), fp.ROW_FRAMES, 1, w.start, w.stop, e)
            stats = hipdsp.masked_stats(far.ctx, far.X(), fp.ROW_FRAMES, 1, w.start, w.stop, [[0.25, 0.75, 0.25]])
        check_hist(hist, v[None, :], 0, L, e, w.name)
        check_masked(stats[0], v, 0.25, 0.75, 0.25, w.name)
        near = (hist, stats) if near is None else near
        same_bits(hist, near[0], w.name)
        same_bits(stats, near[1], w.name)


@pytest.mark.parametrize('step', [1, 3])
def test_region_spectra(far, step):
    from audian_amd import hipdsp
    from test_gpu_regionspectra import bound_and_reference
    chunk, nfft, hop, fs = 8192, 256, 128, 48000.0/step
    L = fp.window_length(chunk)
    v = noise(L, 5, 0.1) + (0.5*np.sin(2*np.pi*0.07*np.arange(L))).astype(np.float32)
    B, ref, n, argmax = bound_and_reference(v, (0, 0, L), nfft, hop, step, fs)
    assert n > 3*16

    def judge(row, info, what):
        assert info[0] == n and np.isfinite(row).all(), what
        err = np.abs(row.astype(np.float64) - ref)
        k = int(np.argmax(err - B))
        assert err[k] <= B[k], '%s: bin %d is %r, reference %r, allowed +-%.3g' % (what, k, row[k], ref[k], B[k])
        assert info[1] == np.argmax(row) == argmax, what

    near = None
    for w in fp.by_index(chunk):
        with placed(far, [w], v):
            rows, info = hipdsp.region_spectra(far.ctx, far.X(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, [(0, w.start, w.stop)],
                                               nfft, hop, step, fs)
        judge(rows[0], info[0], w.name)
        near = (rows[0], info[0]) if near is None else near
        same_bits(rows[0], near[0], w.name)
    windows = fp.by_row(L, chunk)
    with placed(far, windows, v):
        rows, info = hipdsp.region_spectra(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, fp.row_frames(L, chunk),
                                           [(c, A, A + L) for c in range(fp.ROWS)], nfft, hop, step, fs)
    for c in range(fp.ROWS):
        judge(rows[c], info[c], 'row %d' % c)
        same_bits(rows[c], near[0], 'row %d' % c)


@functools.lru_cache(maxsize=None)
def filter_case():
    label = 'lp1 40 Hz @ 96 kHz'
    chunk = 4096                                                # hipdsp.FILTER_TILE
    L = fp.window_length(chunk)
    sos = rd.case_design(label)[0]
    x = rd.case_signal(label, L)[:, :1]
    ref, q = rd.filtfilt_case(sos, x)
    return chunk, L, sos, x[:, 0], ref, q[0]


def test_region_filtfilt(far):
    """Out of place into the output block and in place; the region's own element range is all that is written."""
    from audian_amd import hipdsp
    chunk, L, sos, v, ref, q = filter_case()
    near = None
    for w in fp.by_index(chunk):
        region = [(0, w.start, w.stop)]
        with placed(far, [w], v):
            far.out_rows(np.float32, 0, 1, L, w.start)           # y is the output pointer itself: the row is y[start:stop]
            hipdsp.region_filtfilt(far.ctx, far.X(), fp.ROW_FRAMES, far.Y0(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, region, sos[None])
            got = far.rows(np.float32, 0, 1, L, base=w.start)[0]
            hipdsp.region_filtfilt(far.ctx, far.X(), fp.ROW_FRAMES, far.X(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, region, sos[None])
            here = far.read(far.x, w.start - w.guard, L + 2*w.guard, np.float32)
        ib.assert_within(got[:, None], ref, q, 'by index, ' + w.name, first=0)
        near = got if near is None else near
        same_bits(got, near, w.name)
        same_bits(here[w.guard:w.guard + L], near, w.name + ', in place')
        assert (here[:w.guard] == BIG).all() and (here[w.guard + L:] == BIG).all(), w.name
    windows = fp.by_row(L, chunk)
    regions = [(c, A, A + L) for c in range(fp.ROWS)]
    tables = np.array([sos]*fp.ROWS)
    frames = fp.row_frames(L, chunk)
    with placed(far, windows, v):
        far.out_rows(np.float32, fp.ROW_PITCH, fp.ROWS, L, A)
        hipdsp.region_filtfilt(far.ctx, far.X(), fp.ROW_PITCH, far.Y0(), fp.ROW_PITCH, fp.ROWS, frames, regions, tables)
        got = far.rows(np.float32, fp.ROW_PITCH, fp.ROWS, L, base=A)
        hipdsp.region_filtfilt(far.ctx, far.X(), fp.ROW_PITCH, far.X(), fp.ROW_PITCH, fp.ROWS, frames, regions, tables)
        here = [far.read(far.x, w.start - w.guard, L + 2*w.guard, np.float32) for w in windows]
    for c, w in enumerate(windows):
        ib.assert_within(got[c][:, None], ref, q, 'by row, row %d' % c, first=0)
        same_bits(got[c], near, 'row %d' % c)
        same_bits(here[c][w.guard:w.guard + L], near, 'row %d, in place' % c)
        assert (here[c][:w.guard] == BIG).all() and (here[c][w.guard + L:] == BIG).all(), c


def test_region_crossings(far):
    from audian_amd import hipdsp
    chunk = 4096
    L = fp.window_length(chunk)
    v = noise(L, 7, 0.4)
    want = rd.region_crossings(v, 0, L, 0.5)
    assert want[1] > 100 and want[2] >= 0

    def moved(by):
        return want + np.array([0, 0, by, by, 0, by, 0, 0], dtype=np.float64)

    for w in fp.by_index(chunk):
        with placed(far, [w], v):
            got = hipdsp.region_crossings(far.ctx, far.X(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, [(0, w.start, w.stop)], [0.5])
        assert got[0].tolist() == moved(w.start).tolist(), w.name
    windows = fp.by_row(L, chunk)
    with placed(far, windows, v):
        got = hipdsp.region_crossings(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, fp.row_frames(L, chunk),
                                      [(c, A, A + L) for c in range(fp.ROWS)], [0.5]*fp.ROWS)
    for c in range(fp.ROWS):
        assert got[c].tolist() == moved(A).tolist(), c


@pytest.mark.parametrize('step', fp.MINMAX_STEPS)
def test_minmax_decimate(far, step):
    """Step 7: the kernel that stages tiles of whole segments; step 600: one wave per segment."""
    from audian_amd import hipdsp
    from oracle import oracle as orc
    chunk = 4096
    L = fp.window_length(chunk)
    v = noise(L, 8)
    want = orc.minmax_decimate(v, 0, L, step)
    n = len(want)
    assert n == 2*(-(-L//step))
    for w in fp.by_index(chunk):
        with placed(far, [w], v):
            hipdsp.minmax_decimate(far.ctx, far.X(), fp.ROW_FRAMES, 1, w.start, w.stop, step, far.out_rows(np.float32, n, 1, n), n)
            got = far.rows(np.float32, n, 1, n)[0]
        assert np.array_equal(got.astype(np.float64), want), w.name
    windows = fp.by_row(L, chunk)
    with placed(far, windows, v):
        hipdsp.minmax_decimate(far.ctx, far.X(), fp.ROW_PITCH, fp.ROWS, A, A + L, step, far.out_rows(np.float32, fp.ROW_PITCH, fp.ROWS, n),
                               fp.ROW_PITCH)
        got = far.rows(np.float32, fp.ROW_PITCH, fp.ROWS, n)
    for c in range(fp.ROWS):
        assert np.array_equal(got[c].astype(np.float64), want), c


@pytest.mark.parametrize('carrier', [None, (40000.0, 192000.0)])
def test_channel_mean(far, carrier):
    """By index one channel; by row channels [0, 2, 4] of five rows that all differ."""
    from audian_amd import hipdsp
    from test_gpu_playback_kernels import carrier_ratio, ulp32
    chunk = 4096
    L = fp.window_length(chunk)
    cps = carrier[0]/carrier[1] if carrier else 0.0

    def judge(got, mean, what):
        if carrier:
            ratio = carrier_ratio(got, mean, np.arange(L), *carrier)
        else:
            ratio = np.abs(got.astype(np.longdouble) - mean).astype(np.float64)/((0.5 + 2.0**-20)*ulp32(mean))
        assert ratio.max() <= 1.0, (what, int(np.argmax(ratio)), float(ratio.max()))

    data = [np.random.default_rng(20 + c).uniform(-1.0, 1.0, L).astype(np.float32) for c in range(fp.ROWS)]
    near = None
    for w in fp.by_index(chunk):
        with placed(far, [w], data[0]):
            hipdsp.channel_mean(far.ctx, far.X(), fp.ROW_FRAMES, [0], w.start, L, far.out_rows(np.float32, L, 1, L),
                                heterodyne_cycles_per_sample=cps)
            got = far.rows(np.float32, L, 1, L)[0]
        judge(got, data[0].astype(np.longdouble), w.name)
        near = got if near is None else near
        same_bits(got, near, w.name)
    windows = fp.by_row(L, chunk)
    group = [0, 2, 4]
    with placed(far, windows, data):
        hipdsp.channel_mean(far.ctx, far.X(), fp.ROW_PITCH, group, A, L, far.out_rows(np.float32, L, 1, L),
                            heterodyne_cycles_per_sample=cps)
        got = far.rows(np.float32, L, 1, L)[0]
    judge(got, np.sum([data[c].astype(np.longdouble) for c in group], axis=0)/np.longdouble(3), 'rows 0, 2, 4')


def test_unwrap(far):
    """By row (the call has no start: by index it would touch the whole row); y_pitch in the output block."""
    from audian_amd import hipdsp
    from oracle import oracle as orc
    chunk = 16384
    L = fp.window_length(chunk)
    t = np.arange(L)
    s = 1.6*np.sin(2*np.pi*t/997.0) + 0.01*np.random.default_rng(9).standard_normal(L)
    v = (((s + 1.0) % 2.0) - 1.0).astype(np.float32)            # a signal that left [-1, 1) and wrapped around
    want = orc.unwrap(v, 1.5)
    assert np.abs(want).max() > 0.6                              # halved: the unwrapped signal reaches beyond +-1
    windows = fp.by_row(L, chunk)
    with placed(far, windows, v):
        hipdsp.unwrap(far.ctx, far.X(A), fp.ROW_PITCH, fp.ROWS, L, 1.5, far.out_rows(np.float32, fp.ROW_PITCH, fp.ROWS, L, A),
                      fp.ROW_PITCH)
        got = far.rows(np.float32, fp.ROW_PITCH, fp.ROWS, L, base=A)
    for c in range(fp.ROWS):
        assert got[c].tobytes() == want.tobytes(), c


@pytest.mark.parametrize('step', fp.FIR_STEPS)
def test_fir_bank(far, step):
    """L = 257, K = 3, integer samples and taps: exact.  Steps 1, 7 and 300 take the kernel's three layouts."""
    from audian_amd import hipdsp
    taps_n, K = fp.FIR_TAPS, fp.FIR_KERNELS
    chunk = fp.fir_chunk(step)
    L = fp.window_length(chunk)
    rng = np.random.default_rng(10 + step)
    v = rng.integers(-8, 9, L)
    taps = rng.integers(-4, 5, (K, taps_n))
    n_out = fp.fir_n_out(step)
    lead = (taps_n - 1)//2                                      # output t reads x[t - 128 .. t + 128]
    want = fir_definition(v[None, :], taps, first=lead, step=step, n=n_out)[:, 0, :].astype(np.float32)
    plan = hipdsp.FirPlan(far.ctx, taps)
    for w in fp.by_index(chunk):
        with placed(far, [w], v.astype(np.float32)):
            hipdsp.fir_bank(far.ctx, plan, far.X(), fp.ROW_FRAMES, 1, fp.ROW_FRAMES, w.start + lead, step, n_out,
                            far.out_rows(np.float32, fp.ROW_PITCH, K, n_out), out_pitch=n_out, out_kernel_pitch=fp.ROW_PITCH)
            got = far.rows(np.float32, fp.ROW_PITCH, K, n_out)
        assert np.array_equal(got, want), w.name
    pitch = fp.rows_pitch(K*fp.ROWS, n_out, OUT_GUARD)
    windows = fp.by_row(L, chunk)
    with placed(far, windows, v.astype(np.float32)):
        hipdsp.fir_bank(far.ctx, plan, far.X(), fp.ROW_PITCH, fp.ROWS, fp.row_frames(L, chunk), A + lead, step, n_out,
                        far.out_rows(np.float32, pitch, K*fp.ROWS, n_out), out_pitch=pitch, out_kernel_pitch=fp.ROWS*pitch)
        got = far.rows(np.float32, pitch, K*fp.ROWS, n_out)
    for k in range(K):
        for c in range(fp.ROWS):
            assert np.array_equal(got[k*fp.ROWS + c], want[k]), (k, c)
    plan.close()


# ---- spectrogram-slab consumers: index = frame * F + bin ---------------------------------------------------------

def slab_case():
    F, R = fp.SLAB_F, fp.SLAB_ROWS
    rng = np.random.default_rng(11)
    return (10.0**rng.uniform(-9.0, 1.0, (R, F))).astype(np.float32)


@pytest.mark.parametrize('step', fp.DECIMATE_STEPS)
def test_decibel_image_decimate(far, step):
    """Frames around every boundary; the guard frames hold a larger maximum."""
    from audian_amd import hipdsp
    F, R = fp.SLAB_F, fp.SLAB_ROWS
    spec = slab_case()
    top = np.maximum.reduceat(spec, np.arange(0, R, step), axis=0)
    ncols = len(top)
    near = None
    for w in fp.slab_windows():
        i0 = w.start//F
        with placed(far, [w], spec.reshape(-1), guard_value=1e30):
            hipdsp.decibel_image_decimate(far.ctx, far.X(), far.out_rows(np.float32, F*ncols, 1, F*ncols), i0 + R + 1, F, i0,
                                          i0 + R, step)
            got = far.rows(np.float32, F*ncols, 1, F*ncols)[0]
        dbb.assert_within(got.reshape(F, ncols), top.T, 1.0, 1e-20, 'hipdsp_decibel_image_decimate, ' + w.name)
        near = got if near is None else near
        same_bits(got, near, w.name)


def test_mean_spectrum_db(far):
    from audian_amd import hipdsp
    F, R = fp.SLAB_F, fp.SLAB_ROWS
    spec = slab_case()
    mean = np.sum(spec.astype(np.longdouble), axis=0)/np.longdouble(R)
    near = None
    for w in fp.slab_windows():
        i0 = w.start//F
        with placed(far, [w], spec.reshape(-1), guard_value=1e30):
            hipdsp.mean_spectrum_db(far.ctx, far.X(), F, i0, i0 + R, far.out_rows(np.float32, F, 1, F))
            got = far.rows(np.float32, F, 1, F)[0]
        dbb.assert_within(got, mean.astype(np.float32), 1.0, 1e-20, 'hipdsp_mean_spectrum_db, ' + w.name, extra=1, arg=mean,
                          floor_db=-200.0)
        near = got if near is None else near
        same_bits(got, near, w.name)


def test_band_order_stats(far):
    """row_stride 2^20 and 2052 rows: the last four rows start past element 2^31.  The values and the rank are
    far_placement.band_values': the rows past 2^31 hold the lowest values, rows [0, 1024) the middle and rows [1024, 2048)
    the highest range, and the rank is the last value of the two lower ranges -- tests/test_far_placement.py replays each
    wrap of the row bases on these values and finds both order statistics changed (rows 1024 apart are each other's
    image under the byte wraps; the signed element index sends the four rows past 2^31 to the NaN fill)."""
    from audian_amd import hipdsp
    idx, written, groups, row_groups = fp.band_plan()
    R, C = fp.BAND_ROWS, fp.BAND_COLS
    host, rank, want = fp.band_values()
    try:
        for r, (a, b) in enumerate(written):
            far.write(a, host[r])
        hipdsp.band_order_stats(far.ctx, far.X(), R, C, fp.BAND_STRIDE, rank, far.out_rows(np.float32, 2, 1, 2))
        got = far.rows(np.float32, 2, 1, 2)[0]
    finally:
        far.ctx.synchronize()
        for a, b in written:
            far.refill(a, b - a)
    assert got.tolist() == list(want)
    compact = hipdsp.DeviceArray.from_host(far.ctx, host)
    hipdsp.band_order_stats(far.ctx, compact.view(1, (1,)), R, C, C + 2, rank, far.out_rows(np.float32, 2, 1, 2))
    same_bits(far.rows(np.float32, 2, 1, 2)[0], got, 'rows 2^20 apart')
    compact.free()


def test_unpack_spectrum_f64(far):
    """Five channels ROW_PITCH apart in the input block, three frames of 1025 bins; the float64 output is compact."""
    from audian_amd import hipdsp
    F, T = fp.SLAB_F, 3
    windows = fp.by_row(T*F, OUT_GUARD)
    data = [noise(T*F, 30 + c) for c in range(fp.ROWS)]
    with placed(far, windows, data):
        hipdsp.unpack_spectrum(far.ctx, far.X(A), far.out_rows(np.float64, T*fp.ROWS*F, 1, T*fp.ROWS*F), T, fp.ROWS, F,
                               src_pitch=fp.ROW_PITCH)
        got = far.rows(np.float64, T*fp.ROWS*F, 1, T*fp.ROWS*F)[0].reshape(T, fp.ROWS, F)
    for c in range(fp.ROWS):
        assert np.array_equal(got[:, c, :], data[c].reshape(T, F).astype(np.float64)), c


# ---- layout kernels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pack(far, dtype):
    """hipdsp_pack_f32 / hipdsp_pack_f64: dst_pitch puts the five rows across the boundaries of the output block."""
    from audian_amd import hipdsp
    T = fp.PACK_FRAMES
    src = np.random.default_rng(13).uniform(-1.0, 1.0, (T, fp.ROWS)).astype(dtype)
    dsrc = hipdsp.DeviceArray.from_host(far.ctx, src)
    hipdsp.pack(far.ctx, dsrc, far.out_rows(np.float32, fp.ROW_PITCH, fp.ROWS, T), fp.ROW_PITCH, T, fp.ROWS, src_dtype=dtype)
    got = far.rows(np.float32, fp.ROW_PITCH, fp.ROWS, T)
    assert np.array_equal(got, src.T.astype(np.float32))
    dsrc.free()


@pytest.mark.parametrize('sample_bytes,channels,frames', [(3, fp.ROWS, fp.PACK_FRAMES), (2, fp.ROWS, fp.PACK_FRAMES),
                                                          (2, fp.PCM_TILE_CHANNELS, fp.PCM_TILE_FRAMES),
                                                          (4, fp.PCM_TILE_CHANNELS, fp.PCM_TILE_FRAMES)])
def test_pcm_unpack(far, sample_bytes, channels, frames):
    """Five channels: the generic kernel; eight channels of 2 or 4 bytes: the 16-byte tile kernel."""
    from audian_amd import hipdsp
    bits = 8*sample_bytes
    rng = np.random.default_rng(14)
    ints = rng.integers(-2**(bits - 1), 2**(bits - 1), (frames, channels))
    ints[0, 0], ints[-1, -1] = -2**(bits - 1), 2**(bits - 1) - 1
    raw = ints.astype('<i4').view(np.uint8).reshape(frames, channels, 4)[:, :, :sample_bytes]       # little endian
    pcm = hipdsp.DeviceArray.from_host(far.ctx, np.ascontiguousarray(raw).reshape(-1))
    scale = 2.0**-(bits - 1)
    pitch = fp.ROW_PITCH if channels == fp.ROWS else fp.rows_pitch(channels, frames, OUT_GUARD)
    hipdsp.pcm_unpack(far.ctx, pcm, sample_bytes, frames, channels, scale, far.out_rows(np.float32, pitch, channels, frames), pitch)
    got = far.rows(np.float32, pitch, channels, frames)
    assert np.array_equal(got, (ints.T.astype(np.float64)*scale).astype(np.float32))
    pcm.free()


def test_unpack_f64(far):
    """src_pitch in the input block: five rows ROW_PITCH apart to (T, C) float64."""
    from audian_amd import hipdsp
    T = fp.PACK_FRAMES
    windows = fp.by_row(T, OUT_GUARD)
    data = [noise(T, 40 + c) for c in range(fp.ROWS)]
    with placed(far, windows, data):
        hipdsp.unpack(far.ctx, far.X(A), fp.ROW_PITCH, far.out_rows(np.float64, T*fp.ROWS, 1, T*fp.ROWS), T, fp.ROWS)
        got = far.rows(np.float64, T*fp.ROWS, 1, T*fp.ROWS)[0].reshape(T, fp.ROWS)
    assert np.array_equal(got, np.stack(data, axis=1).astype(np.float64))


def test_stride_copy(far):
    """n > 2^31 and a step that leaves 301 outputs; the elements beside every sample hold another value."""
    from audian_amd import hipdsp
    idx, written = fp.stride_plan()
    m = len(idx)
    values = noise(m, 15)
    try:
        for i, (a, b) in enumerate(written):
            far.write(a, np.array([BIG, values[i], BIG], dtype=np.float32))
        hipdsp.stride_copy(far.ctx, far.X(), fp.STRIDE_N, fp.STRIDE_STEP, far.out_rows(np.float32, m, 1, m))
        got = far.rows(np.float32, m, 1, m)[0]
    finally:
        far.ctx.synchronize()
        for a, b in written:
            far.refill(a, b - a)
    assert got.tobytes() == values.tobytes()


def test_zz_the_blocks_are_as_they_were(far):
    """Every test put back what it wrote: the places the plans use hold the fill again."""
    for chunk in (4096, 16384):
        for w in fp.by_index(chunk) + fp.by_row(fp.window_length(chunk), chunk):
            assert np.isnan(far.read(far.x, w.start - w.guard, w.stop - w.start + 2*w.guard, np.float32)).all(), w.name
    for c in range(fp.ROWS):
        assert untouched(far.read(far.y, c*fp.ROW_PITCH - OUT_GUARD, 8192, np.float32)), c
