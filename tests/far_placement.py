"""Where tests/test_gpu_far_indices.py puts its windows: pure Python, checked on the CPU by tests/test_far_placement.py.

Two device blocks of BLOCK float32 elements each, one for inputs and one for outputs.  The pointer every call is handed
is the block's base + MID elements, so an index is a signed offset from the middle of memory the test owns: an index
that an unwidened product has wrapped lands inside the block, where the input holds NaN (0xff bytes) and the output a
sentinel, and the test fails on a value instead of faulting the device.  The wraps this holds for (WRAPS):
    elem_s32   the element index kept in a signed 32-bit integer
    byte_u32   the byte offset kept in an unsigned 32-bit integer
    byte_s32   the byte offset kept in a signed 32-bit integer
Only the windows and a guard band on each side of them are written.  The by-index windows are written ONE AT A TIME:
the windows that straddle 2^30 and 2^31 are each other's image under byte_u32 (both hold an element that is 0 modulo
2^30), so with both in memory a wrapped read would find the same samples instead of NaN.  The rows of a by-row plan are
written together: no row's image falls on another row's window.

By index: one row of ROW_FRAMES elements, the window near the start, straddling element 2^29 (byte 2^31), 2^30 (byte
2^32) and 2^31, and wholly past 2^31.  By row: ROWS rows ROW_PITCH apart with the same in-row window in each; the row
bases c * ROW_PITCH cross the same boundaries.  All window starts are PHASE modulo 1024 elements, so every placement has
the 4 KB phase of the near one, and a straddled boundary lies strictly inside the middle one of the window's three
chunks."""

from collections import namedtuple

import numpy as np

BLOCK = 2**32 + 2**22                          # float32 elements of a block
MID = 2**31                                    # elements between a block's base and the pointer handed to the calls
ROW_FRAMES = 2**31 + 2**22                     # by index: frames of the one row (all of it is owned: MID + ROW_FRAMES == BLOCK)
ROW_PITCH = 2**29 + 2**19                      # by row: elements between rows
ROWS = 5                                       # row bases 0, 2^29 + 2^19, 2^30 + 2^20, 3 (2^29 + 2^19), 2^31 + 2^21
PHASE = 37                                     # window starts modulo 1024: an odd 4-byte phase inside the 4 KB page
ODD = 77                                       # a window is three chunks and this remainder
NEAR = 2**20                                   # the near window starts here (+ PHASE): clear of every wrapped image
PAST = 2**31 + 2**21                           # the window wholly past 2^31
IN_ROW = 2**17                                 # by row: the window's start inside its row
BOUNDARIES = (('byte_2_31', 2**29), ('byte_2_32', 2**30), ('elem_2_31', 2**31))
MIN_CHUNK = 2048                               # smaller chunks cannot keep a boundary in the middle chunk at a 4 KB phase

Window = namedtuple('Window', 'name start stop guard boundary row')
# start, stop: elements from the pointer; guard: elements written on each side; boundary: the straddled element or None;
# row: the row of a by-row plan (start and stop are then c * pitch + in-row positions), None by index


def window_length(chunk):
    return 3*chunk + ODD


def at_phase(v):
    """The element nearest to v that is PHASE modulo 1024."""
    d = (v - PHASE) % 1024
    return v - d if d < 512 else v + 1024 - d


def by_index(chunk, length=None, guard=None):
    """The five windows of the one-row plan for a kernel that works in chunks of `chunk` elements from the window's
    start."""
    assert chunk >= MIN_CHUNK and chunk % 1024 == 0
    length = window_length(chunk) if length is None else length
    guard = chunk if guard is None else guard
    assert length >= 3*chunk and length + 2*guard < 2**19
    out = [Window('near', NEAR + PHASE, NEAR + PHASE + length, guard, None, None)]
    for name, b in BOUNDARIES:
        start = at_phase(b - chunk - chunk//2)
        out.append(Window(name, start, start + length, guard, b, None))
    out.append(Window('past', PAST + PHASE, PAST + PHASE + length, guard, None, None))
    for w in out:
        assert w.start % 1024 == PHASE and w.start - w.guard >= 0 and w.stop + w.guard <= ROW_FRAMES
        if w.boundary is not None:                              # strictly inside the middle chunk
            assert w.start + chunk <= w.boundary - 1 and w.boundary <= w.start + 2*chunk - 1
    return out


def by_row(length, guard, pitch=ROW_PITCH, rows=ROWS, in_row=IN_ROW):
    """The windows of a by-row plan: row c holds [in_row + PHASE, + length) of its own frames."""
    a = in_row + PHASE
    assert a - guard >= 0 and a + length + guard <= pitch
    return [Window('row%d' % c, c*pitch + a, c*pitch + a + length, guard, None, c) for c in range(rows)]


def row_frames(length, guard, in_row=IN_ROW):
    """frames of a by-row call: the row ends where the window's rear guard ends."""
    return in_row + PHASE + length + guard


def rows_pitch(rows, n, guard):
    """A pitch for `rows` output rows of n elements whose last row starts just past 2^31 elements (by 2^21 or less):
    for the outputs that have more than ROWS rows."""
    pitch = -(-(2**31 + 2**20)//(rows - 1))
    assert (rows - 1)*pitch + n + guard <= ROW_FRAMES and pitch >= n + 2*guard
    return pitch


# ---- the wraps ---------------------------------------------------------------------------------------------------

def _s32(v):
    return (v + 2**31) % 2**32 - 2**31


def elem_s32(i, itemsize=4):
    return _s32(i)


def byte_u32(i, itemsize=4):
    return (i*itemsize) % 2**32//itemsize


def byte_s32(i, itemsize=4):
    return _s32(i*itemsize)//itemsize


WRAPS = (('elem_s32', elem_s32, 2**31), ('byte_u32', byte_u32, 2**32), ('byte_s32', byte_s32, 2**31))
# name, function, and the first index * itemsize (for elem_s32: the first index) the wrap moves


def first_moved(wrap, itemsize):
    name, fn, limit = wrap
    return limit if name == 'elem_s32' else limit//itemsize


def owned(itemsize=4):
    """[lo, hi): the indices of elements of `itemsize` bytes, counted from the pointer, that lie inside the block."""
    return -MID*4//itemsize, (BLOCK - MID)*4//itemsize


def intervals(windows):
    """[(lo, hi)] of everything a plan writes: the windows with their guard bands."""
    return [(w.start - w.guard, w.stop + w.guard) for w in windows]


def check_disjoint(windows):
    spans = sorted(intervals(windows))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, 'windows or guard bands overlap: %r' % (spans,)


def check_wraps(indices, written, itemsize=4, groups=None, written_groups=None):
    """For every touched index and each of the three wraps: the wrapped address lies inside the owned block; where the
    wrap applies (the index, or its byte offset, is at or past the wrap's limit) it is a different address, and it is no
    address the plan has written -- so what a wrapped read finds is the block's fill.  With `groups` (one id per index) and
    `written_groups` (one per interval) a wrapped address may be a written one of ANOTHER group: the plan then has to
    make a sample of the wrong group change the result.  Returns {wrap name: number of touched indices it moves}."""
    idx = np.asarray(indices, dtype=np.int64)
    lo, hi = owned(itemsize)
    assert idx.min() >= lo and idx.max() < hi, 'a touched index lies outside the block'
    moved_counts = {}
    for wrap in WRAPS:
        name, fn, limit = wrap
        img = fn(idx, itemsize)
        assert img.min() >= lo and img.max() < hi, '%s leaves the block' % name
        must = idx >= first_moved(wrap, itemsize)
        moved = img != idx
        assert (moved[must]).all(), '%s leaves an index past its limit in place' % name
        assert not moved[~must & (idx >= 0)].any(), name
        hit = np.zeros(len(idx), dtype=bool)
        for k, (a, b) in enumerate(written):
            inside = (img >= a) & (img < b)
            hit |= inside if groups is None else inside & (np.asarray(groups) == written_groups[k])
        assert not (hit & moved).any(), '%s lands on written memory' % name
        moved_counts[name] = int(moved.sum())
    return moved_counts


def touched(windows):
    """Every index of the windows and their guard bands."""
    return np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in intervals(windows)])


# ---- the plans that are not windows of a row ---------------------------------------------------------------------

SLAB_F = 1025                                  # bins per frame of the spectrogram-slab consumers: index = frame * F + bin
SLAB_ROWS = 3*28 + 5                           # frames per window: three columns of the longest step and a remainder


def slab_windows(rows=SLAB_ROWS, F=SLAB_F, guard_rows=1):
    """Windows of whole frames [i0, i1) of a (frames, F) slab around each boundary; start and stop are elements, the
    guard is whole frames.  The boundary lies inside the middle third of the window."""
    out = [Window('near', 1024*F, (1024 + rows)*F, guard_rows*F, None, None)]
    for name, b in BOUNDARIES:
        i0 = b//F - rows//2
        out.append(Window(name, i0*F, (i0 + rows)*F, guard_rows*F, b, None))
        assert (i0 + rows//3)*F < b < (i0 + rows - rows//3)*F
    i0 = PAST//F + 1
    out.append(Window('past', i0*F, (i0 + rows)*F, guard_rows*F, None, None))
    assert out[-1].stop + guard_rows*F <= ROW_FRAMES
    return out


BAND_STRIDE = 2**20                            # hipdsp_band_order_stats: elements between rows
BAND_ROWS = 2**11 + 4                          # rows 0 ... 2051: the last four start past element 2^31
BAND_COLS = 3


BAND_RANGE = (1.0, 2.0, 0.0)                   # where the values of row groups 0, 1, 2 begin: each spans less than 1
BAND_RANK = (4 + 1024)*BAND_COLS - 1           # the last value of the two lower ranges: rows [2048, 2052) and [0, 1024)
BAND_GUARD = 0.25                              # beside every row: a value of the lowest range


def band_plan():
    """(indices of the band's elements, written intervals, group of every index, group of every interval): every row
    with one guard element on each side.  With the stride the issue sets, rows 1024 apart are each other's image under
    the byte wraps and all of them are read by the one call, so the rows come in groups -- [0, 1024), [1024, 2048),
    [2048, 2052) -- whose values lie in disjoint ranges (band_values)."""
    rows = np.arange(BAND_ROWS, dtype=np.int64)*BAND_STRIDE
    idx = (rows[:, None] + np.arange(BAND_COLS)[None, :]).reshape(-1)
    written = [(int(r) - 1, int(r) + BAND_COLS + 1) for r in rows]
    assert written[-1][1] <= ROW_FRAMES
    row_groups = np.arange(BAND_ROWS)//1024
    return idx, written, np.repeat(row_groups, BAND_COLS), row_groups


def band_values():
    """(host (rows, cols + 2) float32 with the guard elements, rank, (value of rank, value of rank + 1)).  All values are
    distinct.  The four rows past element 2^31 hold the LOWEST range [0, 1), rows [0, 1024) hold [1, 2) and rows
    [1024, 2048) hold [2, 3); the rank asked for is the last value below 2.  So the answer counts the values below 2
    exactly: a row past 2^31 read from the NaN fill (NaN sorts above everything) takes values from under the rank, a row
    of [2, 3) read as its image 1024 rows earlier adds values under it, and a guard element read adds one too --
    band_replay shows that each of the three wraps moves both order statistics."""
    R, C = BAND_ROWS, BAND_COLS
    rng = np.random.default_rng(12)
    unit = (rng.permutation(R*C).reshape(R, C)/np.float64(R*C)).astype(np.float32)              # distinct, in [0, 1)
    lift = np.array(BAND_RANGE, dtype=np.float32)[np.arange(R)//1024]
    values = (unit*np.float32(0.999) + lift[:, None]).astype(np.float32)
    assert len(np.unique(values)) == R*C
    # the largest value below 2 into row 700: byte_s32 sends rows [512, 1024) to the fill and reads rows [1024, 1536) as
    # rows [0, 512), which keeps the count below 2 -- the value of the rank itself has to be one that goes missing
    r, j = np.unravel_index(np.argmax(values[:1024]), (1024, C))
    values[r, j], values[700, 0] = values[700, 0], values[r, j]
    host = np.full((R, C + 2), BAND_GUARD, dtype=np.float32)
    host[:, 1:C + 1] = values
    order = np.sort(values.reshape(-1))
    assert order[BAND_RANK] < 2.0 <= order[BAND_RANK + 1] and order[4*C - 1] < 1.0 <= order[4*C]
    return host, BAND_RANK, (order[BAND_RANK], order[BAND_RANK + 1])


def band_replay(host, rank, wrap=None, itemsize=4):
    """The two order statistics a kernel would give that applied `wrap` (a function of WRAPS, None: none) to the element
    index r * row_stride + j: memory the plan has not written reads NaN, and NaN sorts above everything."""
    R, C = BAND_ROWS, BAND_COLS
    memory = {}
    for r in range(R):
        for j in range(-1, C + 1):
            memory[r*BAND_STRIDE + j] = host[r, j + 1]
    idx = (np.arange(R, dtype=np.int64)[:, None]*BAND_STRIDE + np.arange(C)[None, :]).reshape(-1)
    if wrap is not None:
        idx = wrap(idx, itemsize)
    read = np.array([memory.get(int(i), np.nan) for i in idx], dtype=np.float32)
    order = np.sort(read)                                       # numpy sorts NaN last, as the kernel's keys do
    return order[rank], order[rank + 1]


# ---- the output rows of every call of the GPU module -------------------------------------------------------------

OUT_GUARD = 64                                 # elements checked on each side of every written output row
EVENTS_CAP = 2048                              # capacity (events per channel) of the detect_events calls
PEAKS_CAP = 8192                               # capacity of the find_peaks calls
PROPS_AT = 2**16                               # float64 elements between the output pointer and the props rows
FIR_TAPS, FIR_KERNELS, FIR_STEPS = 257, 3, (1, 7, 300)
MINMAX_STEPS = (7, 600)
DECIMATE_STEPS = (3, 28)
PACK_FRAMES = 3*32 + 5                         # pack / unpack / generic PCM: three 32-frame tiles and a remainder
PCM_TILE_FRAMES, PCM_TILE_CHANNELS = 3*128 + 5, 8


def fir_chunk(step):
    return max(4096, 256*step)


def fir_n_out(step):
    return (window_length(fir_chunk(step)) - FIR_TAPS)//step + 1


def output_plans():
    """{call: (itemsize, [(pitch, rows, n, base)])}: the output rows of every call the GPU module makes into the output
    block, in elements of `itemsize` bytes from the output pointer (one call may write several sets of rows)."""
    p8 = ROW_PITCH//2                                           # 8-byte elements: the byte offsets of the float rows
    a = IN_ROW + PHASE
    L4, L16 = window_length(4096), window_length(16384)
    F = SLAB_F
    plans = {
        'events, by index': (8, [(2*EVENTS_CAP, 1, 2*EVENTS_CAP, 0)]),
        'events, by row': (8, [(p8, ROWS, 2*EVENTS_CAP, 0)]),
        'peaks, by index': (8, [(PEAKS_CAP, 1, PEAKS_CAP, 0), (4*PEAKS_CAP, 1, 4*PEAKS_CAP, PROPS_AT)]),
        'peaks, by row': (8, [(p8, ROWS, PEAKS_CAP, 0), (p8, ROWS, 4*PEAKS_CAP, PROPS_AT)]),
        'filtfilt, by row': (4, [(ROW_PITCH, ROWS, L4, a)]),
        'channel mean': (4, [(L4, 1, L4, 0)]),
        'unwrap': (4, [(ROW_PITCH, ROWS, L16, a)]),
        'mean spectrum': (4, [(F, 1, F, 0)]),
        'band order stats': (4, [(2, 1, 2, 0)]),
        'unpack spectrum': (8, [(3*ROWS*F, 1, 3*ROWS*F, 0)]),
        'pack, generic pcm': (4, [(ROW_PITCH, ROWS, PACK_FRAMES, 0)]),
        'tile pcm': (4, [(rows_pitch(PCM_TILE_CHANNELS, PCM_TILE_FRAMES, OUT_GUARD), PCM_TILE_CHANNELS, PCM_TILE_FRAMES, 0)]),
        'unpack': (8, [(PACK_FRAMES*ROWS, 1, PACK_FRAMES*ROWS, 0)]),
        'stride copy': (4, [(len(stride_plan()[0]), 1, len(stride_plan()[0]), 0)]),
    }
    for w in by_index(4096):
        plans['filtfilt, by index, ' + w.name] = (4, [(0, 1, L4, w.start)])
    for step in MINMAX_STEPS:
        n = 2*(-(-L4//step))
        plans['minmax %d, by index' % step] = (4, [(n, 1, n, 0)])
        plans['minmax %d, by row' % step] = (4, [(ROW_PITCH, ROWS, n, 0)])
    for step in FIR_STEPS:
        n = fir_n_out(step)
        plans['fir %d, by index' % step] = (4, [(ROW_PITCH, FIR_KERNELS, n, 0)])
        plans['fir %d, by row' % step] = (4, [(rows_pitch(FIR_KERNELS*ROWS, n, OUT_GUARD), FIR_KERNELS*ROWS, n, 0)])
    for step in DECIMATE_STEPS:
        n = F*(-(-SLAB_ROWS//step))
        plans['decimate %d' % step] = (4, [(n, 1, n, 0)])
    return plans


def output_windows(sets, guard=OUT_GUARD):
    """The rows of an output plan as windows with their guard elements."""
    return [Window('row%d' % c, base + c*pitch, base + c*pitch + n, guard, None, c)
            for pitch, rows, n, base in sets for c in range(rows)]


STRIDE_N = 2**31 + 2**21                       # hipdsp_stride_copy: n > 2^31
STRIDE_STEP = 7158279                          # leaves 301 outputs


def stride_plan():
    """(indices read, written intervals): out[i] = x[i * step], one guard element on each side of every sample."""
    m = -(-STRIDE_N//STRIDE_STEP)
    idx = np.arange(m, dtype=np.int64)*STRIDE_STEP
    assert 200 <= m <= 400 and idx[-1] > 2**31 and idx[-1] + 2 <= ROW_FRAMES
    return idx, [(int(i) - 1, int(i) + 2) for i in idx]
