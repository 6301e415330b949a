"""The arithmetic of tests/far_placement.py, on the CPU: for every plan tests/test_gpu_far_indices.py uses, the boundary
is inside the window's middle chunk, the phases agree, windows and guard bands do not overlap, and every index a call
touches, wrapped in each of the three ways an unwidened product wraps, is a different address inside the owned block
that the plan has not written."""

import numpy as np
import pytest

import far_placement as fp

CHUNKS = [2048, 4096, 8192, 16384, 76800]      # every chunk size the GPU module plans with (76800: FIR step 300)


def test_the_blocks():
    assert fp.MID + fp.ROW_FRAMES == fp.BLOCK
    assert fp.owned(4) == (-2**31, 2**31 + 2**22) and fp.owned(8) == (-2**30, 2**30 + 2**21)
    assert (fp.ROWS - 1)*fp.ROW_PITCH == 2**31 + 2**21
    bases = [c*fp.ROW_PITCH for c in range(fp.ROWS)]
    for name, b in fp.BOUNDARIES:                               # the row bases cross every boundary
        assert any(lo < b <= hi for lo, hi in zip(bases, bases[1:])), name
    # the three wraps on a few indices, spelled out
    assert fp.elem_s32(2**31 + 5) == -2**31 + 5 and fp.elem_s32(2**31 - 1) == 2**31 - 1
    assert fp.byte_u32(2**30 + 5) == 5 and fp.byte_u32(2**30 - 1) == 2**30 - 1
    assert fp.byte_s32(2**29 + 5) == -2**29 + 5 and fp.byte_s32(2**29 - 1) == 2**29 - 1
    assert fp.byte_u32(2**29 + 5, 8) == 5 and fp.byte_s32(2**28 + 5, 8) == -2**28 + 5


@pytest.mark.parametrize('chunk', CHUNKS)
def test_by_index(chunk):
    windows = fp.by_index(chunk)
    assert [w.name for w in windows] == ['near', 'byte_2_31', 'byte_2_32', 'elem_2_31', 'past']
    assert len({w.start % 1024 for w in windows}) == 1 and len({w.stop - w.start for w in windows}) == 1
    for w in windows:
        assert w.stop - w.start >= 3*chunk and (w.stop - w.start) % 2 == 1 and w.guard >= chunk
        if w.boundary is not None:
            assert w.start + chunk < w.boundary < w.start + 2*chunk - 1
    assert windows[0].stop + windows[0].guard < 2**29 - 2**20 and windows[-1].start - windows[-1].guard > 2**31
    fp.check_disjoint(windows)
    # one placement is written at a time (the straddlers of 2^30 and 2^31 are each other's image under byte_u32)
    per = windows[0].stop - windows[0].start + 2*windows[0].guard
    moved = {w.name: fp.check_wraps(fp.touched([w]), fp.intervals([w])) for w in windows}
    assert moved['near'] == {'elem_s32': 0, 'byte_u32': 0, 'byte_s32': 0}
    assert moved['past'] == {'elem_s32': per, 'byte_u32': per, 'byte_s32': per}
    for name, wrap in (('byte_2_31', 'byte_s32'), ('byte_2_32', 'byte_u32'), ('elem_2_31', 'elem_s32')):
        w = windows[[v.name for v in windows].index(name)]
        assert moved[name][wrap] == w.stop + w.guard - w.boundary           # exactly the indices from the boundary on
    assert moved['byte_2_31'] == dict(moved['byte_2_31'], elem_s32=0, byte_u32=0)
    assert moved['byte_2_32']['byte_s32'] == per and moved['elem_2_31']['byte_u32'] == per


@pytest.mark.parametrize('chunk', CHUNKS)
def test_by_row(chunk):
    length = fp.window_length(chunk)
    windows = fp.by_row(length, chunk)
    assert [w.row for w in windows] == list(range(fp.ROWS))
    assert len({w.start % 1024 for w in windows}) == 1 and windows[0].start % 1024 == fp.PHASE
    assert len({w.start - w.row*fp.ROW_PITCH for w in windows}) == 1
    assert fp.row_frames(length, chunk) <= fp.ROW_PITCH and windows[-1].stop + chunk <= fp.ROW_FRAMES
    assert windows[-1].start > 2**31
    fp.check_disjoint(windows)
    moved = fp.check_wraps(fp.touched(windows), fp.intervals(windows))
    per = length + 2*chunk
    assert moved == {'elem_s32': per, 'byte_u32': 3*per, 'byte_s32': 4*per}     # rows 4; 2, 3, 4; 1 ... 4


@pytest.mark.parametrize('call', sorted(fp.output_plans()))
def test_output_rows(call):
    """The output rows of every call the GPU module makes into the output block, from the constants it uses: the rows
    and the guard elements beside them lie inside the block and apart from each other, and a wrapped write lands inside
    the block on none of them."""
    itemsize, sets = fp.output_plans()[call]
    windows = fp.output_windows(sets)
    lo, hi = fp.owned(itemsize)
    assert all(lo <= w.start - w.guard and w.stop + w.guard <= hi for w in windows)
    fp.check_disjoint(windows)
    moved = fp.check_wraps(fp.touched(windows), fp.intervals(windows), itemsize)
    if len(windows) >= fp.ROWS:                                  # rows placed by a pitch: the last row starts past byte 2^33
        assert windows[-1].start*itemsize > 2**33 and moved['byte_u32'] >= windows[-1].stop - windows[-1].start
        assert moved['byte_s32'] > moved['byte_u32']


def test_output_plans_cover_the_shapes():
    plans = fp.output_plans()
    assert plans['events, by row'] == (8, [(fp.ROW_PITCH//2, 5, 4096, 0)])
    assert plans['peaks, by row'][1][1] == (fp.ROW_PITCH//2, 5, 32768, 2**16)
    assert [plans['fir %d, by row' % s][1][0][2] for s in fp.FIR_STEPS] == [12109, 1730, 768]
    assert plans['filtfilt, by index, past'][1][0][3] == fp.PAST + fp.PHASE
    # the props rows one block of 2^20 further on -- where a first draft had them -- end outside the block: the check fails
    bad = fp.output_windows([(fp.ROW_PITCH//2, 5, 32768, 2**20)])
    with pytest.raises(AssertionError, match='outside the block'):
        fp.check_wraps(fp.touched(bad), fp.intervals(bad), 8)


def test_slab_windows():
    windows = fp.slab_windows()
    F = fp.SLAB_F
    assert len(windows) == 5 and all(w.start % F == 0 and w.stop - w.start == fp.SLAB_ROWS*F for w in windows)
    for w in windows[1:4]:
        assert w.start < w.boundary < w.stop and w.boundary % F != 0       # the boundary falls inside a frame
    fp.check_disjoint(windows)
    for w in windows:                                                       # one at a time, as by index
        fp.check_wraps(fp.touched([w]), fp.intervals([w]))
    # hipdsp_unpack_spectrum_f64: five channels ROW_PITCH apart, three frames of F bins each
    rows = fp.by_row(3*F, 64)
    fp.check_disjoint(rows)
    fp.check_wraps(fp.touched(rows), fp.intervals(rows))


def test_band_and_stride_plans():
    for plan in (fp.band_plan(), fp.stride_plan()):
        idx, written = plan[:2]
        spans = sorted(written)
        assert all(a1 <= b0 for (a0, a1), (b0, b1) in zip(spans, spans[1:]))
        moved = fp.check_wraps(idx, written, 4, *plan[2:])
        assert moved['elem_s32'] >= 1 and moved['byte_u32'] > moved['elem_s32']
    idx, written, groups, row_groups = fp.band_plan()
    with pytest.raises(AssertionError, match='lands on written memory'):       # (without the groups: rows 1024 apart)
        fp.check_wraps(idx, written)
    assert row_groups.tolist() == [0]*1024 + [1]*1024 + [2]*4
    assert len(idx) == fp.BAND_ROWS*fp.BAND_COLS
    assert int((idx >= 2**31).sum()) == 4*fp.BAND_COLS
    idx, written = fp.stride_plan()
    assert len(idx) == 301 and np.all(np.diff(idx) == fp.STRIDE_STEP)


def test_a_plan_that_breaks_a_rule_is_caught():
    """The checks do fail: written together, the windows that straddle 2^30 and 2^31 are each other's image under the
    unsigned byte wrap, and so is a near window at element 0."""
    windows = fp.by_index(4096)
    with pytest.raises(AssertionError, match='byte_u32 lands on written memory'):
        fp.check_wraps(fp.touched(windows), fp.intervals(windows))
    bad = [fp.Window('near', fp.PHASE + 4096, fp.PHASE + 4096 + fp.window_length(4096), 4096, None, None), windows[2]]
    with pytest.raises(AssertionError, match='lands on written memory'):
        fp.check_wraps(fp.touched(bad), fp.intervals(bad))
    with pytest.raises(AssertionError, match='overlap'):
        fp.check_disjoint(windows + [windows[2]._replace(start=windows[2].start + 100)])
    with pytest.raises(AssertionError, match='outside the block'):
        fp.check_wraps([fp.ROW_FRAMES], [])


def test_band_values_show_every_wrap():
    """check_wraps looks at addresses only; whether a wrapped read changes the ANSWER of hipdsp_band_order_stats is
    replayed here on the plan's host values: unwrapped the definition's pair, and under each of the three wraps -- the
    signed element index included, which moves only the four rows past 2^31 -- both order statistics differ."""
    host, rank, want = fp.band_values()
    values = host[:, 1:-1]
    order = np.sort(values.reshape(-1))
    assert want == (order[rank], order[rank + 1]) and fp.band_replay(host, rank) == want
    assert values[2048:].max() < 1.0 <= values[:1024].min() and values[:1024].max() < 2.0 <= values[1024:2048].min()
    assert (host[:, 0] == fp.BAND_GUARD).all() and (host[:, -1] == fp.BAND_GUARD).all()
    for name, fn, limit in fp.WRAPS:
        got = fp.band_replay(host, rank, fn)
        assert got[0] != want[0] and not got[1] == want[1], (name, got, want)
    # a guard element read in place of a value: one more value under the rank
    shifted = host.copy()
    shifted[1500, 1] = shifted[1500, 0]
    assert fp.band_replay(shifted, rank) != want
