"""hipdsp_region_filtfilt on the GPU.  The comparator is never the code under test: iir_bound.sosfiltfilt (scipy's
sosfiltfilt restated in longdouble; gain 1, no rectification, no clamp), pinned to scipy by tests/golden/region_filtfilt.npz.

The kernel extends a region of L samples to E = L + 2 padlen, cuts that sequence into chunks of C = hipdsp.FILTER_CHUNK =
64 samples counted from its first sample (one lane each; the backward pass counts from the last sample) and hands 64
consecutive chunks -- a tile of T = hipdsp.FILTER_TILE = 4096 samples -- to one wave; one thread per region walks the
chunks' states.  So of the extended lengths used here 3 padlen + 1 is the smallest legal region, 63, 64 and 65 lie around
one lane's run, C-1, C, C+1 likewise, 2C+1 and 3C+5 take the hand-over past its first step with a ragged last chunk, and
T-1, T, T+1, 2T+1 and 3T+5 do the same for the tiles: the last lane short by one, a full wave, a second work item of one
sample, three and four items.

Accuracy: e_w <= (1 + 16 q) 2^-24 r_w for every window of 64 samples counted from the region's start, q the case's own
allowance (the sequential float64 recurrence against longdouble, computed here from the same inputs; the case list is
held to q <= Q_CAP by tests/test_refine_host.py).  No extension_term, no between_term."""

import ctypes
import functools

import numpy as np
import pytest

import gpu_helpers as gh
import iir_bound as ib
import refine_definition as rd
from conftest import load_golden

pytestmark = pytest.mark.gpu

C = 64                                          # hipdsp.FILTER_CHUNK
T = 64*C                                        # hipdsp.FILTER_TILE
STARTS = [0, 1, 2, 3, 5]
BASE = 3
SENTINEL = np.float32(12345.0)


def test_constants():
    from audian_amd import hipdsp
    assert (hipdsp.FILTER_CHUNK, hipdsp.FILTER_TILE) == (C, T)


def extended_lengths(pad):
    return sorted({3*pad + 1, 63, 64, 65, C - 1, C, C + 1, 2*C + 1, 3*C + 5, T - 1, T, T + 1, 2*T + 1, 3*T + 5})


class Slab(object):
    """A host (C, frames) float32 array on the device with a base offset of 3 elements and pitch = frames + 7 (as
    test_gpu_regionspectra.Slab), and an output of the same layout prefilled with 12345.0, padding and base included."""

    def __init__(self, x, pitch_extra=7, ctx=None):
        from audian_amd import hipdsp
        self.ctx = gh.ctx() if ctx is None else ctx
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.C, self.frames = self.x.shape
        self.pitch = self.frames + pitch_extra
        self.host = np.full(BASE + self.C*self.pitch, SENTINEL, dtype=np.float32)
        for c in range(self.C):
            self.host[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] = self.x[c]
        self.dev = hipdsp.DeviceArray.from_host(self.ctx, self.host)
        self.view = self.dev.view(BASE, (1,))

    def filtfilt(self, regions, sos, clamp=False, inplace=False, channels=None, frames=None):
        """The whole output allocation (base and padding included) after one call through the C ABI; in place: the
        input allocation, which is restored afterwards."""
        from audian_amd import hipdsp
        if inplace:
            out = self.dev
        else:
            out = hipdsp.DeviceArray.from_host(self.ctx, np.full(len(self.host), SENTINEL, dtype=np.float32))
        try:
            hipdsp.region_filtfilt(self.ctx, self.view, self.pitch, out.view(BASE, (1,)), self.pitch,
                                   self.C if channels is None else channels, self.frames if frames is None else frames,
                                   regions, sos, clamp)
            return out.to_host()
        finally:
            if inplace:
                self.dev.copy_from_host(self.host)
            else:
                out.free()

    def rows(self, flat):
        """(C, frames) view of the valid elements of a whole allocation."""
        return np.stack([flat[BASE + c*self.pitch:BASE + c*self.pitch + self.frames] for c in range(self.C)])

    def outside(self, flat, regions):
        """The elements of a whole allocation outside the regions."""
        mask = np.ones(len(flat), dtype=bool)
        for c, a, b in regions:
            mask[BASE + c*self.pitch + a:BASE + c*self.pitch + b] = False
        return flat[mask]


@functools.lru_cache(maxsize=None)
def accuracy_slab(labels):
    """(slab, regions, sos (R, S, 6), [(label, lane, length)]) for the cases `labels` (of equal section count): one
    region per family and extended length, three channels and the starts taking turns, regions of a channel `start`
    elements apart -- 0 makes neighbours adjacent."""
    pieces, tables = [], []
    for label in labels:
        sos, rate, fams = rd.case_design(label)
        pad = ib.padlen(sos)
        for E in extended_lengths(pad):
            L = E - 2*pad
            if L <= pad:
                continue
            x = rd.case_signal(label, L)
            for lane in range(x.shape[1]):
                pieces.append((label, lane, L, x[:, lane]))
                tables.append(sos)
    cursor = [0, 0, 0]
    regions = []
    for j, (label, lane, L, v) in enumerate(pieces):
        c = j % 3
        a = cursor[c] + STARTS[(j//3) % len(STARTS)]
        regions.append((c, a, a + L))
        cursor[c] = a + L
    frames = max(cursor) + 5
    x = np.zeros((3, frames), dtype=np.float32)
    for (c, a, b), (label, lane, L, v) in zip(regions, pieces):
        x[c, a:b] = v
    return Slab(x), regions, np.array(tables), [(label, lane, L) for label, lane, L, v in pieces]


def check_accuracy(labels):
    slab, regions, sos, what = accuracy_slab(tuple(labels))
    flat = slab.filtfilt(regions, sos)
    got = slab.rows(flat)
    assert np.all(slab.outside(flat, regions) == SENTINEL), 'an element outside the regions was written'
    worst = 0.0
    for (c, a, b), (label, lane, L) in zip(regions, what):
        table = rd.case_design(label)[0]
        ref, q = rd.filtfilt_case(table, rd.case_signal(label, L))
        worst = max(worst, ib.assert_within(got[c, a:b, None], ref[:, lane:lane + 1], q[lane],
                                            '%s, family %d, L %d at channel %d start %d' % (label, lane, L, c, a), first=0))
    print('%s: worst e_w / (2^-24 r_w) = %.4f over %d regions' % (', '.join(labels), worst, len(regions)))


def test_reference_filters_in_one_call_within_the_bound():
    """The three first-order low-passes of the reference ride in ONE call, every region with its own table: a region
    that picks up a neighbour's coefficients fails.  Every window of every region within the bound; nothing outside
    the regions written (adjacent regions included)."""
    check_accuracy(rd.LP1)


@pytest.mark.parametrize('label', [k for k in rd.CASES if k not in rd.LP1])
def test_every_window_within_the_bound(label):
    check_accuracy([label])


# ---- a small slab for the exact properties ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small():
    """(slab, regions, sos): noise on three channels; regions of one- and many-chunk lengths, two of them adjacent,
    every one with its own first-order low-pass."""
    from audian_amd.design import butter_sos
    rng = np.random.default_rng(7)
    x = (0.5 + 0.3*rng.standard_normal((3, 3*T + 200))).astype(np.float32)
    regions = [(0, 0, 7), (0, 7, 7 + 2*T + 9), (1, 5, 5 + 130), (1, 200, 200 + T + 1), (2, 3, 3 + 3*T + 5), (0, 2*T + 30, 2*T + 95)]
    sos = np.array([butter_sos(1, 40.0*(i + 1), 'lowpass', 5000.0) for i in range(len(regions))])
    return Slab(x), regions, sos


def test_in_place_equals_out_of_place():
    slab, regions, sos = small()
    there = slab.filtfilt(regions, sos)
    here = slab.filtfilt(regions, sos, inplace=True)
    for c, a, b in regions:
        lo = BASE + c*slab.pitch
        assert here[lo + a:lo + b].tobytes() == there[lo + a:lo + b].tobytes()
    assert slab.outside(here, regions).tobytes() == slab.outside(slab.host, regions).tobytes()
    assert np.all(slab.outside(there, regions) == SENTINEL)


def test_a_region_does_not_depend_on_the_call():
    """Alone, all together, the table reversed, `channels` raised over unused rows, twice: the same bytes."""
    slab, regions, sos = small()
    full = slab.filtfilt(regions, sos)
    assert slab.filtfilt(regions, sos).tobytes() == full.tobytes()
    assert slab.filtfilt(regions[::-1], sos[::-1]).tobytes() == full.tobytes()
    wide = np.concatenate((slab.x, np.ones((2, slab.frames), dtype=np.float32)))
    wslab = Slab(wide)
    wfull = wslab.filtfilt(regions, sos)
    for i, (c, a, b) in enumerate(regions):
        lo = BASE + c*slab.pitch
        alone = slab.filtfilt([regions[i]], sos[i:i + 1])
        assert alone[lo + a:lo + b].tobytes() == full[lo + a:lo + b].tobytes(), regions[i]
        assert np.all(slab.outside(alone, [regions[i]]) == SENTINEL)
        assert wfull[lo + a:lo + b].tobytes() == full[lo + a:lo + b].tobytes()


def test_two_sections_do_not_depend_on_the_call():
    from audian_amd.design import butter_sos
    slab, regions, _ = small()
    regions = regions[1:]                                                   # (0, 0, 7) is too short for padlen 15
    sos = np.array([butter_sos(4, 100.0*(i + 1), 'lowpass', 48000.0) for i in range(len(regions))])
    full = slab.filtfilt(regions, sos)
    assert slab.filtfilt(regions[::-1], sos[::-1]).tobytes() == full.tobytes()
    for i, (c, a, b) in enumerate(regions):
        lo = BASE + c*slab.pitch
        alone = slab.filtfilt([regions[i]], sos[i:i + 1])
        assert alone[lo + a:lo + b].tobytes() == full[lo + a:lo + b].tobytes(), regions[i]


def test_clamp_is_the_clamp_of_the_unclamped_result():
    slab, regions, sos = small()
    x = slab.x - np.float32(0.5)                                            # around zero: negative results
    s = Slab(x)
    plain = s.filtfilt(regions, sos)
    clamped = s.filtfilt(regions, sos, clamp=True)
    assert np.any(plain < 0)
    assert clamped.tobytes() == np.where(plain < 0, np.float32(0), plain).tobytes()


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_makes_its_region_nan(bad):
    slab, regions, sos = small()
    clean = slab.filtfilt(regions, sos)
    for victim, where in ((1, 2*T + 8), (0, 3), (4, 0), (3, T)):          # last sample, a short region, first sample, last
        x = slab.x.copy()
        c, a, b = regions[victim]
        x[c, a + where] = bad
        flat = Slab(x).filtfilt(regions, sos)
        lo = BASE + c*slab.pitch
        assert np.all(np.isnan(flat[lo + a:lo + b])), (victim, where)
        keep = np.ones(len(flat), dtype=bool)
        keep[lo + a:lo + b] = False
        assert flat[keep].tobytes() == clean[keep].tobytes(), (victim, where)


def test_errors_leave_the_output_alone():
    from audian_amd import _lib, hipdsp
    from audian_amd.design import butter_sos
    slab, regions, sos = small()
    out = hipdsp.DeviceArray.from_host(slab.ctx, np.full(len(slab.host), SENTINEL, dtype=np.float32))
    one = butter_sos(1, 40.0, 'lowpass', 5000.0)

    def call(regs, tables, x=None, y=None, frames=None, n_sections=None, y_pitch=None):
        tab = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 3)
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        st = _lib.lib.hipdsp_region_filtfilt(
            slab.ctx.handle, ctypes.c_void_p(slab.view.ptr if x is None else x), slab.pitch,
            ctypes.c_void_p(out.ptr + 4*BASE if y is None else y), slab.pitch if y_pitch is None else y_pitch, slab.C,
            slab.frames if frames is None else frames, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(tab),
            tables.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            tables.shape[1] if n_sections is None else n_sections, 0)
        slab.ctx.synchronize()
        assert np.all(out.to_host() == SENTINEL), 'an error wrote to the output'
        return st

    good = [(0, 10, 200), (1, 0, 50)]
    both = np.array([one, one])
    assert call([(0, 10, 16), (1, 0, 50)], both) == _lib.ERR_TOO_SHORT                      # L == padlen
    assert 'padlen' in _lib.last_error()
    assert call([(0, 10, 200), (0, 199, 300)], both) == _lib.ERR_INVALID                    # overlap in one channel
    assert 'overlap' in _lib.last_error()
    t = both.copy()
    t[1, 0, 3] = 2.0
    assert call(good, t) == _lib.ERR_INVALID                                                # a0 != 1
    t = both.copy()
    t[1, 0, 4] = -1.0
    assert call(good, t) == _lib.ERR_INVALID                                                # a pole at z = 1
    t = both.copy()
    t[0, 0, 1] = np.nan
    assert call(good, t) == _lib.ERR_INVALID
    assert call([(0, 10, slab.frames + 1), (1, 0, 50)], both) == _lib.ERR_INVALID
    assert call([(0, 200, 10), (1, 0, 50)], both) == _lib.ERR_INVALID
    assert call([(3, 10, 200), (1, 0, 50)], both) == _lib.ERR_INVALID
    assert call([(-1, 10, 200), (1, 0, 50)], both) == _lib.ERR_INVALID
    assert call(good, both, y=slab.view.ptr + 4*16) == _lib.ERR_INVALID                     # partial overlap of x and y
    assert call(good, both, y=slab.view.ptr, y_pitch=slab.pitch + 1) == _lib.ERR_INVALID    # y == x, unequal pitches
    assert call(good, both, x=slab.view.ptr + 1) == _lib.ERR_INVALID                        # misaligned
    assert call(good, both, frames=slab.pitch + 1) == _lib.ERR_INVALID                      # pitch below frames
    assert call(good, both, n_sections=0) == _lib.ERR_UNSUPPORTED
    assert call(good, np.zeros((2, 3, 6)), n_sections=3) == _lib.ERR_UNSUPPORTED
    assert call(np.zeros((0, 3)), np.zeros((0, 1, 6)), n_sections=1) == _lib.OK             # nothing to do is fine
    # adjacent regions are no overlap
    assert _lib.lib.hipdsp_region_filtfilt(
        slab.ctx.handle, ctypes.c_void_p(slab.view.ptr), slab.pitch, ctypes.c_void_p(out.ptr + 4*BASE), slab.pitch, slab.C,
        slab.frames, (ctypes.c_int64*6)(0, 10, 200, 0, 200, 300), 2, both.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1,
        0) == _lib.OK
    slab.ctx.synchronize()
    out.free()


def test_refused_inside_a_graph_capture():
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = hipdsp.Context(0)
    stream = c.create_stream()
    c.set_stream(stream)
    x = np.linspace(0.0, 1.0, 500, dtype=np.float32)[None, :]
    dx = hipdsp.DeviceArray.from_host(c, x)
    dy = hipdsp.DeviceArray.from_host(c, np.full((1, 500), SENTINEL, dtype=np.float32))
    dz = hipdsp.DeviceArray.from_host(c, np.zeros((1, 500), dtype=np.float32))
    sos = butter_sos(1, 40.0, 'lowpass', 5000.0)[None]
    hipdsp.region_filtfilt(c, dx, 500, dz, 500, 1, 500, [(0, 0, 500)], sos)                 # fine outside a capture
    c.synchronize()
    c.graph_begin()
    try:
        hipdsp.decibel(c, dx, dz, 500)                                                      # something legal to capture
        with pytest.raises(ValueError, match='capture'):
            hipdsp.region_filtfilt(c, dx, 500, dy, 500, 1, 500, [(0, 0, 500)], sos)
    finally:
        graph = c.graph_end()
    c.graph_launch(graph)
    c.synchronize()
    assert np.all(dy.to_host() == SENTINEL)
    c.graph_destroy(graph)
    c.set_stream(None)
    c.destroy_stream(stream)


def test_golden_inputs_through_the_c_abi():
    """scipy's own outputs (sosfiltfilt, and filtfilt for the reference's first-order filters) within the bound of what
    the kernel gives for the golden inputs; q from the sequential float64 run of the same inputs."""
    g = load_golden('region_filtfilt')
    off, ffo = g['offsets'], g['ff_offsets']
    for S in (1, 2):
        idx = [i for i in range(len(g['sections'])) if g['sections'][i] == S]
        x = np.zeros((1, sum(int(off[i + 1] - off[i]) for i in idx) + 3*len(idx)), dtype=np.float32)
        regions, a = [], 2
        for i in idx:
            n = int(off[i + 1] - off[i])
            x[0, a:a + n] = g['x'][off[i]:off[i + 1]]
            regions.append((0, a, a + n))
            a += n + 3
        slab = Slab(x)
        got = slab.rows(slab.filtfilt(regions, g['sos'][idx][:, :S]))
        for i, (c, a, b) in zip(idx, regions):
            v = g['x'][off[i]:off[i + 1]][:, None]
            sos = g['sos'][i][:S]
            ref, q = rd.filtfilt_case(sos, v)
            ib.assert_within(got[0, a:b, None], g['y_sosfiltfilt'][off[i]:off[i + 1], None], q, 'golden case %d, sosfiltfilt' % i)
            if S == 1:
                ib.assert_within(got[0, a:b, None], g['y_filtfilt'][ffo[i]:ffo[i + 1], None], q, 'golden case %d, filtfilt' % i)
