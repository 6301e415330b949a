"""hipdsp_common_reference without a GPU: the definition (common_reference_definition.py) against numpy's own mean and
median and against a longdouble evaluation, its NaN, infinity and `use` rules, and BufferedCommonReference's host path in a
host-only TraceGraph: groups, excluded and pass-through channels, update() and every ValueError."""

import os

import numpy as np
import pytest

import common_reference_definition as cd
from conftest import ROOT
from audian_amd.bufferedcommonreference import BufferedCommonReference, common_reference_host
from audian_amd.buffereddata import BufferedData
from audian_amd.tracegraph import TraceGraph

COUNTS = [1, 2, 3, 5, 8, 9, 33, 64, 65, 256]


def spread_rows(n, frames, seed):
    """n rows of normal floats whose scales spread over 12 decades, float32."""
    rng = np.random.default_rng(seed)
    scales = 10.0**rng.uniform(-6, 6, size=(n, 1))
    return (rng.standard_normal((n, frames))*scales).astype(np.float32)


@pytest.mark.parametrize('n', COUNTS)
def test_definition_against_numpy(n):
    """Bit-identical to x64 - np.mean(x64, 0) and x64 - np.median(x64, 0) rounded to float32 (reducing a C-contiguous
    array over axis 0, numpy adds the rows one by one: the same sum)."""
    x = spread_rows(n, 512, n)
    x64 = x.astype(np.float64)
    group = np.zeros(n, dtype=int)
    got = cd.common_reference(x, group, None, cd.MEAN)
    assert got.dtype == np.float32
    assert got.tobytes() == (x64 - np.mean(x64, 0)).astype(np.float32).tobytes()
    got = cd.common_reference(x, group, None, cd.MEDIAN)
    assert got.tobytes() == (x64 - np.median(x64, 0)).astype(np.float32).tobytes()


@pytest.mark.parametrize('n', COUNTS)
def test_mean_within_its_stated_bound(n):
    """|y - exact| <= 2^-24 |y| + (n + 2) 2^-53 sum|x|: one float32 rounding of the result and a float64 sum of n terms,
    a division and a subtraction (each 2^-53 relative to at most sum|x| ... the first-order bound of recursive
    summation), the exact value in longdouble."""
    x = spread_rows(n, 2048, 100 + n)
    got = cd.common_reference(x, np.zeros(n, dtype=int), None, cd.MEAN).astype(np.longdouble)
    xl = x.astype(np.longdouble)
    exact = xl - np.sum(xl, 0)/np.longdouble(n)
    bound = np.longdouble(2.0**-24)*np.abs(exact) + np.longdouble((n + 2)*2.0**-53)*np.sum(np.abs(xl), 0)
    ratio = np.max(np.abs(got - exact)/bound)
    print('n = %d: worst |error| / bound = %.4f' % (n, float(ratio)))
    assert ratio <= 1.0


def test_nan_infinity_and_use_rules():
    x = np.array([[1, 2, 3, 4, 5, 6],
                  [4, np.nan, np.inf, np.inf, -np.inf, 0],
                  [7, 8, 9, -np.inf, -np.inf, -0.0],
                  [10, 11, 12, 13, 14, 0]], dtype=np.float32)
    grp = np.zeros(4, dtype=int)
    y = cd.common_reference(x, grp, None, cd.MEAN)
    assert np.array_equal(y[:, 0], [-4.5, -1.5, 1.5, 4.5])
    assert np.all(np.isnan(y[:, 1]))                                   # a NaN among the refs
    assert np.all(y[[0, 2, 3], 2] == -np.inf) and np.isnan(y[1, 2])    # mean = inf; inf - inf = NaN
    assert np.all(np.isnan(y[:, 3]))                                   # inf + -inf
    assert np.all(y[[0, 3], 4] == np.inf) and np.all(np.isnan(y[[1, 2], 4]))
    y = cd.common_reference(x, grp, None, cd.MEDIAN)
    assert np.array_equal(y[:, 0], [-4.5, -1.5, 1.5, 4.5])             # (4 + 7) / 2
    assert np.all(np.isnan(y[:, 1]))
    assert np.array_equal(y[[0, 2, 3], 2], [-7.5, -1.5, 1.5]) and y[1, 2] == np.inf      # (9 + 12) / 2
    assert np.array_equal(y[[0, 3], 3], [-4.5, 4.5]) and y[1, 3] == np.inf and y[2, 3] == -np.inf   # (4 + 13) / 2
    assert np.all(y[[0, 3], 4] == np.inf) and np.all(np.isnan(y[[1, 2], 4]))      # (-inf + 5) / 2 = -inf
    y3 = cd.common_reference(x[:3], grp[:3], None, cd.MEDIAN)
    assert np.all(np.isnan(y3[1:, 4])) and y3[0, 4] == np.inf          # the middle one is -inf: -inf - -inf = NaN
    assert np.array_equal(cd.common_reference(x, grp, None, cd.MEDIAN)[:, 5], [6, 0, 0, 0])     # zeros of either sign
    # use == 0: re-referenced, does not contribute -- the NaN and the infinities of row 1 stay in row 1
    use = np.array([1, 0, 1, 1])
    for mode in (cd.MEAN, cd.MEDIAN):
        y = cd.common_reference(x[:, :3], grp, use, mode)
        keep = cd.common_reference(x[[0, 2, 3], :3], grp[:3], None, mode)
        assert y[[0, 2, 3]].tobytes() == keep.tobytes()
        assert y[1, 0] == (4 - 6 if mode == cd.MEAN else 4 - 7) and np.isnan(y[1, 1]) and y[1, 2] == np.inf
    # group -1 is copied bit for bit, groups do not see one another
    grp = np.array([1, -1, 1, 3])
    y = cd.common_reference(x, grp, None, cd.MEAN)
    assert y[1].tobytes() == x[1].tobytes() and np.all(y[3] == 0)
    assert y[[0, 2]].tobytes() == cd.common_reference(x[[0, 2]], [0, 0], None, cd.MEAN).tobytes()
    with pytest.raises(AssertionError):
        cd.common_reference(x, grp, [1, 1, 1, 0], cd.MEAN)             # members and no reference channel


def test_comparator():
    a = np.array([1.0, np.nan, 0.0, -0.0, np.inf], dtype=np.float32)
    cd.assert_same(a, a.copy())
    cd.assert_same(a, np.array([1.0, np.nan, -0.0, 0.0, np.inf], dtype=np.float32))
    for i, v in ((0, np.nextafter(np.float32(1), np.float32(2))), (1, 0.0), (2, np.nan), (4, -np.inf), (3, 1e-45)):
        b = a.copy()
        b[i] = v
        with pytest.raises(AssertionError):
            cd.assert_same(b, a)
    with pytest.raises(AssertionError):
        cd.assert_same(a.astype(np.float64), a)


def test_host_twin_is_the_definition():
    x = spread_rows(9, 300, 9)
    x[2, 5], x[4, 7], x[5, 7], x[0, 9] = np.nan, np.inf, -np.inf, -0.0
    group = np.array([0, 0, 2, -1, 2, 2, 0, -1, 2])
    use = np.array([1, 0, 1, 1, 1, 0, 1, 0, 1])
    for mode in (cd.MEAN, cd.MEDIAN):
        got = common_reference_host(x.T.astype(np.float64), group, use, mode)
        cd.assert_same(np.ascontiguousarray(got.T), cd.common_reference(x, group, use, mode), mode)


# ---- the facade on the host -------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True


class HostCopy(BufferedData):
    """A derived trace without a device mirror: its source, computed with numpy."""

    def __init__(self, name='raw', source='data', gain=1.0):
        BufferedData.__init__(self, name, source, panel='trace')
        self.calls, self.gain = 0, gain

    def open(self, source):
        BufferedData.open(self, source, 1)

    def process(self, source, dest, nbefore):
        self._pending = None
        self.calls += 1
        dest[...] = self.gain*np.asarray(source[nbefore:])


def host_graph(x, rate, ref, buffer_time=4.0, back_time=1.0):
    g = TraceGraph(buffer_time, back_time)
    raw, below = HostCopy(), HostCopy('below', ref.name, gain=2.0)
    for t in (raw, ref, below):
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    return g, raw, below


def test_facade_on_the_host():
    rate, C = 1000.0, 7
    n = int(20*rate) + 3
    x = spread_rows(C, n, 21).T.astype(np.float64)
    groups, exclude = [[0, 2, 5], [6, 1]], (2,)
    ref = BufferedCommonReference(source='raw', method='mean', groups=groups, exclude=exclude)
    assert (ref.name, ref.source_name, ref.panel, ref.panel_type) == ('rereferenced', 'raw', 'trace', 'trace')
    assert BufferedCommonReference().source_name == 'data' and BufferedCommonReference().method == 'mean'
    g, raw, below = host_graph(x, rate, ref)
    assert ref.source is raw and below.source is ref
    assert (ref.rate, ref.frames, ref.shape, ref.channels, ref.unit) == (rate, n, (n, C), C, raw.unit)
    assert (ref.ampl_min, ref.ampl_max) == (raw.ampl_min, raw.ampl_max)
    assert (ref.tbefore, ref.tafter, ref.source_tbefore, ref.source_tafter) == (0, 0, 0, 0)
    assert np.array_equal(ref.group, [0, 1, 0, -1, -1, 0, 1]) and np.array_equal(ref.use, [1, 1, 0, 1, 1, 1, 1])

    def check():
        a, b = ref.offset, ref.offset + len(ref.buffer)
        assert (a, b) == (raw.offset, raw.offset + len(raw.buffer)) and b > a
        want = cd.common_reference(np.ascontiguousarray(x[a:b].T).astype(np.float32), ref.group, ref.use, ref.method)
        got = np.asarray(ref.buffer)
        cd.assert_same(np.ascontiguousarray(got.T).astype(np.float32), want, ref.method)
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)
        for c in np.flatnonzero(ref.group < 0):                      # pass-through: the source as float32
            assert np.array_equal(got[:, c], x[a:b, c].astype(np.float32))
        assert np.array_equal(np.asarray(below.buffer), 2.0*got, equal_nan=True)

    for t0, t1 in [(0.0, 2.0), (1.0003, 3.0), (12.0001, 14.0), (11.0, 12.0), (18.0, 20.1)]:
        g.update_times(t0, t1)
        check()
    calls, below_calls = raw.calls, below.calls
    ref.update(method='median')
    check()
    ref.update(groups=[range(C)], exclude=())
    assert np.all(ref.group == 0) and np.all(ref.use)
    check()
    ref.update(exclude=[0, 6])
    assert ref.method == 'median' and ref.groups == [list(range(C))]
    check()
    assert raw.calls == calls and below.calls == below_calls + 3     # the destinations, never the source
    # a bad argument raises before anything is computed and changes nothing
    state = (ref.method, ref.groups, ref.exclude, ref.group.copy(), ref.use.copy())
    for kwargs in (dict(method='mode'), dict(groups=[[0, 1], [1, 2]]), dict(groups=[[0, C]]), dict(groups=[[-1]]),
                   dict(groups=[[0], []]), dict(groups=[[0.5]]), dict(exclude=[C]), dict(exclude=[-1]),
                   dict(groups=[[0, 1], [2]], exclude=[2]), dict(exclude=range(C)),
                   dict(groups=[[c] for c in range(C)] + [[0]])):
        with pytest.raises(ValueError):
            ref.update(**kwargs)
        assert (ref.method, ref.groups, ref.exclude) == state[:3]
        assert np.array_equal(ref.group, state[3]) and np.array_equal(ref.use, state[4])
    assert raw.calls == calls and below.calls == below_calls + 3
    g.update_times(5.0002, 7.0)
    check()


def test_open_refuses_what_update_refuses():
    x = np.zeros((100, 3))
    for kwargs in (dict(groups=[[0, 3]]), dict(exclude=(0, 1, 2)), dict(method='mode'), dict(groups=[[1], [1]])):
        ref = BufferedCommonReference(source='raw', **kwargs)
        with pytest.raises(ValueError):
            host_graph(x, 100.0, ref)

    class Spectra:                                                   # one row of bins per frame: not a trace
        name, shape, dests = 'spectrogram', (100, 2, 129), []

    with pytest.raises(ValueError):
        BufferedCommonReference(source='spectrogram').open(Spectra())


def test_process_on_plain_arrays():
    x = spread_rows(4, 50, 5).T.astype(np.float64)
    g, raw, below = host_graph(x, 100.0, BufferedCommonReference(source='raw', method='median', exclude=[3]))
    ref = below.source
    dest = np.full((47, 4), np.nan)
    ref.process(x, dest, 3)
    want = cd.common_reference(np.ascontiguousarray(x[3:].T).astype(np.float32), [0]*4, [1, 1, 1, 0], cd.MEDIAN)
    cd.assert_same(np.ascontiguousarray(dest.T).astype(np.float32), want)
    with pytest.raises(ValueError):
        ref.process(x, np.zeros((48, 4)), 3)


def test_the_binding_declares_the_entry():
    from audian_amd import _lib, hipdsp
    args, res = _lib._SIGNATURES['hipdsp_common_reference']
    assert len(args) == 10 and res is _lib._int and hasattr(_lib.lib, 'hipdsp_common_reference')
    assert (hipdsp.CREF_MEAN, hipdsp.CREF_MEDIAN, hipdsp.CREF_TILE) == (0, 1, 1024)
    text = open(os.path.join(ROOT, 'include', 'hip_dsp.h')).read()
    for name, value in (('HIPDSP_CREF_MEAN', 0), ('HIPDSP_CREF_MEDIAN', 1), ('HIPDSP_CREF_TILE', 1024)):
        assert '#define %s' % name in text and int(text.split('#define %s' % name)[1].split()[0]) == value
