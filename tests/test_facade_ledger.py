"""The ledger of tests/facade_ledger.py proves itself without a GPU: the walks of tests/test_gpu_facade_all.py over a
host-only graph (the oracle twins of test_gpu_facade.py for filter, envelope and spectrogram, the package's numpy fallbacks
for the rest -- the first walk of their _host_wrote bookkeeping), three mutants that check() must catch by trace and frame,
and the regression of BufferedKernelFilter.update(step=...) with a trace below it."""

import re

import numpy as np
import pytest

import facade_ledger as fl
from audian_amd.bufferedcommonreference import BufferedCommonReference, common_reference_host
from audian_amd.bufferedkernelfilter import BufferedKernelFilter
from audian_amd.bufferedlowpass import BufferedLowpass
from audian_amd.tracegraph import TraceGraph


def host_classes(oracle):
    """Traces without a device: the oracle twins, their results rounded to float32 as a mirror would hold them, and the
    common reference through its numpy definition (with the loader as its source the built-in one goes to the device)."""
    from test_gpu_facade import oracle_twins
    OFilter, OEnvelope, OSpectrogram = oracle_twins(oracle)

    def rounded(cls):
        class Twin(cls):
            def process(self, source, dest, nbefore):
                with np.errstate(all='ignore'):
                    cls.process(self, np.asarray(source[:]), dest, nbefore)
                    dest[...] = dest.astype(np.float32)
        Twin.__name__ = cls.__name__
        return Twin

    class HostReference(BufferedCommonReference):
        def process(self, source, dest, nbefore):
            call = self._take_call(source, dest)
            if len(dest) > 0:
                slab = np.asarray(source[nbefore:]).reshape(len(dest), -1)
                dest[...] = common_reference_host(slab, self.group, self.use, self.method)
                self._host_wrote(call)

    return HostReference, rounded(OFilter), rounded(OEnvelope), rounded(OSpectrogram)


REACHED = fl.new_reached()


@pytest.mark.parametrize('seed', [0, 1])
def test_host_walks(oracle, seed):
    w = fl.walk(host_classes(oracle), oracle, seed, False, REACHED)
    assert all(not t._stale and t._dev is None for t in w.ledger.traces)        # nothing went to a device


def test_host_walk_with_non_finite_samples(oracle):
    fl.walk(host_classes(oracle), oracle, 100, True, REACHED)


def test_zz_the_host_walks_reached():
    """What the walks must have met on the way, and the template match's inputs: the windows the mask cannot decide stay
    under 1 % (the ledger also holds every single call to that)."""
    assert REACHED['walks'] == 3
    names = ['rereferenced', 'filtered', 'envelope', 'features', 'below', 'eventfiltered', 'spectrogram', 'bandpower',
             'peakfreq', 'match', 'power-envelope', 'slow-envelope']
    assert all(REACHED['partial'].get(n, 0) >= 3 for n in names), REACHED['partial']
    assert all(REACHED['source'].get(n, 0) >= 1 for n in names[1:]), REACHED['source']
    assert REACHED['refitted'] >= 1 and REACHED['features step'] >= 1 and REACHED['power-envelope step'] >= 1
    assert REACHED['near'][1] > 1000 and REACHED['near'][0] <= fl.NEAR_CAP*REACHED['near'][1]


# ---- the mutants --------------------------------------------------------------------------------------------------------

class LateStrip(BufferedKernelFilter):
    """A strip (a load of a part of the buffer) written one frame late."""

    strips = ()

    def process(self, source, dest, nbefore):
        call = self._pending
        BufferedKernelFilter.process(self, source, dest, nbefore)
        if call is not None and 1 < call.dnframes < len(self._hostbuf):
            dest[1:] = np.array(dest[:-1])
            dest[0] = 0.0
            self.strips = self.strips + ((self.offset + call.doffset, self.offset + call.doffset + call.dnframes),)


class ShortStrip(BufferedKernelFilter):
    """The last frame of a strip left unwritten."""

    strips = ()

    def process(self, source, dest, nbefore):
        call = self._pending
        BufferedKernelFilter.process(self, source, dest, nbefore)
        if call is not None and 1 < call.dnframes < len(self._hostbuf):
            dest[-1] = 0.0
            self.strips = self.strips + ((self.offset + call.doffset, self.offset + call.doffset + call.dnframes),)


class StuckOverlap(BufferedLowpass):
    """A recycled overlap that is not moved with the buffer: it stays at the indices it had."""

    kept = ()

    def _adopt_buffer(self, new, offset, old_offset, old_nframes, keep0, keep1):
        if keep1 > keep0 and offset != old_offset:
            part = np.array(new[keep0 - offset:keep1 - offset])
            new[keep0 - offset:keep1 - offset] = np.roll(part, offset - old_offset, axis=0)
            self.kept = self.kept + ((keep0, keep1),)
        BufferedLowpass._adopt_buffer(self, new, offset, old_offset, old_nframes, keep0, keep1)


def scroll_a_mutant(oracle, name, cls):
    w = fl.Walk(host_classes(oracle), oracle, 0, False, swap={name: cls})
    w.move(0.0, 1.5)
    assert not (w.g[name].strips if hasattr(cls, 'strips') else w.g[name].kept)       # nothing mutated yet: it passed
    with pytest.raises(AssertionError) as info:
        for t0 in (w.end_zone, w.end_zone + 0.7, w.end_zone + 1.6, 8.0):
            w.move(t0, 1.5)
    found = re.match(r'%s: frame (\d+) ' % name, str(info.value))
    assert found, str(info.value)
    return w.g[name], int(found.group(1))


def test_a_strip_written_one_frame_late_is_caught(oracle):
    t, frame = scroll_a_mutant(oracle, 'features', LateStrip)
    assert any(a <= frame < b for a, b in t.strips), (frame, t.strips)


def test_an_unwritten_last_frame_is_caught(oracle):
    t, frame = scroll_a_mutant(oracle, 'features', ShortStrip)
    assert frame in [b - 1 for a, b in t.strips], (frame, t.strips)


def test_an_overlap_that_is_not_moved_is_caught(oracle):
    t, frame = scroll_a_mutant(oracle, 'slow-envelope', StuckOverlap)
    assert any(a <= frame < b for a, b in t.kept), (frame, t.kept)


# ---- the step of a kernel filter with a trace below it ----------------------------------------------------------------------

def test_kernel_filter_step_change_regrids_the_trace_below(oracle):
    """BufferedKernelFilter.update(step=...) changed its own rate, offset and bufferframes and left the trace below on the
    old grid: ValueError 'could not broadcast input array from shape (4000,) into shape (8000,)' from below.process."""
    x = np.random.default_rng(5).standard_normal((40*8000, 2)).astype(np.float32).astype(np.float64)
    g = TraceGraph(4.0, 1.0)
    g.add_trace(BufferedKernelFilter(source='data', kernel=np.ones(9)/9, step=4))
    g.add_trace(BufferedKernelFilter(name='below', source='features', kernel=np.ones(5)/5))
    g.setup_traces()
    g.open(x, 8000.0)
    for t in g.traces:
        t.plot_items = [fl.Item() for _ in range(t.channels)]
    g.set_need_update()
    ledger = fl.Ledger(g, oracle)
    feat, below = g['features'], g['below']
    for t0, t1 in [(10.0, 12.0), (11.0, 13.0)]:
        g.update_times(t0, t1)
        ledger.check()
    for step in (8, 3, 1, 4):
        feat.update(step=step)
        assert feat.step == step and feat.rate == 8000.0/step
        fl.assert_on_grid(feat)
        fl.assert_on_grid(below)
        assert below.rate == feat.rate and len(below.buffer) == len(feat.buffer) > 0
        ledger.check()
        g.update_times(11.5, 13.5)
        fl.assert_on_grid(below)
        ledger.check()
        g.update_times(11.0, 13.0)
        ledger.check()


def test_frame_arithmetic_is_exact_for_whole_steps():
    """Found by the walks: _load_geometry, align_buffer and _regrid went from a trace's frames to its source's through
    offset*src.rate/self.rate in floating point, which through a rate like 8000/3 is one frame off at some offsets
    (floor(21*8000/(8000/3)) is 62) -- a strip computed one source frame early, or a slab one frame longer than its
    strip ('could not broadcast input array from shape (934,) into shape (933,)')."""
    x = np.zeros((4*8000, 1))
    g = TraceGraph(4.0, 1.0)
    g.add_trace(BufferedKernelFilter(source='data', kernel=np.ones(3)/3, step=3))
    g.add_trace(BufferedKernelFilter(name='below', source='features', kernel=np.ones(3)/3, step=2))
    g.setup_traces()
    g.open(x, 8000.0)
    for t in g.traces:
        t.plot_items = [fl.Item() for _ in range(t.channels)]
    g.set_need_update()
    g.update_times(0.0, 2.0)
    feat, below = g['features'], g['below']
    assert (feat.offset, len(feat.buffer), below.offset, len(below.buffer)) == (0, 10666, 0, 5333)
    for t, step in ((feat, 3), (below, 2)):
        for off in range(0, len(t.buffer) - 5):
            assert t._load_geometry(off, 5) == (off*step, 5*step, 0), (t.name, off)
        for frames in range(0, 3*len(t.buffer)):
            assert (t._own_frames(frames), t._own_frames(frames, up=True)) == (frames//step, -(-frames//step))


def test_regrid_stays_importable_from_the_power_envelope():
    from audian_amd import buffereddata, bufferedpowerenvelope
    assert bufferedpowerenvelope._regrid is buffereddata._regrid
