"""The work one session costs, step by step: one TraceGraph that holds one of every built-in trace is driven through a
fixed script, and after every step the kernel launches, the Context.synchronize calls, the device allocations and every
trace's mirror bookkeeping (_stale, _dev_valid) must be exactly what they were before the process() skeletons were
merged into BufferedData's helpers.  EXPECTED and tests/golden/facade_work.npz were recorded by running this same
script at the commit before that refactoring; they are not derived from the code under test."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE, CHANNELS, SECONDS, SEED = 8000.0, 2, 40, 20240607
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'facade_work.npz')
EVERY = 16                     # the golden file keeps every 16th frame of a buffer (and the spectrogram's ends)


class Item:
    def isVisible(self):
        return True


def build_graph():
    from audian_amd.bufferedbandpower import BufferedBandPower
    from audian_amd.bufferedcommonreference import BufferedCommonReference
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedeventfilter import BufferedEventFilter
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedkernelfilter import BufferedKernelFilter
    from audian_amd.bufferedlowpass import BufferedLowpass
    from audian_amd.bufferedpowerenvelope import BufferedPowerEnvelope
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.events import Events
    from audian_amd.tracegraph import TraceGraph
    x = np.random.default_rng(SEED).standard_normal((int(SECONDS*RATE), CHANNELS))
    g = TraceGraph(buffer_time=4.0, back_time=1.0)
    g.add_trace(BufferedCommonReference(name='rereferenced', source='data'))
    g.add_trace(BufferedFilter(name='filtered', source='rereferenced'))
    g.add_trace(BufferedEnvelope(name='envelope', source='filtered'))
    g.add_trace(BufferedKernelFilter(name='features', source='envelope', kernel=np.ones(9)/9.0))
    g.add_trace(BufferedEventFilter(name='eventfiltered', source='envelope'))
    g.add_trace(BufferedSpectrogram(name='spectrogram', source='filtered', nfft=256, overlap_frac=0.5))
    g.add_trace(BufferedBandPower(name='bandpower', source='spectrogram', fmin=1000.0, fmax=3000.0))
    g.add_trace(BufferedPowerEnvelope(name='power-envelope', source='filtered'))
    g.add_trace(BufferedLowpass(name='slow-envelope', source='power-envelope'))
    g.setup_traces()
    g.open(x, RATE)
    # two events, in frames of the envelope: one inside the first windows, one inside the last (nothing is visible
    # yet, so this computes nothing)
    events = Events([[(16000, 20000)], [(160000, 164000)]], RATE, 'envelope')
    g['eventfiltered'].set_events(events, [np.array([20.0]), np.array([30.0])], 0.05)
    for tr in g.traces:
        tr.plot_items = [Item() for _ in range(tr.channels)]
    g.set_need_update()
    return g


def run_script(monkeypatch):
    """(records, values): one record of the work per step, and what is compared with the golden file."""
    from audian_amd import buffereddata, hipdsp
    monkeypatch.setenv('AUDIAN_AMD_WRITE_PROBE', '1')
    monkeypatch.setattr(buffereddata, 'WRITE_PROBE', 1)
    syncs = [0]
    synchronize = hipdsp.Context.synchronize

    def counted(self):
        syncs[0] += 1
        return synchronize(self)

    monkeypatch.setattr(hipdsp.Context, 'synchronize', counted)
    ctx = hipdsp.default_context()
    g = build_graph()
    derived = g.traces[1:]
    records = []
    last = {}

    def mark():
        cached, hits, misses = ctx.pool_stats()
        last.update(launches=dict(hipdsp.launches), syncs=syncs[0], allocs=hits + misses)

    def record(step):
        before = dict(last)
        mark()
        delta = {k: v - before['launches'].get(k, 0) for k, v in last['launches'].items()}
        records.append({'step': step,
                        'launches': {k: v for k, v in sorted(delta.items()) if v},
                        'syncs': last['syncs'] - before['syncs'],
                        'allocs': last['allocs'] - before['allocs'],
                        'traces': {t.name: ([list(map(int, r)) for r in t._stale],
                                            [list(map(int, r)) for r in t._dev_valid]) for t in derived}})

    mark()
    g.update_times(0.0, 2.0)
    record('window 0-2')
    g.update_times(3.0, 5.0)
    record('window 3-5')
    g.update_times(30.0, 32.0)
    record('window 30-32')
    filt = g['filtered']
    filt.highpass_cutoff, filt.lowpass_cutoff = 500.0, 3000.0
    filt.update()
    record('filter cut-offs')
    g['envelope'].envelope_cutoff = 200.0
    g['envelope'].update()
    record('envelope cut-off')
    g['bandpower'].set_band(500.0, 2000.0)
    record('set_band')
    g['features'].set_kernel(np.hanning(35)[1:-1]/np.sum(np.hanning(35)))
    record('set_kernel')
    g['slow-envelope'].update(cutoff=5.0)
    record('low-pass cut-off')
    step = g['power-envelope'].step
    g['power-envelope'].update(envelope_cutoff=100.0)
    assert g['power-envelope'].step != step
    record('power-envelope cut-off')
    g['rereferenced'].update(method='median')
    record('common-reference method')
    env = g['envelope']
    a, b = env.offset, env.offset + len(env._hostbuf)
    events = env.detect_events(0.5, 0.001, 0.001)
    record('detect_events')
    hist = env.histogram(np.linspace(0.0, 4.0, 33))
    record('histogram')
    stats = env.region_stats([(a, a + (b - a)//2), (a + (b - a)//3, b)])
    record('region_stats')
    values = {'events0': events.frames(0), 'events1': events.frames(1), 'histogram': hist, 'region_stats': stats}
    for t in derived:
        buf = np.asarray(t.buffer)
        values[t.name] = buf[::EVERY]
        values[t.name + ' offset'] = np.array([t.offset, len(buf)])
        if t.name == 'spectrogram':
            values['spectrogram first'], values['spectrogram last'] = buf[:8], buf[-8:]
    record('read back')
    # beyond the script the golden values were taken after: a scroll back that keeps an overlap on every trace
    g.update_times(12.0, 14.0)
    record('window 12-14')
    return records, values


def _whole(frames):
    """Every trace computed over its whole buffer on the device, nothing read back yet."""
    return {name: ([[0, n]], [[0, n]]) for name, n in frames.items()}


# frames in every trace's buffer: at the start of the recording, after the jump to 30 s, after the power envelope's step
# went from 2 to 8
_START = {'rereferenced': 208000, 'filtered': 208000, 'envelope': 208000, 'features': 208000, 'eventfiltered': 208000,
          'spectrogram': 1000, 'bandpower': 1000, 'power-envelope': 104000, 'slow-envelope': 104000}
_LATE = {'rereferenced': 208000, 'filtered': 128000, 'envelope': 120000, 'features': 120000, 'eventfiltered': 120000,
         'spectrogram': 374, 'bandpower': 374, 'power-envelope': 60000, 'slow-envelope': 56000}
_STEP8 = dict(_LATE, **{'power-envelope': 15000, 'slow-envelope': 14000})
_SCROLL = {'band_power': 1, 'common_reference': 1, 'envelope': 2, 'fir_bank': 1, 'power_envelope': 1,
           'region_filtfilt': 1, 'sosfilt': 1, 'spectrogram': 1}
_FUSED = {'band_power': 1, 'chain_forward': 1, 'envelope': 1, 'fir_bank': 1, 'power_envelope': 1, 'region_filtfilt': 1,
          'sosfilt_envelope:2': 1}


def _step(step, launches, syncs, allocs, traces):
    return {'step': step, 'launches': launches, 'syncs': syncs, 'allocs': allocs, 'traces': traces}


# recorded on an MI355X at the commit before the refactoring
EXPECTED = [
    _step('window 0-2', _SCROLL, 1, 11, _whole(_START)),
    _step('window 3-5', {}, 0, 0, _whole(_START)),
    _step('window 30-32', _SCROLL, 10, 11, _whole(_LATE)),
    _step('filter cut-offs', _FUSED, 0, 0, _whole(_LATE)),
    _step('envelope cut-off', {'envelope': 1, 'fir_bank': 1, 'region_filtfilt': 1}, 0, 0, _whole(_LATE)),
    _step('set_band', {'band_power': 1}, 0, 0, _whole(_LATE)),
    _step('set_kernel', {'fir_bank': 1}, 0, 0, _whole(_LATE)),
    _step('low-pass cut-off', {'envelope': 1}, 0, 0, _whole(_LATE)),
    _step('power-envelope cut-off', {'envelope': 1, 'power_envelope': 1}, 0, 2, _whole(_STEP8)),
    _step('common-reference method', dict(_FUSED, common_reference=1), 1, 2, _whole(_STEP8)),
    _step('detect_events', {'detect_events': 1}, 0, 2, _whole(_STEP8)),
    _step('histogram', {'histogram': 1}, 0, 1, _whole(_STEP8)),
    _step('region_stats', {'region_stats': 1}, 0, 1, _whole(_STEP8)),
    _step('read back', {}, 0, 9, {name: ([], [[0, n]]) for name, n in _STEP8.items()}),
    _step('window 12-14', _SCROLL, 10, 11,
          {'rereferenced': ([[0, 40000]], [[0, 208000]]), 'filtered': ([[0, 120000]], [[0, 208000]]),
           'envelope': ([[0, 128000]], [[0, 208000]]), 'features': ([[0, 128000]], [[0, 208000]]),
           'eventfiltered': ([[0, 208000]], [[0, 208000]]), 'spectrogram': ([[0, 938]], [[0, 1000]]),
           'bandpower': ([[0, 938]], [[0, 1000]]), 'power-envelope': ([[0, 16000]], [[0, 26000]]),
           'slow-envelope': ([[0, 17000]], [[0, 26000]])}),
]


def test_same_work_and_same_values_as_before_the_refactoring(monkeypatch):
    records, values = run_script(monkeypatch)
    assert [r['step'] for r in records] == [e['step'] for e in EXPECTED]
    for got, want in zip(records, EXPECTED):
        assert got == want, got['step']
    golden = np.load(GOLDEN)
    assert sorted(golden.files) == sorted(values)
    for name in golden.files:
        # (the golden file holds the buffers as float32: every value of a mirror is one, nothing was rounded)
        assert np.array_equal(np.asarray(values[name], dtype=np.float64), golden[name].astype(np.float64),
                              equal_nan=True), name
