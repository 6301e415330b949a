"""Every derived trace in one graph, walked at random on the GPU under the ledger of tests/facade_ledger.py:

    data -> rereferenced -> filtered -> envelope       -> features (kernel, step s) -> below (kernel filter or low-pass)
                                                       -> eventfiltered
                                     -> spectrogram    -> bandpower, peakfreq, match
                                     -> power-envelope -> slow-envelope

Every load of every trace is shadowed by its definition on the source slab as the device held it, and after every action
every frame of every buffer must have been computed by some call and agree with it (facade_ledger.py has the rules).  What
is under test is the BufferedData state machine -- _stale, _dev_valid, _carry, _adopt_buffer, _fused_token, _raw_cache, the
geometry overrides -- not the kernels, which their own tests hold to tighter bounds.

(The filtered trace's source is the rereferenced trace here, so its pass-through never becomes a view of the loader's slab:
_alias_mirror stays with tests/test_gpu_facade.py.)"""

import numpy as np
import pytest

import facade_ledger as fl
import gpu_helpers as gh

pytestmark = pytest.mark.gpu

REACHED = fl.new_reached()
NAMES = ('rereferenced', 'filtered', 'envelope', 'features', 'below', 'eventfiltered', 'spectrogram', 'bandpower', 'peakfreq',
         'match', 'power-envelope', 'slow-envelope')
# what the nine newer classes launch (and the three older ones, alone or fused)
ENTRY_POINTS = ('common_reference', 'fir_bank', 'region_filtfilt', 'band_power', 'spectral_features', 'template_match',
                'power_envelope', 'envelope', 'sosfilt', 'spectrogram')


def device_db(power, floor):
    """v of the template match's definition: hipdsp_decibel on the same powers (ref_power 1, min_power 0), clamped on the
    host -- as tests/test_gpu_template_match.py obtains them."""
    from audian_amd import hipdsp
    c = gh.ctx()
    power = np.ascontiguousarray(power, dtype=np.float32)
    d = hipdsp.DeviceArray.from_host(c, power)
    o = hipdsp.DeviceArray(c, power.shape, np.float32)
    hipdsp.decibel(c, d, o, power.size, 1.0, 0.0)
    v = o.to_host()
    d.free()
    o.free()
    return np.where(v < np.float32(floor), np.float32(floor), v)


def walk(oracle, seed, poison):
    from audian_amd import hipdsp
    before = dict(hipdsp.launches)
    w = fl.walk(fl.device_classes(), oracle, seed, poison, REACHED, db=device_db, launches=lambda: hipdsp.launches)
    for k, v in hipdsp.launches.items():
        REACHED['launches'][k] = REACHED['launches'].get(k, 0) + v - before.get(k, 0)
    # no silent host fallback: every buffer lives on its mirror (a match without a fitting template is NaN on the host)
    for t in w.ledger.traces:
        if t.name != 'match' or (t.template is not None and not t.stale):
            assert t._mirror_valid(0, len(t._hostbuf)), t.name
    return w


@pytest.mark.parametrize('seed', range(6))
def test_walks(oracle, seed):
    """A short fixed prologue, then 14 seeded actions -- scrolls towards the end and jumps back, cut-offs, envelope
    parameters, spectrogram resolution (the template goes stale and is cut again), bands, features, kernels, thresholds,
    steps, reference method and groups, templates, events at the buffer's borders, partial reads -- with the ledger's check
    after each."""
    walk(oracle, seed, poison=False)


@pytest.mark.parametrize('seed', range(100, 103))
def test_walks_with_non_finite_samples(oracle, seed):
    """The same over recordings that hold a few NaN / infinite samples: non-finite exactly where the definition on the
    slab has it, for every trace."""
    walk(oracle, seed, poison=True)


def test_zz_the_walks_reached():
    """Counted over all seeds above: the states the walks are there for."""
    r = REACHED
    assert r['walks'] == 9
    assert all(r['partial'].get(n, 0) >= 3 for n in NAMES), r['partial']
    assert all(r['own'].get(n, 0) >= 1 for n in NAMES), r['own']
    assert all(r['source'].get(n, 0) >= 1 for n in NAMES[1:]), r['source']           # (the loader has no update)
    assert r['fused'] >= 1 and (r['launches'].get('chain_forward', 0) or any(k.startswith('sosfilt_envelope') and v
                                                                          for k, v in r['launches'].items()))
    assert r['carry'] >= 1                               # a move made while _stale was non-empty on a valid mirror
    assert r['refitted'] >= 1
    assert r['features step'] >= 1 and r['power-envelope step'] >= 1
    assert all(r['launches'].get(k, 0) > 0 for k in ENTRY_POINTS), r['launches']
    assert r['near'][1] > 1000 and r['near'][0] <= fl.NEAR_CAP*r['near'][1]
