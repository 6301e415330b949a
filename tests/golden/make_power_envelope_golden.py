"""Writes tests/golden/power_envelope.npz: test inputs and what the REFERENCE's envelope() (songdetector.py:57-69) and
lowpass_filter() (songdetector.py:49-54) give for them.  Runs only where the reference and scipy are at hand:

    python tests/golden/make_power_envelope_golden.py /path/to/reference/songdetector.py

The module cannot be imported (matplotlib, audioio and thunderlab are absent), so its source is parsed with `ast` and only
the functions `envelope` and `lowpass_filter` are compiled, with numpy as `np` and scipy.signal as `sig` in their
namespace.  Nothing of the reference's text is written anywhere: the npz holds inputs and recorded results.

Two cases, inputs float32 (frames, 3) from iir_bound.families(['stepdown', 'burst', 'offset']); the functions run on the
float64 copy of the float32 samples:

    a_   96 kHz, cut-off 500 Hz:  envrate 5 kHz, step 19
    b_   44.1 kHz, cut-off 6 kHz: 10 * 6 kHz > rate, envrate capped at the rate, step 1

Per case: x, rate, freq, step, envelope (the function's first result), envrate (its second) and slow =
lowpass_filter(envelope, envrate, 2.0), the detector's slow envelope at minduration 0.5 s."""

import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the package: audian_amd.design

import power_envelope_definition as pd                       # noqa: E402
import iir_bound as ib                                       # noqa: E402

CASES = (('a_', 96000.0, 500.0, 5003), ('b_', 44100.0, 6000.0, 1501))
NAMES = ['stepdown', 'burst', 'offset']
SLOW_CUTOFF = 2.0


def reference_functions(path):
    import scipy.signal as sig
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('envelope', 'lowpass_filter')]
    assert len(nodes) == 2
    namespace = {'np': np, 'sig': sig}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), namespace)
    return namespace['envelope'], namespace['lowpass_filter']


def main():
    envelope, lowpass_filter = reference_functions(sys.argv[1])
    out = {}
    for prefix, rate, freq, frames in CASES:
        x = ib.families(NAMES, frames, rate)
        env, envrate = envelope(x.astype(np.float64), rate, freq)
        slow = lowpass_filter(env, envrate, SLOW_CUTOFF)
        step = pd.reference_step(rate, freq)
        assert envrate == rate/step and env.shape == (pd.grid_size(frames, 0, step), len(NAMES))
        # the definition restates the function: 2 sqrt(f) against sqrt(2 f) sqrt(2), both in float64
        sos = pd.first_order_sos(freq, rate)
        f = pd.filtered_squares(sos, x, np.float64)[::step]
        own = 2.0*np.sqrt(np.maximum(f, 0.0))
        err = np.max(np.abs(own - env), axis=0)/np.max(np.abs(env), axis=0)
        slow_own = ib.sosfiltfilt(pd.first_order_sos(SLOW_CUTOFF, envrate), env, np.float64, gain=1.0, rectify=False,
                                  clamp=False)
        slow_err = np.max(np.abs(slow_own - slow), axis=0)/np.max(np.abs(slow), axis=0)
        print('%s %s at %g Hz, cut-off %g Hz: step %d, definition vs reference %.3g, slow envelope %.3g'
              % (prefix, x.shape, rate, freq, step, err.max(), slow_err.max()))
        assert err.max() <= 1e-12 and slow_err.max() <= 1e-12
        out.update({prefix + 'x': x, prefix + 'rate': rate, prefix + 'freq': freq, prefix + 'step': step,
                    prefix + 'envelope': env, prefix + 'envrate': envrate, prefix + 'slow': slow})
    out['slow_cutoff'] = SLOW_CUTOFF
    path = os.path.join(HERE, 'power_envelope.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 200000
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
