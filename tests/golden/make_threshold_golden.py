"""Writes tests/golden/threshold_estimates.npz: test inputs and the thresholds the REFERENCE's threshold_estimates
(songdetector.py:85-117) gives for them.  Runs only where the reference is at hand:

    python tests/golden/make_threshold_golden.py /path/to/reference/songdetector.py

The module cannot be imported (matplotlib, audioio and thunderlab are absent), so its source is parsed with `ast` and
only the function `threshold_estimates` is compiled, with numpy in its namespace.  Nothing of the reference's text is
written anywhere: the npz holds inputs, recorded thresholds and the margins below.

Inputs, float32: |N(0, 0.01)| + 0.02 per sample; even channels c add 3 + c Hann bursts of amplitude 0.3 + 0.1 c and
length n/100 ... n/20.  One 5000 x 4 case is stored; the multi-chunk case is that case tiled (threshold_definition.tiled)
so that the tests need no random stream.  The function runs on the float64 copy of the float32 samples.

Margins, asserted here and stored: no sample within 1e-7 relative of mean + 3 std, |uppermean - (mean + 6 std)| at
least 1e-2 relative, both branches of the final rule taken.  Without them a last-bit difference in a mean could flip a
sample or the branch and no tolerance would mean anything."""

import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import threshold_definition as td                            # noqa: E402

FRAMES, CHANNELS = 5000, 4
TILED_TIMES, TILED_FRAMES = 9, 40961                         # three chunks of 16384, the last one partial, odd length


def reference_function(path):
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'threshold_estimates']
    assert len(nodes) == 1
    namespace = {'np': np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), namespace)
    return namespace['threshold_estimates']


def make_input(rng, n, channels):
    x = np.abs(rng.normal(0.0, 0.01, size=(n, channels))) + 0.02
    for c in range(0, channels, 2):
        for _ in range(3 + c):
            length = int(rng.integers(n//100, n//20 + 1))
            at = int(rng.integers(0, n - length))
            x[at:at + length, c] += (0.3 + 0.1*c)*np.hanning(length)
    return x.astype(np.float32)


def margins(x):
    """(smallest relative gap of a sample to mean + 3 std, smallest relative branch margin, branch per channel)."""
    thresholds, details = td.threshold_estimates(x)
    gap, margin, upper_branch = np.inf, np.inf, []
    for c, (maxi, mean, std, uppermean) in enumerate(details):
        cut = mean + 3.0*std
        gap = min(gap, np.min(np.abs(x[:, c].astype(np.float64) - cut))/cut)
        assert np.isfinite(uppermean)
        margin = min(margin, abs(uppermean - (mean + 6.0*std))/(mean + 6.0*std))
        upper_branch.append(bool(uppermean > mean + 6.0*std))
    return gap, margin, upper_branch, thresholds


def main():
    ref = reference_function(sys.argv[1])
    x = make_input(np.random.default_rng(20260117), FRAMES, CHANNELS)
    xt = td.tiled(x, TILED_TIMES, TILED_FRAMES)
    out = {'x': x, 'tiled_times': TILED_TIMES, 'tiled_frames': TILED_FRAMES}
    for name, data in (('', x), ('tiled_', xt)):
        want = np.array(ref(data.astype(np.float64)), dtype=np.float64)
        gap, margin, upper_branch, own = margins(data)
        print('%scase %s: gap %.3g  branch margin %.3g  branches %s  decomposition vs reference %.3g'
              % (name, data.shape, gap, margin, upper_branch, np.max(np.abs(own - want)/np.abs(want))))
        assert gap >= 1e-7 and margin >= 1e-2
        assert any(upper_branch) and not all(upper_branch)
        assert np.allclose(own, want, rtol=1e-13, atol=0)
        out[name + 'thresholds'] = want
        out[name + 'gap'] = gap
        out[name + 'branch_margin'] = margin
        out[name + 'upper_branch'] = np.array(upper_branch)
    path = os.path.join(HERE, 'threshold_estimates.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 200000
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
