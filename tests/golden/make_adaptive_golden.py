"""Writes tests/golden/adaptive_spectrogram.npz: the adaptive spectrogram of a small slab by scipy.signal.lfilter and
numpy float64, which pins tests/adaptive_spectrogram_definition.py to the smoother librosa's pcen uses.
    python tests/golden/make_adaptive_golden.py
2 channels x 300 frames x 9 bins, all four modes in float64 -- of every third frame and the last six (`rows`; the
recursion has run through all frames in front of them), which keeps the file under 100 kB."""
import os

import numpy as np
from scipy.signal import lfilter, lfilter_zi

HERE = os.path.dirname(os.path.abspath(__file__))
C, FRAMES, F = 2, 300, 9
SMOOTH, GAIN, BIAS, POWER, EPS = 0.05193, 0.98, 2.0, 0.5, 1e-20
ROWS = np.unique(np.concatenate((np.arange(0, FRAMES, 3), np.arange(FRAMES - 6, FRAMES))))

rng = np.random.default_rng(20261021)
spec = (np.power(10.0, rng.uniform(-9.0, -3.0, (C, 1, F)))*rng.chisquare(2, (C, FRAMES, F))).astype(np.float32)
spec[:, 120:150] *= np.float32(300.0)                 # a passing car
spec[:, FRAMES - 3:] = 0.0                            # the spectrogram's zero tail
x = spec.astype(np.float64)
b, a = [SMOOTH], [1.0, SMOOTH - 1.0]
zi = lfilter_zi(b, a)
M = np.empty_like(x)
for c in range(C):
    for k in range(F):
        M[c, :, k] = lfilter(b, a, x[c, :, k], zi=zi*x[c, 0, k])[0]
xs, Ms = x[:, ROWS], M[:, ROWS]
out = {'spec': spec, 'smooth': SMOOTH, 'gain': GAIN, 'bias': BIAS, 'power': POWER, 'eps': EPS, 'rows': ROWS.astype(np.int32),
       'background': Ms, 'divide': xs/(EPS + Ms), 'subtract': np.maximum(xs - Ms, 0.0),
       'pcen': (xs/(EPS + Ms)**GAIN + BIAS)**POWER - BIAS**POWER}
np.savez_compressed(os.path.join(HERE, 'adaptive_spectrogram.npz'), **out)
