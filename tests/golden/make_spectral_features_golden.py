"""Writes tests/golden/spectral_features.npz: the spectral contour features of a small seeded slab as numpy computes
them in float64 with its library functions -- np.argmax, np.sum, np.log, np.exp, np.sqrt, np.flatnonzero -- the pin of
tests/spectral_features_definition.py.  numpy only.  Run it by hand when the file has to be made again:

    python tests/golden/make_spectral_features_golden.py

The interpolated peak (bit 1) has no library form to pin against: it is written out here once more, from np.log of
the three bins, and agrees with the definitions file only in so far as two statements of the same formula agree.

Layout: spec (2, 24, 97) float32 (spectral_features_definition.family_slab when the file was made: every input family,
NaN and +inf included); bands (B, 2) int64; scale, min_power, ratio; values (B, 8, 2, 24) float64 in bit order, NaN where
the definition masks."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spectral_features_definition as sd  # noqa: E402

BANDS = [(0, 97), (10, 75), (40, 41), (91, 97), (30, 30), (1, 64)]
SCALE, MIN_POWER, RATIO = 31.25, 1e-30, 0.1


def features(P, k0, k1):
    out = np.full(8, np.nan)
    band = P[k0:k1].astype(np.float64)
    if len(band) == 0:
        return out
    j = int(np.argmax(band))
    kp, peak = j + k0, band[j]
    out[2] = peak
    if not (np.isfinite(peak) and peak > MIN_POWER):
        return out
    k = np.arange(k0, k1, dtype=np.float64)
    S = np.sum(band)
    m = np.sum((k - kp)*band)/S
    var = np.sum((k - kp)**2*band)/S - m*m
    hit = np.flatnonzero(band >= RATIO*peak)
    d = 0.0
    if 0 < j < len(band) - 1 and band[j - 1] > 0 and band[j + 1] > 0:
        a, b, c = np.log(band[j - 1]), np.log(peak), np.log(band[j + 1])
        if a - 2*b + c < 0:
            d = 0.5*(a - c)/(a - 2*b + c)
    with np.errstate(divide='ignore'):
        flat = np.exp(np.sum(np.log(band))/len(band))/(S/len(band))
    out[[0, 1, 3, 4, 5, 6, 7]] = [SCALE*kp, SCALE*(kp + d), SCALE*(kp + m), SCALE*np.sqrt(max(var, 0.0)), flat,
                                  SCALE*(hit[0] + k0), SCALE*(hit[-1] + k0)]
    return out


def main():
    spec = sd.family_slab(97, 24, 2, 10, 75, 1)
    values = np.array([[[[features(spec[c, t], k0, k1)[bit] for t in range(spec.shape[1])] for c in range(spec.shape[0])]
                        for bit in range(8)] for k0, k1 in BANDS])
    out = os.path.join(HERE, 'spectral_features.npz')
    np.savez_compressed(out, spec=spec, bands=np.array(BANDS, dtype=np.int64), scale=SCALE, min_power=MIN_POWER,
                        ratio=RATIO, values=values)
    print('%s: %d bands, %d values, %d of them NaN, numpy %s, %d bytes'
          % (out, len(BANDS), values.size, int(np.isnan(values).sum()), np.__version__, os.path.getsize(out)))


if __name__ == '__main__':
    main()
