"""Writes tests/golden/region_filtfilt.npz: what scipy (1.15.3 when the file was made) returns for the zero-phase filters
of the event refinement.  Run it by hand when the file has to be made again:

    python tests/golden/make_refine_golden.py

Cases: the reference's lowpass_filter -- scipy.signal.filtfilt(*scipy.signal.butter(1, Wn), v) -- at 4 Hz and 400 Hz of
5 kHz and at 40 Hz of 96 kHz, and one two-section table (scipy.signal.butter(4, 300 Hz of 48 kHz, output='sos')), each at
lengths 7 (padlen + 1 of the one-section filters; 16 for the two sections, whose padlen is 15), 65 and 4099.  Layout:
sos (N, 2, 6) float64 -- the table of every case, one-section cases [b0 b1 0 1 a1 0] with an all-pass second row that is
not part of the filter; sections (N,) int64; offsets (N + 1,) int64 into x (float32 inputs, back to back) and into
y_sosfiltfilt (float64, scipy.signal.sosfiltfilt(sos, v)); y_filtfilt (float64, scipy.signal.filtfilt(b, a, v)) for
the one-section cases back to back, ff_offsets (N + 1,) int64 (empty ranges for the two-section cases)."""

import os

import numpy as np
import scipy
import scipy.signal


def signal(n, seed):
    rng = np.random.default_rng([2024, seed, n])
    t = np.arange(n)
    return (0.3 + 0.2*np.sin(2*np.pi*t/37.0) + 0.1*rng.standard_normal(n) + (t > n//2)*0.5).astype(np.float32)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    filters = [(1, 4.0, 5000.0), (1, 400.0, 5000.0), (1, 40.0, 96000.0), (4, 300.0, 48000.0)]
    sos_all, sections, xs, ys, ffs = [], [], [], [], []
    worst = 0.0
    for k, (order, cut, rate) in enumerate(filters):
        for length in (7 if order == 1 else 16, 65, 4099):
            v = signal(length, k)
            tab = np.zeros((2, 6))
            tab[:, 0] = tab[:, 3] = 1.0
            if order == 1:
                b, a = scipy.signal.butter(1, cut/(0.5*rate))
                tab[0] = b[0], b[1], 0.0, 1.0, a[1], 0.0
                S = 1
                ff = scipy.signal.filtfilt(b, a, v.astype(np.float64))
            else:
                tab[:] = scipy.signal.butter(order, cut, 'lowpass', fs=rate, output='sos')
                S = 2
                ff = np.zeros(0)
            y = scipy.signal.sosfiltfilt(tab[:S], v.astype(np.float64))
            if order == 1:
                worst = max(worst, float(np.max(np.abs(y - ff))))
            sos_all.append(tab)
            sections.append(S)
            xs.append(v)
            ys.append(y)
            ffs.append(ff)
    out = os.path.join(here, 'region_filtfilt.npz')
    np.savez_compressed(out, sos=np.array(sos_all), sections=np.array(sections, dtype=np.int64),
                        offsets=np.cumsum([0] + [len(v) for v in xs]), x=np.concatenate(xs),
                        y_sosfiltfilt=np.concatenate(ys), y_filtfilt=np.concatenate(ffs),
                        ff_offsets=np.cumsum([0] + [len(v) for v in ffs]))
    print('%s: %d cases, largest |sosfiltfilt - filtfilt| %.3g, scipy %s, %d bytes'
          % (out, len(xs), worst, scipy.__version__, os.path.getsize(out)))


if __name__ == '__main__':
    main()
