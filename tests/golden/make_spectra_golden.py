"""Writes tests/golden/region_spectra.npz: what scipy.signal.welch (scipy 1.15.3 when the file was made) returns for
regions of spectra_definition.golden_signal, and the main peak of every such spectrum with and without a prominence
threshold, the candidates being scipy.signal.find_peaks(10 log10(row), prominence=thresh).  Run it by hand when the file
has to be made again:

    python tests/golden/make_spectra_golden.py

Cases: nfft 8, 16, 256, 1024; hop nfft/2, nfft, 3; step 1, 2, 7; nfft - 1, nfft, nfft + hop - 1 and nfft + hop decimated
samples, the region starting at 0, 1, 2, 3 or 5.  Layout: cases (N, 6) int64 -- nfft, hop, step, start, stop, n_frames;
fs (N,) float64; rows / row_offsets -- the float64 spectra of the cases with a frame back to back (none for n_frames
0); peak_plain, peak_thresh (N,) float64 -- the peak frequency in Hz without a threshold and with THRESH dB (NaN: no
spectrum or no such peak); thresh -- THRESH."""

import os
import sys

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spectra_definition as sd  # noqa: E402

THRESH = 10.0
STARTS = [0, 1, 2, 3, 5]


def main():
    x = sd.golden_signal(5 + 7*(1024 + 1024))
    cases, fss, rows, plain, above = [], [], [], [], []
    nearest = np.inf
    k = 0
    for nfft in (8, 16, 256, 1024):
        for hop in (nfft//2, nfft, 3):
            for step in (1, 2, 7):
                for length in (nfft - 1, nfft, nfft + hop - 1, nfft + hop):
                    start = STARTS[k % len(STARTS)]
                    stop = start + (length - 1)*step + 1 + (k % step)       # any stop that gives `length` samples
                    k += 1
                    fs = 1000.0/step
                    v = x[start:stop:step].astype(np.float64)
                    assert len(v) == length
                    n = sd.count_frames(length, nfft, hop)
                    cases.append([nfft, hop, step, start, stop, n])
                    fss.append(fs)
                    if n == 0:
                        plain.append(np.nan)
                        above.append(np.nan)
                        continue
                    f, row = scipy.signal.welch(v, fs, 'hann', nperseg=nfft, noverlap=nfft - hop, detrend='constant',
                                                scaling='density')
                    assert len(row) == nfft//2 + 1 and f[1] == fs/nfft
                    rows.append(row)
                    plain.append(f[np.argmax(row)])
                    db = 10.0*np.log10(row)
                    p, props = scipy.signal.find_peaks(db, prominence=0.0)
                    if len(p):
                        nearest = min(nearest, np.min(np.abs(props['prominences'] - THRESH)))
                    p = p[props['prominences'] >= THRESH]
                    above.append(f[p[np.argmax(row[p])]] if len(p) else np.nan)
    assert nearest > 1e-3, nearest                 # no prominence that float32 rounding of the dB could move across
    out = os.path.join(HERE, 'region_spectra.npz')
    np.savez_compressed(out, cases=np.array(cases, dtype=np.int64), fs=np.array(fss), rows=np.concatenate(rows),
                        row_offsets=np.cumsum([0] + [len(r) for r in rows]), peak_plain=np.array(plain),
                        peak_thresh=np.array(above), thresh=np.array(THRESH))
    print('%s: %d cases, %d with a spectrum, %d with a peak above %g dB, nearest prominence %.3g dB off, scipy %s, %d bytes'
          % (out, len(cases), len(rows), int(np.isfinite(above).sum()), THRESH, nearest, scipy.__version__,
             os.path.getsize(out)))


if __name__ == '__main__':
    main()
