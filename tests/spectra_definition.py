"""The definition of hipdsp_region_spectra (include/hip_dsp.h) and of the peak rule of audian_amd/spectra.py, written
from their sentences as plain sequential numpy float64 and sharing nothing with the code under test: the comparator of
tests/test_spectra_host.py and tests/test_gpu_regionspectra.py.  tests/golden/region_spectra.npz pins it to
scipy.signal.welch and scipy.signal.find_peaks (scipy 1.15.3).  thunderlab, whose peak_freqs the reference's
songdetector.py calls (songdetector.py:151), is neither in the reference tree nor installed: its peak detector is
restated here as the project's own find_peaks with a prominence, parity with thunderlab is unpinned."""

import numpy as np

import peaks_definition


def count_frames(length, nfft, hop):
    return (length - nfft)//hop + 1 if length >= nfft else 0


def region_frames(x, start, stop, nfft, hop, step):
    """(n_frames, nfft) float64: frame k is v[k*hop : k*hop + nfft] of v = x[start:stop:step]."""
    v = np.asarray(x[start:stop:step], dtype=np.float64)
    n = count_frames(len(v), nfft, hop)
    out = np.zeros((n, nfft))
    for k in range(n):
        out[k] = v[k*hop:k*hop + nfft]
    return out


def frame_psd(frame, fs):
    """One frame's one-sided PSD: mean removed, periodic Hann, |rfft|^2 / (fs sum w^2), bins 1 ... F-2 doubled."""
    nfft = len(frame)
    w = 0.5 - 0.5*np.cos(2.0*np.pi*np.arange(nfft)/nfft)
    X = np.fft.rfft((frame - np.mean(frame))*w)
    P = (X.real**2 + X.imag**2)/(fs*np.sum(w*w))
    P[1:-1] *= 2.0
    return P


def frame_psds(frames, fs):
    """(n_frames, F) float64 of frame_psd; the rows of a frame with a non-finite sample are NaN."""
    nfft = frames.shape[1]
    out = np.zeros((len(frames), nfft//2 + 1))
    with np.errstate(all='ignore'):
        for k, frame in enumerate(frames):
            out[k] = frame_psd(frame, fs) if np.isfinite(frame).all() else np.nan
    return out


def region_spectrum(x, start, stop, nfft, hop, step, fs):
    """(row (F,) float64, n_frames, argmax) of one region of the row x."""
    frames = region_frames(x, start, stop, nfft, hop, step)
    F = nfft//2 + 1
    if len(frames) == 0:
        return np.full(F, np.nan), 0, -1
    if not np.isfinite(frames).all():
        return np.full(F, np.nan), len(frames), 0
    row = np.mean(frame_psds(frames, fs), axis=0)
    return row, len(frames), int(np.argmax(row))


def pick_peak(row, thresh=None, fs=1.0):
    """The main peak of a spectrum row of nfft/2 + 1 bins in Hz: NaN for a NaN row; argmax(row)*fs/nfft without
    `thresh`; else the bin of largest power among find_peaks(10 log10(row), prominence=thresh), NaN when there is
    none.  -inf dB only where the power is exactly 0."""
    row = np.asarray(row)
    nfft = 2*(len(row) - 1)
    if np.isnan(row).any():
        return np.nan
    if thresh is None:
        return int(np.argmax(row))*fs/nfft
    with np.errstate(divide='ignore'):
        db = 10.0*np.log10(row.astype(np.float64))
    positions, _ = peaks_definition.find_peaks(db, prominence=(float(thresh), np.inf))
    if not positions:
        return np.nan
    best = positions[0]
    for p in positions[1:]:
        if row[p] > row[best]:
            best = p
    return best*fs/nfft


def golden_signal(n):
    """The row behind tests/golden/region_spectra.npz: n float32 samples made with integer arithmetic only (so that the
    file need not store them): pseudo-random integers in [-510, 510], a triangle wave of period 12 and 200 times that
    height, a slower one of period 50, all over 512, plus an offset of 3."""
    i = np.arange(n, dtype=np.int64)
    noise = (i*i*7 + i*13 + (i//3)*(i % 11)*5) % 1021 - 510
    fast = np.abs(i % 12 - 6) - 3
    slow = np.abs(i % 50 - 25) - 12
    return ((noise + 200*fast + 40*slow)/512.0 + 3.0).astype(np.float32)
