"""Event spectra: the Welch power spectral density of every detected event and its main peak -- the step that follows
event detection in the reference's ``songdetector.py`` (``env_freqs``, songdetector.py:146-152, called at :761: the power
spectrum of the envelope inside every song and its peak above 10 dB prominence, the pulse rate; on the filtered trace
the same gives the carrier frequency of every call).  thunderlab, whose ``psd`` and ``peak_freqs`` songdetector.py
calls, is neither installed nor part of the reference tree: its choice of nfft (``welch_nfft``, ``event_nfft``) and its
peak detector (``pick_peak``: the project's own find_peaks with a prominence) are restated, parity with thunderlab is
unpinned.  The contract of the spectra is the definition in ``include/hip_dsp.h`` (hipdsp_region_spectra), which is
``scipy.signal.welch(v, fs, 'hann', nperseg=nfft, noverlap=nfft - hop, detrend='constant', scaling='density')``.

``host_region_spectrum`` is that definition in numpy on one row (the fallback of ``BufferedArray.region_spectra``);
``Spectra`` is what ``region_spectra`` returns.
"""

import numpy as np

MIN_NFFT, MAX_NFFT = 8, 8192            # what hipdsp_region_spectra transforms


def welch_nfft(rate, freq_resolution, min_nfft=16, max_nfft=8192):
    """The smallest power of two >= rate/freq_resolution, clamped to [min_nfft, max_nfft]."""
    want = float(rate)/float(freq_resolution)
    nfft = 1
    while nfft < want and nfft < max_nfft:
        nfft *= 2
    return int(min(max(nfft, min_nfft), max_nfft))


def event_nfft(length, nfft, min_nfft=16):
    """The nfft of one event of `length` decimated samples: min(nfft, the largest power of two <= length) -- thunderlab's
    use of max_nfft = i1 - i0, restated -- or 0 for an event shorter than min_nfft (no spectrum: NaN)."""
    length = int(length)
    if length < min_nfft or length < MIN_NFFT:
        return 0
    return int(min(nfft, 1 << (length.bit_length() - 1)))


def host_region_spectrum(row, nfft, hop, fs):
    """(power (F,) float64, n_frames, argmax) of one decimated row v: the mean over the frames v[k*hop : k*hop + nfft] of
    the one-sided PSD of the mean-free, Hann-windowed frame; NaN and -1 without a whole frame, NaN and 0 with a
    non-finite sample in a used frame."""
    v = np.asarray(row, dtype=np.float64).reshape(-1)
    F = nfft//2 + 1
    n = (len(v) - nfft)//hop + 1 if len(v) >= nfft else 0
    if n == 0:
        return np.full(F, np.nan), 0, -1
    frames = np.lib.stride_tricks.as_strided(v, (n, nfft), (hop*v.strides[0], v.strides[0]))
    if not np.isfinite(frames).all():
        return np.full(F, np.nan), n, 0
    w = 0.5 - 0.5*np.cos(2.0*np.pi*np.arange(nfft)/nfft)
    power = np.zeros(F)
    for k in range(0, n, 256):
        block = frames[k:k + 256]
        X = np.fft.rfft((block - block.mean(axis=1, keepdims=True))*w, axis=1)
        power += np.sum(X.real**2 + X.imag**2, axis=0)
    power /= n*fs*np.sum(w*w)
    power[1:-1] *= 2.0
    return power, n, int(np.argmax(power))


def pick_peak(row, thresh=None, fs=1.0):
    """The main peak of a spectrum row (nfft/2 + 1 powers) in Hz.  NaN for a NaN row.  Without `thresh`:
    argmax(row)*fs/nfft.  With it: the candidates are find_peaks(10 log10(row), prominence=thresh) (peaks.py; -inf dB
    only where the power is exactly 0), the result is the candidate of largest power, NaN when there is none -- how
    songdetector.py:151 uses thunderlab's peak_freqs with thresh=10 dB."""
    from .peaks import host_find_peaks
    row = np.asarray(row)
    nfft = 2*(len(row) - 1)
    if np.isnan(row).any():
        return np.nan
    if thresh is None:
        return int(np.argmax(row))*float(fs)/nfft
    with np.errstate(divide='ignore'):
        db = 10.0*np.log10(row.astype(np.float64))
    positions, _ = host_find_peaks(db, prominence=(float(thresh), None))
    if len(positions) == 0:
        return np.nan
    return int(positions[np.argmax(row[positions])])*float(fs)/nfft


class Spectra(object):
    """The spectra of a list of regions: ``regions`` (R, 3) int64 of channel, start, stop (absolute frames of the trace),
    ``power[i]`` the (nfft/2 + 1,) row of region i in the trace's squared unit per Hz, ``n_frames[i]`` the number of
    Welch frames it is the mean of (0: a row of NaN), ``argmax[i]`` its largest bin (-1 without a frame); ``nfft``,
    ``hop``, ``step`` as asked for and ``fs`` = rate/step, the rate of the decimated samples."""

    def __init__(self, regions, power, n_frames, argmax, nfft, hop, step, fs, trace_name=None):
        self.regions = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
        self.nfft, self.hop, self.step, self.fs = int(nfft), int(hop), int(step), float(fs)
        self.power = np.asarray(power).reshape(len(self.regions), self.nfft//2 + 1)
        self.n_frames = np.asarray(n_frames, dtype=np.int64).reshape(-1)
        self.argmax = np.asarray(argmax, dtype=np.int64).reshape(-1)
        self.trace_name = trace_name

    def __len__(self):
        return len(self.regions)

    def frequencies(self, i=0):
        """The frequencies of the bins of row i in Hz (the same for every row)."""
        return np.arange(self.nfft//2 + 1)*self.fs/self.nfft

    def peak_freqs(self, thresh=None):
        """pick_peak of every row in Hz: (R,) float64, NaN where there is no spectrum or no peak."""
        return np.array([pick_peak(self.power[i], thresh, self.fs) if self.n_frames[i] > 0 else np.nan
                         for i in range(len(self))], dtype=np.float64)
