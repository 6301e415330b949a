"""Noise profiles: one power per channel and frequency bin -- a percentile over time of every bin of a spectrogram, which
a stationary band (mains hum, an insect chorus, microphone noise rising towards the Nyquist bin) dominates and a call
does not -- and the spectrogram equalised by it: divided (a whitened image, 0 dB = the profile) or reduced (spectral
subtraction).  The contract is the definition in ``include/hip_dsp.h`` (hipdsp_bin_quantiles, hipdsp_spec_equalize);
``host_bin_quantiles`` and ``host_equalize`` restate it in numpy for a host-only graph, and give the same bits.

The profile is the percentile itself: the median of exponentially distributed periodogram values lies below their mean
(by ln 2), and no correction towards the mean is applied."""

import numpy as np

from .bufferedspectrogram import decibel

RESOLUTION_RTOL = 1e-9
MODES = ('divide', 'subtract')


def host_bin_quantiles(slab, first, n_frames, frame_step, k0, k1, q):
    """hipdsp_bin_quantiles on a host slab (frames, channels, nfreq), taken as float32: of the values
    slab[first + j*frame_step, c, k], j < n_frames, NaNs dropped and sorted, the two elements at k_lo = floor(q*(n - 1))
    and min(k_lo + 1, n - 1) and the count n -- (lo_hi (channels, k1 - k0, 2) float32, count (channels, k1 - k0) int32),
    NaN, NaN, 0 for a column without a value."""
    if not 0.0 <= float(q) <= 1.0:
        raise ValueError(f'q must lie in [0, 1], got {q}')
    if frame_step < 1 or first < 0 or n_frames < 0 or (n_frames > 0 and first + (n_frames - 1)*frame_step >= len(slab)):
        raise ValueError('frame range outside the slab')
    rows = first + frame_step*np.arange(n_frames)
    x = np.sort(np.asarray(slab[first:first + max(0, (n_frames - 1)*frame_step + 1)], dtype=np.float32)[::frame_step, :, k0:k1],
                axis=0) if n_frames > 0 else np.zeros((0,) + tuple(np.shape(slab)[1:2]) + (k1 - k0,), dtype=np.float32)
    assert len(x) == len(rows)
    count = np.sum(~np.isnan(x), axis=0).astype(np.int32)                 # np.sort puts the NaNs behind the values
    lo_hi = np.full(count.shape + (2,), np.nan, dtype=np.float32)
    if n_frames == 0 or count.size == 0:
        return lo_hi, count
    n = count.astype(np.int64)
    pos = float(q)*(n - 1).astype(np.float64)
    k_lo = np.maximum(np.floor(pos).astype(np.int64), 0)
    k_hi = np.maximum(np.minimum(k_lo + 1, n - 1), 0)
    lo_hi[..., 0] = np.where(n > 0, np.take_along_axis(x, k_lo[None], axis=0)[0], np.float32(np.nan))
    lo_hi[..., 1] = np.where(n > 0, np.take_along_axis(x, k_hi[None], axis=0)[0], np.float32(np.nan))
    return lo_hi, count


def finish_quantiles(lo_hi, count, q):
    """The percentile of the two order statistics, float64: with pos = q*(n - 1) and frac = pos - floor(pos), lo when
    frac == 0 or hi == lo, else lo + frac*(hi - lo) -- np.percentile's linear interpolation, the formula of
    BufferedSpectrogram.estimate_noiselevels.  NaN for a column without a value."""
    lo = np.asarray(lo_hi[..., 0], dtype=np.float64)
    hi = np.asarray(lo_hi[..., 1], dtype=np.float64)
    n = np.asarray(count, dtype=np.int64)
    pos = float(q)*np.maximum(n - 1, 0).astype(np.float64)
    frac = pos - np.floor(pos)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where((frac == 0) | (hi == lo), lo, lo + frac*(hi - lo))


def host_equalize(slab, profile, mode='divide'):
    """hipdsp_spec_equalize on a host slab (frames, channels, nfreq) with a profile (channels, nfreq), both taken as
    float32, in numpy's float32 arithmetic: slab/profile, or slab - profile and 0 where that is negative.  Returns
    float32 of the slab's shape."""
    if mode not in MODES:
        raise ValueError(f'unknown equalisation mode {mode!r}: one of {", ".join(MODES)}')
    p = np.asarray(slab, dtype=np.float32)
    n = np.asarray(profile, dtype=np.float32)[None]
    with np.errstate(all='ignore'):
        if mode == 'divide':
            return (p/n).astype(np.float32)
        d = (p - n).astype(np.float32)
        return np.where(d < 0, np.float32(0), d)


class NoiseProfile(object):
    """A per-channel, per-bin power profile: `values` (channels, nfreq) float32 on a grid of `fresolution` Hz, taken as
    the `percentile` of frames `tresolution` seconds apart between `t0` and `t1` seconds.  Entries below `min_power`
    (the library's dB floor) are raised to it, so that dividing by the profile stays finite in silence; a NaN entry -- a
    bin without a single valid frame -- is a ValueError naming the channel and the bin."""

    def __init__(self, values, fresolution, tresolution, percentile=50.0, min_power=1e-20, t0=0.0, t1=0.0):
        values = np.array(values, dtype=np.float32)
        if values.ndim != 2 or values.size == 0:
            raise ValueError('profile values must be shape (channels, bins), at least one of each')
        bad = np.argwhere(np.isnan(values))
        if len(bad):
            raise ValueError(f'noise profile: channel {int(bad[0][0])} bin {int(bad[0][1])} has no valid frame '
                             f'({len(bad)} such entries)')
        if not float(min_power) >= 0:
            raise ValueError(f'min_power must be >= 0, got {min_power}')
        self.min_power = float(min_power)
        floor = np.float32(self.min_power)
        self.values = np.where(values < floor, floor, values).astype(np.float32)
        self.fresolution, self.tresolution = float(fresolution), float(tresolution)
        self.percentile, self.t0, self.t1 = float(percentile), float(t0), float(t1)

    @property
    def channels(self):
        return self.values.shape[0]

    @property
    def nfreq(self):
        return self.values.shape[1]

    def db(self, ref_power=1.0):
        """The profile in dB re `ref_power`, float64 (channels, nfreq)."""
        return decibel(self.values, ref_power, 0.0)

    def fits(self, spec):
        """Does the profile belong on `spec` (a spectrogram-shaped trace)?  The channel and bin counts and the frequency
        resolution (relative 1e-9) must match."""
        shape = tuple(getattr(spec, 'shape', ()))
        if len(shape) != 3 or int(shape[2]) != self.nfreq or int(spec.channels) != self.channels:
            return False
        its = float(spec.fresolution)
        return abs(self.fresolution - its) <= RESOLUTION_RTOL*abs(its)

    def save(self, path):
        np.savez(path, values=self.values, fresolution=self.fresolution, tresolution=self.tresolution,
                 percentile=self.percentile, min_power=self.min_power, t0=self.t0, t1=self.t1)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z['values'], float(z['fresolution']), float(z['tresolution']), float(z['percentile']),
                       float(z['min_power']), float(z['t0']), float(z['t1']))
