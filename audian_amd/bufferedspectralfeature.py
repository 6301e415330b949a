"""Spectral contours on the fly: where the power of a spectrogram's frequency band sits, per frame and channel, as a
trace -- peak frequency, centroid, bandwidth, flatness, the band's extent.

A sibling of ``BufferedBandPower``: a derived trace whose SOURCE is the spectrogram.  Written as a plain plug-in it
would pull the (frames, channels, nfreq) slab to the host for an ``np.argmax``; here ``process()`` is one
``hipdsp_spectral_features`` launch on the spectrogram's device mirror, and moving the band or switching the feature
recomputes this trace only.  Frames without a call (peak power at or below `min_power`) are NaN, so the contour is
drawn only where there is one."""

import numpy as np

from . import hipdsp
from .bufferedbandpower import BufferedBandPower
from .hipdsp import SPECTRAL_FEATURES, drop_ratio, feature_mask

FREQUENCY_FEATURES = ('peak_bin_freq', 'peak_freq', 'centroid', 'bandwidth', 'freq_low', 'freq_high')


def host_spectral_features(spec, k0, k1, features, scale, min_power=0.0, drop_db=10.0):
    """hipdsp_spectral_features in numpy, float64: the requested features (names or a mask; rows in bit order) of the
    bins [k0, k1) of every row of `spec` (..., nfreq), as float32 (n_features, ...).  The formulas are those of
    include/hip_dsp.h; only the order of the sums is numpy's."""
    mask, ratio = feature_mask(features), drop_ratio(drop_db)
    P = np.asarray(spec, dtype=np.float64)[..., int(k0):int(k1)]
    lead, n = P.shape[:-1], P.shape[-1]
    val = np.full((len(SPECTRAL_FEATURES),) + lead, np.nan)
    if n > 0 and P.size > 0:
        with np.errstate(all='ignore'):
            j = np.argmax(P, axis=-1)                           # the first NaN, else the first of the largest
            kp = (j + int(k0)).astype(np.float64)
            peak = np.take_along_axis(P, j[..., None], axis=-1)[..., 0]
            valid = np.isfinite(peak) & (peak > min_power)
            dk = np.arange(int(k0), int(k1), dtype=np.float64) - kp[..., None]
            S, M1, M2 = P.sum(axis=-1), (dk*P).sum(axis=-1), ((dk*dk)*P).sum(axis=-1)
            pa = np.take_along_axis(P, np.clip(j - 1, 0, n - 1)[..., None], axis=-1)[..., 0]
            pc = np.take_along_axis(P, np.clip(j + 1, 0, n - 1)[..., None], axis=-1)[..., 0]
            la, lb, lc = np.log(pa), np.log(peak), np.log(pc)
            den = (la - 2.0*lb) + lc
            ok = (j - 1 >= 0) & (j + 1 < n) & (pa > 0) & (pc > 0) & (den < 0)
            d = np.where(ok, (0.5*(la - lc))/np.where(ok, den, 1.0), 0.0)
            m = M1/S
            var = M2/S - m*m
            above = P >= (ratio*peak)[..., None]
            klo = np.argmax(above, axis=-1) + int(k0)
            khi = int(k1) - 1 - np.argmax(above[..., ::-1], axis=-1)
            val[0] = scale*kp
            val[1] = scale*(kp + d)
            val[3] = scale*(kp + m)
            val[4] = scale*np.sqrt(np.where(var > 0, var, 0.0))
            if mask & 32:
                val[5] = np.exp(np.log(P).sum(axis=-1)/n)/(S/n)
            val[6], val[7] = scale*klo, scale*khi
            val[...] = np.where(valid, val, np.nan)
            val[2] = peak
    with np.errstate(over='ignore'):
        return val[[b for b in range(len(SPECTRAL_FEATURES)) if mask >> b & 1]].astype(np.float32)


class BufferedSpectralFeature(BufferedBandPower):
    """One of hipdsp.SPECTRAL_FEATURES of the spectrogram's bins with frequencies in [fmin, fmax] (fmax None: up to the
    Nyquist bin), one frame per spectrogram frame, shape (frames, channels); NaN where the band's peak power is not
    above `min_power`.  `drop_db` is how far below the peak 'freq_low' and 'freq_high' bound the call.

    The geometry follows the source exactly as BufferedBandPower's does (its recompute(), its bins).  The frequency
    features carry 'Hz' and the spectrogram's frequency axis as amplitude range, so the contour overlays the
    spectrogram panel; 'peak_power' carries the spectrogram's unit, 'flatness' none and 0 ... 1."""

    def __init__(self, name='peakfreq', source='spectrogram', panel='spectrogram', color='#ffffff', lw_thin=1.5,
                 lw_thick=3, feature='peak_freq', fmin=0.0, fmax=None, min_power=1e-20, drop_db=10.0):
        BufferedBandPower.__init__(self, name, source, panel=panel, color=color, lw_thin=lw_thin, lw_thick=lw_thick,
                                   fmin=fmin, fmax=fmax, log=False, min_power=min_power)
        self.feature, self.drop_db = self._checked(feature, drop_db)

    @staticmethod
    def _checked(feature, drop_db):
        """(feature, drop_db) or ValueError: before anything is launched or changed."""
        if not isinstance(feature, str) or feature not in SPECTRAL_FEATURES:
            raise ValueError(f'unknown spectral feature {feature!r}: one of {", ".join(SPECTRAL_FEATURES)}')
        drop_ratio(drop_db)
        return feature, float(drop_db)

    def _set_range(self):
        src = self.source
        if self.feature in FREQUENCY_FEATURES:
            nyquist = 0.5*src.source.rate if hasattr(src, 'source') and src.source is not None else src.ampl_max
            self.unit, self.ampl_min, self.ampl_max = 'Hz', 0, nyquist
        elif self.feature == 'flatness':
            self.unit, self.ampl_min, self.ampl_max = '', 0, 1
        else:
            full = float(getattr(getattr(src, 'source', None), 'ampl_max', 1.0))**2
            self.unit, self.ampl_min, self.ampl_max = src.unit, 0, full/float(src.fresolution)

    def update(self, feature=None, min_power=None, drop_db=None):
        """Another feature, floor or drop: recomputes this trace and what hangs below it, never the spectrogram."""
        feature, drop_db = self._checked(self.feature if feature is None else feature,
                                         self.drop_db if drop_db is None else drop_db)
        self.feature, self.drop_db = feature, drop_db
        if min_power is not None:
            self.min_power = float(min_power)
        self._set_range()
        self.recompute_all()

    def _launch(self, spec, spitch, n, ddst, dpitch):
        """BufferedBandPower.process()'s launch: the spectrogram's zero tail frames give NaN."""
        hipdsp.spectral_features(self.ctx, spec, spitch, self.channels, n, self.source._inner(), self.k0, self.k1,
                                 (self.feature,), self.scale, ddst, min_power=self.min_power, drop_db=self.drop_db,
                                 out_pitch=dpitch)

    def _host_values(self, slab):
        return host_spectral_features(slab, self.k0, self.k1, (self.feature,), self.scale, self.min_power,
                                      self.drop_db)[0]
