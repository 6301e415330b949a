"""Band power on the fly: the power inside a frequency band of a spectrogram, per frame and channel, as a trace.

The reference names this trace as the next test of its plug-in surface ("Envelope from visible frequency range of
spectrogram", README.md:63 of the reference) and does not ship it: a derived trace whose SOURCE is the
spectrogram.  Written as a plain plug-in it would be ``np.sum(source[:, :, k0:k1], axis=2)`` in ``process()``, which
drags the spectrogram slab to the host; here ``process()`` is one ``hipdsp_band_power`` launch on the
spectrogram's device mirror, and moving the band recomputes this trace only."""

import numpy as np

from .buffereddata import BufferedData
from .bufferedspectrogram import band_bins, decibel


class BufferedBandPower(BufferedData):
    """``fresolution * sum(spectrogram[:, :, k0:k1], axis=2)``: the integral of the PSD over the bins whose
    frequencies lie in [fmin, fmax] (fmax None: up to the Nyquist bin) -- by Parseval the window-weighted mean
    square of the band's share of the detrended frame, in the signal's squared unit; in dB (re 1, -inf at or
    below `min_power`) with `log`.  One frame per spectrogram frame, shape (frames, channels).

    `k0`, `k1` are the current bin range.  Unlike any dest of the reference's base class, which keeps the geometry
    it was opened with, this trace follows its source: recompute() first takes over the spectrogram's current rate,
    frames, offset and frequency resolution, so BufferedSpectrogram.update(nfft, overlap_frac) carries through."""

    def __init__(self, name='bandpower', source='spectrogram', panel='trace', color='#ff8800', lw_thin=2.5,
                 lw_thick=4, fmin=0.0, fmax=None, log=False, min_power=1e-20):
        BufferedData.__init__(self, name, source, panel=panel, panel_type='trace', color=color, lw_thin=lw_thin,
                              lw_thick=lw_thick)
        self.fmin, self.fmax, self.log, self.min_power = fmin, fmax, bool(log), min_power
        self.k0 = self.k1 = 0
        self.scale = 1.0

    def open(self, source):
        BufferedData.open(self, source, 1)
        self._set_range()
        self._set_bins()

    def _set_range(self):
        """Unit and amplitude range: the spectrogram's own are its unit per Hz and its FREQUENCY axis
        (bufferedspectrogram.py:66-67); this trace spans 0 ... the square of the signal's full scale."""
        src = self.source
        full = float(getattr(getattr(src, 'source', None), 'ampl_max', 1.0))**2
        unit = src.unit[:-3] if src.unit.endswith('/Hz') else src.unit
        if self.log:
            self.unit = 'dB'
            self.ampl_min, self.ampl_max = 10.0*np.log10(self.min_power), 10.0*np.log10(full)
        else:
            self.unit = unit
            self.ampl_min, self.ampl_max = 0, full

    def _set_bins(self):
        src = self.source
        self.scale = float(src.fresolution)
        self.k0, self.k1 = band_bins(self.fmin, self.fmax, src.fresolution, int(src.shape[2]))

    def set_band(self, fmin, fmax):
        """A new band in Hz (the spectrogram panel's visible y-range, two draggable lines): recomputes this trace
        and what hangs below it, never the spectrogram."""
        self.fmin, self.fmax = fmin, fmax
        self._set_bins()
        self.recompute_all()

    def update(self, log=None):
        """Switch between linear power and dB."""
        if log is not None:
            self.log = bool(log)
        self._set_range()
        self.recompute_all()

    def recompute(self):
        """Take over the source's current geometry (one frame per spectrogram frame, the buffer exactly over the
        spectrogram's), redo the bins, then allocate and compute as the base class does."""
        src = self.source
        self.update_step(1)
        self.offset, self.bufferframes = src.offset, self._source_len()
        self._set_bins()
        BufferedData.recompute(self)

    def process(self, source, dest, nbefore):
        """dest[t, c] = scale * sum(source[nbefore + t, c, k0:k1]), in dB with `log`; the spectrogram's zero tail
        frames give 0 (-inf).  The steps are shared with the traces derived from this class, which supply
        _launch() and _host_values()."""
        n = len(dest)
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if n == 0:
            return
        on_mirror = self._source_mirror(call, nbefore)
        if on_mirror is not None:
            spec, spitch = on_mirror
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            self._launch(spec, spitch, n, ddst, dpitch)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        dest[...] = self._host_values(np.asarray(source[nbefore:nbefore + n], dtype=np.float64))
        self._host_wrote(call)

    def _launch(self, spec, spitch, n, ddst, dpitch):
        """One launch over `n` frames of the spectrogram's mirror at `spec` into the planar rows at `ddst`."""
        from . import hipdsp
        hipdsp.band_power(self.ctx, spec, spitch, self.channels, n, self.source._inner(), [(self.k0, self.k1)],
                          self.scale, ddst, db=self.log, min_power=self.min_power, out_pitch=dpitch)

    def _host_values(self, slab):
        """The same values of a (frames, channels, nfreq) float64 host slab."""
        power = self.scale*np.sum(slab[:, :, self.k0:self.k1], axis=2)
        return decibel(power, 1.0, self.min_power) if self.log else power
