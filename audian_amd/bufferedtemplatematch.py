"""Template matching on the fly: the correlation of one example call with the spectrogram under it, per frame and
channel, as a trace -- the score row of spectrogram cross-correlation, whose peaks are the calls of that kind.

A sibling of ``BufferedBandPower``: a derived trace whose SOURCE is the spectrogram.  Written as a plain plug-in it
would pull the (frames, channels, nfreq) slab to the host and correlate there; here ``process()`` is one
``hipdsp_template_match`` launch on the spectrogram's device mirror (float32 products on the matrix cores), and a new
template recomputes this trace only."""

import numpy as np

from .buffereddata import BufferedData
from .templates import Template, default_pivot, host_template_scores


class BufferedTemplateMatch(BufferedData):
    """The score of `template` (a templates.Template) against the spectrogram: one frame per spectrogram frame, shape
    (frames, channels).  The value at frame t belongs to the window of Tt frames that starts at t - Tt//2 -- a peak
    marks the middle of a call -- and is NaN where that window leaves the recording (or what the source's buffer held of
    it when the frame was computed).  With `normalize` the score is the correlation coefficient, -1 ... 1, NaN where
    the patch holds a non-finite value or its standard deviation is at most `min_std` (in the template's unit, dB for a
    log template); without it the plain sum of products.

    `min_std` = 0.1 dB is a choice that keeps silence at the floor and the spectrogram's zero tail frames from matching
    anything; it is not calibrated on recordings.  `pivot` (None: the template's own mean, as float32) is what the
    values are taken relative to before they meet the float32 matrix core (hipdsp_template_match); the result does not
    depend on it, only its rounding error does.

    The geometry follows the source exactly as BufferedBandPower's does.  A template that does not fit the spectrogram
    (another frequency or time resolution, relative 1e-9; a band outside its bins) is a ValueError from set_template()
    and open(), before anything is launched; when a later BufferedSpectrogram.update(nfft, overlap_frac) makes the
    template stale, the trace fills with NaN and `stale` is True until a fitting template is set."""

    def __init__(self, name='match', source='spectrogram', panel='trace', color='#ff00aa', lw_thin=2.5, lw_thick=4,
                 template=None, normalize=True, min_std=0.1, pivot=None):
        BufferedData.__init__(self, name, source, panel=panel, panel_type='trace', color=color, lw_thin=lw_thin,
                              lw_thick=lw_thick)
        self.template = self._checked(template, normalize)
        self.normalize, self.min_std = bool(normalize), self._checked_std(min_std)
        self.pivot = None if pivot is None else float(pivot)
        self.k0 = 0
        self.stale = False

    @staticmethod
    def _checked(template, normalize):
        """The template, or ValueError: no Template, or one the preparation refuses (a constant one when normalised)."""
        if template is None:
            return None
        if not isinstance(template, Template):
            raise ValueError('template must be a templates.Template (TraceGraph.cut_template, Template.load)')
        from . import hipdsp
        hipdsp.template_prepare(template.values, normalize)
        return template

    @staticmethod
    def _checked_std(min_std):
        if not float(min_std) >= 0:
            raise ValueError(f'min_std must be >= 0, got {min_std}')
        return float(min_std)

    def open(self, source):
        if len(getattr(source, 'shape', ())) != 3:
            raise ValueError(f'{self.name}: the source must be a spectrogram (frames, channels, bins)')
        if self.template is not None:
            self.template.first_bin(source)
        BufferedData.open(self, source, 1)
        self._set_range()
        self._fit()

    def _set_range(self):
        if self.normalize:
            self.unit, self.ampl_min, self.ampl_max = '', -1, 1
            return
        t = self.template
        top = 1.0 if t is None else float(np.sum(np.abs(t.values)))
        if t is not None and t.log:
            self.unit, top = 'dB^2', top*abs(t.floor_db)
        else:
            src = self.source
            full = float(getattr(getattr(src, 'source', None), 'ampl_max', 1.0))**2
            self.unit, top = src.unit, top*full/float(src.fresolution)
        self.ampl_min, self.ampl_max = -top, top

    def _fit(self):
        """Take the first bin from the source's current geometry; `stale` when the template no longer fits it."""
        self.stale = False
        if self.template is not None:
            try:
                self.k0 = self.template.first_bin(self.source)
            except ValueError:
                self.stale = True

    def set_template(self, template):
        """Another template (None: none, the trace is NaN): recomputes this trace and what hangs below it, never the
        spectrogram.  ValueError, with nothing changed or launched, for one that does not fit."""
        template = self._checked(template, self.normalize)
        if template is not None and self.source is not None:
            template.first_bin(self.source)
        self.template = template
        self._set_range()
        self.recompute_all()

    def update(self, min_std=None, normalize=None):
        """Another flatness mask or the other mode; recomputes this trace and what hangs below it, never the
        spectrogram."""
        min_std = self.min_std if min_std is None else self._checked_std(min_std)
        normalize = self.normalize if normalize is None else bool(normalize)
        self._checked(self.template, normalize)
        self.min_std, self.normalize = min_std, normalize
        self._set_range()
        self.recompute_all()

    def recompute(self):
        """Take over the source's current geometry (one frame per spectrogram frame, the buffer exactly over the
        spectrogram's), see whether the template still fits, then allocate and compute as the base class does."""
        src = self.source
        self.update_step(1)
        self.offset, self.bufferframes = src.offset, self._source_len()
        self._fit()
        BufferedData.recompute(self)

    def _device_plan(self, hipdsp):
        values = self.template.values
        return self._keyed_plan(hipdsp.TmplPlan, (values.tobytes(), values.shape, self.normalize), values, self.normalize)

    def _span(self, s0, n):
        """(lo, hi): the frames of the source's buffer the windows of dest frames [s0, s0 + n) lie in -- beyond the slab
        of this call where the source holds them -- clipped to the buffer."""
        Tt = self.template.values.shape[0]
        return max(0, s0 - Tt//2), min(self._source_len(), s0 + n - 1 - Tt//2 + Tt)

    def process(self, source, dest, nbefore):
        """dest[t, c] = the score of the window of the source that starts at frame nbefore + t - Tt//2."""
        n = len(dest)
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if n == 0:
            return
        t = self.template
        if t is None or self.stale:
            dest[...] = np.nan
            self._host_wrote(call)
            return
        Tt = t.values.shape[0]
        pivot = default_pivot(t.values) if self.pivot is None else self.pivot
        on_mirror = self._source_mirror(call, nbefore)
        if on_mirror is not None:
            from . import hipdsp
            src = self.source
            F = src._inner()
            s0 = call.soffset + nbefore
            lo, hi = self._span(s0, n)
            if not src._mirror_valid(lo, hi):
                lo, hi = s0, call.soffset + call.snframes
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            hipdsp.template_match(self.ctx, self._device_plan(hipdsp), src._dev.view(lo*F, (1,)), src._pitch(),
                                  self.channels, hi - lo, F, self.k0, s0 - Tt//2 - lo, n, ddst, db=t.log, ref_power=1.0,
                                  min_power=0.0, floor=t.floor, pivot=pivot, min_std=self.min_std, out_pitch=dpitch)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        slab, first = source, nbefore - Tt//2
        if call is not None:
            s0 = call.soffset + nbefore
            lo, hi = self._span(s0, n)
            slab, first = self.source.buffer[lo:hi], s0 - Tt//2 - lo
        dest[...] = host_template_scores(slab, t.values[None], self.k0, first, n, self.normalize, t.log, t.floor,
                                         self.min_std)[0].T
        self._host_wrote(call)
