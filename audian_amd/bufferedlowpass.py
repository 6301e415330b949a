"""Zero-phase low-pass on the fly: the reference's ``lowpass_filter`` (songdetector.py:49-54), ``filtfilt(*butter(1,
cutoff), source)``, as a derived trace at its source's rate -- on the power envelope with cutoff = 1/minduration it is
the slow envelope the detector's thresholds and events run on (songdetector.py:755).  ``process()`` is one
``hipdsp_envelope`` call without rectification, gain or clamp, i.e. plain ``sosfiltfilt``."""

import numpy as np

from .buffereddata import BufferedData
from .design import butter_sos


class BufferedLowpass(BufferedData):
    """``sosfiltfilt(butter(filter_order, cutoff), source)`` per channel, one second of pre-roll like BufferedEnvelope."""

    def __init__(self, name='slow-envelope', source='power-envelope', cutoff=2.0, filter_order=1, panel='trace',
                 color='#aa0000', lw_thin=2.5, lw_thick=4):
        BufferedData.__init__(self, name, source, tbefore=1, panel=panel, panel_type='trace', color=color,
                              lw_thin=lw_thin, lw_thick=lw_thick)
        self.cutoff, self.filter_order, self.sos = cutoff, filter_order, None
        self._design_key = None

    def open(self, source):
        BufferedData.open(self, source)
        self.sos, self._design_key = None, None
        self.update()

    def update(self, cutoff=None):
        """A new cut-off (None: as it is).  Recomputes this trace and what hangs below it, never the source."""
        if cutoff is not None:
            self.cutoff = cutoff
        self._design()
        self.recompute_all()

    def _design(self):
        """The low-pass at this trace's rate (which follows its source's: a power envelope may change its step); a design
        scipy would reject leaves sos = None, i.e. a zero trace."""
        key = (self.filter_order, self.cutoff, self.rate)
        if key != self._design_key:
            try:
                self.sos = butter_sos(self.filter_order, self.cutoff, 'lowpass', self.rate)
            except ValueError:
                self.sos = None
            self._design_key = key

    def process(self, source, dest, nbefore):
        """dest = sosfiltfilt(sos, source, axis=0)[nbefore:]; zeros when the design failed.  Raises ValueError like scipy
        when the slab is not longer than the pad length."""
        from . import hipdsp
        self._design()
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if len(dest) == 0:
            return
        on_mirror = self._source_mirror(call)
        if on_mirror is not None:
            x, spitch = on_mirror
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            if self.sos is None:
                self._zero_dest(ddst, dpitch, len(dest))
            else:
                hipdsp.envelope(self.ctx, self._sos_plan(), x, spitch, ddst, dpitch, self.channels, len(source), nbefore,
                                rectify=False, gain=1.0, clamp=False)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        if self.sos is None:
            dest[...] = 0.0
        else:
            from .refine import host_region_filtfilt
            slab = np.asarray(source[:]).reshape(len(source), -1)
            for c in range(slab.shape[1]):
                dest[:, c] = host_region_filtfilt(slab[:, c], self.sos)[nbefore:]
        self._host_wrote(call)
