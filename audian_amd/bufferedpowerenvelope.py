"""Power envelope on the fly: the first step of the reference's song detector, ``envelope()`` (songdetector.py:57-69) --
the squares of a band-passed trace, ``filtfilt(*butter(1, cutoff))`` of them, every ``step``-th sample, the clamp at zero
and the root -- as a derived trace at the envelope rate ``source.rate/step`` (5 kHz instead of 96 kHz for the default
cut-off).  ``process()`` is one ``hipdsp_power_envelope`` call on the source's device mirror: three sweeps over the source,
nothing written at full rate.  This is NOT ``BufferedEnvelope`` (``pi/2 |x|`` filtered at second order, at full rate): it
is the trace the detector's thresholds, events and pulse rates are defined on."""

import numpy as np

from .buffereddata import BufferedData, _KEEP, _regrid      # (_regrid lived here first: it stays importable)
from .design import butter_sos


def power_envelope_step(rate, cutoff):
    """The reference's decimation (songdetector.py:63-66): round(rate / min(10 cutoff, rate))."""
    rate, cutoff = float(rate), float(cutoff)
    return max(1, int(np.round(rate/min(10.0*cutoff, rate)))) if cutoff > 0 else 1


def power_envelope_host(sos, slab, first=0, step=1, n_out=None, gain=4.0, root=True):
    """The definition of hipdsp_power_envelope in numpy float64 on a host slab (frames, channels): f = sosfiltfilt(sos,
    slab**2) per channel (refine.host_region_filtfilt's passes, unrounded), float32(gain max(f[first + j step], 0)), j <
    n_out, and its float32 root with `root`.  (n_out, channels) float32; ValueError when the slab is not longer than the
    pad length; a channel with a NaN or an infinity comes out all NaN."""
    from .refine import _sosfilt, _zi, padlen
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    slab = np.asarray(slab)
    u = np.asarray(slab, dtype=np.float32).astype(np.float64).reshape(len(slab), -1)**2
    frames, edge = len(u), int(padlen(sos))
    if frames <= edge:
        raise ValueError('The length of the input vector x must be greater than padlen, which is %d.' % edge)
    if n_out is None:
        n_out = max(0, -(-(frames - first)//step))
    if step < 1 or first < 0 or (n_out > 0 and first + (n_out - 1)*step >= frames):
        raise ValueError('the grid first + j step, j < n_out, leaves the slab')
    out = np.empty((n_out, u.shape[1]), dtype=np.float32)
    zi = _zi(sos)
    for c in range(u.shape[1]):
        v = u[:, c]
        if not np.all(np.isfinite(v)):
            out[:, c] = np.nan
            continue
        ext = np.concatenate((2*v[0] - v[edge:0:-1], v, 2*v[-1] - v[-2:-(edge + 2):-1]))
        y = _sosfilt(sos, ext, zi*ext[0])
        f = _sosfilt(sos, y[::-1], zi*y[-1])[::-1][edge:edge + frames]
        out[:, c] = (float(gain)*np.maximum(f[first::step][:n_out], 0.0)).astype(np.float32)
    return np.sqrt(out) if root else out


class BufferedPowerEnvelope(BufferedData):
    """``sqrt(4 max(filtfilt(butter(filter_order, envelope_cutoff), source**2), 0))[::step]`` per channel (without `root`:
    ``2 max(..., 0)[::step]``, the reference's edata): one frame per `step` source frames, frame j of the trace is source
    frame j*step of the RECORDING -- the grid is absolute, a scroll never changes a value that stays in the buffer.
    step=None takes the reference's rule, round(rate / min(10 envelope_cutoff, rate)).  One second of pre-roll like
    BufferedEnvelope.  Filters of one or two sections (filter_order <= 4)."""

    def __init__(self, name='power-envelope', source='filtered', envelope_cutoff=500, filter_order=1, step=None,
                 root=True, panel='trace', color='#ff4400', lw_thin=2.5, lw_thick=4):
        BufferedData.__init__(self, name, source, tbefore=1, panel=panel, panel_type='trace', color=color,
                              lw_thin=lw_thin, lw_thick=lw_thick)
        self.envelope_cutoff, self.filter_order = envelope_cutoff, filter_order
        self.fixed_step = None if step is None else max(1, int(step))
        self.root = bool(root)
        self.step, self.sos = 1, None

    @property
    def gain(self):
        """4 under the root (sqrt(2 f) sqrt(2) = 2 sqrt(f)), 2 without (the reference's edata)."""
        return 4.0 if self.root else 2.0

    def _step_for(self, source):
        return self.fixed_step if self.fixed_step is not None else power_envelope_step(source.rate, self.envelope_cutoff)

    def open(self, source):
        self._require_trace_source(source)
        self.step = self._step_for(source)
        BufferedData.open(self, source, self.step)
        self.ampl_min, self.ampl_max = 0, 2.0*float(source.ampl_max)*(1.0 if self.root else float(source.ampl_max))
        self.sos = None
        self.update()

    def update(self, envelope_cutoff=_KEEP, step=_KEEP):
        """A new cut-off and / or a new step (None: the reference's rule again); designs the low-pass -- a design scipy
        would reject leaves sos = None, i.e. a zero trace -- and recomputes this trace and what hangs below it, never
        the source."""
        if envelope_cutoff is not _KEEP:
            self.envelope_cutoff = envelope_cutoff
        if step is not _KEEP:
            self.fixed_step = None if step is None else max(1, int(step))
        src = self.source
        new_step = self._step_for(src)
        if new_step != self.step:
            self.step = new_step
            _regrid(self, new_step, self._source_len())
        try:
            self.sos = butter_sos(self.filter_order, self.envelope_cutoff, 'lowpass', src.rate)
        except ValueError:
            self.sos = None
        self.recompute_all()

    def process(self, source, dest, nbefore):
        """dest[i, c] = the power envelope of the slab `source` at its frame nbefore + i*step.  Raises ValueError like
        scipy when the slab is not longer than the pad length; zeros when the design failed."""
        from . import hipdsp
        n = len(dest)
        self._check_lengths(source, dest, nbefore, self.step)
        call = self._take_call(source, dest)
        if n == 0:
            return
        on_mirror = self._source_mirror(call)
        if on_mirror is not None:
            x, spitch = on_mirror
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            if self.sos is None:
                self._zero_dest(ddst, dpitch, n)
            else:
                hipdsp.power_envelope(self.ctx, self._sos_plan(), x, spitch, self.channels, call.snframes, ddst, dpitch,
                                      nbefore, self.step, n, self.gain, self.root)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        if self.sos is None:
            dest[...] = 0.0
        else:
            dest[...] = power_envelope_host(self.sos, np.asarray(source[:]), nbefore, self.step, n, self.gain, self.root)
        self._host_wrote(call)
