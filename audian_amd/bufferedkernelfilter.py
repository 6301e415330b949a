"""Kernel filter on the fly: a trace convolved with an FIR kernel, the feature expansion the reference names as an
open test of its plug-in surface ("Feature expansion (kernel filter)", README.md:64 of the reference) and does not
ship.  Written as a plain plug-in it would be ``np.convolve(source[:, c], kernel, 'same')`` per channel in
``process()``, at CPU speed and with the source slab on the host; here ``process()`` is one ``hipdsp_fir_bank``
launch on the source's device mirror (float32 products on the matrix cores), and a new kernel recomputes this trace
only.  ``kernel_bank()`` runs a whole bank (one feature trace per kernel) in one pass."""

import numpy as np

from .buffereddata import BufferedData, _KEEP, _regrid

MAX_KERNELS = 16


def fir_same(slab, taps, first=0, step=1, n=None):
    """The definition in float64 on a host slab (frames, channels), zero outside it:
    y[t, c] = sum_j taps[j] * slab[t + (L-1)//2 - j, c], returned at t = first + i*step, i < n
    (np.convolve(slab[:, c], taps, 'same')[t] when the slab is at least as long as the kernel)."""
    slab = np.asarray(slab, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    frames, n_taps = len(slab), len(taps)
    if n is None:
        n = max(0, -(-(frames - first)//step))
    out = np.zeros((n,) + slab.shape[1:])
    if n == 0 or frames == 0:
        return out
    lead = (n_taps - 1)//2
    flat = slab.reshape(frames, -1)
    res = out.reshape(n, -1)
    for c in range(flat.shape[1]):
        full = np.convolve(flat[:, c], taps)                 # full[m] = sum_j taps[j] x[m - j]
        picked = full[first + lead::step][:n]
        res[:len(picked), c] = picked
    return out


class BufferedKernelFilter(BufferedData):
    """``max(convolve(source, kernel, 'same')[::step] - threshold, 0)`` per channel (linear without a threshold): one
    frame per `step` source frames, shape (frames, channels).  `kernel` is a 1-D tap array, None makes the trace a copy
    of its source.

    The margins stay 0: the slab process() is handed is zero-extended at both ends, so within (L-1)/2 frames of the
    ends of a load the trace rises from / decays to what the zeros give.  Declared margins would not help: the
    reference's load_buffer divides them by the rate where it means to multiply (buffereddata.py:96,99) and drops
    them, exactly as it restarts BufferedFilter from zero state at every load.  A whole-buffer recompute
    (set_kernel, update) sees the source's whole buffer."""

    def __init__(self, name='features', source='envelope', panel='trace', color='#00aaff', lw_thin=2.5, lw_thick=4,
                 kernel=None, step=1, threshold=None):
        BufferedData.__init__(self, name, source, panel=panel, panel_type='trace', color=color, lw_thin=lw_thin,
                              lw_thick=lw_thick)
        self.step = max(1, int(step))
        self.threshold = None if threshold is None else float(threshold)
        self.kernel = self._taps(kernel)

    @staticmethod
    def _taps(kernel):
        if kernel is None:
            return np.ones(1)
        taps = np.array(kernel, dtype=np.float64)
        if taps.ndim != 1 or len(taps) < 1:
            raise ValueError('kernel must be a 1-D array of at least one tap')
        return taps

    def open(self, source):
        self._require_trace_source(source)
        BufferedData.open(self, source, self.step)
        self._set_range()

    def _set_range(self):
        """Unit of the source; the amplitude range is what a full-scale source can give, sum |h| times its own."""
        src = self.source
        self.unit = src.unit
        self.ampl_max = float(src.ampl_max)*float(np.sum(np.abs(self.kernel)))
        self.ampl_min = 0 if self.threshold is not None else -self.ampl_max

    def set_kernel(self, taps):
        """New taps (None: copy): recomputes this trace and what hangs below it, never the source."""
        self.kernel = self._taps(taps)
        self._set_range()
        self.recompute_all()

    def update(self, threshold=_KEEP, step=None):
        """A new threshold (None: linear; a number: max(y - threshold, 0)) and / or a new step; recomputes this
        trace and what hangs below it, never the source."""
        if threshold is not _KEEP:
            self.threshold = None if threshold is None else float(threshold)
        if step is not None and max(1, int(step)) != self.step:
            self.step = max(1, int(step))
            # the buffer over what the source holds, as align_buffer would put it; the traces below follow the new grid
            _regrid(self, self.step, self._source_len())
        self._set_range()
        self.recompute_all()

    def _device_plan(self, hipdsp):
        return self._keyed_plan(hipdsp.FirPlan, (self.kernel.tobytes(), self.threshold), self.kernel[None, :],
                                None if self.threshold is None else [self.threshold])

    def process(self, source, dest, nbefore):
        """dest[i, c] = y[c, nbefore + i*step], y the kernel over the slab `source` zero-extended at both ends."""
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
            hipdsp.fir_bank(self.ctx, self._device_plan(hipdsp), x, spitch, self.channels, call.snframes, nbefore,
                            self.step, n, ddst, rectify=self.threshold is not None, out_pitch=dpitch)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        y = fir_same(np.asarray(source[:], dtype=np.float64), self.kernel, nbefore, self.step, n)
        dest[...] = np.maximum(y - self.threshold, 0.0) if self.threshold is not None else y
        self._host_wrote(call)


def kernel_bank(trace, kernels, step=1, thresholds=None):
    """A whole bank over the current buffer of `trace` in one pass: kernels (K, L) float64, K feature traces
    out[k, c, i] = y_k[c, i*step] over the buffer zero-extended at both ends, max(y - thresholds[k], 0) with
    `thresholds`.  Reads the trace's device mirror when it is valid (a host buffer is uploaded first), 16 kernels per
    launch, and returns a (K, channels, ceil(len(buffer)/step)) float32 device array: nothing crosses PCIe."""
    from . import hipdsp
    kernels = np.atleast_2d(np.asarray(kernels, dtype=np.float64))
    step = max(1, int(step))
    if thresholds is not None:
        thresholds = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(kernels),))
    ctx = trace.ctx if isinstance(trace, BufferedData) else hipdsp.default_context()
    frames = len(trace._hostbuf) if isinstance(trace, BufferedData) else len(trace.buffer)
    channels = int(trace.channels)
    n = -(-frames//step)
    out = hipdsp.DeviceArray(ctx, (len(kernels), channels, n), np.float32)
    if n == 0 or channels == 0:
        return out
    if isinstance(trace, BufferedData) and trace._mirror_valid(0, frames):
        x, pitch = trace._dev, trace._pitch()
    else:
        host = np.asarray(trace.buffer[:], dtype=np.float32).reshape(frames, channels)
        x, pitch = hipdsp.DeviceArray.from_host(ctx, np.ascontiguousarray(host.T)), frames
    plan = hipdsp.FirPlan(ctx)
    for j in range(0, len(kernels), MAX_KERNELS):
        plan.set(kernels[j:j + MAX_KERNELS], None if thresholds is None else thresholds[j:j + MAX_KERNELS])
        hipdsp.fir_bank(ctx, plan, x, pitch, channels, frames, 0, step, n, out.view(j*channels*n, (1,)),
                        rectify=thresholds is not None)
    plan.close()           # waits for the stream
    return out
