"""Thin Python host layer over the libhip_dsp C ABI: context, device arrays, filter
plans and the hot-path calls.  Device-native layout is planar float32
(channels, frames); see ``include/hip_dsp.h``.
"""

import contextlib
import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib


class _Handle:
    """Owns one C handle `_h`: close() destroys it once (_destroy, the subclass's), __del__ swallows errors."""

    _h = None

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h is not None and self._h.value:
            self._destroy()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Memory:
    """Owns the block at `ptr` unless `_own` is False: free() releases it once (_release, the subclass's), __del__
    swallows errors."""

    ptr = 0
    _own = True

    def free(self):
        if self._own and self.ptr:
            self._release()
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context(_Handle):
    """A device + HIP stream on which libhip_dsp enqueues its work."""

    def __init__(self, device=0, stream=None):
        h = ctypes.c_void_p()
        check(lib.hipdsp_ctx_create(int(device), ctypes.c_void_p(stream or 0), ctypes.byref(h)))
        self._h = h
        self.device = int(device)

    def _destroy(self):
        lib.hipdsp_ctx_destroy(self._h)

    def set_stream(self, stream):
        check(lib.hipdsp_ctx_set_stream(self._h, ctypes.c_void_p(stream or 0)))

    def synchronize(self):
        check(lib.hipdsp_ctx_synchronize(self._h))

    def set_max_segments(self, n):
        check(lib.hipdsp_ctx_set_max_segments(self._h, int(n)))

    def set_option(self, name, value):
        check(lib.hipdsp_ctx_set_option(self._h, name.encode(), int(value)))

    def set_mid_event(self, ev):
        check(lib.hipdsp_ctx_set_mid_event(self._h, ev if ev is not None else ctypes.c_void_p(0)))

    def pool_stats(self):
        """(cached bytes, hits, misses) of the context's block cache behind hipdsp_malloc/free."""
        cached, hits, misses = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.hipdsp_pool_stats(self._h, ctypes.byref(cached), ctypes.byref(hits), ctypes.byref(misses)))
        return int(cached.value), int(hits.value), int(misses.value)

    def pool_trim(self):
        check(lib.hipdsp_pool_trim(self._h))

    def reserve(self, nbytes):
        check(lib.hipdsp_ctx_reserve(self._h, int(nbytes)))

    # streams and graphs ---------------------------------------------------
    def create_stream(self):
        st = ctypes.c_void_p()
        check(lib.hipdsp_stream_create(self._h, ctypes.byref(st)))
        return st.value

    def destroy_stream(self, stream):
        check(lib.hipdsp_stream_destroy(self._h, ctypes.c_void_p(stream)))

    def graph_begin(self):
        check(lib.hipdsp_graph_begin(self._h))

    def graph_end(self):
        g = ctypes.c_void_p()
        check(lib.hipdsp_graph_end(self._h, ctypes.byref(g)))
        return g

    def graph_launch(self, graph):
        check(lib.hipdsp_graph_launch(self._h, graph))

    def graph_destroy(self, graph):
        check(lib.hipdsp_graph_destroy(self._h, graph))

    # events -------------------------------------------------------------
    def event(self):
        ev = ctypes.c_void_p()
        check(lib.hipdsp_event_create(self._h, ctypes.byref(ev)))
        return ev

    def record(self, ev):
        check(lib.hipdsp_event_record(self._h, ev))

    def wait_event(self, ev):
        """Later work on this context's stream waits for `ev` (recorded on any stream)."""
        check(lib.hipdsp_event_wait(self._h, ev))

    def elapsed_ms(self, start, stop):
        ms = ctypes.c_float()
        check(lib.hipdsp_event_elapsed_ms(self._h, start, stop, ctypes.byref(ms)))
        return float(ms.value)

    def destroy_event(self, ev):
        check(lib.hipdsp_event_destroy(self._h, ev))



_default_ctx = None


def default_context():
    """The process-wide context on device 0 / LOCAL_RANK (created on first use)."""
    global _default_ctx
    if _default_ctx is None:
        import os
        _default_ctx = Context(int(os.environ.get('LOCAL_RANK', '0')))
    return _default_ctx


class DeviceArray(_Memory):
    """A caller-owned block of HBM with a NumPy-like shape/dtype (C-contiguous)."""

    def __init__(self, ctx, shape, dtype=np.float32, ptr=None, owner=None, write_probe=0):
        """write_probe = N > 1: the block kernels will write a trace into -- the best of N allocations by the time of
        a memset over each (hipdsp_malloc_probed: where a block lies in HBM moves a write stream by up to 12 %)."""
        self.ctx = ctx
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64))*self.dtype.itemsize
        self._own = ptr is None
        self._owner = owner
        if ptr is None:
            p = ctypes.c_void_p()
            if write_probe > 1:
                check(lib.hipdsp_malloc_probed(ctx.handle, self.nbytes, int(write_probe), ctypes.byref(p)))
            else:
                check(lib.hipdsp_malloc(ctx.handle, self.nbytes, ctypes.byref(p)))
            self.ptr = p.value or 0
        else:
            self.ptr = int(ptr)

    @classmethod
    def from_host(cls, ctx, array, dtype=None):
        a = np.ascontiguousarray(array, dtype=dtype)
        d = cls(ctx, a.shape, a.dtype)
        d.copy_from_host(a)
        return d

    def copy_from_host(self, array):
        a = np.ascontiguousarray(array, dtype=self.dtype)
        if a.nbytes != self.nbytes:
            raise ValueError('size mismatch in copy_from_host')
        check(lib.hipdsp_memcpy_h2d(self.ctx.handle, ctypes.c_void_p(self.ptr),
                                    ctypes.c_void_p(a.ctypes.data), self.nbytes))

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(lib.hipdsp_memcpy_d2h(self.ctx.handle, ctypes.c_void_p(out.ctypes.data),
                                    ctypes.c_void_p(self.ptr), self.nbytes))
        return out

    def zero_(self):
        check(lib.hipdsp_memset(self.ctx.handle, ctypes.c_void_p(self.ptr), 0, self.nbytes))
        return self

    def view(self, offset_elems, shape):
        """A non-owning sub-block starting `offset_elems` elements into this array."""
        v = DeviceArray(self.ctx, shape, self.dtype,
                        ptr=self.ptr + int(offset_elems)*self.dtype.itemsize, owner=self)
        if v.ptr + v.nbytes > self.ptr + self.nbytes:
            raise ValueError('view exceeds the parent array')
        return v

    def _release(self):
        lib.hipdsp_free(self.ctx.handle, ctypes.c_void_p(self.ptr))


def _p(x):
    """Device pointer of a DeviceArray, a torch tensor, an int, or None."""
    if x is None:
        return ctypes.c_void_p(0)
    if isinstance(x, DeviceArray):
        return ctypes.c_void_p(x.ptr)
    if hasattr(x, 'data_ptr'):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(int(x))


class _Plan(_Handle):
    """A device-resident plan behind hipdsp_<_prefix>_create / _set / _set_host / _upload / _destroy (hip_dsp.h).  A
    subclass names the prefix and turns the arguments of set() and set_host() into the C arguments (_args)."""

    _prefix = None

    def __init__(self, ctx):
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(self._c('create')(ctx.handle, ctypes.byref(h)))
        self._h = h

    def _c(self, name):
        return getattr(lib, f'hipdsp_{self._prefix}_{name}')

    def _set(self, name, *args):
        """hipdsp_<prefix>_<name> with the C arguments _args() makes of `args`; _args() returns them behind the arrays
        they point into, which have to live until the call returns."""
        keep, cargs = self._args(*args)
        check(self._c(name)(self.ctx.handle, self._h, *cargs))
        return keep

    def upload(self):
        check(self._c('upload')(self.ctx.handle, self._h))

    def _destroy(self):
        self._c('destroy')(self.ctx.handle, self._h)


class SosPlan(_Plan):
    """Device-resident plan for one SOS table (see hipdsp_sosplan_* in hip_dsp.h)."""

    _prefix = 'sosplan'

    def __init__(self, ctx, sos=None):
        _Plan.__init__(self, ctx)
        self.n_sections = 0
        if sos is not None:
            self.set(sos)

    @staticmethod
    def _args(sos):
        sos = np.ascontiguousarray(sos, dtype=np.float64)
        if sos.ndim != 2 or sos.shape[1] != 6:
            raise ValueError('sos must be shape (n_sections, 6)')
        return sos, (ctypes.c_void_p(sos.ctypes.data), len(sos))

    def set(self, sos):
        self.n_sections = len(self._set('set', sos))

    def set_host(self, sos):
        self.n_sections = len(self._set('set_host', sos))

    def info(self):
        w = ctypes.c_int64()
        e = ctypes.c_int()
        check(lib.hipdsp_sosplan_info(self.ctx.handle, self._h, ctypes.byref(w), ctypes.byref(e)))
        return int(w.value), int(e.value)


class FirPlan(_Plan):
    """Device-resident taps and thresholds of up to 16 FIR kernels of one length (hipdsp_firplan_* in hip_dsp.h)."""

    _prefix = 'firplan'

    def __init__(self, ctx, taps=None, thresholds=None):
        _Plan.__init__(self, ctx)
        self.n_kernels = self.n_taps = 0
        if taps is not None:
            self.set(taps, thresholds)

    @staticmethod
    def _args(taps, thresholds):
        taps = np.ascontiguousarray(np.atleast_2d(np.asarray(taps, dtype=np.float64)))
        if taps.ndim != 2:
            raise ValueError('taps must be shape (n_kernels, n_taps)')
        thr = thresholds
        if thr is not None:
            thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, dtype=np.float64), (len(taps),)))
        return (taps, thr), (ctypes.c_void_p(taps.ctypes.data), taps.shape[0], taps.shape[1],
                             ctypes.c_void_p(thr.ctypes.data if thr is not None else 0))

    def set(self, taps, thresholds=None):
        self.n_kernels, self.n_taps = self._set('set', taps, thresholds)[0].shape

    def set_host(self, taps, thresholds=None):
        self.n_kernels, self.n_taps = self._set('set_host', taps, thresholds)[0].shape


class TmplPlan(_Plan):
    """Device-resident taps of up to 16 spectrogram templates of one shape (Tt frames, Fb bins), raw or normalised
    (hipdsp_tmplplan_* in hip_dsp.h)."""

    _prefix = 'tmplplan'

    def __init__(self, ctx, templates=None, normalize=True):
        _Plan.__init__(self, ctx)
        self.n_templates = self.rows = self.cols = 0
        self.normalize = bool(normalize)
        if templates is not None:
            self.set(templates, normalize)

    @staticmethod
    def _args(templates, normalize):
        t = _templates(templates)
        return t, (ctypes.c_void_p(t.ctypes.data), t.shape[0], t.shape[1], t.shape[2], int(bool(normalize)))

    def set(self, templates, normalize=True):
        self.n_templates, self.rows, self.cols = self._set('set', templates, normalize).shape
        self.normalize = bool(normalize)

    def set_host(self, templates, normalize=True):
        self.n_templates, self.rows, self.cols = self._set('set_host', templates, normalize).shape
        self.normalize = bool(normalize)


def _templates(templates):
    t = np.asarray(templates, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3:
        raise ValueError('templates must be shape (n_templates, frames, bins)')
    return np.ascontiguousarray(t)


def template_prepare(templates, normalize=True):
    """The taps the matrix core multiplies by, float32 (K, Tt, Fb), their sums H0 and centred square sums Q, float64
    (hipdsp_template_prepare_host: no context, no device)."""
    t = _templates(templates)
    taps = np.empty(t.shape, np.float32)
    h0, q = np.empty(len(t)), np.empty(len(t))
    check(lib.hipdsp_template_prepare_host(ctypes.c_void_p(t.ctypes.data), t.shape[0], t.shape[1], t.shape[2],
                                           int(bool(normalize)), ctypes.c_void_p(taps.ctypes.data),
                                           ctypes.c_void_p(h0.ctypes.data), ctypes.c_void_p(q.ctypes.data)))
    return taps, h0, q


class Comm(_Handle):
    """RCCL communicator behind the C ABI (hipdsp_comm_*): rank 0 calls
    `Comm.unique_id()` and ships the 128 bytes to the other ranks."""

    def __init__(self, ctx, unique_id, rank, nranks):
        self.ctx = ctx
        self.rank, self.nranks = int(rank), int(nranks)
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        h = ctypes.c_void_p()
        check(lib.hipdsp_comm_create(ctx.handle, buf, self.rank, self.nranks, ctypes.byref(h)))
        self._h = h

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        check(lib.hipdsp_comm_unique_id(buf))
        return buf.raw

    def allgather(self, send, recv, count_per_rank):
        check(lib.hipdsp_allgather_f32(self.ctx.handle, self._h, _p(send), _p(recv),
                                       int(count_per_rank)))

    def _destroy(self):
        lib.hipdsp_comm_destroy(self.ctx.handle, self._h)


def _plan(plan):
    return plan.handle if plan is not None else ctypes.c_void_p(0)


# How often each hot-path entry point has been called in this process: tests (and integrators) read these to see
# WHICH launches a BufferedData.recompute_all() turned into (e.g. that the fused forward sweep ran).
launches = {}


def _count(name):
    launches[name] = launches.get(name, 0) + 1


@contextlib.contextmanager
def _result(ctx, out, shape, dtype):
    """The device array a call writes its result into: `out` when the caller gave one (it is filled and returned as it
    is), else a temporary of `shape` (None: nothing to write, no array) that is read back inside the block and freed
    at its end, also when the call fails."""
    dev = out
    if out is None and shape is not None:
        dev = DeviceArray(ctx, shape, dtype)
    try:
        yield dev
    finally:
        if out is None and dev is not None:
            dev.free()


def sosfilt(ctx, plan, x, x_pitch, y, y_pitch, channels, frames, skip=0):
    _count('sosfilt')
    check(lib.hipdsp_sosfilt(ctx.handle, _plan(plan), _p(x), int(x_pitch), _p(y), int(y_pitch),
                             int(channels), int(frames), int(skip)))


def envelope(ctx, plan, x, x_pitch, y, y_pitch, channels, frames, skip=0, rectify=True,
             gain=np.pi/2, clamp=True):
    _count('envelope')
    check(lib.hipdsp_envelope(ctx.handle, _plan(plan), _p(x), int(x_pitch), _p(y), int(y_pitch),
                              int(channels), int(frames), int(skip), int(bool(rectify)),
                              float(gain), int(bool(clamp))))


def envelope_multi(ctx, plans, x, x_pitch, y, y_pitch, channels, frames, skip=0, rectify=True,
                   gain=np.pi/2, clamp=True):
    """sosfiltfilt envelope over a cascade split into several plans (hipdsp_envelope_multi)."""
    arr = (ctypes.c_void_p*len(plans))(*[p.handle for p in plans])
    _count('envelope_multi')
    check(lib.hipdsp_envelope_multi(ctx.handle, arr, len(plans), _p(x), int(x_pitch), _p(y), int(y_pitch),
                                    int(channels), int(frames), int(skip), int(bool(rectify)), float(gain),
                                    int(bool(clamp))))


def sosfilt_envelope(ctx, fplan, eplan, x, x_pitch, yf, yf_pitch, env, env_pitch, channels, frames,
                     rectify=True, gain=np.pi/2, clamp=True, phase=0, env_first=0):
    """yf = sosfilt(fplan, x); env = sosfiltfilt(eplan, gain*|yf[env_first:]|) (hipdsp_sosfilt_envelope): env rows hold
    frames - env_first samples.  phase 0 = both sweeps, 1 = forward only, 2 = backward only (after phase 1 or
    chain_forward with the same env_first)."""
    _count('sosfilt_envelope:%d' % phase)
    check(lib.hipdsp_sosfilt_envelope(ctx.handle, fplan.handle, eplan.handle, _p(x), int(x_pitch),
                                      _p(yf), int(yf_pitch), _p(env), int(env_pitch), int(channels),
                                      int(frames), int(bool(rectify)), float(gain), int(bool(clamp)),
                                      int(phase), int(env_first)))


def chain_forward(ctx, fplan, eplan, x, x_pitch, yf, yf_pitch, channels, frames, nfft, hop, fs, psd,
                  frames_out, psd_pitch=0, rectify=True, gain=np.pi/2, db_out=None, spec_frames=0, spec_first=0,
                  env_first=0):
    """Band-pass + envelope state sweep + spectrogram of the filtered trace in one pass over x
    (nfft/hop 2048/1024, 2048/512, 1024/512, 1024/256, 512/256, 256/128; NotImplementedError otherwise).  The envelope follows with
    sosfilt_envelope(..., phase=2).  eplan None: no envelope (filter + spectrogram only); spec_frames: the
    spectrogram is handed only that many samples of the filtered trace (0 = all); spec_first: frame 0 of the
    spectrogram starts at that sample of the filtered trace (spec_frames counts from there); env_first: the envelope
    is that of yf[env_first:] (pass the same env_first to sosfilt_envelope(phase=2))."""
    _count('chain_forward')
    check(lib.hipdsp_chain_forward(ctx.handle, fplan.handle, _plan(eplan), _p(x), int(x_pitch), _p(yf),
                                   int(yf_pitch), int(channels), int(frames), int(bool(rectify)),
                                   float(gain), int(nfft), int(hop), float(fs), _p(psd), _p(db_out),
                                   int(frames_out), int(psd_pitch), int(spec_frames), int(spec_first),
                                   int(env_first)))


def chain_backward(ctx, eplan, yf, yf_pitch, env, env_pitch, channels, frames, nfft, hop, fs, psd, frames_out,
                   psd_pitch=0, rectify=True, gain=np.pi/2, clamp=True):
    """Envelope backward sweep + the odd spectrogram frames (after chain_forward with the context option
    "chain_split_frames"; hipdsp_chain_backward)."""
    check(lib.hipdsp_chain_backward(ctx.handle, eplan.handle, _p(yf), int(yf_pitch), _p(env), int(env_pitch),
                                    int(channels), int(frames), int(bool(rectify)), float(gain), int(bool(clamp)),
                                    int(nfft), int(hop), float(fs), _p(psd), int(frames_out), int(psd_pitch)))


def chain_backward_plan(ctx, eplan, channels, frames):
    """(first_border, segment_frames, n_segments) of chain_backward: its internal borders are
    first_border - s*segment_frames, s = 0 ... n_segments - 2 (hipdsp_chain_backward_plan)."""
    fb, seg, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    check(lib.hipdsp_chain_backward_plan(ctx.handle, eplan.handle, int(channels), int(frames), ctypes.byref(fb),
                                         ctypes.byref(seg), ctypes.byref(n)))
    return int(fb.value), int(seg.value), int(n.value)


def chain_plan(ctx, fplan, eplan, channels, frames):
    """(segment_frames, n_segments) of chain_forward for this shape (hipdsp_chain_plan)."""
    seg, n = ctypes.c_int64(), ctypes.c_int()
    check(lib.hipdsp_chain_plan(ctx.handle, fplan.handle, _plan(eplan), int(channels), int(frames),
                                ctypes.byref(seg), ctypes.byref(n)))
    return int(seg.value), int(n.value)


def spectrogram(ctx, x, x_pitch, channels, frames, nfft, hop, fs, out, frames_out, db_out=None,
                out_pitch=0):
    _count('spectrogram')
    check(lib.hipdsp_spectrogram(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames),
                                 int(nfft), int(hop), float(fs), _p(out), _p(db_out),
                                 int(frames_out), int(out_pitch)))


def decibel(ctx, p, out, n, ref_power=1.0, min_power=1e-20):
    check(lib.hipdsp_decibel(ctx.handle, _p(p), _p(out), int(n), float(ref_power),
                             float(min_power)))


def decibel_image(ctx, spec_tf, image_ft, frames, nfreq, ref_power=1.0, min_power=1e-20):
    check(lib.hipdsp_decibel_image(ctx.handle, _p(spec_tf), _p(image_ft), int(frames), int(nfreq),
                                   float(ref_power), float(min_power)))


def decibel_image_decimate(ctx, spec_tf, image_fc, frames, nfreq, start, stop, step, ref_power=1.0,
                           min_power=1e-20):
    check(lib.hipdsp_decibel_image_decimate(ctx.handle, _p(spec_tf), _p(image_fc), int(frames), int(nfreq),
                                            int(start), int(stop), int(step), float(ref_power),
                                            float(min_power)))


def pack(ctx, src_tc, dst, dst_pitch, frames, channels, src_dtype=np.float64):
    fn = lib.hipdsp_pack_f64 if np.dtype(src_dtype) == np.float64 else lib.hipdsp_pack_f32
    check(fn(ctx.handle, _p(src_tc), _p(dst), int(dst_pitch), int(frames), int(channels)))


def unpack(ctx, src, src_pitch, dst_tc, frames, channels):
    check(lib.hipdsp_unpack_f64(ctx.handle, _p(src), int(src_pitch), _p(dst_tc), int(frames),
                                int(channels)))


def unpack_spectrum(ctx, src, dst_tcf, frames, channels, nfreq, src_pitch=0):
    check(lib.hipdsp_unpack_spectrum_f64(ctx.handle, _p(src), int(src_pitch), _p(dst_tcf),
                                         int(frames), int(channels), int(nfreq)))


def channel_mean(ctx, x, x_pitch, channels, start, n, out, heterodyne_cycles_per_sample=0.0):
    arr = (ctypes.c_int*len(channels))(*[int(c) for c in channels])
    check(lib.hipdsp_channel_mean(ctx.handle, _p(x), int(x_pitch), arr, len(channels), int(start),
                                  int(n), float(heterodyne_cycles_per_sample), _p(out)))


CREF_MEAN, CREF_MEDIAN = 0, 1                # HIPDSP_CREF_MEAN / _MEDIAN
CREF_TILE = 1024                             # HIPDSP_CREF_TILE: frames per workgroup up to 16 reference channels a group
CREF_TILES = (32, 512, 1024)                 # ... and the tiles of the other kernels: means beyond 64, up to 64
CREF_MODES = {'mean': CREF_MEAN, 'median': CREF_MEDIAN}


def common_reference(ctx, x, x_pitch, y, y_pitch, channels, frames, group, use=None, mode='mean'):
    """hipdsp_common_reference: y[c] = x[c] - mean or median over the reference channels of c's group.  `group`: one
    id in [0, channels) or -1 (pass through) per channel; `use`: 0/1 per channel (None: all 1); `mode`: 'mean',
    'median' or the C constant."""
    _count('common_reference')
    garr = (ctypes.c_int*len(group))(*[int(g) for g in group])
    uarr = None if use is None else (ctypes.c_ubyte*len(use))(*[1 if u else 0 for u in use])
    check(lib.hipdsp_common_reference(ctx.handle, _p(x), int(x_pitch), _p(y), int(y_pitch), int(channels), int(frames),
                                      garr, uarr, int(CREF_MODES.get(mode, mode))))


def stride_copy(ctx, x, n, step, out):
    check(lib.hipdsp_stride_copy(ctx.handle, _p(x), int(n), int(step), _p(out)))


def max_nonneg(ctx, x, n, out):
    check(lib.hipdsp_max_nonneg(ctx.handle, _p(x), int(n), _p(out)))


def band_order_stats(ctx, x, rows, cols, row_stride, rank, out2):
    check(lib.hipdsp_band_order_stats(ctx.handle, _p(x), int(rows), int(cols), int(row_stride), int(rank),
                                      _p(out2)))


def unwrap(ctx, x, x_pitch, channels, frames, thresh, y, y_pitch, ampl_max=1.0, clips=False, down_scale=True):
    check(lib.hipdsp_unwrap(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames), float(thresh),
                            float(ampl_max), int(bool(clips)), int(bool(down_scale)), _p(y), int(y_pitch)))


def pcm_unpack(ctx, pcm_tc, sample_bytes, frames, channels, scale, dst, dst_pitch):
    check(lib.hipdsp_pcm_unpack(ctx.handle, _p(pcm_tc), int(sample_bytes), int(frames), int(channels),
                                float(scale), _p(dst), int(dst_pitch)))


def pcm_minmax(ctx, pcm_tc, sample_bytes, frames, channels, step, scale, out_rc, out_pitch,
               unwrap_thresh=0.0, ampl_max=1.0, clips=False, down_scale=False):
    """Full-trace overview of a block of interleaved PCM (hipdsp_pcm_minmax): out_rc gets float64
    (2*ceil(frames/step), channels) rows of min, max, min, ... with row pitch out_pitch elements."""
    check(lib.hipdsp_pcm_minmax(ctx.handle, _p(pcm_tc), int(sample_bytes), int(frames), int(channels), int(step),
                                float(scale), float(unwrap_thresh), float(ampl_max), int(bool(clips)),
                                int(bool(down_scale)), _p(out_rc), int(out_pitch)))


class HostBuffer(_Memory):
    """Page-locked host memory (hipdsp_host_malloc) seen as a NumPy uint8 array: the source of
    hipdsp_memcpy_h2d_async."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(lib.hipdsp_host_malloc(ctx.handle, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value or 0
        if self.nbytes:
            self.array = np.ctypeslib.as_array((ctypes.c_uint8*self.nbytes).from_address(self.ptr))
        else:
            self.array = np.zeros(0, dtype=np.uint8)

    def _release(self):
        self.array = None
        lib.hipdsp_host_free(self.ctx.handle, ctypes.c_void_p(self.ptr))


def memcpy_h2d_async(ctx, dst, host_src, nbytes):
    """Copy `nbytes` from page-locked host memory (a HostBuffer or its address) to the device, ordered on
    the context's stream and NOT waited for."""
    src = host_src.ptr if isinstance(host_src, HostBuffer) else int(host_src)
    check(lib.hipdsp_memcpy_h2d_async(ctx.handle, _p(dst), ctypes.c_void_p(src), int(nbytes)))


def minmax_decimate(ctx, x, x_pitch, channels, start, stop, step, out, out_pitch):
    check(lib.hipdsp_minmax_decimate(ctx.handle, _p(x), int(x_pitch), int(channels), int(start),
                                     int(stop), int(step), _p(out), int(out_pitch)))


def mean_spectrum_db(ctx, spec_tf, nfreq, i0, i1, out, ref_power=1.0, min_power=1e-20,
                     floor_db=-200.0):
    check(lib.hipdsp_mean_spectrum_db(ctx.handle, _p(spec_tf), int(nfreq), int(i0), int(i1),
                                      float(ref_power), float(min_power), float(floor_db), _p(out)))


def band_power(ctx, spec, spec_pitch, channels, frames, nfreq, bands, scale, out, db=False, ref_power=1.0,
               min_power=1e-20, out_pitch=0, out_band_pitch=0):
    """out[b, c, t] = scale * sum(spec[c, t, k0:k1]) for every (k0, k1) of `bands` (bin ranges; at most 16), float32,
    decibel of that with db (hipdsp_band_power): one pass over the bins the bands cover."""
    bands = [(int(k0), int(k1)) for k0, k1 in bands]
    k0 = (ctypes.c_int64*max(1, len(bands)))(*[b[0] for b in bands])
    k1 = (ctypes.c_int64*max(1, len(bands)))(*[b[1] for b in bands])
    _count('band_power')
    check(lib.hipdsp_band_power(ctx.handle, _p(spec), int(spec_pitch), int(channels), int(frames), int(nfreq), k0, k1,
                                len(bands), float(scale), int(bool(db)), float(ref_power), float(min_power), _p(out),
                                int(out_pitch), int(out_band_pitch)))


# the bits of hipdsp_spectral_features' mask, in bit order (HIPDSP_FEATURE_ in include/hip_dsp.h)
SPECTRAL_FEATURES = ('peak_bin_freq', 'peak_freq', 'peak_power', 'centroid', 'bandwidth', 'flatness', 'freq_low',
                     'freq_high')


def feature_mask(features):
    """The mask of a tuple of names of SPECTRAL_FEATURES (or of one name; a mask is checked and passed through);
    ValueError for an unknown name, an empty selection or bits above 7."""
    if isinstance(features, str):
        features = (features,)
    if isinstance(features, (int, np.integer)):
        mask = int(features)
    else:
        mask = 0
        for name in features:
            if name not in SPECTRAL_FEATURES:
                raise ValueError(f'unknown spectral feature {name!r}: one of {", ".join(SPECTRAL_FEATURES)}')
            mask |= 1 << SPECTRAL_FEATURES.index(name)
    if mask <= 0 or mask >= 1 << len(SPECTRAL_FEATURES):
        raise ValueError(f'spectral features: mask {mask:#x} selects nothing or bits above {len(SPECTRAL_FEATURES) - 1}')
    return mask


def feature_names(mask):
    """The names of a mask's features in the order their rows are stored (ascending bit order)."""
    return tuple(name for b, name in enumerate(SPECTRAL_FEATURES) if feature_mask(mask) >> b & 1)


def drop_ratio(drop_db):
    """10^(-drop_db/10), the fraction of the peak power that bounds freq_low / freq_high; ValueError for drop_db < 0."""
    drop_db = float(drop_db)
    if not drop_db >= 0:
        raise ValueError(f'drop_db must be >= 0, got {drop_db}')
    return 10.0**(-drop_db/10.0)


def spectral_features(ctx, spec, spec_pitch, channels, frames, nfreq, k0, k1, features, scale, out, min_power=0.0,
                      drop_db=10.0, out_pitch=0, out_feature_pitch=0):
    """out[j, c, t] = the j-th of the requested `features` (names of SPECTRAL_FEATURES or a mask; rows in bit order) of
    the bins [k0, k1) of spec[c, t], float32 (hipdsp_spectral_features): peak, centroid, bandwidth, flatness and extent
    of the band in one launch; NaN where the peak power is not finite or not above min_power."""
    mask, ratio = feature_mask(features), drop_ratio(drop_db)
    if not ratio > 0:
        raise ValueError(f'drop_db {drop_db} is too large: 10^(-drop_db/10) underflows')
    _count('spectral_features')
    check(lib.hipdsp_spectral_features(ctx.handle, _p(spec), int(spec_pitch), int(channels), int(frames), int(nfreq),
                                       int(k0), int(k1), mask, float(scale), float(min_power), ratio, _p(out),
                                       int(out_pitch), int(out_feature_pitch)))


EQ_MODES = {'divide': 0, 'subtract': 1}          # HIPDSP_EQ_ in include/hip_dsp.h


def eq_mode(mode):
    """HIPDSP_EQ_DIVIDE / HIPDSP_EQ_SUBTRACT of 'divide' / 'subtract' (or of the number itself); ValueError else."""
    if mode in EQ_MODES:
        return EQ_MODES[mode]
    if mode in (0, 1) and not isinstance(mode, bool):
        return int(mode)
    raise ValueError(f'unknown equalisation mode {mode!r}: one of {", ".join(EQ_MODES)}')


def bin_quantiles(ctx, spec, spec_pitch, channels, frames, nfreq, first, n_frames, frame_step, k0, k1, q, out_lo_hi,
                  out_count=None):
    """out_lo_hi[c, k - k0] = the two order statistics v[floor(q (n-1))], v[min(that + 1, n-1)] of the n non-NaN values
    spec[c, first + j*frame_step, k], j < n_frames, out_count[c, k - k0] = n (hipdsp_bin_quantiles): an exact radix
    select per column of the slab."""
    _count('bin_quantiles')
    check(lib.hipdsp_bin_quantiles(ctx.handle, _p(spec), int(spec_pitch), int(channels), int(frames), int(nfreq),
                                   int(first), int(n_frames), int(frame_step), int(k0), int(k1), float(q), _p(out_lo_hi),
                                   _p(out_count)))


def spec_equalize(ctx, spec, spec_pitch, out, out_pitch, channels, frames, nfreq, profile, profile_pitch=0, mode='divide'):
    """out[c, t, k] = spec[c, t, k] / profile[c, k] ('divide') or max(spec[c, t, k] - profile[c, k], 0) ('subtract') in
    numpy's float32 arithmetic (hipdsp_spec_equalize); out may be spec itself."""
    _count('spec_equalize')
    check(lib.hipdsp_spec_equalize(ctx.handle, _p(spec), int(spec_pitch), _p(out), int(out_pitch), int(channels),
                                   int(frames), int(nfreq), _p(profile), int(profile_pitch), eq_mode(mode)))


ADAPT_MODES = {'background': 0, 'divide': 1, 'subtract': 2, 'pcen': 3}          # HIPDSP_ADAPT_ in include/hip_dsp.h
ADAPT_CHUNK = 256                                                               # HIPDSP_ADAPT_CHUNK


def adapt_mode(mode):
    """HIPDSP_ADAPT_BACKGROUND ... HIPDSP_ADAPT_PCEN of the mode's name (or of the number itself); ValueError else."""
    if mode in ADAPT_MODES:
        return ADAPT_MODES[mode]
    if mode in (0, 1, 2, 3) and not isinstance(mode, bool):
        return int(mode)
    raise ValueError(f'unknown adaptive mode {mode!r}: one of {", ".join(ADAPT_MODES)}')


def adapt_scratch_bytes(channels, frames, nfreq):
    """The context scratch one spec_adapt call of these sizes uses (Context.reserve() it before a capture)."""
    return 8*int(channels)*max(-(-int(frames)//ADAPT_CHUNK) - 1, 0)*int(nfreq)


def spec_adapt(ctx, spec, spec_pitch, out, out_pitch, channels, frames, nfreq, nbefore, smooth, mode='pcen', gain=0.98,
               bias=2.0, power=0.5, eps=1e-20):
    """out[c, i, k] = the spectrogram slab spec[c, nbefore + i, k] normalised by its running noise floor M (M_0 = x_0,
    M_t = (1 - smooth) M_(t-1) + smooth x_t along time, per channel and bin): M itself ('background'), x/(eps + M)
    ('divide'), max(x - M, 0) ('subtract') or (x/(eps + M)**gain + bias)**power - bias**power ('pcen'), float64 rounded
    once to float32 (hipdsp_spec_adapt); out may be spec itself when nbefore is 0."""
    _count('spec_adapt')
    check(lib.hipdsp_spec_adapt(ctx.handle, _p(spec), int(spec_pitch), _p(out), int(out_pitch), int(channels),
                                int(frames), int(nfreq), int(nbefore), float(smooth), adapt_mode(mode), float(gain),
                                float(bias), float(power), float(eps)))


def fir_bank(ctx, plan, x, x_pitch, channels, frames, first, step, n_out, out, rectify=False, out_pitch=0,
             out_kernel_pitch=0):
    """out[k, c, i] = sum_j taps[k, j] * x[c, first + i*step + (L-1)//2 - j] for every kernel of `plan`, x zero outside
    [0, frames); max(. - threshold[k], 0) with rectify (hipdsp_fir_bank): float32 products on the matrix cores."""
    _count('fir_bank')
    check(lib.hipdsp_fir_bank(ctx.handle, _plan(plan), _p(x), int(x_pitch), int(channels), int(frames), int(first),
                              int(step), int(n_out), int(bool(rectify)), _p(out), int(out_pitch),
                              int(out_kernel_pitch)))


def template_match(ctx, plan, spec, spec_pitch, channels, frames, nfreq, k0, first, n_out, out, db=False, ref_power=1.0,
                   min_power=1e-20, floor=-np.inf, pivot=0.0, min_std=0.0, out_pitch=0, out_template_pitch=0):
    """out[k, c, i] = the score of template k of `plan` against the window of Tt frames that starts at frame first + i
    of spec[c], bins [k0, k0 + Fb): the correlation coefficient (a normalised plan) or the plain sum of products; NaN
    where the window leaves [0, frames) or, normalised, is flatter than min_std (hipdsp_template_match): float32
    products on the matrix cores."""
    _count('template_match')
    check(lib.hipdsp_template_match(ctx.handle, _plan(plan), _p(spec), int(spec_pitch), int(channels), int(frames),
                                    int(nfreq), int(k0), int(first), int(n_out), int(bool(db)), float(ref_power),
                                    float(min_power), float(floor), float(pivot), float(min_std), _p(out),
                                    int(out_pitch), int(out_template_pitch)))


def region_stats(ctx, x, x_pitch, channels, frames, regions, out=None):
    """n, mean, std, min, max, argmin, argmax, 0 of x[c, start:stop] for every (start, stop) of `regions` (element ranges;
    at most 16) and every channel (hipdsp_region_stats): one pass over the regions on the device.  Returns the
    (len(regions), channels, 8) float64 host array -- those 64 bytes per region and channel are all that crosses to the
    host -- or, with `out` (a DeviceArray of that shape), fills it and returns it without any copy."""
    regions = [(int(a), int(b)) for a, b in regions]
    start = (ctypes.c_int64*max(1, len(regions)))(*[r[0] for r in regions])
    stop = (ctypes.c_int64*max(1, len(regions)))(*[r[1] for r in regions])
    with _result(ctx, out, (max(1, len(regions)), max(1, int(channels)), 8), np.float64) as dev:
        _count('region_stats')
        check(lib.hipdsp_region_stats(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames), start, stop,
                                      len(regions), _p(dev)))
        if out is not None:
            return out
        return dev.to_host()[:len(regions), :int(channels)] if int(channels) > 0 else np.zeros((len(regions), 0, 8))


SPECTRA_GROUP = 16                      # frames per work item of hipdsp_region_spectra (csrc/regionspectra.hip: SP_GROUP)


def region_spectra_into(ctx, x, x_pitch, channels, frames, regions, nfft, hop, step, fs, out, info, out_pitch=0):
    """One hipdsp_region_spectra launch, the results staying on the device: `out` (len(regions), nfft//2 + 1) float32
    and `info` (len(regions), 2) int64 are DeviceArrays; `regions` is an (n, 3) int64 host table of channel, start,
    stop."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    _count('region_spectra')
    check(lib.hipdsp_region_spectra(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames),
                                    tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(tab), int(nfft), int(hop),
                                    int(step), float(fs), _p(out), int(out_pitch), _p(info)))


def region_spectra(ctx, x, x_pitch, channels, frames, regions, nfft, hop, step, fs):
    """Welch PSDs of x[channel, start:stop:step] for every (channel, start, stop) of `regions` (hipdsp_region_spectra:
    Hann frames of `nfft` every `hop` decimated samples, mean removed, density scaling at rate `fs`).  Returns the
    (len(regions), nfft//2 + 1) float32 rows and the (len(regions), 2) int64 array of n_frames and np.argmax(row)."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    n, F = len(tab), int(nfft)//2 + 1
    if n == 0:
        region_spectra_into(ctx, x, x_pitch, channels, frames, tab, nfft, hop, step, fs, None, None)
        return np.zeros((0, F), dtype=np.float32), np.zeros((0, 2), dtype=np.int64)
    out = DeviceArray(ctx, (n, F), np.float32)
    info = DeviceArray(ctx, (n, 2), np.int64)
    try:
        region_spectra_into(ctx, x, x_pitch, channels, frames, tab, nfft, hop, step, fs, out, info)
        return out.to_host(), info.to_host()
    finally:
        out.free()
        info.free()


XCORR_TILE = 2048                       # samples of hipdsp_region_xcorr staged at a time (csrc/regionxcorr.hip: XC_TILE)
XCORR_CHUNK = 32*XCORR_TILE             # samples per work item of it (XC_CHUNK), anchored at the region's start
XCORR_LAGS = 9                          # consecutive lags a thread owns (XC_RL)
XCORR_MAX_LAG = 1024


def region_xcorr_scratch(regions, n_partners, max_lag):
    """Bytes of context scratch one hipdsp_region_xcorr call over these regions takes (the formula of include/hip_dsp.h)."""
    tab = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
    items = int(n_partners)*int(((tab[:, 2] - tab[:, 1] + XCORR_CHUNK - 1)//XCORR_CHUNK).sum())
    tables = -(-(48*(len(tab) + 1) + 4*int(n_partners))//8)*8          # the float64 rows behind them start at a multiple of 8
    return tables + 8*(4 + 3*XCORR_LAGS*(-(-(2*int(max_lag) + 1)//XCORR_LAGS)))*items


def region_xcorr_into(ctx, x, x_pitch, channels, frames, regions, partners, max_lag, out, info, out_pitch=0):
    """One hipdsp_region_xcorr launch, the results staying on the device: `out` (len(regions), len(partners), 2 max_lag +
    1) float32 and `info` (len(regions), len(partners), 4) float64 are DeviceArrays; `regions` is an (n, 3) int64 host
    table of channel, start, stop, `partners` a host list of channel ids."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    par = np.ascontiguousarray(partners, dtype=np.intc).reshape(-1)
    _count('region_xcorr')
    check(lib.hipdsp_region_xcorr(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames),
                                  tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(tab),
                                  par.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(par), int(max_lag), _p(out),
                                  int(out_pitch), _p(info)))


def region_xcorr(ctx, x, x_pitch, channels, frames, regions, partners, max_lag):
    """Correlation coefficients of x[channel, start:stop] with x[p, start+l:stop+l] for every (channel, start, stop) of
    `regions`, every p of `partners` and every lag l in [-max_lag, max_lag] (hipdsp_region_xcorr: np.corrcoef per lag, NaN
    where the shifted window leaves the row; a positive peak lag: the partner carries the waveform later).  Returns the
    (len(regions), len(partners), 2 max_lag + 1) float32 rows and the (len(regions), len(partners), 4) float64 array of
    the number of lags with a value, the position of the largest, std of the event window and of the partner's there."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    par = np.ascontiguousarray(partners, dtype=np.intc).reshape(-1)
    n, P, W = len(tab), len(par), 2*int(max_lag) + 1
    if n == 0 or P == 0:
        region_xcorr_into(ctx, x, x_pitch, channels, frames, tab, par, max_lag, None, None)
        return np.zeros((n, P, max(W, 0)), dtype=np.float32), np.zeros((n, P, 4), dtype=np.float64)
    if W < 1:
        raise ValueError('max_lag %d is negative' % int(max_lag))
    out = DeviceArray(ctx, (n, P, W), np.float32)
    info = DeviceArray(ctx, (n, P, 4), np.float64)
    try:
        region_xcorr_into(ctx, x, x_pitch, channels, frames, tab, par, max_lag, out, info)
        return out.to_host(), info.to_host()
    finally:
        out.free()
        info.free()


FILTER_CHUNK = 64                       # samples per hand-over of hipdsp_region_filtfilt (csrc/regionfilter.hip: RF_CHUNK),
#                                         anchored at the first sample of a region's extended sequence
FILTER_TILE = 64*FILTER_CHUNK           # samples per wave of it: 64 consecutive chunks staged together
CROSSINGS_CHUNK = 4096                  # samples per chunk of hipdsp_region_crossings (RC_CHUNK), anchored at the region's start


def region_filtfilt_scratch(regions, sos):
    """Bytes of context scratch one hipdsp_region_filtfilt call over these regions takes (the formula of
    include/hip_dsp.h)."""
    from .refine import padlen
    tab = np.asarray(regions, dtype=np.int64).reshape(-1, 3)
    sos = np.asarray(sos, dtype=np.float64).reshape(len(tab), -1, 6)
    ext = tab[:, 2] - tab[:, 1] + 2*padlen(sos)
    return int(1072*(len(tab) + 1) + 8*len(tab) + 8*ext.sum() +
               16*sos.shape[1]*(((ext + FILTER_CHUNK - 1)//FILTER_CHUNK).sum() + ((ext + FILTER_TILE - 1)//FILTER_TILE).sum()))


def region_filtfilt(ctx, x, x_pitch, y, y_pitch, channels, frames, regions, sos, clamp=False):
    """y[channel, start:stop] = float32(scipy.signal.sosfiltfilt(sos_r, x[channel, start:stop])) for every (channel,
    start, stop) of `regions` ((R, 3) int64, host) with the region's own filter sos[r] ((R, S, 6) float64, S 1 or 2), in
    one hipdsp_region_filtfilt call; nothing else of y is written; y may be x (with equal pitches)."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 3 or sos.shape[0] != len(tab) or sos.shape[2] != 6:
        raise ValueError('sos must be (len(regions), n_sections, 6), got %r' % (sos.shape,))
    _count('region_filtfilt')
    check(lib.hipdsp_region_filtfilt(ctx.handle, _p(x), int(x_pitch), _p(y), int(y_pitch), int(channels), int(frames),
                                     tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(tab),
                                     sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(sos.shape[1]),
                                     int(bool(clamp))))


POWER_ENVELOPE_CHUNK = 64               # samples per lane of hipdsp_power_envelope (csrc/powerenv.hip: PE_CHUNK), anchored at
#                                         the first sample of a row's extended sequence
POWER_ENVELOPE_TILE = 64*POWER_ENVELOPE_CHUNK     # samples per wave of it


def power_envelope_scratch(channels, frames, n_sections, padlen):
    """Bytes of context scratch one hipdsp_power_envelope call takes (the formula of include/hip_dsp.h)."""
    tiles = -(-(int(frames) + 2*int(padlen))//POWER_ENVELOPE_TILE)
    return int(channels)*(32*int(n_sections)*65*tiles + 4)


def power_envelope(ctx, plan, x, x_pitch, channels, frames, y, y_pitch, first=0, step=1, n_out=None, gain=4.0, root=True):
    """y[c, j] = float32(gain max(sosfiltfilt(plan, x[c]**2)[first + j step], 0)), j < n_out, and its root with `root`:
    one hipdsp_power_envelope call (the reference's envelope(), songdetector.py:57-69, is the defaults with its step).
    n_out None: every grid sample of the row.  Returns n_out."""
    if n_out is None:
        n_out = max(0, -(-(int(frames) - int(first))//int(step))) if step >= 1 else 0
    _count('power_envelope')
    check(lib.hipdsp_power_envelope(ctx.handle, _plan(plan), _p(x), int(x_pitch), int(channels), int(frames), int(first),
                                    int(step), int(n_out), float(gain), int(bool(root)), _p(y), int(y_pitch)))
    return int(n_out)


def region_crossings(ctx, x, x_pitch, channels, frames, regions, thresholds, out=None):
    """n, number above, first above, one past the last above, max, argmax, 0, 0 of x[channel, start:stop] for every
    (channel, start, stop) of `regions` against the region's own threshold (hipdsp_region_crossings; positions in the
    row, -1 for none).  Returns the (len(regions), 8) float64 host array, or fills `out` (a DeviceArray of that shape)
    and returns it without any copy."""
    tab = np.ascontiguousarray(regions, dtype=np.int64).reshape(-1, 3)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(tab),)))
    if len(thr) == 0:
        thr = np.zeros(1)
    with _result(ctx, out, (len(tab), 8) if len(tab) else None, np.float64) as dev:
        _count('region_crossings')
        check(lib.hipdsp_region_crossings(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames),
                                          tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          thr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(tab), _p(dev)))
        if out is not None:
            return out
        return dev.to_host() if dev is not None else np.zeros((0, 8))


def detect_events_into(ctx, x, x_pitch, channels, start, stop, thresholds, min_gap, min_len, capacity, events, counts,
                       events_pitch=0):
    """One hipdsp_detect_events launch, everything staying on the device: `events` (channels, capacity, 2) int64 (None with
    capacity 0) and `counts` (channels,) int64 are DeviceArrays; `thresholds` is a number for all channels or a
    DeviceArray of `channels` float32."""
    per_channel = isinstance(thresholds, DeviceArray) or hasattr(thresholds, 'data_ptr')
    _count('detect_events')
    check(lib.hipdsp_detect_events(ctx.handle, _p(x), int(x_pitch), int(channels), int(start), int(stop),
                                   _p(thresholds if per_channel else None), 0.0 if per_channel else float(thresholds),
                                   int(min_gap), int(min_len), int(capacity), _p(events), int(events_pitch), _p(counts)))


def detect_events(ctx, x, x_pitch, channels, start, stop, thresholds, min_gap, min_len, capacity=None):
    """Threshold events of x[c, start:stop] (hipdsp_detect_events): runs of samples > threshold, runs at most `min_gap`
    samples apart merged, merged events shorter than `min_len` dropped.  `thresholds` is one number or one per channel.
    Returns a list of `channels` (K, 2) int64 arrays of (onset, offset) row positions, ascending.  With capacity=None
    the call starts with room for 4096 events per channel and is repeated once, with the largest count, if a channel
    has more; with a number, at most that many events per channel come back.  Only the counts and the written pairs
    cross to the host."""
    channels = int(channels)
    if channels <= 0:
        return []
    thr = np.asarray(thresholds, dtype=np.float64)
    dthr = None
    if thr.ndim > 0:
        if thr.shape != (channels,):
            raise ValueError('thresholds: one value or one per channel')
        dthr = DeviceArray.from_host(ctx, thr.astype(np.float32))
    cap = 4096 if capacity is None else int(capacity)
    dcounts = DeviceArray(ctx, (channels,), np.int64)
    try:
        while True:
            dev = DeviceArray(ctx, (channels, cap, 2), np.int64) if cap > 0 else None
            detect_events_into(ctx, x, x_pitch, channels, start, stop, dthr if dthr is not None else float(thr), min_gap,
                               min_len, cap, dev, dcounts)
            counts = dcounts.to_host()
            most = int(counts.max())
            if capacity is None and most > cap:
                dev.free()
                cap = most
                continue
            out = []
            for c in range(channels):
                k = min(int(counts[c]), cap)
                out.append(dev.view(c*cap*2, (k, 2)).to_host() if k > 0 else np.zeros((0, 2), dtype=np.int64))
            if dev is not None:
                dev.free()
            return out
    finally:
        dcounts.free()
        if dthr is not None:
            dthr.free()


PEAKS_CHUNK = 4096                      # samples per chunk of hipdsp_find_peaks (csrc/peaks.hip: PK_CHUNK), anchored at start
PEAKS_BLOCKS = (64, 4096, 262144)       # samples per entry of the three levels of its min/max table


def find_peaks_into(ctx, x, x_pitch, channels, start, stop, borders, wlen, capacity, peaks, props, counts, peaks_pitch=0,
                    props_pitch=0):
    """One hipdsp_find_peaks launch, everything staying on the device: `peaks` (channels, capacity) int64 (None with
    capacity 0), `props` (channels, capacity, 4) float64 or None and `counts` (channels,) int64 are DeviceArrays;
    `borders` is hmin, hmax, tmin, tmax, pmin, pmax for all channels (-inf / +inf: open) or a DeviceArray
    (channels, 6) of float64."""
    per_channel = isinstance(borders, DeviceArray) or hasattr(borders, 'data_ptr')
    by_value = [0.0]*6 if per_channel else [float(b) for b in borders]
    if len(by_value) != 6:
        raise ValueError('borders: hmin, hmax, tmin, tmax, pmin, pmax')
    _count('find_peaks')
    check(lib.hipdsp_find_peaks(ctx.handle, _p(x), int(x_pitch), int(channels), int(start), int(stop),
                                _p(borders if per_channel else None), *by_value, int(wlen), int(capacity), _p(peaks),
                                int(peaks_pitch), _p(props), int(props_pitch), _p(counts)))


def find_peaks(ctx, x, x_pitch, channels, start, stop, conditions, wlen=0, props=True, capacity=None):
    """Peaks of x[c, start:stop] (hipdsp_find_peaks: scipy.signal.find_peaks with height, threshold, prominence and
    wlen; no distance, width or plateau_size).  `conditions` is hmin, hmax, tmin, tmax, pmin, pmax (-inf / +inf: an
    open border) for all channels, or (channels, 6) of them; `wlen` is in samples, 0 or 1 the whole range.  Returns a
    list of `channels` (positions, properties) pairs: (K,) int64 row positions, ascending, and (K, 4) float64 of
    height, prominence, left base, right base (None with props=False).  With capacity=None a first call counts only
    and a second one stores with the largest count as capacity; with a number, at most that many peaks per channel
    come back from one call.  Only the counts and the written entries cross to the host."""
    channels = int(channels)
    if channels <= 0:
        return []
    cond = np.asarray(conditions, dtype=np.float64)
    if cond.shape not in ((6,), (channels, 6)):
        raise ValueError('conditions: six borders, or six per channel')
    dcond = DeviceArray.from_host(ctx, cond) if cond.ndim == 2 else None
    borders = dcond if dcond is not None else cond
    dcounts = DeviceArray(ctx, (channels,), np.int64)
    dpeaks = dprops = None
    try:
        if capacity is None:
            find_peaks_into(ctx, x, x_pitch, channels, start, stop, borders, wlen, 0, None, None, dcounts)
            cap = int(dcounts.to_host().max())
        else:
            cap = int(capacity)
        if cap > 0:
            dpeaks = DeviceArray(ctx, (channels, cap), np.int64)
            dprops = DeviceArray(ctx, (channels, cap, 4), np.float64) if props else None
        if cap > 0 or capacity is not None:
            find_peaks_into(ctx, x, x_pitch, channels, start, stop, borders, wlen, cap, dpeaks, dprops, dcounts)
        counts = dcounts.to_host()
        out = []
        for c in range(channels):
            k = min(int(counts[c]), cap)
            pos = dpeaks.view(c*cap, (k,)).to_host() if k > 0 else np.zeros(0, dtype=np.int64)
            pr = None
            if props:
                pr = dprops.view(c*cap*4, (k, 4)).to_host() if k > 0 else np.zeros((0, 4))
            out.append((pos, pr))
        return out
    finally:
        for d in (dcounts, dcond, dpeaks, dprops):
            if d is not None:
                d.free()


def histogram(ctx, x, x_pitch, channels, start, stop, edges, out=None, out_pitch=0):
    """Amplitude histogram of x[c, start:stop] over the float64 `edges` (B + 1 finite, non-decreasing values, B <= 1024)
    for every channel (hipdsp_histogram): np.histogram's counts in slots 0 .. B-1, then the samples below edges[0],
    above edges[-1] and the NaNs.  Returns the (channels, B + 3) int64 host array -- all that crosses to the host -- or,
    with `out` (a DeviceArray of int64, rows `out_pitch` elements apart, 0 = B + 3), fills it and returns it."""
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    B, channels = len(e) - 1, int(channels)
    with _result(ctx, out, (max(1, channels), max(1, B) + 3), np.int64) as dev:
        _count('histogram')
        check(lib.hipdsp_histogram(ctx.handle, _p(x), int(x_pitch), channels, int(start), int(stop),
                                   e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), B, _p(dev), int(out_pitch)))
        if out is not None:
            return out
        return dev.to_host()[:channels] if channels > 0 else np.zeros((0, B + 3), dtype=np.int64)


def masked_stats(ctx, x, x_pitch, channels, start, stop, bounds, out=None):
    """Number, mean and std (ddof 0) of the samples of x[c, start:stop] with lo < x < hi, and a reserved 0, for every
    channel (hipdsp_masked_stats).  `bounds` is (channels, 3) float64 -- lo, hi, pivot per channel -- on the host or a
    DeviceArray.  Returns the (channels, 4) float64 host array, or, with `out` (a DeviceArray of that shape), fills it
    and returns it without any copy."""
    channels = int(channels)
    dbounds = bounds
    if not isinstance(bounds, DeviceArray):
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        if b.shape != (channels, 3):
            raise ValueError('bounds: (channels, 3) values lo, hi, pivot')
        dbounds = DeviceArray.from_host(ctx, b if channels > 0 else np.zeros((1, 3)))
    try:
        with _result(ctx, out, (max(1, channels), 4), np.float64) as dev:
            _count('masked_stats')
            check(lib.hipdsp_masked_stats(ctx.handle, _p(x), int(x_pitch), channels, int(start), int(stop), _p(dbounds),
                                          _p(dev)))
            if out is not None:
                return out
            return dev.to_host()[:channels] if channels > 0 else np.zeros((0, 4))
    finally:
        if dbounds is not bounds:
            dbounds.free()


def memcpy2d(ctx, dst, dst_pitch_bytes, src, src_pitch_bytes, width_bytes, height):
    check(lib.hipdsp_memcpy2d_d2d(ctx.handle, _p(dst), int(dst_pitch_bytes), _p(src),
                                  int(src_pitch_bytes), int(width_bytes), int(height)))


def synth(ctx, x, x_pitch, channels, frames, rate, seed, c0=0, c_total=None):
    check(lib.hipdsp_synth(ctx.handle, _p(x), int(x_pitch), int(channels), int(frames),
                           float(rate), int(seed), int(c0),
                           int(c_total if c_total is not None else channels)))
