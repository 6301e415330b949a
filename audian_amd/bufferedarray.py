"""Minimal ring-buffer base class standing in for ``audioio.BufferedArray``.

audioio is not part of the reference tree (``src/audian/buffereddata.py:7`` imports
it), so this module supplies the contract the ``BufferedData`` surface relies on,
derived from the reference's call sites:

  attributes  rate, channels, frames, shape, ndim, size, offset, buffer, bufferframes,
              backframes, follow, ampl_min, ampl_max, unit, buffer_changed, verbose
  methods     __len__ (frames), __getitem__ (moves the buffer on demand,
              data.py:112), update_time(t0, t1) (data.py:227), update_buffer,
              move_buffer(offset, nframes) (buffereddata.py:87: keeps the overlapping
              part, calls load_buffer for what is missing, sets buffer_changed),
              allocate_buffer() (buffereddata.py:114), reload_buffer() (:115),
              load_buffer(offset, nframes, view) -- the subclass hook.

It is written from that contract, not from audioio's source.
"""

import numpy as np


def _host_region_stats(block):
    """The eight slots of hipdsp_region_stats for every channel of a (frames, channels[, F]) float64 block, with
    numpy itself: (channels, 8)."""
    channels = block.shape[1]
    out = np.zeros((channels, 8))
    out[:, 0] = block.size//max(1, channels)
    if block.size == 0:
        out[:, 1:5] = np.nan
        out[:, 5:7] = -1
        return out
    with np.errstate(all='ignore'):
        for c in range(channels):
            v = block[:, c].reshape(-1)
            out[c, 1:7] = np.mean(v), np.std(v), np.min(v), np.max(v), np.argmin(v), np.argmax(v)
    return out


class BufferedArray(object):

    def __init__(self, verbose=0):
        self.rate = 0.0
        self.channels = 0
        self.frames = 0
        self.shape = (0, 0)
        self.ndim = 2
        self.size = 0
        self.offset = 0
        self.bufferframes = 0
        self.backframes = 0
        self.follow = 0
        self.ampl_min = -1.0
        self.ampl_max = 1.0
        self.unit = ''
        self.verbose = verbose
        self.buffer_changed = np.zeros(0, dtype=bool)
        self.buffer = np.zeros((0, 0))
        self.unwrap_thresh = 0.0
        self.unwrap_clips = False
        self.unwrap_down_scale = True
        self.unwrap_ampl = 1.0

    def __len__(self):
        return self.frames

    # -- unwrap of clipped recordings (audioio: BufferedArray.set_unwrap / unwrap()) -----------
    def set_unwrap(self, thresh, clips=False, down_scale=True, unit=''):
        """Arm audioio's unwrap() for every slab this loader reads from now on, as the reference does
        right after opening the recording (``self.data.set_unwrap(unwrap, unwrap_clip, False, unit)``,
        src/audian/data.py:180; CLI ``-u`` / ``-U``, src/audian/audian.py:1485-1512).  ``thresh`` <= 1e-3
        turns it off.  Without clipping and down-scaling the amplitude range doubles.  audioio's source
        is not available here: restated from its documentation -- UNVERIFIED against audioio (parity
        unpinned; `unit` is accepted and ignored).  Like audioio's per-buffer call, every slab a loader
        reads is unwrapped on its own, starting from zero offset at its first frame: a buffer move that
        keeps an overlap and loads the rest can therefore carry different offsets in the kept and the new
        part of a recording that is wrapped at the seam (tests/test_gpu_facade.py pins exactly this
        behaviour, not audioio's)."""
        self.unwrap_ampl = float(self.ampl_max if self.unwrap_thresh <= 1e-3 else self.unwrap_ampl)
        self.unwrap_thresh = float(thresh)
        self.unwrap_clips = bool(clips)
        self.unwrap_down_scale = bool(down_scale)
        if self.unwrap_thresh > 1e-3:
            grow = 1.0 if (self.unwrap_clips or self.unwrap_down_scale) else 2.0
            self.ampl_min, self.ampl_max = -grow*self.unwrap_ampl, grow*self.unwrap_ampl
            if getattr(self, 'view', False):
                self.view = False              # the buffer must be this loader's own copy now
                self.buffer = np.zeros((0, self.channels))
                self.move_buffer(self.offset, self.bufferframes)
                return
        else:
            self.ampl_min, self.ampl_max = -self.unwrap_ampl, self.unwrap_ampl
        if len(self._buf()) > 0:
            self.reload_buffer()

    def _apply_unwrap(self, buffer):
        """Unwrap a freshly loaded (frames, channels) slab in place (device kernels: hipdsp_unwrap);
        like audioio, every slab starts again from zero offset."""
        if self.unwrap_thresh <= 1e-3 or len(buffer) == 0:
            return
        from . import hipdsp
        ctx = hipdsp.default_context()
        n, nch = buffer.shape
        host = np.ascontiguousarray(buffer, dtype=np.float32)
        up = hipdsp.DeviceArray.from_host(ctx, host)
        planar = hipdsp.DeviceArray(ctx, (nch, n), np.float32)
        hipdsp.pack(ctx, up, planar, n, n, nch, src_dtype=np.float32)
        out = hipdsp.DeviceArray(ctx, (nch, n), np.float32)
        hipdsp.unwrap(ctx, planar, n, nch, n, self.unwrap_thresh, out, n, ampl_max=self.unwrap_ampl,
                      clips=self.unwrap_clips, down_scale=self.unwrap_down_scale)
        tmp = hipdsp.DeviceArray(ctx, (n, nch), np.float64)
        hipdsp.unpack(ctx, out, n, tmp, n, nch)
        buffer[:, :] = tmp.to_host()
        for d in (up, planar, out, tmp):
            d.free()

    # -- subclass hook ---------------------------------------------------------
    def load_buffer(self, offset, nframes, buffer):
        raise NotImplementedError

    # -- buffer management -----------------------------------------------------
    def _buf(self):
        """The buffer as stored (subclasses with a lazy host copy return it unsynced)."""
        return self.buffer

    def _prepare_keep(self, a, b):
        """Hook: frames [a, b) of the current buffer are about to be copied.  Returns False when
        the host copy of that range is not worth copying (a subclass keeps it elsewhere)."""
        return True

    def _blank(self, nframes):
        return np.zeros((int(nframes),) + tuple(self.shape[1:]))

    def allocate_buffer(self, nframes=None, force=False):
        """Size ``buffer`` to ``bufferframes`` frames (clipped to the data)."""
        if nframes is None:
            nframes = self.bufferframes
        if self.offset + nframes > self.frames:
            nframes = max(0, self.frames - self.offset)
        cur = self._buf()
        if force or nframes != len(cur) or tuple(cur.shape[1:]) != tuple(self.shape[1:]):
            self.buffer = self._blank(nframes)

    def reload_buffer(self):
        """Recompute the whole current buffer in place."""
        cur = self._buf()
        if len(cur) > 0:
            self.load_buffer(self.offset, len(cur), cur)
            self.buffer_changed[:] = True

    def move_buffer(self, offset, nframes):
        """Make the buffer cover frames [offset, offset + nframes): the part that
        overlaps the current buffer is kept, the rest comes from ``load_buffer``."""
        offset = int(max(0, offset))
        nframes = int(max(0, min(nframes, self.frames - offset)))
        old, old_off = self._buf(), self.offset
        if offset == old_off and nframes == len(old):
            return
        new = self._blank(nframes)
        keep0 = max(offset, old_off)
        keep1 = min(offset + nframes, old_off + len(old))
        if tuple(old.shape[1:]) != tuple(new.shape[1:]):
            keep0 = keep1 = 0
        todo = []
        if keep1 > keep0:
            if self._prepare_keep(keep0 - old_off, keep1 - old_off) is not False:
                new[keep0 - offset:keep1 - offset] = old[keep0 - old_off:keep1 - old_off]
            if keep0 > offset:
                todo.append((offset, keep0 - offset))
            if keep1 < offset + nframes:
                todo.append((keep1, offset + nframes - keep1))
        elif nframes > 0:
            todo.append((offset, nframes))
        self._adopt_buffer(new, offset, old_off, len(old), keep0, keep1)
        for r_offset, r_nframes in todo:
            self.load_buffer(r_offset, r_nframes,
                             self.buffer[r_offset - offset:r_offset - offset + r_nframes])
        self.buffer_changed[:] = True

    def _adopt_buffer(self, new, offset, old_offset, old_nframes, keep0, keep1):
        """Install the recycled buffer (hook for subclasses that mirror it elsewhere)."""
        self.buffer = new
        self.offset = offset

    def _buffer_position(self, start, stop):
        """Where to put the buffer so that frames [start, stop) are inside it."""
        nframes = max(self.bufferframes, stop - start)
        offset = start - self.backframes
        if offset + nframes > self.frames:
            offset = self.frames - nframes
        if offset < 0:
            offset = 0
        if offset + nframes > self.frames:
            nframes = self.frames - offset
        return offset, nframes

    def update_buffer(self, start, stop):
        start = int(max(0, start))
        stop = int(min(self.frames, stop))
        if stop <= start:
            return
        if start < self.offset or stop > self.offset + len(self.buffer):
            offset, nframes = self._buffer_position(start, stop)
            self.move_buffer(offset, nframes)

    def update_time(self, start, stop):
        self.update_buffer(int(start*self.rate), int(stop*self.rate) + 1)

    def region_stats(self, regions, channel=None):
        """n, mean, std, min, max, argmin, argmax, 0 of frames [start, stop) (absolute, inside the current buffer) for
        every (start, stop) of `regions`, with numpy on the host buffer: (R, channels, 8), or (R, 8) for one channel
        (BufferedData.region_stats is the same on the device mirror)."""
        n = len(self._buf())
        rel = [(int(a) - self.offset, int(b) - self.offset) for a, b in regions]
        if any(a < 0 or b > n or b < a for a, b in rel):
            raise IndexError('range outside the loaded buffer')
        res = np.zeros((len(rel), self.channels, 8))
        for k, (a, b) in enumerate(rel):
            res[k] = _host_region_stats(np.asarray(self.buffer[a:b], dtype=np.float64))
        return res[:, channel] if channel is not None else res

    def _event_arguments(self, thresholds, min_gap, min_duration, start, stop):
        """(per-channel float64 thresholds, min_gap frames, min_len frames, first, last relative to the buffer)."""
        a, b = self._trace_range('detect_events', start, stop)
        thr = np.asarray(thresholds, dtype=np.float64)
        if thr.ndim > 0 and thr.shape != (self.channels,):
            raise ValueError('thresholds: one value or one per channel')
        if min_gap < 0 or min_duration < 0:
            raise ValueError('negative min_gap or min_duration')
        # seconds to frames as songdetector.py:137-139 does it
        return np.broadcast_to(thr, (self.channels,)), int(min_gap*self.rate), int(min_duration*self.rate), a, b

    def detect_events(self, thresholds, min_gap=0.0, min_duration=0.0, start=None, stop=None):
        """Threshold events of frames [start, stop) (absolute, inside the current buffer; the whole buffer by default)
        of every channel, with numpy on the host buffer: runs of samples above the channel's threshold (float32
        comparison, as on the device mirror), runs less than or exactly `min_gap` seconds apart merged, events shorter
        than `min_duration` seconds dropped (events.py; BufferedData.detect_events is the same on the device mirror).
        Returns an Events object of absolute frame indices."""
        from .events import Events, host_detect_events
        thr, gap, length, a, b = self._event_arguments(thresholds, min_gap, min_duration, start, stop)
        buf = self.buffer
        pairs = [host_detect_events(buf[a:b, c], thr[c], gap, length, first=self.offset + a)
                 for c in range(self.channels)]
        return Events(pairs, self.rate, getattr(self, 'name', None))

    def _peak_border(self, value, what, open_border):
        """One side of a condition of find_peaks for every channel: None (open), a number or one per channel."""
        if value is None:
            return np.full(self.channels, open_border)
        v = np.asarray(value, dtype=np.float64)
        if v.ndim > 0 and v.shape != (self.channels,):
            raise ValueError('%s: a number, a (min, max) pair, or one value per channel in either place' % what)
        return np.broadcast_to(v, (self.channels,)).copy()

    def _peak_arguments(self, height, threshold, prominence, wlen, start, stop):
        """((channels, 6) float64 borders hmin, hmax, tmin, tmax, pmin, pmax with -inf / +inf for an open one, wlen in
        frames (0: the whole range), first, last relative to the buffer).  A condition is None, the lower border, or a
        (min, max) tuple or list of two; a border is None, a number or an array of one value per channel."""
        a, b = self._trace_range('find_peaks', start, stop)
        borders = np.zeros((self.channels, 6))
        for k, (cond, what) in enumerate(((height, 'height'), (threshold, 'threshold'), (prominence, 'prominence'))):
            lo, hi = cond if isinstance(cond, (tuple, list)) and len(cond) == 2 else (cond, None)
            borders[:, 2*k] = self._peak_border(lo, what, -np.inf)
            borders[:, 2*k + 1] = self._peak_border(hi, what, np.inf)
        frames = 0
        if wlen is not None:
            frames = int(np.ceil(float(wlen)*self.rate))
            if frames <= 1:
                raise ValueError('wlen must be larger than one frame, it is %g frames' % (float(wlen)*self.rate))
        return borders, frames, a, b

    def find_peaks(self, height=None, threshold=None, prominence=None, wlen=None, start=None, stop=None):
        """Peaks of frames [start, stop) (absolute, inside the current buffer; the whole buffer by default) of every
        channel, with numpy on the host buffer: scipy.signal.find_peaks with its height, threshold, prominence and wlen
        arguments on the float32 samples (peaks.py; the definition: hipdsp_find_peaks in include/hip_dsp.h;
        BufferedData.find_peaks is the same on the device mirror).  No distance, width or plateau_size.  Every
        condition is None, a number (the lower border), a (min, max) pair with None for an open side, or arrays of one
        value per channel in either place (as event_thresholds gives them).  `wlen` is in seconds, ceil(wlen*rate)
        frames; ValueError when that is <= 1, as in scipy.  TypeError for spectrogram-shaped traces.  Returns a Peaks
        object of absolute frame indices."""
        from .peaks import Peaks, host_find_peaks
        borders, frames, a, b = self._peak_arguments(height, threshold, prominence, wlen, start, stop)
        buf = self.buffer
        results = [host_find_peaks(buf[a:b, c], borders[c, 0:2], borders[c, 2:4], borders[c, 4:6], frames,
                                   first=self.offset + a) for c in range(self.channels)]
        return Peaks(results, self.rate, getattr(self, 'name', None))

    def _spectra_arguments(self, regions, nfft, hop, step):
        """((R, 3) int64 table of channel, start, stop relative to the buffer, hop) of a region_spectra call."""
        from .spectra import MAX_NFFT, MIN_NFFT
        self._require_trace('region_spectra')
        nfft = int(nfft)
        if nfft < MIN_NFFT or nfft > MAX_NFFT or nfft & (nfft - 1):
            raise ValueError('nfft %d is not a power of two in [%d, %d]' % (nfft, MIN_NFFT, MAX_NFFT))
        hop = nfft//2 if hop is None else int(hop)
        if hop < 1 or hop > nfft or int(step) < 1:
            raise ValueError('hop %d not in [1, nfft], or step %d < 1' % (hop, int(step)))
        return self._region_table(regions, 'region_spectra'), hop

    def region_spectra(self, regions, nfft, hop=None, step=1):
        """Welch power spectral densities of frames [start, stop) (absolute, inside the current buffer) of one channel
        for every (channel, start, stop) of `regions`, with numpy on the host buffer: Hann frames of `nfft` every `hop`
        (nfft//2 by default) of the samples trace[start:stop:step, channel] (float32, as on the device mirror), mean
        removed per frame, density scaling at rate/step (spectra.py; the definition: hipdsp_region_spectra in
        include/hip_dsp.h, which is scipy.signal.welch; BufferedData.region_spectra is the same on the device
        mirror).  `nfft` is a power of two in 8 ... 8192.  TypeError for spectrogram-shaped traces.  Returns a Spectra
        object."""
        from .spectra import Spectra, host_region_spectrum
        tab, hop = self._spectra_arguments(regions, nfft, hop, step)
        step, fs = int(step), self.rate/int(step)
        F = int(nfft)//2 + 1
        power, info = np.zeros((len(tab), F)), np.zeros((len(tab), 2), dtype=np.int64)
        buf = self.buffer
        for i, (c, a, b) in enumerate(tab):
            v = np.asarray(buf[a:b:step, c], dtype=np.float32)
            power[i], info[i, 0], info[i, 1] = host_region_spectrum(v, int(nfft), hop, fs)
        tab[:, 1:] += self.offset
        return Spectra(tab, power, info[:, 0], info[:, 1], nfft, hop, step, fs, getattr(self, 'name', None))

    def _spectra_peaks(self, regions, nfft, hop, step, thresh):
        """(peak frequencies in Hz, their powers) of the regions' spectra at one nfft: what peak_freqs asks of every
        group of events (BufferedData answers it on the device mirror)."""
        sp = self.region_spectra(regions, nfft, hop, step)
        freqs = sp.peak_freqs(thresh)
        bins = np.rint(np.nan_to_num(freqs)*sp.nfft/sp.fs).astype(np.int64)
        powers = np.where(np.isnan(freqs), np.nan, sp.power[np.arange(len(sp)), bins])
        return freqs, powers.astype(np.float64)

    def _region_table(self, regions, what):
        """(R, 3) int64 table of channel, start, stop relative to the buffer of a region_spectra / region_filtfilt /
        region_crossings / region_xcorr call."""
        self._require_trace(what)
        tab = np.asarray([(int(c), int(a), int(b)) for c, a, b in regions], dtype=np.int64).reshape(-1, 3)
        if len(tab) and (tab[:, 0].min() < 0 or tab[:, 0].max() >= self.channels):
            raise IndexError('channel outside the trace')
        tab[:, 1:] -= self.offset
        n = len(self._buf())
        if len(tab) and (tab[:, 1].min() < 0 or tab[:, 2].max() > n or (tab[:, 2] < tab[:, 1]).any()):
            raise IndexError('range outside the loaded buffer')
        return tab

    def _filtfilt_arguments(self, regions, sos, out):
        """(table relative to the buffer, sos (R, S, 6)) of a region_filtfilt call, checked as hipdsp_region_filtfilt
        checks them: ValueError for a bad filter, a region not longer than its padlen, overlapping regions of one
        channel; NotImplementedError for more than two sections."""
        from .refine import check_sos, padlen
        if out is not None and out is not self:
            raise TypeError('out is None (the filtered regions are returned) or the trace itself (in place)')
        tab = self._region_table(regions, 'region_filtfilt')
        sos = check_sos(np.asarray(sos, dtype=np.float64).reshape(len(tab), -1, 6) if len(tab) else np.zeros((0, 1, 6)))
        if len(tab):
            pad = padlen(sos)
            short = np.flatnonzero(tab[:, 2] - tab[:, 1] <= pad)
            if len(short):
                raise ValueError('region %d: the length of the input vector x must be greater than padlen, which is %d'
                                 % (short[0], pad[short[0]]))
            order = np.lexsort((tab[:, 2], tab[:, 1], tab[:, 0]))
            p, q = tab[order[:-1]], tab[order[1:]]
            if np.any((p[:, 0] == q[:, 0]) & (p[:, 2] > q[:, 1])):
                raise ValueError('regions of one channel overlap')
        return tab, sos

    def region_filtfilt(self, regions, sos, clamp=False, out=None, max_scratch=2**30):
        """Zero-phase filtering of frames [start, stop) (absolute, inside the current buffer) of one channel for every
        (channel, start, stop) of `regions`, each with its own filter sos[r] ((R, S, 6), S 1 or 2):
        float32(scipy.signal.sosfiltfilt(sos[r], trace[start:stop, channel])) of the float32 samples, negative values
        set to 0 with `clamp` (refine.host_region_filtfilt in numpy float64 on the host buffer; the definition:
        hipdsp_region_filtfilt in include/hip_dsp.h; BufferedData.region_filtfilt is the same on the device mirror,
        where `max_scratch` bounds the scratch of one call).  out=None returns the filtered regions, one float32
        array each, and leaves the trace as it is; out=self writes them into the trace (regions of one channel must not
        overlap either way) and returns the trace."""
        from .refine import host_region_filtfilt
        tab, sos = self._filtfilt_arguments(regions, sos, out)
        buf = self.buffer
        res = [host_region_filtfilt(np.asarray(buf[a:b, c], dtype=np.float32), sos[i], clamp)
               for i, (c, a, b) in enumerate(tab)]
        if out is None:
            return res
        for (c, a, b), y in zip(tab, res):
            buf[a:b, c] = y
        return self

    def region_crossings(self, regions, thresholds):
        """(R, 8) float64 per (channel, start, stop) of `regions` (absolute frames inside the current buffer) and its
        own threshold (one value for all, or one per region): n, the number of samples above, the first sample above,
        one past the last sample above, the largest sample, its first position, 0, 0 -- positions absolute, -1 for
        none; float32 comparisons (refine.host_region_crossings on the host buffer; the definition:
        hipdsp_region_crossings; BufferedData.region_crossings is the same on the device mirror)."""
        from .refine import host_region_crossings
        tab = self._region_table(regions, 'region_crossings')
        thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(tab),))
        buf = self.buffer
        res = np.zeros((len(tab), 8))
        for i, (c, a, b) in enumerate(tab):
            res[i] = host_region_crossings(np.asarray(buf[a:b, c], dtype=np.float32), 0, b - a, thr[i])
            res[i, [2, 3, 5]] += np.where(res[i, [2, 3, 5]] >= 0, a + self.offset, 0)
        return res

    def _xcorr_arguments(self, regions, partners, max_lag):
        """((R, 3) int64 table relative to the buffer, partner channels, max_lag) of a region_xcorr call."""
        from .xcorr import MAX_LAG
        tab = self._region_table(regions, 'region_xcorr')
        L = int(max_lag)
        if L < 0 or L > MAX_LAG or L != max_lag:
            raise ValueError('max_lag %r is not a whole number of frames in [0, %d]' % (max_lag, MAX_LAG))
        partners = list(range(self.channels)) if partners is None else [int(p) for p in partners]
        if any(p < 0 or p >= self.channels for p in partners):
            raise ValueError('partner channel outside the trace')
        return tab, partners, L

    def region_xcorr(self, regions, partners=None, max_lag=0):
        """The correlation coefficient of frames [start, stop) (absolute, inside the current buffer) of one channel with
        the frames [start + l, stop + l) of every channel of `partners` (None: every channel; the region's own channel
        and repeats are allowed), for every (channel, start, stop) of `regions` and every lag l in [-max_lag, max_lag]
        (at most 1024), with numpy on the host buffer: np.corrcoef per lag on the float32 samples, NaN where the shifted
        window leaves the buffer, where a window is constant or holds a NaN or an infinity (xcorr.host_region_xcorr; the
        definition: hipdsp_region_xcorr in include/hip_dsp.h; BufferedData.region_xcorr is the same on the device
        mirror).  A positive lag: the partner carries the waveform later.  TypeError for spectrogram-shaped traces,
        ValueError for a bad lag or partner.  Returns a CrossCorrelation object."""
        from .xcorr import CrossCorrelation, host_region_xcorr
        tab, partners, L = self._xcorr_arguments(regions, partners, max_lag)
        r = np.full((len(tab), len(partners), 2*L + 1), np.nan, dtype=np.float32)
        info = np.zeros((len(tab), len(partners), 4))
        buf = self.buffer
        for i, (c, a, b) in enumerate(tab):
            row = np.asarray(buf[:, c], dtype=np.float32)
            for j, p in enumerate(partners):
                r[i, j], info[i, j] = host_region_xcorr(row, np.asarray(buf[:, p], dtype=np.float32), int(a), int(b), L)
        tab[:, 1:] += self.offset
        return CrossCorrelation(tab, partners, r, info, L, self.rate, getattr(self, 'name', None))

    def peak_freqs(self, events, freq_resolution, min_nfft=16, max_nfft=8192, thresh=None, step=1, powers=False):
        """The main spectral peak of every event in Hz -- env_freqs of the reference's songdetector.py
        (songdetector.py:146-152): on an envelope the pulse rate of every song, on a filtered trace the carrier of every
        call.  `events` is an Events object or a list of (channel, start, stop) in absolute frames inside the current
        buffer.  Every event gets nfft = min(welch_nfft(rate/step, freq_resolution, min_nfft, max_nfft), the largest
        power of two <= its length in decimated samples) -- thunderlab's use of max_nfft = i1 - i0, restated -- and a
        hop of nfft//2; events shorter than min_nfft give NaN.  Events are grouped by nfft (at most ten groups), one
        region_spectra call per group.  `thresh`: None takes the largest bin, a number the largest peak of at least that
        prominence in dB (spectra.pick_peak; songdetector.py uses 10).  Returns one float64 array of Hz per channel,
        aligned with events.onsets[channel] (for a list: in the order given); with powers=True a pair of such lists,
        the second holding the power at the peak."""
        from .spectra import event_nfft, welch_nfft
        step = int(step)
        if step < 1:
            raise ValueError('step must be at least 1')
        if hasattr(events, 'onsets'):
            table = [(c, int(a), int(b)) for c in range(events.channels)
                     for a, b in zip(events.onsets[c], events.offsets[c])]
            channels = events.channels
        else:
            table = [(int(c), int(a), int(b)) for c, a, b in events]
            channels = self.channels
        top = welch_nfft(self.rate/step, freq_resolution, min_nfft, max_nfft)
        sizes = np.array([event_nfft(-(-(b - a)//step), top, min_nfft) for c, a, b in table], dtype=np.int64)
        freqs, power = np.full(len(table), np.nan), np.full(len(table), np.nan)
        for nfft in sorted(set(sizes.tolist()) - {0}):
            idx = np.flatnonzero(sizes == nfft)
            freqs[idx], power[idx] = self._spectra_peaks([table[i] for i in idx], nfft, nfft//2, step, thresh)
        owner = np.array([c for c, a, b in table], dtype=np.int64)
        per_channel = [freqs[owner == c] for c in range(channels)]
        if powers:
            return per_channel, [power[owner == c] for c in range(channels)]
        return per_channel

    def event_thresholds(self, factor, start=None, stop=None, method='std'):
        """Per-channel thresholds of a detector over frames [start, stop).  method='std': mean + factor*std (the
        alternative songdetector.py:119-127 leaves commented out), from ONE region_stats call over the range.
        method='histogram': threshold_estimates(start, stop), the reference's live function (songdetector.py:85-117);
        `factor` is ignored then, as the reference ignores its own `fac`."""
        if method == 'histogram':
            return self.threshold_estimates(start, stop)
        if method != 'std':
            raise ValueError("method: 'std' or 'histogram'")
        a = self.offset if start is None else int(start)
        b = self.offset + len(self._buf()) if stop is None else int(stop)
        stats = self.region_stats([(a, b)])[0]
        return stats[:, 1] + float(factor)*stats[:, 2]

    def _require_trace(self, what):
        """TypeError when `what` is asked of spectrogram-shaped data."""
        if len(self.shape) > 2:
            raise TypeError('%s is for traces, not for spectrogram-shaped data' % what)

    def _trace_range(self, what, start, stop):
        """Frames [start, stop) (absolute; by default the whole buffer) relative to the buffer, for a trace."""
        self._require_trace(what)
        n = len(self._buf())
        a = 0 if start is None else int(start) - self.offset
        b = n if stop is None else int(stop) - self.offset
        if a < 0 or b > n or b < a:
            raise IndexError('range outside the loaded buffer')
        return a, b

    @staticmethod
    def _histogram_edges(edges):
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if len(e) < 2:
            raise ValueError('edges: at least two values (one bin)')
        if len(e) > 1025:
            raise NotImplementedError('at most 1024 bins per call, got %d' % (len(e) - 1))
        if not np.isfinite(e).all() or (np.diff(e) < 0).any():
            raise ValueError('edges: finite, non-decreasing values')
        return e

    def _masked_bounds(self, lo, hi, pivot):
        """(channels, 3) float64: lo, hi, pivot per channel, each given as one value or one per channel.  The default
        pivot is the finite one of the two bounds (lo if both are), 0 if neither is."""
        bounds = np.zeros((self.channels, 3))
        try:
            bounds[:, 0] = np.asarray(lo, dtype=np.float64)
            bounds[:, 1] = np.asarray(hi, dtype=np.float64)
            if pivot is None:
                bounds[:, 2] = np.where(np.isfinite(bounds[:, 0]), bounds[:, 0],
                                        np.where(np.isfinite(bounds[:, 1]), bounds[:, 1], 0.0))
            else:
                bounds[:, 2] = np.asarray(pivot, dtype=np.float64)
        except ValueError:
            raise ValueError('lo, hi, pivot: one value or one per channel')
        if not np.isfinite(bounds[:, 2]).all():
            raise ValueError('pivot must be finite')
        return bounds

    def histogram(self, edges, start=None, stop=None, channel=None):
        """Amplitude histogram of frames [start, stop) (absolute, inside the current buffer; the whole buffer by default)
        of every channel over `edges` (B + 1 finite, non-decreasing values, B <= 1024), with numpy on the host buffer:
        int64 (channels, B + 3), or (B + 3,) for one channel.  Slots 0 .. B-1 are np.histogram's counts (bin = the
        number of interior edges <= x, for edges[0] <= x <= edges[-1]: the last bin is closed), slot B counts the
        samples below edges[0], B + 1 those above edges[-1], B + 2 the NaNs; a row sums to stop - start
        (hipdsp_histogram in include/hip_dsp.h; BufferedData.histogram is the same on the device mirror).  TypeError
        for spectrogram-shaped traces."""
        a, b = self._trace_range('histogram', start, stop)
        e = self._histogram_edges(edges)
        B = len(e) - 1
        res = np.zeros((self.channels, B + 3), dtype=np.int64)
        block = np.asarray(self.buffer[a:b], dtype=np.float64)
        for c in range(self.channels):
            v = block[:, c]
            inside = v[(v >= e[0]) & (v <= e[-1])]
            res[c, :B] = np.bincount(np.searchsorted(e[1:-1], inside, side='right'), minlength=B)
            res[c, B:] = np.sum(v < e[0]), np.sum(v > e[-1]), np.sum(np.isnan(v))
        return res[channel] if channel is not None else res

    def masked_stats(self, lo, hi, pivot=None, start=None, stop=None):
        """Number, mean and std (ddof 0) of the samples with lo < x < hi (both strict; -inf / +inf switch a side off;
        NaN and infinite samples are never selected, a NaN bound selects nothing) of frames [start, stop) of every
        channel, and a reserved 0: (channels, 4), NaN mean and std where nothing is selected.  lo, hi and pivot are
        each one value or one per channel.  Here numpy on the host buffer (np.mean, np.std; the pivot is checked and
        not used); BufferedData.masked_stats is the same on the device mirror, where the sums are shifted by `pivot`
        (hipdsp_masked_stats in include/hip_dsp.h; default: the finite one of the two bounds, 0 if neither is).
        TypeError for spectrogram-shaped traces."""
        a, b = self._trace_range('masked_stats', start, stop)
        bounds = self._masked_bounds(lo, hi, pivot)
        res = np.zeros((self.channels, 4))
        block = np.asarray(self.buffer[a:b], dtype=np.float64)
        with np.errstate(invalid='ignore'):
            for c in range(self.channels):
                v = block[:, c]
                sel = v[(v > bounds[c, 0]) & (v < bounds[c, 1]) & np.isfinite(v)]
                res[c, :3] = (len(sel), np.mean(sel), np.std(sel)) if len(sel) else (0, np.nan, np.nan)
        return res

    def threshold_estimates(self, start=None, stop=None):
        """The reference's histogram threshold (threshold_estimates, songdetector.py:85-117) of frames [start, stop) of
        an envelope-like trace, one float64 per channel, from four reductions over the range:
          1. maxe, the maximum over all channels (one region_stats call);
          2. per channel the histogram over b = np.linspace(0, maxe, 50); mini = the first non-empty bin, maxi = the
             fullest bin + 1, widened by maxi - mini and clamped to 49 (on the host, from the 49 counts);
          3. mean and std of the samples below b[maxi] (masked_stats, pivot b[maxi]);
          4. uppermean, the mean of the samples above mean + 3*std (masked_stats);
        the threshold is 0.5*(mean + uppermean) if uppermean > mean + 6*std, else maxe + std -- also when no sample
        lies above mean + 3*std (uppermean is NaN and the comparison false, as in the reference).
        Deviation: where the reference fails with an IndexError or a numpy error -- the maximum over the range NaN,
        infinite or <= 0 (an empty range included), or a channel without a sample in [0, maxe] -- this raises a
        ValueError that says so.  TypeError for spectrogram-shaped traces."""
        a, b = self._trace_range('threshold_estimates', start, stop)
        first, last = self.offset + a, self.offset + b
        maxe = np.max(self.region_stats([(first, last)])[0][:, 4]) if b > a and self.channels > 0 else np.nan
        if not (np.isfinite(maxe) and maxe > 0.0):
            raise ValueError('threshold_estimates: the maximum over the range is %r; it must be finite and > 0' % float(maxe))
        edges = np.linspace(0.0, maxe, 50)
        counts = self.histogram(edges, first, last)[:, :49]
        if (counts.sum(axis=1) == 0).any():
            raise ValueError('threshold_estimates: a channel has no sample between 0 and the maximum %r' % float(maxe))
        mini = np.argmax(counts > 0, axis=1)
        maxi = np.argmax(counts, axis=1) + 1
        maxi = np.minimum(maxi + (maxi - mini), 49)
        cut = edges[maxi]
        lower = self.masked_stats(-np.inf, cut, cut, first, last)
        mean, std = lower[:, 1], lower[:, 2]
        above = mean + 3.0*std
        upper = self.masked_stats(above, np.inf, np.where(np.isfinite(above), above, 0.0), first, last)
        with np.errstate(invalid='ignore'):
            return np.where(upper[:, 1] > mean + 6.0*std, 0.5*(mean + upper[:, 1]), maxe + std)

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        first, rest = key[0], key[1:]
        if isinstance(first, slice):
            start, stop, step = first.indices(self.frames)
            if step < 1:
                raise IndexError('negative steps are not supported')
            if stop <= start:
                return self.buffer[(slice(0, 0),) + rest]
            self.update_buffer(start, stop)
            return self.buffer[(slice(start - self.offset, stop - self.offset, step),) + rest]
        index = int(first)
        if index < 0:
            index += self.frames
        if index < 0 or index >= self.frames:
            raise IndexError('frame index out of range')
        self.update_buffer(index, index + 1)
        return self.buffer[(index - self.offset,) + rest]


class ArrayLoader(BufferedArray):
    """An in-memory (frames, channels) recording behind the BufferedArray interface:
    stands in for ``thunderlab.dataloader.DataLoader`` (``src/audian/data.py:172``)
    with its ``buffer_time`` / ``back_time`` arguments."""

    def __init__(self, data, rate, buffer_time=60.0, back_time=20.0, unit='a.u.',
                 ampl_max=1.0, verbose=0, view=False):
        super().__init__(verbose)
        self.view = view          # buffer = a window onto `data` instead of a float64 copy of it
        data = np.asarray(data)
        if data.ndim == 1:
            data = data[:, None]
        self.data = data
        self.rate = float(rate)
        self.frames, self.channels = data.shape
        self.shape = (self.frames, self.channels)
        self.ndim = 2
        self.size = self.frames*self.channels
        self.unit = unit
        self.ampl_min = -ampl_max
        self.ampl_max = ampl_max
        self.bufferframes = min(self.frames, int(buffer_time*self.rate))
        self.backframes = int(back_time*self.rate)
        self.buffer_changed = np.zeros(self.channels, dtype=bool)
        self.buffer = np.zeros((0, self.channels))
        self.name = 'data'
        self.dests = []
        self.need_update = False
        self.plot_items = [None]*self.channels
        self.move_buffer(0, self.bufferframes)

    def load_buffer(self, offset, nframes, buffer):
        buffer[:, :] = self.data[offset:offset + nframes, :]
        self._apply_unwrap(buffer)

    def move_buffer(self, offset, nframes):
        if not self.view:
            return BufferedArray.move_buffer(self, offset, nframes)
        # the recording is in memory anyway: moving the buffer is re-slicing it
        offset = int(max(0, offset))
        nframes = int(max(0, min(nframes, self.frames - offset)))
        self.buffer = self.data[offset:offset + nframes]
        self.offset = offset
        self.buffer_changed[:] = True


class WavLoader(BufferedArray):
    """A PCM WAV file behind the BufferedArray interface (stdlib ``wave``): stands in for
    ``thunderlab.dataloader.DataLoader`` on plain WAV recordings such as the reference's
    ``data/Gryllus_campestris.wav``.  Samples become float64 in [-1, 1) exactly as audioio
    scales them (integer / 2**(bits-1)); ``pcm_slab`` additionally hands the file's own
    bytes to the device path (``hipdsp_pcm_unpack``)."""

    def __init__(self, path, buffer_time=60.0, back_time=20.0, unit='a.u.', verbose=0):
        import wave
        super().__init__(verbose)
        self._wav = wave.open(path, 'rb')
        if self._wav.getcomptype() != 'NONE' or self._wav.getsampwidth() not in (2, 3, 4):
            raise ValueError('only uncompressed 16/24/32-bit PCM WAV files are supported')
        self.filepath = path
        self.file_paths = [path]       # the attribute audian's CompressedData reads (one file per loader here)
        self.sample_bytes = self._wav.getsampwidth()
        self.scale = 1.0/float(1 << (8*self.sample_bytes - 1))
        self.rate = float(self._wav.getframerate())
        self.channels = self._wav.getnchannels()
        self.frames = self._wav.getnframes()
        self.shape = (self.frames, self.channels)
        self.ndim = 2
        self.size = self.frames*self.channels
        self.unit = unit
        self.ampl_min, self.ampl_max = -1.0, 1.0
        self.bufferframes = min(self.frames, int(buffer_time*self.rate))
        self.backframes = int(back_time*self.rate)
        self.buffer_changed = np.zeros(self.channels, dtype=bool)
        self.buffer = np.zeros((0, self.channels))
        self.name = 'data'
        self.dests = []
        self.need_update = False
        self.plot_items = [None]*self.channels
        self.move_buffer(0, self.bufferframes)

    def pcm_slab(self, offset, nframes):
        """Raw interleaved bytes of frames [offset, offset + nframes) as a uint8 array."""
        self._wav.setpos(int(offset))
        raw = self._wav.readframes(int(nframes))
        return np.frombuffer(raw, dtype=np.uint8)

    def load_buffer(self, offset, nframes, buffer):
        raw = self.pcm_slab(offset, nframes)
        nb = self.sample_bytes
        if nb == 2:
            ints = raw.view('<i2').astype(np.int64)
        elif nb == 4:
            ints = raw.view('<i4').astype(np.int64)
        else:
            b = raw.reshape(-1, 3).astype(np.int64)
            ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            ints = np.where(ints >= 1 << 23, ints - (1 << 24), ints)
        buffer[:, :] = ints.reshape(-1, self.channels)*self.scale
        self._apply_unwrap(buffer)

    def close(self):
        self._wav.close()
