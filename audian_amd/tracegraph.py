"""A GUI-free stand-in for the part of audian's ``Data`` model that drives the trace graph
(``src/audian/data.py:121-236`` in /root/reference): put the traces in dependency order, add up
the pre/post-roll every level needs, open the raw loader and the derived traces, and re-align
the derived buffers whenever the visible time window moves.  Tests, the streaming demo and
integrators use it; the Qt application keeps its own ``Data``.  It also carries the region analysis the reference
splits between ``Data.get_region`` (data.py:102-118) and ``DataBrowser.analyze_region`` (databrowser.py:1759-1775), and
the event detection that the reference's ``songdetector.py`` puts in front of it (detect_songs, songdetector.py:113-139)."""

import numpy as np

from .analyzer import Region
from .bufferedarray import ArrayLoader
from .bufferedspectrogram import BufferedSpectrogram

ROOT = 'data'          # name of the raw recording every chain starts from


def _widen(a, b):
    return max(a[0], b[0]), max(a[1], b[1])


class TraceGraph(object):

    def __init__(self, buffer_time=60.0, back_time=20.0):
        self.buffer_time, self.back_time = buffer_time, back_time
        self.data = None
        self.traces, self.sources = [], []
        self.analyzers = []
        self.tbefore = self.tafter = 0

    def add_trace(self, trace):
        self.traces.append(trace)

    def __getitem__(self, key):
        wanted = key.lower()
        return next((t for t in self.traces if t.name.lower() == wanted), None)

    def setup_traces(self):
        """Depth-first order: every trace directly after its source and before its source's
        next sibling, siblings in the order they were added -- the order data.py:121-147 builds by
        repeated insertion.  `sources[k]` is the position of trace k's source, -1 for the raw data."""
        children = {}
        for trace in self.traces:
            children.setdefault(trace.source_name, []).append(trace)
        ordered, parents = [], []

        def place(source_name, position):
            for trace in children.pop(source_name, []):
                ordered.append(trace)
                parents.append(position)
                place(trace.name, len(ordered) - 1)

        place(ROOT, -1)
        if children:
            orphans = [f'{t.name} <- {t.source_name}' for group in children.values() for t in group]
            raise ValueError('source not found for traces: ' + ', '.join(orphans))
        self.traces, self.sources = ordered, parents

    def open(self, samples, rate, unwrap=0.0, unwrap_clip=False, **kwargs):
        """What Data.open does around the loader (data.py:150-204): walk the ordered traces
        from the leaves up, let each add the margins its dependants need to its own
        (expand_times) and pass the sum on to its source; the raw loader is then opened with
        buffer_time / back_time widened by what arrives at the root, and every derived trace is
        opened on its source."""
        n = len(self.traces)
        needed = [(0, 0)]*n                 # margins the traces derived from k ask of k
        root = (0, 0)
        for k in range(n - 1, -1, -1):
            ask = self.traces[k].expand_times(*needed[k])
            parent = self.sources[k]
            if parent < 0:
                root = _widen(root, ask)
            else:
                needed[parent] = _widen(needed[parent], ask)
        self.tbefore, self.tafter = root
        self.data = ArrayLoader(samples, rate, self.buffer_time + self.tbefore + self.tafter,
                                self.back_time + self.tbefore, **kwargs)
        if unwrap > 1e-3:
            # what Data.open does right behind the loader (data.py:180; CLI -u / -U, audian.py:1485-1512)
            self.data.set_unwrap(unwrap, unwrap_clip, False, self.data.unit)
        # position 0 is the raw data from now on
        self.traces = [self.data] + self.traces
        self.sources = [None] + [p + 1 for p in self.sources]
        for trace, parent in zip(self.traces[1:], self.sources[1:]):
            trace.open(self.traces[parent])
        self.set_need_update()

    def set_need_update(self):
        """The raw data is needed if it is shown itself; the derived traces then report their own
        need, which climbs back up (BufferedData.set_need_update)."""
        raw = self.data
        raw.need_update = any(item is not None and item.isVisible() for item in raw.plot_items)
        for dest in raw.dests:
            dest.set_need_update()

    def update_times(self, t0, t1):
        """A new visible window [t0, t1] s: move the raw buffer (widened by the accumulated
        margins), then re-align every derived trace that is needed, sources first (data.py:225-231)."""
        if self.data.need_update:
            self.data.update_time(t0 - self.tbefore, t1 + self.tafter)
        for trace in self.traces[1:]:
            if trace.need_update:
                trace.align_buffer()

    # ---- region analysis ------------------------------------------------------------------
    def add_analyzer(self, analyzer):
        self.analyzers.append(analyzer)

    @staticmethod
    def region_frames(trace, t0, t1):
        """Frames [i0, i1) of `trace` that Data.get_region cuts for the times [t0, t1] (data.py:105-110)."""
        i0 = max(int(t0*trace.rate), 0)
        i1 = min(int(t1*trace.rate) + 1, len(trace))
        return i0, max(i0, i1)

    def get_region(self, t0, t1, channel):
        """Every trace cut to [t0, t1] s of one channel, as Data.get_region returns it (data.py:102-118):
        ``{name: (time, data)}``, ``(time, frequencies, data)`` for a spectrogram.  `data` is a lazy Region: numpy's
        mean / std / min / max / argmin / argmax of it are reduced on the device, anything else makes it the array
        ``trace[i0:i1, channel]``."""
        traces = {}
        for t in self.traces:
            i0, i1 = self.region_frames(t, t0, t1)
            time = np.arange(i0, i1)/t.rate
            data = Region(t, i0, i1, channel)
            if isinstance(t, BufferedSpectrogram):
                traces[t.name] = (time, t.frequencies, data)
            else:
                traces[t.name] = (time, data)
        return traces

    def _clip_times(self, t0, t1):
        return max(t0, 0), min(t1, self.data.frames/self.data.rate)

    def analyze_region(self, t0, t1, channel):
        """Hand the region to every analyzer (DataBrowser.analyze_region, databrowser.py:1759-1768)."""
        t0, t1 = self._clip_times(t0, t1)
        traces = self.get_region(t0, t1, channel)
        for a in self.analyzers:
            a.analyze(t0, t1, channel, traces)

    def analyze_regions(self, regions, channels=None):
        """Fill the analyzers' tables for many (t0, t1) regions and channels (all of them by default), rows in
        region-major order.  An analyzer that implements analyze_many() -- StatisticsAnalyzer: one launch per 16
        regions, all channels at once -- does it in one go; every other one is called region by region."""
        regions = [self._clip_times(t0, t1) for t0, t1 in regions]
        channels = list(range(self.data.channels)) if channels is None else list(channels)
        for a in self.analyzers:
            if a.analyze_many(regions, channels):
                continue
            for t0, t1 in regions:
                for c in channels:
                    a.analyze(t0, t1, c, self.get_region(t0, t1, c))

    # ---- event detection ---------------------------------------------------------------------
    def _event_frames(self, trace, t0, t1):
        """The frames of `trace` for the times [t0, t1] (None: the buffer as it is), with the buffers moved there as for
        a visible window (update_times)."""
        if t0 is None and t1 is None:
            return None, None
        t0 = 0.0 if t0 is None else t0
        t1 = len(trace)/trace.rate if t1 is None else t1
        self.update_times(t0, t1)               # the raw buffer, then the derived traces that are needed
        i0, i1 = self.region_frames(trace, t0, t1)
        if trace is self.data:
            trace.update_buffer(i0, i1)         # (a raw loader that is not shown does not follow update_times)
        return i0, i1

    def event_thresholds(self, trace_name, factor, t0=None, t1=None, method='std'):
        """mean + factor*std of the trace between t0 and t1 (by default its current buffer), one value per channel:
        the usual threshold of a detector (songdetector.py:119-127), from one region_stats call.  With
        method='histogram' the reference's histogram threshold instead (threshold_estimates, songdetector.py:85-117;
        BufferedArray.threshold_estimates), which ignores `factor`."""
        trace = self[trace_name]
        i0, i1 = self._event_frames(trace, t0, t1)
        return trace.event_thresholds(factor, i0, i1, method=method)

    def detect_events(self, trace_name, thresholds, min_gap=0.0, min_duration=0.0, t0=None, t1=None):
        """Threshold events of a trace between t0 and t1 seconds (by default its current buffer): the buffer is moved
        to cover the range, then the trace detects (BufferedData.detect_events: on its device mirror when it has
        one).  The buffers move as for a visible window (update_times), so the graph's buffer_time has to hold the
        range as it has to hold a window; a range that is not resident afterwards is an IndexError.  Returns an Events
        object."""
        trace = self[trace_name]
        i0, i1 = self._event_frames(trace, t0, t1)
        return trace.detect_events(thresholds, min_gap, min_duration, i0, i1)

    def find_peaks(self, trace_name, height=None, threshold=None, prominence=None, wlen=None, t0=None, t1=None):
        """Peaks of a trace between t0 and t1 seconds (by default its current buffer): the buffers are moved as for
        detect_events, then the trace finds its peaks (BufferedData.find_peaks: on its device mirror when it has one;
        scipy.signal.find_peaks with height, threshold, prominence and wlen, `wlen` in seconds).  Returns a Peaks
        object of absolute frame indices."""
        trace = self[trace_name]
        i0, i1 = self._event_frames(trace, t0, t1)
        return trace.find_peaks(height, threshold, prominence, wlen, i0, i1)

    def event_peak_freqs(self, events, trace_name=None, freq_resolution=1.0, thresh=None, step=None, min_nfft=16,
                         max_nfft=8192):
        """The main spectral peak of every event in Hz -- env_freqs of the reference's songdetector.py
        (songdetector.py:146-152, called at :761) -- taken on `trace_name` (by default the trace the events were
        detected on): on an envelope the pulse rate of every song, on the filtered trace the carrier of every call.
        The buffers are moved as in detect_events so that the trace holds all events, then the trace computes
        (BufferedData.peak_freqs: on its device mirror when it has one, one call per nfft).  `step` decimates the
        trace before the spectra; None means 1, except on a BufferedEnvelope, which lives at the full rate here: there
        it is max(1, round(rate / (10*envelope_cutoff))), the reference's envrate (songdetector.py:63-66).  A
        BufferedPowerEnvelope already lives at the envelope rate: step 1.  Returns one array of Hz per channel, aligned
        with events.onsets[channel]."""
        from .bufferedenvelope import BufferedEnvelope
        trace = self[events.trace_name if trace_name is None else trace_name]
        if step is None:
            step = 1
            if isinstance(trace, BufferedEnvelope):
                step = max(1, int(round(trace.rate/(10.0*trace.envelope_cutoff))))
        if len(events) > 0:
            first = min(int(o.min()) for o in events.onsets if len(o))
            last = max(int(o.max()) for o in events.offsets if len(o))
            scale = trace.rate/events.rate
            a, b = int(np.floor(first*scale)), int(np.ceil(last*scale))
            if a < trace.offset or b > trace.offset + len(trace._buf()):
                self._event_frames(trace, (first + 0.5)/events.rate, (last - 0.5)/events.rate)   # as Events.regions
            if scale != 1.0:
                from .events import Events
                events = Events([np.stack((np.floor(events.onsets[c]*scale), np.ceil(events.offsets[c]*scale)), axis=1)
                                 for c in range(events.channels)], trace.rate, trace.name)
        return trace.peak_freqs(events, freq_resolution, min_nfft, max_nfft, thresh, step)

    def event_cross_correlation(self, events, trace_name=None, max_delay=0.001, channels=None):
        """The correlation of every event with the other channels over the lags of +-`max_delay` seconds, taken on
        `trace_name` (by default the trace the events were detected on): what tells an animal's own song from its
        crosstalk on the neighbouring microphones (xcorr.py).  max_lag = round(max_delay * rate) frames, at most 1024.
        The buffers are moved as in event_peak_freqs so that the trace holds all events, then the trace computes
        (BufferedData.region_xcorr: on its device mirror when it has one, ONE call for all events and partners).
        `channels`: the partner channels, by default all.  Returns ONE CrossCorrelation over all events, channel by
        channel in the events' order (xcorr.event_table); a positive lag: the partner carries the event later."""
        from .xcorr import MAX_LAG, event_table
        trace = self[events.trace_name if trace_name is None else trace_name]
        max_lag = int(round(float(max_delay)*trace.rate))
        if max_lag < 0 or max_lag > MAX_LAG:
            raise ValueError('max_delay %g s is %d frames of %s: at most %d frames (%g s) to either side'
                             % (max_delay, max_lag, trace.name, MAX_LAG, MAX_LAG/trace.rate))
        table = event_table(events, trace.rate/events.rate)
        if len(table):
            a, b = int(table[:, 1].min()), int(table[:, 2].max())
            if a < trace.offset or b > trace.offset + len(trace._buf()):
                self._event_frames(trace, (a + 0.5)/trace.rate, (b - 0.5)/trace.rate)       # as Events.regions
        return trace.region_xcorr(table, channels, max_lag)

    def region_contours(self, rows, spec_name='spectrogram', fmin=0.0, fmax=None, min_power=1e-20, drop_db=10.0):
        """The frequency contours (contours.Contours) of the (channel, t_on, t_off) `rows` in seconds on the spectrogram
        `spec_name`, inside the band [fmin, fmax] Hz: every row owns the frames whose centre lies in it.  The buffers are
        moved as in detect_events so that the spectrogram holds all rows, then ONE spectral_features call over the frames
        they span (BufferedSpectrogram.spectral_features: on its device mirror when it has one) brings seven floats per
        frame and channel, and the per-event reduction runs on the host."""
        from .contours import CONTOUR_FEATURES, Contours, frame_table
        spec = self[spec_name]
        rate = spec.sample_rate
        table = frame_table(rows, rate, spec.nfft, spec.hop, spec.frames)
        a = int(table[:, 1].min()) if len(table) else spec.offset
        b = max(a, int(table[:, 2].max())) if len(table) else a
        if b > a and (a < spec.offset or b > spec.offset + len(spec._buf())):
            self._event_frames(spec, (a + 0.5)/spec.rate, (b - 0.5)/spec.rate)      # as Events.regions
        feats = spec.spectral_features(a, b, fmin, fmax, CONTOUR_FEATURES, min_power, drop_db)
        return Contours(table, a, feats, 0.5*spec.nfft/rate, spec.hop/rate, spec.name)

    def event_contours(self, events, spec_name='spectrogram', fmin=0.0, fmax=None, min_power=1e-20, drop_db=10.0):
        """region_contours of every event [onset, offset) / events.rate, channel by channel in the events' order:
        start, end, minimum, maximum and peak frequency of every call, its extent, centroid, bandwidth and flatness."""
        rows = [(c, a/events.rate, b/events.rate) for c in range(events.channels)
                for a, b in events.frames(c).tolist()]
        return self.region_contours(rows, spec_name, fmin, fmax, min_power, drop_db)

    # ---- spectrogram template matching ----------------------------------------------------------
    def cut_template(self, t0, t1, fmin, fmax, channel, spec_name='spectrogram', log=True, floor_db=-120.0, name='template'):
        """The patch of the spectrogram `spec_name` between t0 and t1 seconds and fmin and fmax Hz (the bins of
        band_bins()) of one channel as a templates.Template: in dB floored at `floor_db` with `log`, else the powers.
        The buffers are moved as in detect_events; with a device mirror only the patch crosses to the host."""
        from . import hipdsp
        from .bufferedspectrogram import band_bins
        from .templates import Template, host_values
        spec = self[spec_name]
        i0, i1 = self._event_frames(spec, t0, t1)
        F = int(spec.shape[2])
        k0, k1 = band_bins(fmin, fmax, spec.fresolution, F)
        a, b = i0 - spec.offset, i1 - spec.offset
        n = len(spec._buf())
        if a < 0 or b > n:
            raise IndexError('range outside the loaded buffer')
        if b <= a or k1 <= k0:
            raise ValueError('the template would be empty: no frame or no bin inside the range')
        if not 0 <= int(channel) < spec.channels:
            raise IndexError(f'channel {channel} of {spec.channels}')
        if spec._mirror_valid(a, b):
            patch = hipdsp.DeviceArray(spec.ctx, (b - a, k1 - k0), np.float32)
            hipdsp.memcpy2d(spec.ctx, patch, 4*(k1 - k0), spec._dev.view(int(channel)*spec._pitch() + a*F + k0, (1,)),
                            4*F, 4*(k1 - k0), b - a)
            power = patch.to_host().astype(np.float64)
            patch.free()
        else:
            power = np.asarray(spec.buffer[a:b, int(channel), k0:k1], dtype=np.float64)
        return Template(host_values(power, log, floor_db if log else -np.inf), k0*spec.fresolution, spec.fresolution,
                        spec.tresolution, log, floor_db, name)

    def match_templates(self, templates, spec_name='spectrogram', t0=None, t1=None, normalize=True, min_std=0.1,
                        pivot=None):
        """The score rows of all `templates` on the spectrogram `spec_name` between t0 and t1 seconds (by default its
        current buffer): the buffers are moved as in detect_events, then templates.template_scores.  Returns
        (scores, i0): (K, channels, frames) float32 -- a device array when the spectrogram has a device mirror -- and
        the absolute frame of column 0."""
        from .templates import template_scores
        spec = self[spec_name]
        i0, i1 = self._event_frames(spec, t0, t1)
        if i0 is None:
            i0, i1 = spec.offset, spec.offset + len(spec._buf())
        return template_scores(spec, templates, i0, i1, normalize, min_std, pivot), i0

    def detect_calls(self, templates, min_r=0.5, spec_name='spectrogram', t0=None, t1=None, min_std=0.1, pivot=None):
        """Spectrogram cross-correlation as a detector: the correlation rows of all `templates` (match_templates),
        their peaks of at least `min_r` (hipdsp_find_peaks on the rows, which stay on the device; numpy on a host-only
        graph), and per channel the windows [peak - Tt//2, peak - Tt//2 + Tt) of all templates, overlapping ones merged,
        as an Events on the spectrogram's frame grid (rate = the spectrogram's) -- what analyze_events, event_contours,
        event_cross_correlation and attribute_events take as it is.  Returns (events, best_template, best_score): per
        channel, aligned with the events, the index of the template with the highest peak inside each call and that
        score."""
        from . import hipdsp
        from .events import Events
        from .peaks import host_find_peaks
        templates = list(templates)
        spec = self[spec_name]
        scores, i0 = self.match_templates(templates, spec_name, t0, t1, True, min_std, pivot)
        K, C, n = scores.shape
        if isinstance(scores, hipdsp.DeviceArray):
            found = hipdsp.find_peaks(spec.ctx, scores, n, K*C, 0, n, (float(min_r), np.inf, -np.inf, np.inf, -np.inf, np.inf)) \
                if K*C > 0 and n > 0 else []
            scores.free()
        else:
            found = [host_find_peaks(scores[k, c], height=(float(min_r), None)) for k in range(K) for c in range(C)]
        pairs, best, best_r = [], [], []
        for c in range(C):
            rows = []
            for k in range(K if found else 0):
                pos, props = found[k*C + c]
                Tt = templates[k].values.shape[0]
                rows.extend((int(p) - Tt//2 + i0, int(p) - Tt//2 + i0 + Tt, float(h), k) for p, h in zip(pos, props[:, 0]))
            rows.sort()
            merged = []
            for a, b, r, k in rows:
                if merged and a < merged[-1][1]:
                    last = merged[-1]
                    last[1] = max(last[1], b)
                    if r > last[2]:
                        last[2], last[3] = r, k
                else:
                    merged.append([a, b, r, k])
            pairs.append(np.array([m[:2] for m in merged], dtype=np.int64).reshape(-1, 2))
            best.append(np.array([m[3] for m in merged], dtype=np.int64))
            best_r.append(np.array([m[2] for m in merged], dtype=np.float64))
        return Events(pairs, spec.rate, spec.name), best, best_r

    # ---- noise profile -----------------------------------------------------------------------------
    def estimate_noise_profile(self, t0=None, t1=None, percentile=50.0, spec_name='spectrogram', frame_step=1,
                               min_power=1e-20):
        """The noise profile (noiseprofile.NoiseProfile) of the spectrogram `spec_name` between t0 and t1 seconds (by
        default its current buffer): per channel and bin the `percentile` over every `frame_step`-th frame.  The buffers
        are moved as in detect_events, then BufferedSpectrogram.noise_profile (on the device mirror when the trace has
        one: one radix select per column, twelve bytes per column come back).  What BufferedEqualizedSpectrogram
        .set_profile takes."""
        spec = self[spec_name]
        i0, i1 = self._event_frames(spec, t0, t1)
        if i0 is None:
            i0, i1 = spec.offset, spec.offset + len(spec._buf())
        return spec.noise_profile(i0, i1, percentile, frame_step, min_power)

    def attribute_events(self, events, trace_name=None, max_delay=0.001, channels=None, min_r=0.5, min_ratio=1.0):
        """event_cross_correlation followed by the attribution rule (xcorr.attribute_events, whose two thresholds are
        not calibrated on recordings): returns (own, sources, delays) -- the Events that are their own source, and per
        channel the source channel of ALL events and the source's delay in seconds."""
        from .xcorr import attribute_events
        xc = self.event_cross_correlation(events, trace_name, max_delay, channels)
        return attribute_events(events, xc, min_r, min_ratio)

    def clean_event_freqs(self, events, freqs, fac=6.0):
        """clean_env_freqs of the reference's songdetector.py (songdetector.py:155-175, called at :763): frequencies
        further than fac standard deviations from the mean of the pooled frequencies' middle half become NaN, and
        events without a frequency are dropped (refine.clean_event_freqs).  Returns (Events, frequencies per
        channel)."""
        from .refine import clean_event_freqs
        return clean_event_freqs(events, freqs, fac)

    def refine_events(self, events, freqs, thresholds, trace_name=None, min_duration=0.1, min_thresh_fac=1.0):
        """analyse_songs of the reference's songdetector.py (songdetector.py:195-244, called at :767) on `trace_name`
        (by default the trace the events were detected on; the reference takes the envelope that filter_envelopes
        smoothed -- a BufferedEventFilter here): around every event a local threshold, 1.2 times the largest sample
        of the noise windows beside it but at least min_thresh_fac * the channel's threshold, and the event's borders
        again as the first and last sample above it inside the event widened by int(min_duration * rate) frames;
        events without a frequency, or with nothing above, are dropped (refine.py has the bookkeeping and the two
        deviations from the reference).  The buffers are moved as in event_peak_freqs so that the trace holds all
        windows; then ONE region_crossings call with NaN thresholds over all noise windows brings their maxima, two
        floats per event, the thresholds are computed on the host, and ONE region_crossings call over the widened
        events brings the borders.  `thresholds`: one value, or one per channel.  Returns an Events object."""
        from .events import Events
        from .refine import local_thresholds, noise_windows
        trace = self[events.trace_name if trace_name is None else trace_name]
        thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (events.channels,))
        scale = trace.rate/events.rate
        pairs = [events.frames(c) if scale == 1.0 else
                 np.stack((np.floor(events.onsets[c]*scale), np.ceil(events.offsets[c]*scale)), axis=1).astype(np.int64)
                 for c in range(events.channels)]
        w = int(min_duration*trace.rate)
        n = len(trace)
        windows = [noise_windows(pairs[c], freqs[c], w, n) for c in range(events.channels)]
        noise, wide = [], []
        for c, (wd, before, after) in enumerate(windows):
            for a, b in np.concatenate((before, after)):
                noise.append((c, int(a), int(max(a, b))))
            wide.extend((c, int(a), int(max(a, b))) for a, b in wd)
        if not wide:
            return Events([np.zeros((0, 2)) for c in range(events.channels)], trace.rate, trace.name)
        first, last = min(r[1] for r in noise + wide), max(r[2] for r in noise + wide)
        if first < trace.offset or last > trace.offset + len(trace._buf()):
            self._event_frames(trace, (first + 0.5)/trace.rate, (last - 0.5)/trace.rate)
        maxima = trace.region_crossings(noise, np.nan)[:, 4]
        local, k = [], 0
        for c, (wd, before, after) in enumerate(windows):
            K = len(wd)
            local.append(local_thresholds(before, after, maxima[k:k + K], maxima[k + K:k + 2*K], freqs[c], float(thr[c]), w,
                                          min_thresh_fac))
            k += 2*K
        found = trace.region_crossings(wide, np.concatenate(local))
        out, k = [], 0
        for c, (wd, before, after) in enumerate(windows):
            rows = found[k:k + len(wd)]
            k += len(wd)
            keep = rows[:, 2] >= 0
            out.append(rows[keep][:, 2:4].astype(np.int64))
        return Events(out, trace.rate, trace.name)

    def detect_songs(self, env_name, slow_name, min_duration=0.5, peak_thresh=10.0, min_thresh_fac=1.0, t0=None, t1=None):
        """The reference's song detector behind its envelope (main(), songdetector.py:757-767) as one call over the
        methods above: histogram thresholds of the slow envelope `slow_name` (a BufferedLowpass of the envelope at 1 /
        min_duration), its events with min_gap = min_duration = `min_duration`, the pulse rate of every event on the
        envelope `env_name` (a BufferedPowerEnvelope; spectral peaks of at least `peak_thresh` dB prominence), the
        cleaning of those rates and the events' borders again from local thresholds on the envelope.  No arithmetic of
        its own.  Returns (events, freqs, thresholds): the refined Events (frames of the envelope), the cleaned rates per
        channel (aligned with the events the refinement was given) and the thresholds per channel."""
        thresholds = self.event_thresholds(slow_name, 0.0, t0, t1, method='histogram')
        events = self.detect_events(slow_name, thresholds, min_gap=min_duration, min_duration=min_duration, t0=t0, t1=t1)
        freqs = self.event_peak_freqs(events, env_name, thresh=peak_thresh)
        events, freqs = self.clean_event_freqs(events, freqs)
        events = self.refine_events(events, freqs, thresholds, trace_name=env_name, min_duration=min_duration,
                                    min_thresh_fac=min_thresh_fac)
        return events, freqs, thresholds

    @staticmethod
    def mark_peaks(analyzer, name, peaks):
        """Fill the analyzer's point events `name` (Analyzer.make_trace_events) with the peaks: (times, heights) of
        every channel, whatever `name` held before erased."""
        analyzer.set_events(name, -1, [], [])
        for c in range(min(peaks.channels, len(analyzer.events[name]))):
            analyzer.add_events(name, c, *peaks.points(c))

    def analyze_events(self, events, channels=None):
        """Fill the analyzers' tables with the regions of the events, channel by channel: every event is analyzed on
        its own channel only, so StatisticsAnalyzer gets one row per event (songdetector.py:141-143 analyzes each
        detected song's region the same way)."""
        for c in (range(events.channels) if channels is None else channels):
            regions = events.regions(c)
            if regions:
                self.analyze_regions(regions, channels=[c])
