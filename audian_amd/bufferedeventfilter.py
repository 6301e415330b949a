"""Event filter on the fly: a trace whose detected events are smoothed, each by a zero-phase low-pass of its own --
``filter_envelopes`` of the reference's ``songdetector.py`` (songdetector.py:178-192, called at :765: the envelope inside
every widened song is low-pass filtered at four times that song's pulse rate, in place) as a derived trace.  The
reference rewrites its envelope array; here the source stays as it is and this trace holds the filtered copy, so new
events or another factor recompute this trace only.  ``process()`` is a copy on the device; the events inside the buffer
are then filtered in place on this trace's mirror by ONE ``hipdsp_region_filtfilt`` call, every region with its own
filter."""

import numpy as np

from .buffereddata import BufferedData


class BufferedEventFilter(BufferedData):
    """A copy of its source in which every region of ``set_events`` is replaced by
    ``float32(scipy.signal.sosfiltfilt(sos_r, source[start:stop, channel]))``.  One frame per source frame, shape
    (frames, channels).

    `regions` is the (R, 3) int64 table of channel, start, stop in absolute frames and `sos` the (R, S, 6) filters, as
    set_events left them.  After every update of the buffer the regions that lie wholly inside it are filtered;
    regions cut by the buffer's border stay unfiltered -- a filter's history starts at the region's own border, half a
    region cannot be filtered -- and their rows of `regions` are listed in `skipped`.  Whatever moves the buffer
    recomputes the whole buffer: a copy on the device and one call."""

    def __init__(self, name='eventfiltered', source='envelope', panel='trace', color='#ee00ee', lw_thin=2.5, lw_thick=4):
        BufferedData.__init__(self, name, source, panel=panel, panel_type='trace', color=color, lw_thin=lw_thin,
                              lw_thick=lw_thick)
        self.regions = np.zeros((0, 3), dtype=np.int64)
        self.sos = np.zeros((0, 1, 6))
        self.clamp = False
        self.skipped = []

    def open(self, source):
        self._require_trace_source(source)
        BufferedData.open(self, source, 1)

    def set_events(self, events, freqs, min_duration, factor=4.0, order=1, clamp=False):
        """The events to smooth (an Events object in frames of this trace's rate) and their frequencies (one array per
        channel, as TraceGraph.event_peak_freqs returns them): every event widened by round(2 * min_duration * rate)
        frames (refine.widen_events: widened events never overlap) and given the Butterworth low-pass of `order` at
        factor * its frequency (refine.event_filters); events without a frequency, or with a cut-off at or beyond
        rate/2, are left alone.  ValueError when a widened event is not longer than its filter's padlen.  Recomputes
        this trace and what hangs below it, never the source."""
        from .refine import event_filters, padlen, widen_events
        width = int(round(2.0*min_duration*self.rate))
        rows, tables = [], []
        for c in range(events.channels):
            on, off = widen_events(events.onsets[c], events.offsets[c], self.frames, width)
            sos, valid = event_filters(freqs[c], self.rate, factor, order)
            if len(sos) != len(on):
                raise ValueError('channel %d: %d frequencies for %d events' % (c, len(sos), len(on)))
            for i in np.flatnonzero(valid):
                rows.append((c, int(on[i]), int(off[i])))
                tables.append(sos[i])
        regions = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        sos = np.asarray(tables, dtype=np.float64).reshape(len(rows), -1, 6) if rows else np.zeros((0, 1, 6))
        if len(regions) and np.any(regions[:, 2] - regions[:, 1] <= padlen(sos)):
            raise ValueError('a widened event is not longer than the padlen of its filter')
        self.regions, self.sos, self.clamp = regions, sos, bool(clamp)
        self.recompute_all()

    def load_buffer(self, offset, nframes, buffer):
        """Whatever span is asked for, the WHOLE buffer is copied from the source again and its regions filtered: a
        region that was cut by the old border and is whole now must be filtered from unfiltered samples, and one that
        was whole must not be filtered twice."""
        n = len(self._hostbuf)
        if n == 0:
            return
        BufferedData.load_buffer(self, self.offset, n, self._hostbuf)
        lo, hi = self.offset, self.offset + n
        a, b = self.regions[:, 1], self.regions[:, 2]
        inside = (a >= lo) & (b <= hi)
        cut = ~inside & (a < hi) & (b > lo)
        self.skipped = [tuple(int(v) for v in row) for row in self.regions[cut]]
        if inside.any():
            self.region_filtfilt(self.regions[inside], self.sos[inside], self.clamp, out=self)

    def process(self, source, dest, nbefore):
        """dest[i, c] = source[nbefore + i, c]."""
        from . import hipdsp
        n = len(dest)
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if n == 0:
            return
        on_mirror = self._source_mirror(call, nbefore)
        if on_mirror is not None:
            x, spitch = on_mirror
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            hipdsp.memcpy2d(self.ctx, ddst, 4*dpitch, x, 4*spitch, 4*n, self.channels)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph)
        dest[...] = np.asarray(source[nbefore:nbefore + n], dtype=np.float64)
        self._host_wrote(call)
