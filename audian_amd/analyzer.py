"""Region analysis: audian's ``Analyzer`` plug-in surface (``src/audian/analyzer.py``,
``src/audian/statisticsanalyzer.py``) without Qt, on top of regions that are reduced on the
device.

The reference cuts every trace to the selected region (``Data.get_region``, data.py:102-118) and hands the cuts to
every ``Analyzer.analyze(t0, t1, channel, traces)`` (analyzer.py:100; driven by ``DataBrowser.analyze_region``,
databrowser.py:1759-1775).  Here ``TraceGraph.get_region`` hands out ``Region`` objects instead of arrays: a
``Region`` looks like ``trace[i0:i1, channel]``, but ``np.mean``, ``np.std``, ``np.min``, ``np.max``,
``np.argmin`` and ``np.argmax`` of it -- numpy calls the object's own methods for anything that is not an
ndarray -- are served by ONE ``hipdsp_region_stats`` launch over the trace's device mirror, and 64 bytes come
back.  Only an analyzer that indexes the region (or asks numpy for anything else) makes it an array, once.

The event surface (``make_trace_events``, ``make_panel_events``, ``set_events``, ``add_events``; analyzer.py:186-308)
is there without Qt: where the reference keeps one ``pyqtgraph.ScatterPlotItem`` per channel, ``events[name][channel]``
holds the marker coordinates as a plain ``(x, y)`` pair of arrays and ``event_styles[name]`` what the item would have
been given.  ``TraceGraph.detect_events`` / ``analyze_events`` supply the events of a trace and analyze their regions.

What is left out: thunderlab's ``TableData`` (a plain column / row table stands in for it), the drawing of the event
markers and the Qt table dialog.
"""

from math import floor, log10

import numpy as np


class Region(object):
    """Frames [i0, i1) of one channel of a trace, as ``Data.get_region`` cuts them (data.py:112), lazily.

    ``shape``, ``ndim``, ``dtype`` (float64) and ``len()`` touch nothing.  ``mean / std / min / max / argmin /
    argmax`` with the arguments numpy's free functions pass (``axis=None, dtype=None, out=None, ddof=0``) come from
    one cached ``trace.region_stats`` call; with any other argument, and for indexing, ``np.asarray`` and every
    other attribute, the region becomes ``trace[i0:i1, channel]`` (once; ``materialised`` counts it) and numpy
    does the rest."""

    materialised = 0           # how many regions have become arrays in this process (tests read it)

    def __init__(self, trace, i0, i1, channel):
        self._trace, self._channel = trace, channel
        self._i0, self._i1 = int(i0), max(int(i0), int(i1))
        self._data = None
        self._slots = None

    @property
    def shape(self):
        return (self._i1 - self._i0,) + tuple(self._trace.shape[2:])

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    dtype = np.dtype(np.float64)

    def __len__(self):
        return self._i1 - self._i0

    def _materialise(self):
        if self._data is None:
            self._data = np.asarray(self._trace[self._i0:self._i1, self._channel], dtype=np.float64)
            Region.materialised += 1
        return self._data

    def _stats(self):
        """The eight slots of BufferedData.region_stats for this region (one launch, cached)."""
        if self._slots is None:
            self._trace.update_buffer(self._i0, self._i1)        # what trace[i0:i1] does before it reads
            self._slots = self._trace.region_stats([(self._i0, self._i1)], self._channel)[0]
        return self._slots

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self._materialise(), dtype=dtype)

    def __getitem__(self, key):
        return self._materialise()[key]

    def __iter__(self):
        return iter(self._materialise())

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self._materialise(), name)

    def _plain(self, axis, dtype, out, kwargs):
        """Is this the call of numpy's free function with nothing but its defaults, on a region that has samples?"""
        rest = {k: v for k, v in kwargs.items()
                if not ((k == 'keepdims' and v is False) or (k == 'where' and v is True) or (k == 'ddof' and v == 0))}
        return axis is None and dtype is None and out is None and not rest and self.size > 0

    def mean(self, axis=None, dtype=None, out=None, **kwargs):
        if self._plain(axis, dtype, out, kwargs):
            return np.float64(self._stats()[1])
        return np.mean(self._materialise(), axis=axis, dtype=dtype, out=out, **kwargs)

    def std(self, axis=None, dtype=None, out=None, ddof=0, **kwargs):
        if self._plain(axis, dtype, out, dict(kwargs, ddof=ddof)):
            return np.float64(self._stats()[2])
        return np.std(self._materialise(), axis=axis, dtype=dtype, out=out, ddof=ddof, **kwargs)

    def min(self, axis=None, out=None, **kwargs):
        if self._plain(axis, None, out, kwargs):
            return np.float64(self._stats()[3])
        return np.min(self._materialise(), axis=axis, out=out, **kwargs)

    def max(self, axis=None, out=None, **kwargs):
        if self._plain(axis, None, out, kwargs):
            return np.float64(self._stats()[4])
        return np.max(self._materialise(), axis=axis, out=out, **kwargs)

    def argmin(self, axis=None, out=None, **kwargs):
        if self._plain(axis, None, out, kwargs):
            return np.intp(self._stats()[5])
        return np.argmin(self._materialise(), axis=axis, out=out, **kwargs)

    def argmax(self, axis=None, out=None, **kwargs):
        if self._plain(axis, None, out, kwargs):
            return np.intp(self._stats()[6])
        return np.argmax(self._materialise(), axis=axis, out=out, **kwargs)


class Table(object):
    """Columns with a label, a unit and a format, and rows of values: the part of thunderlab's TableData the
    analyzers use (``append``, ``add``, ``clear_data``, ``rows``, ``columns``)."""

    def __init__(self):
        self.labels, self.units, self.formats = [], [], []
        self.data = []

    def append(self, label, unit=None, formats=None):
        self.labels.append(label)
        self.units.append(unit or '')
        self.formats.append(formats or '%g')

    def add(self, values, column=0):
        values = list(values)
        if column != 0 or len(values) != len(self.labels):
            raise ValueError(f'{len(values)} values for {len(self.labels)} columns')
        self.data.append(values)

    def clear_data(self):
        self.data = []

    def rows(self):
        return len(self.data)

    def columns(self):
        return len(self.labels)

    def __len__(self):
        return len(self.data)

    def write_csv(self, path):
        with open(path, 'w') as f:
            f.write(','.join(f'{lb}/{u}' if u else lb for lb, u in zip(self.labels, self.units)) + '\n')
            for row in self.data:
                f.write(','.join(fm % v if isinstance(v, (int, float, np.number)) else str(v)
                                 for fm, v in zip(self.formats, row)) + '\n')


class Analyzer(object):
    """Base class for analyzing selected regions (analyzer.py:13-308, the event markers as plain arrays): implement
    ``analyze()``; the constructor adds columns with ``make_column()``, ``analyze()`` fills a row with
    ``store()``.  `graph` is the TraceGraph (the reference passes its DataBrowser); the analyzer registers
    itself there."""

    def __init__(self, graph, name, source_name):
        self.graph = graph
        self.name = name
        self.source_name = source_name
        self.source = self.trace(self.source_name)
        self.data = Table()
        self.events = {}
        self.event_styles = {}
        graph.add_analyzer(self)

    def clear(self):
        """Clear the data table and the markers (analyzer.py:91-97)."""
        self.data.clear_data()
        for name in self.events:
            for c in range(len(self.events[name])):
                self.events[name][c] = self._no_events()

    def analyze(self, t0, t1, channel, traces):
        """Called for every analyzed region with ``traces[name] = (time, data)`` -- ``(time, frequencies, data)``
        for a spectrogram -- of `channel` between `t0` and `t1`; `data` is a Region."""
        pass

    def analyze_many(self, regions, channels):
        """The table rows of many regions and channels at once (TraceGraph.analyze_regions): return False to be
        called region by region through analyze() instead."""
        return False

    def traces(self):
        return [t.name for t in self.graph.traces]

    def trace(self, name):
        return self.graph[name]

    def make_column(self, label, unit=None, formats=None):
        self.data.append(label, unit, formats)

    def store(self, *args):
        self.data.add(args, 0)

    # ---- event markers (analyzer.py:186-308) without plot items ------------------------
    @staticmethod
    def _no_events():
        return np.zeros(0), np.zeros(0)

    def _make_events(self, name, style):
        self.events[name] = [self._no_events() for c in range(self.graph.data.channels)]
        self.event_styles[name] = style

    def make_trace_events(self, name, trace_name, symbol, color, size):
        """Prepare events `name` for marking on top of a trace: one (x, y) pair of arrays per channel."""
        self._make_events(name, dict(trace=trace_name, panel=None, symbol=symbol, color=color, size=size))

    def make_panel_events(self, name, panel_name, symbol, color, size):
        """Prepare events `name` for marking in a panel: one (x, y) pair of arrays per channel."""
        self._make_events(name, dict(trace=None, panel=panel_name, symbol=symbol, color=color, size=size))

    def set_events(self, name, channel, x, y):
        """Set the markers of `channel` (all channels if negative); those of the other channels are erased."""
        for c in range(len(self.events[name])):
            if c == channel or channel < 0:
                self.events[name][c] = (np.array(x, dtype=np.float64).reshape(-1), np.array(y, dtype=np.float64).reshape(-1))
            else:
                self.events[name][c] = self._no_events()

    def add_events(self, name, channel, x, y):
        """Add markers to `channel` (all channels if negative); nothing is erased."""
        for c in range(len(self.events[name])):
            if c == channel or channel < 0:
                ox, oy = self.events[name][c]
                self.events[name][c] = (np.concatenate((ox, np.asarray(x, dtype=np.float64).reshape(-1))),
                                        np.concatenate((oy, np.asarray(y, dtype=np.float64).reshape(-1))))

    def rows(self):
        """The stored rows, a list of lists in the order of the columns."""
        return [list(row) for row in self.data.data]

    def save_csv(self, path):
        """The table as CSV: a header line of ``label/unit``, then the rows in the columns' formats."""
        self.data.write_csv(path)


class PlainAnalyzer(Analyzer):
    """Stores start, end and duration of the region and the channel (analyzer.py:311-343)."""

    def __init__(self, graph):
        super().__init__(graph, 'plain', 'data')
        nd = max(0, int(floor(-log10(1/self.source.rate))))
        self.make_column('tstart', 's', f'%.{nd}f')
        self.make_column('tend', 's', f'%.{nd}f')
        self.make_column('duration', 's', f'%.{nd}f')
        self.make_column('channel', '', '%.0f')

    def analyze(self, t0, t1, channel, traces):
        self.store(t0, t1, t1 - t0, channel)

    def analyze_many(self, regions, channels):
        for t0, t1 in regions:
            for c in channels:
                self.store(t0, t1, t1 - t0, c)
        return True


class StatisticsAnalyzer(Analyzer):
    """Mean and standard deviation of the region of one trace (statisticsanalyzer.py:6-20)."""

    def __init__(self, graph, source_name='filtered'):
        super().__init__(graph, 'statistics', source_name)
        nd = max(0, int(-np.floor(np.log10(self.source.ampl_max/4e4))))
        us = self.source.unit
        self.make_column(f'{self.source_name} mean', us, f'%.{nd}f')
        self.make_column(f'{self.source_name} stdev', us, f'%.{nd}f')

    def analyze(self, t0, t1, channel, traces):
        source = traces[self.source_name][-1]      # the reference's [1]; for a spectrogram that is the frequencies
        self.store(np.mean(source), np.std(source))

    def analyze_many(self, regions, channels):
        trace = self.source
        spans = [self.graph.region_frames(trace, t0, t1) for t0, t1 in regions]
        if spans:
            trace.update_buffer(min(a for a, b in spans), max(b for a, b in spans))
        stats = trace.region_stats(spans)                       # 16 regions per launch
        for k in range(len(spans)):
            for c in channels:
                self.store(stats[k, c, 1], stats[k, c, 2])
        return True


class PeakFrequencyAnalyzer(Analyzer):
    """Frequency and power of the main spectral peak of the region of one trace: env_freqs of the reference's
    songdetector.py (songdetector.py:146-152) as an analyzer -- on the filtered trace the carrier of a call, on an
    envelope the pulse rate of a song (BufferedArray.peak_freqs: Welch spectrum with a window of rate/freq_resolution
    samples or the largest power of two the region holds; `thresh` in dB of prominence, None for the largest bin).  The
    frequency is NaN for a region shorter than min_nfft samples."""

    def __init__(self, graph, source_name='filtered', freq_resolution=10.0, thresh=None, min_nfft=16, max_nfft=8192,
                 step=1):
        super().__init__(graph, 'peak frequency', source_name)
        self.freq_resolution, self.thresh = float(freq_resolution), thresh
        self.min_nfft, self.max_nfft, self.step = int(min_nfft), int(max_nfft), int(step)
        us = self.source.unit
        self.make_column('peak frequency', 'Hz', '%.2f')
        self.make_column('peak power', f'{us}^2/Hz' if us else '1/Hz', '%.4g')

    def _peaks(self, table):
        trace = self.source
        if table:
            trace.update_buffer(min(a for c, a, b in table), max(b for c, a, b in table))
        freqs, powers = trace.peak_freqs(table, self.freq_resolution, self.min_nfft, self.max_nfft, self.thresh,
                                         self.step, powers=True)
        return freqs, powers

    def analyze(self, t0, t1, channel, traces):
        i0, i1 = self.graph.region_frames(self.source, t0, t1)
        freqs, powers = self._peaks([(channel, i0, i1)])
        self.store(float(freqs[channel][0]), float(powers[channel][0]))

    def analyze_many(self, regions, channels):
        spans = [self.graph.region_frames(self.source, t0, t1) for t0, t1 in regions]
        # one device call per nfft for all regions and channels; the rows come back per channel in region order
        freqs, powers = self._peaks([(c, a, b) for a, b in spans for c in channels])
        for k in range(len(spans)):
            for c in channels:
                self.store(float(freqs[c][k]), float(powers[c][k]))
        return True


class CrossCorrelationAnalyzer(Analyzer):
    """The source channel of the region of one trace, how much later than the region the source carries it, and their
    correlation (xcorr.attribute_events over BufferedArray.region_xcorr): for every region of a channel the other
    channels are searched, over the lags of +-`max_delay` seconds, for the same waveform at least `min_ratio` times as
    loud and correlated by at least `min_r`.  A region that is its own source stores its own channel, 0 and 1.  The two
    thresholds are not calibrated on recordings."""

    def __init__(self, graph, source_name='filtered', max_delay=0.001, min_r=0.5, min_ratio=1.0, channels=None):
        super().__init__(graph, 'cross correlation', source_name)
        from .xcorr import MAX_LAG
        self.max_lag = int(round(float(max_delay)*self.source.rate))
        if self.max_lag < 0 or self.max_lag > MAX_LAG:
            raise ValueError('max_delay %g s is %d frames: at most %d' % (max_delay, self.max_lag, MAX_LAG))
        self.min_r, self.min_ratio, self.channels = float(min_r), float(min_ratio), channels
        nd = max(0, int(floor(-log10(1/self.source.rate))))
        self.make_column('source channel', '', '%.0f')
        self.make_column('delay', 's', f'%.{nd}f')
        self.make_column('correlation', '', '%.3f')

    def _attribute(self, table):
        from .xcorr import attribute_table
        trace = self.source
        if table:
            trace.update_buffer(min(a for c, a, b in table), max(b for c, a, b in table))
        return attribute_table(trace.region_xcorr(table, self.channels, self.max_lag), self.min_r, self.min_ratio)

    def analyze(self, t0, t1, channel, traces):
        i0, i1 = self.graph.region_frames(self.source, t0, t1)
        src, delay, corr = self._attribute([(channel, i0, i1)])
        self.store(int(src[0]), float(delay[0]), float(corr[0]))

    def analyze_many(self, regions, channels):
        spans = [self.graph.region_frames(self.source, t0, t1) for t0, t1 in regions]
        # one device call for all regions and channels, the rows in region-major order
        src, delay, corr = self._attribute([(c, a, b) for a, b in spans for c in channels])
        for k in range(len(src)):
            self.store(int(src[k]), float(delay[k]), float(corr[k]))
        return True


class ContourAnalyzer(Analyzer):
    """The frequency contour of the region on a spectrogram (TraceGraph.region_contours; contours.Contours has the
    definitions): where the call starts, ends and peaks in frequency, its lowest and highest frequency, the extent
    `drop_db` below the peak, power-weighted centroid, bandwidth and flatness, the region's frames and the share of them
    with a peak above `min_power`.  One row per region and channel; NaN where no frame is above the floor."""

    def __init__(self, graph, source_name='spectrogram', fmin=0.0, fmax=None, min_power=1e-20, drop_db=10.0):
        super().__init__(graph, 'contour', source_name)
        from .contours import FIELDS
        from .hipdsp import drop_ratio
        drop_ratio(drop_db)
        self.fmin, self.fmax, self.min_power, self.drop_db = fmin, fmax, float(min_power), float(drop_db)
        for name in FIELDS:
            if name in ('n_frames', 'voiced', 'flatness'):
                self.make_column(name.replace('_', ' '), '', '%.0f' if name == 'n_frames' else '%.3f')
            else:
                self.make_column(name.replace('_', ' '), 'Hz', '%.1f')

    def _store(self, rows):
        contours = self.graph.region_contours(rows, self.source_name, self.fmin, self.fmax, self.min_power, self.drop_db)
        for i in range(len(contours)):
            self.store(*contours.row(i))

    def analyze(self, t0, t1, channel, traces):
        self._store([(channel, t0, t1)])

    def analyze_many(self, regions, channels):
        # one device call for all regions and channels, the rows in region-major order
        self._store([(c, t0, t1) for t0, t1 in regions for c in channels])
        return True
