"""Frequency contours of events: what a user reads off the spectrogram of a call -- where it starts and ends in
frequency, how far it sweeps, whether it is tonal -- reduced from the per-frame spectral features
(``hipdsp_spectral_features``: ONE launch over the spectrogram frames the events span) on the host, over the few
floats per frame that come back.

An event [t_on, t_off) owns the spectrogram frames whose centre (t*hop + nfft/2)/rate lies in it.  A frame is
*unmasked* when its PEAK_FREQ is not NaN, i.e. its peak power is finite and above the floor.

``Contours`` is what ``TraceGraph.event_contours`` returns; ``ContourAnalyzer`` (analyzer.py) stores its fields."""

import numpy as np

# the features an event's contour is reduced from, and the fields of Contours in the order of ContourAnalyzer's columns
CONTOUR_FEATURES = ('peak_freq', 'peak_power', 'centroid', 'bandwidth', 'flatness', 'freq_low', 'freq_high')
FIELDS = ('start_freq', 'end_freq', 'min_freq', 'max_freq', 'peak_freq', 'low_freq', 'high_freq', 'centroid',
          'bandwidth', 'flatness', 'n_frames', 'voiced')


def centre_frames(t_on, t_off, rate, nfft, hop, nframes):
    """Frames [a, b) of a spectrogram (`nfft`, `hop`, source `rate`, `nframes` frames) whose centre
    (t*hop + nfft/2)/rate lies in [t_on, t_off)."""
    def first_at_or_after(time):
        t = int(np.ceil((time*rate - 0.5*nfft)/hop))
        while (t*hop + 0.5*nfft)/rate < time:
            t += 1
        while ((t - 1)*hop + 0.5*nfft)/rate >= time:
            t -= 1
        return min(max(t, 0), int(nframes))
    a = first_at_or_after(float(t_on))
    return a, max(a, first_at_or_after(float(t_off)))


def frame_table(rows, rate, nfft, hop, nframes):
    """(R, 3) int64 rows (channel, a, b) of spectrogram frames for the (channel, t_on, t_off) `rows` in seconds."""
    tab = [(int(c),) + centre_frames(t0, t1, rate, nfft, hop, nframes) for c, t0, t1 in rows]
    return np.array(tab, dtype=np.int64).reshape(-1, 3)


def _weighted(values, weights):
    ok = ~np.isnan(values) & ~np.isnan(weights)
    total = float(np.sum(weights[ok]))
    return float(np.sum(values[ok]*weights[ok])/total) if total > 0 else np.nan


class Contours(object):
    """The contours of R events.  `table`: (R, 3) rows (channel, a, b) of absolute spectrogram frames; `features`:
    ``{name: (m, channels)}`` of CONTOUR_FEATURES for the frames [first, first + m), which cover every row; frame t is
    centred at ``t0 + t*dt`` seconds.  Every field of FIELDS is an array over the events:

    start_freq / end_freq   PEAK_FREQ at the first / last unmasked frame
    min_freq / max_freq     nanmin / nanmax of PEAK_FREQ
    peak_freq               PEAK_FREQ at the frame of the largest PEAK_POWER (the first of equal ones)
    low_freq / high_freq    nanmin of FREQ_LOW / nanmax of FREQ_HIGH
    centroid, bandwidth, flatness   means over the unmasked frames, weighted by PEAK_POWER
    n_frames, voiced        the event's frames, and the share of them that is unmasked

    An event without an unmasked frame has NaN everywhere and voiced 0."""

    def __init__(self, table, first, features, t0=0.0, dt=1.0, trace_name=None):
        self.table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
        self.first, self.t0, self.dt, self.trace_name = int(first), float(t0), float(dt), trace_name
        self.features = {name: np.asarray(features[name], dtype=np.float64) for name in CONTOUR_FEATURES}
        R = len(self.table)
        for name in FIELDS:
            setattr(self, name, np.full(R, np.nan))
        self.n_frames = np.zeros(R, dtype=np.int64)
        self.voiced = np.zeros(R)
        for i in range(R):
            self._reduce(i)

    def __len__(self):
        return len(self.table)

    def _rows(self, i):
        c, a, b = self.table[i].tolist()
        return {name: v[a - self.first:b - self.first, c] for name, v in self.features.items()}

    def _reduce(self, i):
        f = self._rows(i)
        pf, power = f['peak_freq'], f['peak_power']
        live = np.flatnonzero(~np.isnan(pf))
        self.n_frames[i] = len(pf)
        if len(live) == 0:
            return
        self.voiced[i] = len(live)/len(pf)
        self.start_freq[i], self.end_freq[i] = pf[live[0]], pf[live[-1]]
        self.min_freq[i], self.max_freq[i] = np.min(pf[live]), np.max(pf[live])
        self.peak_freq[i] = pf[live[np.argmax(power[live])]]
        self.low_freq[i], self.high_freq[i] = np.nanmin(f['freq_low'][live]), np.nanmax(f['freq_high'][live])
        for name in ('centroid', 'bandwidth', 'flatness'):
            getattr(self, name)[i] = _weighted(f[name][live], power[live])

    def contour(self, i):
        """(times in seconds, PEAK_FREQ) of the frames of event `i`, NaN where a frame is masked."""
        c, a, b = self.table[i].tolist()
        return self.t0 + np.arange(a, b)*self.dt, self.features['peak_freq'][a - self.first:b - self.first, c].copy()

    def row(self, i):
        """The fields of event `i` in the order of FIELDS."""
        return [getattr(self, name)[i].item() for name in FIELDS]
