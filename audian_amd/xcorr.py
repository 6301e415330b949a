"""Event cross-correlation across channels: which channel an event belongs to, and how much later it arrived elsewhere.
The reference's ``songdetector.py`` ends on the problem ("crosstalk in front of songs in trace 0", its last two lines)
and has no code for it: on an array of microphones a song on channel 3 also crosses the threshold on channels 2 and 4,
and ``detect_songs`` reports one animal's song as three events.  ``BufferedCommonReference`` removes what is common to
ALL channels; it cannot remove a neighbour.

The primitive is the windowed correlation coefficient of an event against other channels over a small range of lags.
Its contract is the definition in ``include/hip_dsp.h`` (hipdsp_region_xcorr), which is ``np.corrcoef(a, b_l)[0, 1]``
per lag l with a = x[c, start:stop] and b_l = x[p, start+l:stop+l]; tests/xcorr_definition.py restates it in long double.

Sign convention: a POSITIVE lag means the partner carries the same waveform LATER, so the event's channel leads.

``host_region_xcorr`` is that definition in numpy float64 on two rows (the fallback of ``BufferedArray.region_xcorr``);
``CrossCorrelation`` is what ``region_xcorr`` returns; ``attribute_events`` is the rule that names an event's source.
"""

import numpy as np

MAX_LAG = 1024                          # what hipdsp_region_xcorr serves to either side


def host_region_xcorr(row_a, row_b, start, stop, max_lag):
    """(r (2 max_lag + 1,) float32, info (4,) float64) of the window [start, stop) of row_a against row_b (float32 rows
    of equal length): per lag the correlation coefficient from pivot-shifted float64 sums, NaN where the shifted window
    leaves the row, where a window is constant, or where it holds a NaN or an infinity; info is the number of lags with a
    value, the position of the largest (first occurrence, -1 for none), std of the window and std of row_b's there."""
    L = int(max_lag)
    frames, n = len(row_a), int(stop) - int(start)
    r = np.full(2*L + 1, np.nan, dtype=np.float32)
    info = np.array([0.0, -1.0, np.nan, np.nan])
    if n < 1:
        return r, info
    a = np.asarray(row_a[start:stop], dtype=np.float32)
    if not np.isfinite(a).all():
        return r, info
    d = a.astype(np.float64) - float(a[0])
    ma = d.sum()/n
    va = max(np.dot(d, d)/n - ma*ma, 0.0)
    info[2] = np.sqrt(va)
    Kb = float(row_b[start]) if np.isfinite(row_b[start]) else 0.0
    lo, hi = max(-L, -int(start)), min(L, frames - int(stop))
    wide = np.asarray(row_b[start + lo:stop + hi], dtype=np.float32)
    e_all = wide.astype(np.float64) - Kb
    bad = np.concatenate(([0], np.cumsum(~np.isfinite(wide))))
    sdb = np.full(2*L + 1, np.nan)
    for l in range(lo, hi + 1):
        k = l - lo
        if bad[k + n] != bad[k]:
            continue
        e = e_all[k:k + n]
        mb = e.sum()/n
        vb = max(np.dot(e, e)/n - mb*mb, 0.0)
        sdb[L + l] = np.sqrt(vb)
        if va > 0.0 and vb > 0.0:
            r[L + l] = min(max((np.dot(d, e)/n - ma*mb)/(np.sqrt(va)*np.sqrt(vb)), -1.0), 1.0)
    has = ~np.isnan(r)
    info[0] = np.count_nonzero(has)
    if has.any():
        info[1] = int(np.nanargmax(r))
        info[3] = sdb[int(info[1])]
    return r, info


class CrossCorrelation(object):
    """The correlations of a list of regions with a list of partner channels: ``table`` (R, 3) int64 of channel, start,
    stop (absolute frames of the trace), ``partners`` (P,) channel ids, ``r[i]`` the (P, 2 max_lag + 1) float32
    coefficients of region i (NaN where there is none), ``info`` (R, P, 4) as hipdsp_region_xcorr gives it, ``max_lag``
    in frames, ``rate`` the trace's.  A positive lag: the partner carries the waveform later than the region's channel."""

    def __init__(self, table, partners, r, info, max_lag, rate, trace_name=None):
        self.table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
        self.partners = np.asarray(partners, dtype=np.int64).reshape(-1)
        self.max_lag, self.rate = int(max_lag), float(rate)
        R, P, W = len(self.table), len(self.partners), 2*self.max_lag + 1
        self.r = np.asarray(r, dtype=np.float32).reshape(R, P, W)
        self.info = np.asarray(info, dtype=np.float64).reshape(R, P, 4)
        self.trace_name = trace_name

    def __len__(self):
        return len(self.table)

    @property
    def lags(self):
        """The lags of the columns of r in frames: -max_lag ... max_lag."""
        return np.arange(-self.max_lag, self.max_lag + 1)

    def best_lag(self, i):
        """The lag in frames of the largest coefficient of region i, per partner: (P,) float64, NaN where no lag has one."""
        pos = self.info[i, :, 1]
        return np.where(pos >= 0, pos - self.max_lag, np.nan)

    def best_r(self, i):
        """The largest coefficient of region i, per partner: (P,) float64, NaN where no lag has one."""
        pos = self.info[i, :, 1].astype(np.int64)
        return np.where(pos >= 0, self.r[i, np.arange(len(self.partners)), np.maximum(pos, 0)].astype(np.float64), np.nan)

    def delays(self, i):
        """best_lag in seconds: how much later the partner carries the waveform."""
        return self.best_lag(i)/self.rate

    def std_event(self, i):
        """The standard deviation of region i's own window, once per partner: (P,)."""
        return self.info[i, :, 2]

    def std_partner(self, i):
        """The standard deviation of the partner's window at best_lag: (P,), NaN where no lag has a coefficient."""
        return self.info[i, :, 3]


def attribute_table(xc, min_r=0.5, min_ratio=1.0):
    """The rule of attribute_events over the rows of a CrossCorrelation: (source channel (R,) int64, delay in seconds
    (R,), correlation (R,)) -- for an event that is its own source its own channel, 0 and 1."""
    R = len(xc)
    sources, delays, corr = xc.table[:, 0].copy(), np.zeros(R), np.ones(R)
    for i in range(R):
        c = xc.table[i, 0]
        r, loud, quiet = xc.best_r(i), xc.std_partner(i), xc.std_event(i)
        with np.errstate(invalid='ignore'):
            ok = (xc.partners != c) & (r >= min_r) & (loud >= min_ratio*quiet)         # NaN passes no comparison
        if ok.any():
            idx = np.flatnonzero(ok)
            j = idx[np.lexsort((xc.partners[idx], -loud[idx]))[0]]                       # the loudest, then the lowest channel
            sources[i], delays[i], corr[i] = xc.partners[j], xc.delays(i)[j], r[j]
    return sources, delays, corr


def event_table(events, scale=1.0):
    """(R, 3) int64 rows of channel, onset, offset of an Events object, channel by channel in the events' order, in frames
    of a trace whose rate is `scale` times the events'."""
    rows = []
    for c in range(events.channels):
        for a, b in zip(events.onsets[c], events.offsets[c]):
            rows.append((c, int(np.floor(a*scale)), int(np.ceil(b*scale))) if scale != 1.0 else (c, int(a), int(b)))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def attribute_events(events, xc, min_r=0.5, min_ratio=1.0):
    """Which channel every event belongs to.  `xc` is the CrossCorrelation of the events (one row per event, channel by
    channel in the events' order, as TraceGraph.event_cross_correlation returns it).  An event on channel c is
    crosstalk when some partner p != c has best_r >= min_r and std_partner >= min_ratio * std_event: the same waveform,
    at least as loud, on another channel.  Its source is the one such partner with the largest std_partner, the lowest
    channel among equally loud ones; otherwise the source is c itself.  An undefined (NaN) correlation or standard
    deviation never makes an event crosstalk.
    The defaults min_r = 0.5 and min_ratio = 1.0 are a choice, NOT calibrated on recordings.
    Returns (own, sources, delays): the Events that are their own source, and for ALL events per channel the source
    channel (int64) and how much later than the event the source carries the waveform in seconds (0 for an own event; a
    negative delay: the source leads)."""
    from .events import Events
    if len(xc) != len(events):
        raise ValueError('%d correlations for %d events' % (len(xc), len(events)))
    owner = np.concatenate([np.full(len(events.onsets[c]), c, dtype=np.int64) for c in range(events.channels)]
                           + [np.zeros(0, dtype=np.int64)])
    if not np.array_equal(owner, xc.table[:, 0]):
        raise ValueError('the correlations are not those of these events, channel by channel')
    src, dly, _ = attribute_table(xc, min_r, min_ratio)
    sources = [src[owner == c] for c in range(events.channels)]
    delays = [dly[owner == c] for c in range(events.channels)]
    own = Events([events.frames(c)[sources[c] == c] for c in range(events.channels)], events.rate, events.trace_name)
    return own, sources, delays
