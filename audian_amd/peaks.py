"""Peaks of a trace: the local maxima of an envelope, a band-power or a kernel-filter trace with their heights and
prominences -- ``sig.find_peaks(envelopes[:,c])`` of the reference's ``songdetector.py`` (songdetector.py:110-115) --
which are the reference's point events: "Events are channel specific points. Plotted as dot at data amplitude. Many
events per label. Result from some analysis." (README.md:113-117).  The call is ``scipy.signal.find_peaks`` with its
``height``, ``threshold``, ``prominence`` and ``wlen`` arguments (pinned to scipy 1.15.3 by
``tests/golden/find_peaks.npz``); ``distance``, ``width``, ``rel_height`` and ``plateau_size`` are not part of it
(``distance`` is a greedy pass in order of height before the prominence: a later entry point on the compacted list).
thunderlab's ``detect_peaks`` is neither installed nor part of the reference tree: parity with it is unpinned.  The
contract is the definition in ``include/hip_dsp.h`` (hipdsp_find_peaks).

``host_find_peaks`` is that definition in numpy on one row (the fallback of ``BufferedArray.find_peaks``); ``Peaks`` is
what ``BufferedData.find_peaks`` returns.
"""

import numpy as np

_WINDOW = 32            # samples per side that host_find_peaks looks at for all peaks at once


def _inside(values, lo, hi):
    """lo <= values <= hi, an open border (-inf below, +inf above) not compared; a NaN border keeps nothing."""
    keep = np.ones(len(values), dtype=bool)
    with np.errstate(invalid='ignore'):
        if not lo == -np.inf:
            keep &= lo <= values
        if not hi == np.inf:
            keep &= values <= hi
    return keep


def _walk_one(v, m, lim, h, step):
    """(minimum, base) of scipy's walk from m towards lim (step -1: left, +1: right) while v[i] <= h, on slices that
    grow by a factor of four."""
    reach = 256
    while True:
        if step < 0:
            a = max(lim, m - reach)
            bad = np.flatnonzero(~(v[a:m] <= h))
            if len(bad) or a == lim:
                a = a + bad[-1] + 1 if len(bad) else a
                window = v[a:m + 1][::-1]
                break
        else:
            b = min(lim, m + reach)
            bad = np.flatnonzero(~(v[m + 1:b + 1] <= h))
            if len(bad) or b == lim:
                b = m + bad[0] if len(bad) else b
                window = v[m:b + 1]
                break
        reach *= 4
    k = int(np.argmin(window))                   # the first of equal minima: the nearest to m; 0 if nothing is lower
    return window[k], m + step*k


def _walk_all(v, m, lim, h, step):
    """The walks of all peaks towards one side: (minima, bases).  A window of _WINDOW samples decides most of them at
    once; the peaks whose walk goes on beyond it are walked one by one."""
    n, W = len(v), _WINDOW
    padded = np.concatenate((np.full(W, np.nan), v, np.full(W, np.nan)))
    pos = m[:, None] + step*(1 + np.arange(W))[None, :]
    vals = padded[pos + W]
    with np.errstate(invalid='ignore'):
        ok = (vals <= h[:, None]) & ((pos >= lim[:, None]) if step < 0 else (pos <= lim[:, None]))
    stopped = ~ok.all(axis=1)
    k = np.where(stopped, np.argmin(ok, axis=1), W)
    walked = np.where(np.arange(W)[None, :] < k[:, None], vals, np.inf)
    low = walked.min(axis=1) if W else np.full(len(m), np.inf)
    col = np.argmax(walked == low[:, None], axis=1)
    lower = low < h
    minima = np.where(lower, low, h)
    bases = np.where(lower, m + step*(1 + col), m)
    for i in np.flatnonzero(~stopped):
        minima[i], bases[i] = _walk_one(v, int(m[i]), int(lim[i]), h[i], step)
    return minima, bases


def host_find_peaks(row, height=None, threshold=None, prominence=None, wlen=None, first=0):
    """(positions, properties) of the peaks of one row: (K,) int64, ascending, `first` added, and (K, 4) float64 of
    height, prominence, left base, right base (bases with `first` added).  `height`, `threshold` and `prominence` are
    None (open) or a (lower, upper) pair of numbers, -inf / +inf or None an open border; `wlen` is in samples, None, 0
    and 1 the whole row.  The definition of hipdsp_find_peaks in include/hip_dsp.h."""
    v = np.asarray(row, dtype=np.float32).astype(np.float64).reshape(-1)
    n = len(v)
    borders = []
    for pair in (height, threshold, prominence):
        lo, hi = (None, None) if pair is None else pair
        borders.append((-np.inf if lo is None else float(lo), np.inf if hi is None else float(hi)))
    if n < 3:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 4))
    with np.errstate(invalid='ignore'):
        starts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1))    # runs of equal samples: [l, r]
        ends = np.concatenate((starts[1:] - 1, [n - 1]))
        inner = (starts >= 1) & (ends <= n - 2)
        l, r = starts[inner], ends[inner]
        peak = (v[l - 1] < v[l]) & (v[r + 1] < v[r])
        m = (l[peak] + r[peak])//2
        h = v[m]
        keep = _inside(h, *borders[0])
        tl, tr = h - v[m - 1], h - v[m + 1]
        keep &= _inside(tl, *borders[1]) & _inside(tr, *borders[1])            # numpy's min and max pass a NaN on
        m, h = m[keep], h[keep]
        lo, hi = np.zeros(len(m), dtype=np.int64), np.full(len(m), n - 1, dtype=np.int64)
        if wlen is not None and int(wlen) >= 2:
            lo, hi = np.maximum(m - int(wlen)//2, 0), np.minimum(m + int(wlen)//2, n - 1)
        lmin, lbase = _walk_all(v, m, lo, h, -1)
        rmin, rbase = _walk_all(v, m, hi, h, +1)
        prom = h - np.maximum(lmin, rmin)
    keep = _inside(prom, *borders[2])
    props = np.stack((h, prom, (lbase + int(first)).astype(np.float64), (rbase + int(first)).astype(np.float64)), axis=1)
    return (m[keep] + int(first)).astype(np.int64), props[keep]


class Peaks(object):
    """The peaks of every channel of a trace: ``indices[c]`` (int64, absolute frame indices of the trace, ascending),
    ``heights[c]``, ``prominences[c]`` (float64), ``left_bases[c]`` and ``right_bases[c]`` (int64 frame indices);
    ``rate`` is the trace's."""

    def __init__(self, results, rate, trace_name=None):
        """`results`: per channel (positions, (K, 4) properties)."""
        self.indices, self.heights, self.prominences, self.left_bases, self.right_bases = [], [], [], [], []
        for pos, props in results:
            props = np.asarray(props, dtype=np.float64).reshape(-1, 4)
            self.indices.append(np.asarray(pos, dtype=np.int64).reshape(-1).copy())
            self.heights.append(props[:, 0].copy())
            self.prominences.append(props[:, 1].copy())
            self.left_bases.append(props[:, 2].astype(np.int64))
            self.right_bases.append(props[:, 3].astype(np.int64))
        self.rate = float(rate)
        self.trace_name = trace_name

    @property
    def channels(self):
        return len(self.indices)

    def __len__(self):
        return sum(len(i) for i in self.indices)

    def times(self, channel):
        """Peak times in seconds: frame/rate."""
        return self.indices[channel]/self.rate

    def points(self, channel):
        """(times, heights): the (x, y) markers of the channel for Analyzer.add_events."""
        return self.times(channel), self.heights[channel]

    def in_events(self, events, channel):
        """For every event of the channel of an Events object (frames [onset, offset)) the number of peaks inside it:
        the pulses per song."""
        idx = self.indices[channel]
        return (np.searchsorted(idx, events.offsets[channel], side='left') -
                np.searchsorted(idx, events.onsets[channel], side='left')).astype(np.int64)
