"""Threshold events of a trace: what the reference's ``songdetector.py`` does between an envelope and the analysis of
its events (``detect_songs``, songdetector.py:113-139: threshold crossings per channel, ``merge_events`` below a minimum
distance, ``remove_events`` below a minimum duration), and the reference's open item "Add events ... / Provide
interface for event detectors" (README.md:66-69).  thunderlab, which supplies ``merge_events`` / ``remove_events``, is
neither installed nor part of the reference tree: merging and filtering follow songdetector.py's use of them, parity
with thunderlab is unpinned.  The contract is the definition in ``include/hip_dsp.h`` (hipdsp_detect_events).

``host_detect_events`` is that definition in numpy on one row (the fallback of ``BufferedArray.detect_events``);
``Events`` is what ``BufferedData.detect_events`` returns.
"""

import numpy as np


def host_detect_events(row, threshold, min_gap, min_len, first=0):
    """(K, 2) int64 (onset, offset) pairs of one row: runs of ``float32(row) > float32(threshold)``, runs with at most
    `min_gap` samples between them merged, merged events shorter than `min_len` dropped; `first` is added to every
    position."""
    with np.errstate(all='ignore'):
        above = np.asarray(row, dtype=np.float32) > np.float32(threshold)
    edges = np.flatnonzero(above[1:] != above[:-1]) + 1
    if len(above) and above[0]:
        edges = np.concatenate(([0], edges))
    if len(above) and above[-1]:
        edges = np.concatenate((edges, [len(above)]))
    onsets, offsets = edges[0::2], edges[1::2]
    if len(onsets) > 1:
        apart = onsets[1:] - offsets[:-1] > int(min_gap)
        onsets = onsets[np.concatenate(([True], apart))]
        offsets = offsets[np.concatenate((apart, [True]))]
    keep = offsets - onsets >= int(min_len)
    return np.stack((onsets[keep], offsets[keep]), axis=1).astype(np.int64) + int(first)


class Events(object):
    """The events of every channel of a trace: ``onsets[c]`` and ``offsets[c]`` are int64 arrays of absolute frame
    indices of the trace, an event being frames [onset, offset); ``rate`` is the trace's."""

    def __init__(self, pairs, rate, trace_name=None):
        self.onsets = [np.asarray(p, dtype=np.int64).reshape(-1, 2)[:, 0].copy() for p in pairs]
        self.offsets = [np.asarray(p, dtype=np.int64).reshape(-1, 2)[:, 1].copy() for p in pairs]
        self.rate = float(rate)
        self.trace_name = trace_name

    @property
    def channels(self):
        return len(self.onsets)

    def __len__(self):
        return sum(len(o) for o in self.onsets)

    def frames(self, channel):
        """(K, 2) int64 (onset, offset) pairs of one channel."""
        return np.stack((self.onsets[channel], self.offsets[channel]), axis=1)

    def times(self, channel):
        """(onset times, offset times) in seconds: frame/rate."""
        return self.onsets[channel]/self.rate, self.offsets[channel]/self.rate

    def regions(self, channel):
        """(t0, t1) second pairs for TraceGraph.analyze_regions, chosen so that TraceGraph.region_frames -- ``int(t0*rate)``
        and ``int(t1*rate) + 1`` -- gives back exactly (onset, offset) on a trace of this rate: the middle of the first
        and of the last frame of the event.  Half a frame is far beyond the rounding of t*rate (2^-52 relative)."""
        return [((int(a) + 0.5)/self.rate, (int(b) - 0.5)/self.rate)
                for a, b in zip(self.onsets[channel], self.offsets[channel])]
