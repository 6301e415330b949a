"""Refining detected events: what the reference's ``songdetector.py`` does with the pulse rates of its songs
(``clean_env_freqs``, songdetector.py:155-175; ``filter_envelopes``, :178-192; ``analyse_songs``, :195-244): songs with an
undefined or outlying pulse rate are dropped, the envelope inside every widened song is smoothed by a zero-phase
low-pass at four times that song's own pulse rate, and every song's borders are found again on the smoothed envelope
against a local threshold taken from the noise just outside it.

thunderlab, which supplies ``widen_events`` and ``threshold_crossings``, is neither installed nor part of the reference
tree: both are restated here from songdetector.py's use of them, parity with thunderlab is unpinned.  The two device
steps are ``hipdsp_region_filtfilt`` and ``hipdsp_region_crossings`` (the contracts are in ``include/hip_dsp.h``);
``host_region_filtfilt`` and ``host_region_crossings`` are those definitions in numpy float64, the fallbacks of
``BufferedArray.region_filtfilt`` / ``region_crossings`` for traces without a device mirror.

Two deviations from the reference, on purpose:

* ``len(envelopes[c])`` at songdetector.py:209 (the number of channels) is a slip for the trace's length: the window
  behind the last song ends at the trace's end here.
* An event that begins or ends above the threshold is reported at the window's border -- rule 2 of
  ``hipdsp_detect_events`` -- where thunderlab's ``threshold_crossings`` trims it to its first upward crossing.
"""

import numpy as np

from .events import Events


def widen_events(onsets, offsets, n, width):
    """(onsets, offsets) int64 of the events widened by `width` frames on both sides inside a trace of `n` frames: the
    first onset max(onset - width, 0), the last offset min(offset + width, n), between neighbours offset_i + width and
    onset_(i+1) - width -- or, where those would cross, both the middle (offset_i + onset_(i+1)) // 2 of the gap.
    Widened events never overlap (the events are ascending and do not overlap themselves)."""
    onsets = np.asarray(onsets, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    width = int(width)
    won, woff = onsets - width, offsets + width
    if len(onsets):
        won[0] = max(won[0], 0)
        woff[-1] = min(woff[-1], int(n))
        cross = np.flatnonzero(woff[:-1] > won[1:])
        mid = (offsets[:-1] + onsets[1:])//2
        woff[cross] = mid[cross]
        won[cross + 1] = mid[cross]
    return won, woff


def clean_event_freqs(events, freqs, fac=6.0):
    """clean_env_freqs of songdetector.py:155-175: over the frequencies of all channels together, mean and standard
    deviation of the non-NaN values between the quartiles (np.percentile 25 and 75 of all values); values further than
    fac * std from that mean become NaN; events whose frequency is NaN are dropped.  `freqs` is one array per channel.
    Returns (Events, list of float64 arrays); nothing is modified in place."""
    freqs = [np.array(f, dtype=np.float64) for f in freqs]
    pooled = np.concatenate(freqs) if len(freqs) else np.zeros(0)
    if len(pooled):
        with np.errstate(all='ignore'):
            lq, uq = np.percentile(pooled, [25.0, 75.0])
            core = pooled[(~np.isnan(pooled)) & (pooled >= lq) & (pooled <= uq)]
            m, s = (np.mean(core), np.std(core)) if len(core) else (np.nan, np.nan)
            for f in freqs:
                f[(~np.isnan(f)) & ((f < m - fac*s) | (f > m + fac*s))] = np.nan
    keep = [~np.isnan(f) for f in freqs]
    pairs = [events.frames(c)[keep[c]] for c in range(events.channels)]
    return Events(pairs, events.rate, events.trace_name), [f[k] for f, k in zip(freqs, keep)]


def event_filters(freqs, rate, factor=4.0, order=1):
    """One Butterworth low-pass table per event, cut-off factor * f: (sos (K, S, 6) float64, valid (K,) bool).  An event
    whose frequency is NaN or whose cut-off is not inside (0, rate/2) gets no filter (valid False, an all-pass row)."""
    from .design import butter_sos
    if not 1 <= int(order) <= 4:
        raise ValueError('order %r not in 1 ... 4' % (order,))
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    S = (int(order) + 1)//2
    sos = np.zeros((len(freqs), S, 6))
    sos[:, :, 0] = sos[:, :, 3] = 1.0
    valid = np.zeros(len(freqs), dtype=bool)
    for i, f in enumerate(freqs):
        cut = factor*f
        if np.isnan(cut) or not 0.0 < cut < 0.5*rate:
            continue
        sos[i] = butter_sos(int(order), float(cut), 'lowpass', float(rate))
        valid[i] = True
    return sos, valid


# ---- the two device steps in numpy float64 ------------------------------------------------------------------------------

def padlen(sos):
    """scipy's default sosfiltfilt pad length of an (S, 6) table, or of every table of an (R, S, 6) array: 3 ntaps, ntaps
    = 2 S + 1 reduced by the first-order sections."""
    sos = np.asarray(sos, dtype=np.float64)
    zeros = np.minimum(np.sum(sos[..., 2] == 0, axis=-1), np.sum(sos[..., 5] == 0, axis=-1))
    return 3*(2*sos.shape[-2] + 1 - zeros)


def _zi(sos):
    """scipy.signal.sosfilt_zi: (I - A) zi = B per section, scaled by the DC gain of the sections in front."""
    zi = np.zeros((len(sos), 2))
    scale = 1.0
    for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        B0, B1, det = b1 - a1*b0, b2 - a2*b0, (1 + a1) + a2
        zi[s] = scale*(B0 + B1)/det, scale*((1 + a1)*B1 - a2*B0)/det
        scale = scale*(b0 + b1 + b2)/(1 + a1 + a2)
    return zi


def _sosfilt(sos, x, z):
    """The cascade in direct form II transposed from the state z (S, 2), section after section over the whole sequence, on
    Python floats: the same IEEE double arithmetic as numpy scalars sample by sample, in a tenth of the time."""
    y = np.asarray(x, dtype=np.float64).tolist()
    for (b0, b1, b2, _, a1, a2), (z0, z1) in zip(np.asarray(sos, dtype=np.float64).tolist(),
                                                 np.asarray(z, dtype=np.float64).tolist()):
        for i, cur in enumerate(y):
            out = b0*cur + z0
            z0 = b1*cur - a1*out + z1
            z1 = b2*cur - a2*out
            y[i] = out
    return np.array(y, dtype=np.float64)


def check_sos(sos):
    """ValueError for what hipdsp_region_filtfilt refuses in a filter table: a0 != 1, a coefficient that is not finite, a
    pole on or outside the unit circle; NotImplementedError for more than two sections."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 3 or sos.shape[2] != 6:
        raise ValueError('sos must be (regions, sections, 6), got %r' % (sos.shape,))
    if not 1 <= sos.shape[1] <= 2:
        raise NotImplementedError('%d sections per region, 1 or 2 are served' % sos.shape[1])
    if not np.all(np.isfinite(sos)):
        raise ValueError('a coefficient is not finite')
    if np.any(sos[:, :, 3] != 1.0):
        raise ValueError('a0 is not 1')
    if not np.all((np.abs(sos[:, :, 5]) < 1.0) & (np.abs(sos[:, :, 4]) < 1.0 + sos[:, :, 5])):
        raise ValueError('a section has a pole on or outside the unit circle')
    return sos


def host_region_filtfilt(v, sos, clamp=False):
    """float32(scipy.signal.sosfiltfilt(sos, v)) of one region in numpy float64 (the definition of
    hipdsp_region_filtfilt: odd extension by the default padlen, forward pass from zi ext[0], reversal, forward pass
    from zi y[-1], reversal, trim); all NaN when v holds a NaN or an infinity; ValueError when len(v) <= padlen."""
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    edge = int(padlen(sos))
    if len(v) <= edge:
        raise ValueError('The length of the input vector x must be greater than padlen, which is %d.' % edge)
    if not np.all(np.isfinite(v)):
        return np.full(len(v), np.nan, dtype=np.float32)
    ext = np.concatenate((2*v[0] - v[edge:0:-1], v, 2*v[-1] - v[-2:-(edge + 2):-1]))
    zi = _zi(sos)
    y = _sosfilt(sos, ext, zi*ext[0])
    y = _sosfilt(sos, y[::-1], zi*y[-1])[::-1][edge:edge + len(v)]
    with np.errstate(over='ignore'):
        y = y.astype(np.float32)
    return np.where(y < 0, np.float32(0), y) if clamp else y


def host_region_crossings(row, start, stop, threshold):
    """The eight values of hipdsp_region_crossings for row[start:stop] (float32) against one threshold."""
    v = np.asarray(row[start:stop], dtype=np.float32)
    with np.errstate(all='ignore'):
        above = np.flatnonzero(v > np.float32(threshold))
    out = np.zeros(8)
    out[0], out[1] = len(v), len(above)
    out[2] = start + above[0] if len(above) else -1
    out[3] = start + above[-1] + 1 if len(above) else -1
    out[4] = np.max(v) if len(v) else np.nan
    out[5] = start + int(np.argmax(v)) if len(v) else -1
    return out


# ---- analyse_songs: the sequential bookkeeping around the two calls ------------------------------------------------------

def noise_windows(events_c, freqs_c, w, n):
    """The windows of analyse_songs for one channel's events ((K, 2) frames) in a trace of n frames: (wide, before,
    after), each (K, 2) int64 -- the event widened by w, the noise window in front of it [noiseon, wideon) and behind it
    [wideoff, noiseoff), after the reference's two adjustments (a window shorter than w is stretched to w, but not into
    the previous or the next widened event).  Events with a NaN frequency are skipped as the reference skips them; their
    rows are still filled in."""
    events_c = np.asarray(events_c, dtype=np.int64).reshape(-1, 2)
    w = int(w)
    won, woff = widen_events(events_c[:, 0], events_c[:, 1], n, w)
    non, noff = widen_events(events_c[:, 0], events_c[:, 1], n, 2*w)
    next_won = np.concatenate((won[1:], [int(n)]))
    before, after = np.zeros((len(won), 2), dtype=np.int64), np.zeros((len(won), 2), dtype=np.int64)
    prev_wideoff = 0
    for i in range(len(won)):
        noiseon, noiseoff = int(non[i]), int(noff[i])
        if not np.isnan(freqs_c[i]):
            if won[i] - noiseon < w:
                noiseon = max(int(won[i]) - w, prev_wideoff)
            if noiseoff - woff[i] < w:
                noiseoff = min(int(woff[i]) + w, int(next_won[i]))
        before[i] = noiseon, won[i]
        after[i] = woff[i], noiseoff
        prev_wideoff = int(woff[i])
    return np.stack((won, woff), axis=1), before, after


def local_thresholds(before, after, max_before, max_after, freqs_c, threshold, w, min_thresh_fac=1.0):
    """The threshold of every event of one channel: thresh0 (thresh1) = 1.2 * the largest sample of the noise window in
    front of (behind) the event where that window is longer than w/2, carried over from the previous event otherwise
    (the channel's `threshold` at first); max(thresh0, thresh1, min_thresh_fac * threshold).  NaN for events without a
    frequency, which carry nothing over."""
    out = np.full(len(before), np.nan)
    t0 = t1 = float(threshold)
    for i in range(len(before)):
        if np.isnan(freqs_c[i]):
            continue
        if before[i, 1] - before[i, 0] > w/2:
            t0 = float(max_before[i])*1.2
        if after[i, 1] - after[i, 0] > w/2:
            t1 = float(max_after[i])*1.2
        t = max(t0, t1)
        if t < min_thresh_fac*threshold:
            t = min_thresh_fac*threshold
        out[i] = t
    return out


def refine(events_c, freqs_c, maxima, crossings, threshold_c, w, n, min_thresh_fac=1.0):
    """analyse_songs for one channel: (K', 2) int64 new (onset, offset) pairs.  `maxima(windows)` returns the largest
    sample of every (start, stop) row of `windows` (never asked for an empty one's value: it may return NaN there);
    `crossings(windows, thresholds)` returns (first above, one past last above) per row, -1 for none.  The new event
    is [first above, one past last above) inside the window widened by w, dropped when nothing is above."""
    events_c = np.asarray(events_c, dtype=np.int64).reshape(-1, 2)
    freqs_c = np.asarray(freqs_c, dtype=np.float64).reshape(-1)
    wide, before, after = noise_windows(events_c, freqs_c, w, n)
    both = np.asarray(maxima(np.concatenate((before, after))), dtype=np.float64)
    thresh = local_thresholds(before, after, both[:len(wide)], both[len(wide):], freqs_c, threshold_c, int(w),
                              min_thresh_fac)
    first, last = crossings(wide, thresh)
    keep = (~np.isnan(thresh)) & (np.asarray(first) >= 0)
    return np.stack((np.asarray(first, dtype=np.int64)[keep], np.asarray(last, dtype=np.int64)[keep]), axis=1)
