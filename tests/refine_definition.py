"""Sequential numpy definitions of the event refinement -- what hipdsp_region_crossings, audian_amd.refine.widen_events,
clean_event_freqs and refine must give.  Plain loops over samples and events, written from include/hip_dsp.h and from the
reference's songdetector.py:155-244, sharing no code with audian_amd.  The filter's definition is
iir_bound.sosfiltfilt (gain 1, no rectification, no clamp)."""

import numpy as np

import iir_bound as ib


def region_crossings(row, start, stop, threshold):
    """The eight float64 values of one region of one float32 row.  (Python floats: the float32 samples and the float32
    threshold are exact in float64, so the comparisons are the float32 ones.)"""
    vals = np.asarray(row, dtype=np.float32)[start:stop].astype(np.float64).tolist()
    with np.errstate(over='ignore'):
        thr = float(np.float32(threshold))
    count, first, last = 0, -1, -1
    best, arg = float('nan'), -1
    for i, s in enumerate(vals, start):
        if s > thr:                     # false for a NaN on either side
            count += 1
            if first < 0:
                first = i
            last = i + 1
        if arg < 0:
            best, arg = s, i
        elif best != best:
            pass                        # the first NaN stays
        elif s != s or s > best:
            best, arg = s, i
    return np.array([stop - start, count, first, last, best, arg, 0.0, 0.0], dtype=np.float64)


def widen_events(onsets, offsets, n, width):
    on = [int(v) - width for v in onsets]
    off = [int(v) + width for v in offsets]
    if on:
        on[0] = max(on[0], 0)
        off[-1] = min(off[-1], n)
    for i in range(len(on) - 1):
        if off[i] > on[i + 1]:
            off[i] = on[i + 1] = (int(offsets[i]) + int(onsets[i + 1]))//2
    return np.array(on, dtype=np.int64), np.array(off, dtype=np.int64)


def clean_event_freqs(onsets, offsets, freqs, fac=6.0):
    """songdetector.py:155-175 on copies: (onsets, offsets, freqs), a list per channel each."""
    freqs = [np.array(f, dtype=np.float64) for f in freqs]
    ffreqs = np.concatenate(freqs)
    if len(ffreqs) == 0:
        return [np.array(o) for o in onsets], [np.array(o) for o in offsets], freqs
    with np.errstate(all='ignore'):
        lq, uq = np.percentile(ffreqs, [25.0, 75.0])
        cfreqs = ffreqs[(~np.isnan(ffreqs)) & (ffreqs >= lq) & (ffreqs <= uq)]
        m = np.mean(cfreqs) if len(cfreqs) else np.nan
        s = np.std(cfreqs) if len(cfreqs) else np.nan
        for c in range(len(freqs)):
            freqs[c][(~np.isnan(freqs[c])) & ((freqs[c] < m - fac*s) | (freqs[c] > m + fac*s))] = np.nan
    keep = [~np.isnan(f) for f in freqs]
    return ([np.asarray(onsets[c])[keep[c]] for c in range(len(freqs))],
            [np.asarray(offsets[c])[keep[c]] for c in range(len(freqs))], [freqs[c][keep[c]] for c in range(len(freqs))])


def refine(onsets, offsets, freqs, env, threshold, w, min_thresh_fac=1.0):
    """analyse_songs (songdetector.py:195-244) for one channel on the float32 row `env`, with the trace's length where the
    reference has len(envelopes[c]), and an event [first sample above, one past the last sample above) inside the wide
    window.  Returns a list of (onset, offset)."""
    env = np.asarray(env, dtype=np.float32)
    n = len(env)
    wide_on, wide_off = widen_events(onsets, offsets, n, w)
    noise_on, noise_off = widen_events(onsets, offsets, n, 2*w)
    prev_wideoff = 0
    thresh0 = thresh1 = threshold
    out = []
    for i in range(len(wide_on)):
        noiseon, wideon, wideoff, noiseoff = int(noise_on[i]), int(wide_on[i]), int(wide_off[i]), int(noise_off[i])
        next_wideon = int(wide_on[i + 1]) if i + 1 < len(wide_on) else n
        if np.isnan(freqs[i]):
            prev_wideoff = wideoff
            continue
        if wideon - noiseon < w:
            noiseon = wideon - w
            if noiseon < prev_wideoff:
                noiseon = prev_wideoff
        if noiseoff - wideoff < w:
            noiseoff = wideoff + w
            if noiseoff > next_wideon:
                noiseoff = next_wideon
        if wideon - noiseon > w/2:
            thresh0 = float(np.max(env[noiseon:wideon]))*1.2
        if noiseoff - wideoff > w/2:
            thresh1 = float(np.max(env[wideoff:noiseoff]))*1.2
        thresh = max(thresh0, thresh1)
        if thresh < min_thresh_fac*threshold:
            thresh = min_thresh_fac*threshold
        with np.errstate(all='ignore'):
            above = np.flatnonzero(env[wideon:wideoff] > np.float32(thresh))
        if len(above):
            out.append((wideon + int(above[0]), wideon + int(above[-1]) + 1))
        prev_wideoff = wideoff
    return out


# ---- the filter cases of the accuracy tests (CPU calibration and GPU) ------------------------------------------------------

LP_FAMILIES = ('stepdown', 'stepup', 'offset', 'burst')
# label: (order, Wn, btype, rate, families)                                               sections, largest q
CASES = {
    'lp1 4 Hz @ 5 kHz': (1, 4.0, 'lowpass', 5000.0, LP_FAMILIES),                        # 1, 1.0e-6
    'lp1 40 Hz @ 96 kHz': (1, 40.0, 'lowpass', 96000.0, LP_FAMILIES),                    # 1, 9.0e-7
    'lp1 400 Hz @ 5 kHz': (1, 400.0, 'lowpass', 5000.0, LP_FAMILIES),                    # 1, 7.1e-9
    'lp2 20 Hz @ 96 kHz': (2, 20.0, 'lowpass', 96000.0, LP_FAMILIES),                    # 1, 8.9e-3
    'lp4 300 Hz @ 48 kHz': (4, 300.0, 'lowpass', 48000.0, LP_FAMILIES),                  # 2, 3.2e-5
    # one section with a zero at DC: `offset` at its default level is over the cap (2.6e-2), 1 + 1e-1 s meets it (2.6e-4)
    'bp1 10-500 Hz @ 48 kHz': (1, (10.0, 500.0), 'bandpass', 48000.0, ('stepdown', 'stepup', ('offset', 1e-1), 'burst')),   # 1, 1.1e-3
}
LP1 = ('lp1 4 Hz @ 5 kHz', 'lp1 40 Hz @ 96 kHz', 'lp1 400 Hz @ 5 kHz')      # the reference's filters: one call


def case_design(label):
    """(sos (S, 6), rate, families) of a case."""
    return ib.design(label, CASES)


def case_signal(label, length, seed=0):
    """(length, len(families)) float32: the case's families as lanes."""
    sos, rate, fams = case_design(label)
    return ib.families(fams, length, rate, seed=seed)


def filtfilt_runs(sos, x):
    """(reference (T, lanes) longdouble, sequential float64 run) of scipy's sosfiltfilt of the float32 lanes of x."""
    return ib.envelope_runs(sos, x, rectify=False, gain=1.0)


def filtfilt_case(sos, x):
    """(reference, q per lane)."""
    ref, run = filtfilt_runs(sos, x)
    return ref, ib.allowance(run, ref)
