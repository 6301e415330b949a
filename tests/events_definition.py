"""The sequential definition of threshold event detection (include/hip_dsp.h: hipdsp_detect_events), the comparator of
tests/test_events_host.py and tests/test_gpu_events.py.  Written from the five steps of the definition, independently of
BufferedArray.detect_events and of the kernels: find the runs, merge them from left to right, filter them.  Every
result is a list of (onset, offset) integer pairs, positions in the row; comparisons against it are exact."""

import numpy as np


def above_of(row, thr):
    """Step 1: x > thr as a float32 comparison (NaN is not above, a sample equal to thr is not above)."""
    with np.errstate(all='ignore'):
        return np.asarray(row, dtype=np.float32) > np.float32(thr)


def runs_by_loop(above, start):
    """Step 2: maximal runs of above samples, a plain loop over the samples."""
    runs, begin = [], None
    flags = [bool(a) for a in above]
    for i, a in enumerate(flags):
        if a and begin is None:
            begin = i
        elif not a and begin is not None:
            runs.append((start + begin, start + i))
            begin = None
    if begin is not None:
        runs.append((start + begin, start + len(flags)))
    return runs


def runs_by_diff(above, start):
    """Step 2 for long rows: the borders of the runs from np.diff of above."""
    a = np.concatenate(([0], np.asarray(above, dtype=np.int8), [0]))
    d = np.diff(a)
    return list(zip((np.flatnonzero(d == 1) + start).tolist(), (np.flatnonzero(d == -1) + start).tolist()))


def merge_and_filter(runs, min_gap, min_len):
    """Steps 3 and 4: a run joins the event before it when at most min_gap samples lie between them; then events
    shorter than min_len go."""
    merged = []
    for onset, offset in runs:
        if merged and onset - merged[-1][1] <= min_gap:
            merged[-1][1] = offset
        else:
            merged.append([onset, offset])
    return [(a, b) for a, b in merged if b - a >= min_len]


def detect(row, start, stop, thr, min_gap, min_len, sparse=False):
    """Events of row[start:stop]; sparse=True finds the runs with np.diff (for rows of millions of samples)."""
    above = above_of(np.asarray(row)[start:stop], thr)
    runs = runs_by_diff(above, start) if sparse else runs_by_loop(above, start)
    return merge_and_filter(runs, int(min_gap), int(min_len))
