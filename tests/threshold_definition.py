"""The definitions of include/hip_dsp.h (hipdsp_histogram, hipdsp_masked_stats) and of
BufferedArray.threshold_estimates in plain numpy, written from the header's text: the comparator of the tests where
numpy alone is not enough.  Samples are float32 values widened exactly to float64."""

import numpy as np


def histogram_slots(v, edges):
    """The B + 3 slots of one row: a sample with e[0] <= x <= e[B] goes to the bin numbered by how many interior edges
    e[1..B-1] are <= x (one comparison per edge, no search); then the samples below e[0], above e[B], and the NaNs."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges, dtype=np.float64)
    B = len(e) - 1
    out = np.zeros(B + 3, dtype=np.int64)
    inside = v[(v >= e[0]) & (v <= e[B])]
    bins = np.zeros(len(inside), dtype=np.int64)
    for i in range(1, B):
        bins += e[i] <= inside
    out[:B] = np.bincount(bins, minlength=B)
    out[B] = np.count_nonzero(v < e[0])
    out[B + 1] = np.count_nonzero(v > e[B])
    out[B + 2] = np.count_nonzero(np.isnan(v))
    return out


def numpy_slots(v, edges):
    """The same from np.histogram: its counts, and the three outside counts."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges, dtype=np.float64)
    finite = v[~np.isnan(v)]
    counts = np.histogram(finite, bins=e)[0]
    return np.concatenate((counts, [np.count_nonzero(v < e[0]), np.count_nonzero(v > e[-1]),
                                    np.count_nonzero(np.isnan(v))])).astype(np.int64)


def selected(v, lo, hi):
    """The samples of one row with lo < x < hi: strict, never NaN or infinite samples, nothing for a NaN bound."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return v[(v > lo) & (v < hi) & np.isfinite(v)]


def masked_slots(v, lo, hi):
    """[n, mean, std, 0] of the selected samples with numpy's float64 mean and std; NaN where nothing is selected."""
    s = selected(v, lo, hi)
    if len(s) == 0:
        return np.array([0.0, np.nan, np.nan, 0.0])
    return np.array([len(s), np.mean(s), np.std(s), 0.0])


def threshold_estimates(x):
    """The decomposition of BufferedArray.threshold_estimates on a (frames, channels) float array, in float64: maximum,
    49-bin histogram over linspace(0, max, 50), the cut at the widened mode, moments below the cut, the mean above
    mean + 3 std, the final rule.  Returns (thresholds, details); details[c] = (maxi, mean, std, uppermean)."""
    x = np.asarray(x, dtype=np.float64)
    maxe = np.max(x)
    edges = np.linspace(0.0, maxe, 50)
    thresholds, details = [], []
    for c in range(x.shape[1]):
        counts = histogram_slots(x[:, c], edges)[:49]
        mini = int(np.nonzero(counts > 0)[0][0])
        maxi = int(np.argmax(counts)) + 1
        maxi = min(maxi + (maxi - mini), 49)
        n, mean, std, _ = masked_slots(x[:, c], -np.inf, edges[maxi])
        uppermean = masked_slots(x[:, c], mean + 3.0*std, np.inf)[1]
        thresholds.append(0.5*(mean + uppermean) if uppermean > mean + 6.0*std else maxe + std)
        details.append((maxi, mean, std, uppermean))
    return np.array(thresholds), details


def tiled(x, times, frames):
    """The multi-chunk case of the golden file: the stored (5000, C) case repeated `times` times and cut to `frames`
    rows -- built from stored samples only, no random stream at test time."""
    return np.tile(np.asarray(x), (times, 1))[:frames]
