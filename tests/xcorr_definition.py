"""The definition of hipdsp_region_xcorr (include/hip_dsp.h) written out as plain loops over the lags in long double,
the bound T of its accuracy contract as a function of the exact quantities of a case, the comparator the host and the
GPU tests share, the sequential form of the attribution rule of audian_amd/xcorr.py, and the ONE table of inputs the GPU
tests use (tests/test_xcorr_host.py asserts T < 2^-30 for every one of them).  tests/golden/region_xcorr.npz pins the
definition to np.corrcoef.  numpy only."""
import numpy as np

LD = np.longdouble
U = 2.0**-53
T_LIMIT = 2.0**-30                      # what the GPU inputs must stay under: the tests then hold r to one float32 rounding

# the shape of the kernel's grid (csrc/regionxcorr.hip), which the lengths and lags of the cases are chosen around
TILE, CHUNK, LAGS_PER_THREAD, MAX_LAG = 2048, 65536, 9, 1024


def valid_lags(start, stop, frames, L):
    """(first valid lag, number of valid lags) of a region: start + l >= 0 and stop + l <= frames, none for n == 0."""
    if stop - start < 1:
        return 0, 0
    lo, hi = max(-L, -start), min(L, frames - stop)
    return lo, hi - lo + 1


def region_xcorr(x, channel, start, stop, partner, L):
    """One (region, partner) of the contract on the host array x (channels, frames) float32.  Returns a dict:
    r (W,) long double with NaN where the contract has NaN, BEFORE the rounding to float32; info (4,) as the contract
    states it from the float32 row; and per lag the exact quantities T() needs."""
    frames = x.shape[1]
    W = 2*L + 1
    n = stop - start
    r = np.full(W, np.nan, dtype=LD)
    q = dict(n=n, D2=np.nan, va=np.nan, E2=np.full(W, np.nan, dtype=LD), vb=np.full(W, np.nan, dtype=LD),
             cov=np.full(W, np.nan, dtype=LD))
    a_ok = False
    if n >= 1:
        a = x[channel, start:stop].astype(LD)
        a_ok = bool(np.all(np.isfinite(x[channel, start:stop])))
        if a_ok:
            ma = a.sum()/n
            q['va'] = ((a - ma)**2).sum()/n
            q['D2'] = ((a - a[0])**2).sum()/n
        Kb = LD(x[partner, start]) if np.isfinite(x[partner, start]) else LD(0)
        for l in range(-L, L + 1):                                      # plain loop over the lags
            if start + l < 0 or stop + l > frames or not a_ok:
                continue
            bf = x[partner, start + l:stop + l]
            if not np.all(np.isfinite(bf)):
                continue
            b = bf.astype(LD)
            mb = b.sum()/n
            vb = ((b - mb)**2).sum()/n
            cov = ((a - ma)*(b - mb)).sum()/n
            q['vb'][L + l], q['cov'][L + l], q['E2'][L + l] = vb, cov, ((b - Kb)**2).sum()/n
            if q['va'] > 0 and vb > 0:
                r[L + l] = min(max(cov/(np.sqrt(q['va'])*np.sqrt(vb)), LD(-1)), LD(1))
    row = r.astype(np.float32)
    info = np.array([np.count_nonzero(~np.isnan(row)), -1.0, np.nan, np.nan])
    if n >= 1 and a_ok:
        info[2] = float(np.sqrt(q['va']))
    if info[0] > 0:
        info[1] = int(np.nanargmax(row))                                 # first occurrence of the largest value
        info[3] = float(np.sqrt(q['vb'][int(info[1])]))
    q.update(r=r, info=info)
    return q


def variance_error(n, S2, var):
    """Ea / Eb of the contract: S2 the exact mean square of the pivot-shifted samples, var the exact variance."""
    g = (n + 3)*U/(1 - (n + 3)*U)
    return 4*g*S2 + U*var


def bound_T(q):
    """T of the contract per lag (NaN where r is): (1 + 2^-24) |r^ - r| <= T for every summation order of the float64
    sums; the factor is what rounding r^, not r, to float32 takes, so that |out - r| <= 2^-24 |r| + T."""
    n = q['n']
    T = np.full(len(q['r']), np.nan)
    if n < 1 or not np.isfinite(float(q['va'])) or not q['va'] > 0:
        return T
    g = (n + 3)*U/(1 - (n + 3)*U)
    Ea = variance_error(n, q['D2'], q['va'])
    for i in np.flatnonzero(~np.isnan(q['r'])):
        Eb = variance_error(n, q['E2'][i], q['vb'][i])
        Ec = 4*g*np.sqrt(q['D2']*q['E2'][i]) + U*abs(q['cov'][i])
        eta = (1 + Ea/q['va'])*(1 + Eb/q['vb'][i])*(1 + U)**4 - 1
        T[i] = float((1 + 2.0**-24)*(Ec/np.sqrt(q['va']*q['vb'][i]) + abs(q['r'][i])*eta)/(1 - eta)) if eta < 1 else np.inf
    return T


def std_bound(n, S2, var):
    """hipdsp_region_stats' bound on a standard deviation with the variance error above."""
    E = float(variance_error(n, S2, var))
    s = float(np.sqrt(var))
    return min(np.sqrt(E), E/s) if s > 0 else np.sqrt(E)


def compare(q, row, info, what='', limit=None):
    """Holds one (region, partner) result -- row (W,) float32, info (4,) float64 -- to the contract: the exact NaN pattern,
    info[0] and [1] exactly, info[2] and [3] to the standard deviation bound, every value to 2^-24 |r| + T.
    With `limit` (T_LIMIT for an input that is not in GPU_CASES) the condition T < limit is asserted beside it.
    Returns the largest error in units of its allowance."""
    r, T = q['r'], bound_T(q)
    assert limit is None or np.isnan(T).all() or np.nanmax(T) < limit, (what, 'T', float(np.nanmax(T)))
    row = np.asarray(row)
    assert row.dtype == np.float32 and row.shape == r.shape, what
    nan = np.isnan(r)
    assert np.array_equal(np.isnan(row), nan), (what, np.flatnonzero(np.isnan(row) != nan))
    assert info[0] == np.count_nonzero(~nan), (what, info)
    worst = 0.0
    if nan.all():
        assert info[1] == -1 and np.isnan(info[3]), (what, info)
    else:
        tol = 2.0**-24*np.abs(r[~nan]).astype(np.float64) + T[~nan]
        err = np.abs(row[~nan].astype(LD) - r[~nan]).astype(np.float64)
        assert np.all(err <= tol), (what, float(np.max(err/tol)), np.flatnonzero(~nan)[np.argmax(err/tol)])
        worst = float(np.max(err/tol))
        # the position: exactly the first largest value of the row as stored, and a largest value of the definition's
        pos = int(info[1])
        assert pos == int(np.nanargmax(row)), (what, info)
        assert r[pos] >= np.nanmax(r) - 2*tol.max(), (what, info)
        sb = float(np.sqrt(q['vb'][pos]))
        assert abs(info[3] - sb) <= std_bound(q['n'], q['E2'][pos], q['vb'][pos]) + U*sb, (what, info, sb)
    if np.isnan(q['info'][2]):
        assert np.isnan(info[2]), (what, info)
    else:
        sa = float(np.sqrt(q['va']))
        assert abs(info[2] - sa) <= std_bound(q['n'], q['D2'], q['va']) + U*sa, (what, info, sa)
    return worst


def compare_call(x, regions, partners, L, rows, info, what='', limit=None):
    """compare() over a whole call: rows (R, P, W), info (R, P, 4)."""
    worst = 0.0
    for i, (c, a, b) in enumerate(regions):
        for j, p in enumerate(partners):
            worst = max(worst, compare(region_xcorr(x, int(c), int(a), int(b), int(p), L), rows[i, j], info[i, j],
                                       '%s region %d (%d, %d, %d) partner %d L %d' % (what, i, c, a, b, p, L), limit))
    return worst


# ---- the attribution rule, one event after the other ---------------------------------------------------------------------

def attribute(channel, partners, best_r, best_lag, std_event, std_partner, min_r=0.5, min_ratio=1.0):
    """(source channel, lag of the source in samples or NaN) of one event on `channel`: crosstalk when some partner p !=
    channel has best_r >= min_r and std_partner >= min_ratio * std_event; the source is the one such partner with the
    largest std_partner, the lowest channel among equals; otherwise the event's own channel (lag 0).  NaN never passes."""
    source, lag, loudest = channel, 0.0, None
    for j in np.argsort(np.asarray(partners), kind='stable'):
        p = int(partners[j])
        if p == channel or not best_r[j] >= min_r or not std_partner[j] >= min_ratio*std_event[j]:
            continue
        if loudest is None or std_partner[j] > loudest:
            source, lag, loudest = p, float(best_lag[j]), std_partner[j]
    return source, lag


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------

DELAY = 3                               # channel 1 of the main slab is channel 0, DELAY samples later
MAIN_FRAMES = 140000


def _noise(seed, shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape)


def slab(name):
    """The (channels, frames) float32 array of a case, made from a fixed seed."""
    if name in ('main', 'const', 'nonfinite'):
        v = _noise(11, (5, MAIN_FRAMES))
        v[2] = 0.6*v[0] + 0.8*v[2]                                      # partly correlated with channel 0 at lag 0
        v[3] = -0.7*np.roll(v[0], -2) + 0.5*v[3]                        # negatively, two samples early
        x = v.astype(np.float32)
        x[1] = np.roll(x[0], DELAY)
        x[1, :DELAY] = 0.25
        if name == 'const':
            x[0, 6000:6100] = 0.375                                     # a constant event window
            x[2, 9000:9400] = -1.5                                      # a constant partner window, and then some
        if name == 'nonfinite':
            x[0, 6050] = np.nan
            x[0, 7050] = np.inf
            x[0, 8050] = -np.inf
            x[2, 9100] = np.nan                                         # partner samples
            x[3, 9130] = np.inf
            x[3, 9190] = -np.inf
            x[4, 9000] = np.nan                                         # the pivot of a region that starts at 9000
        return x
    if name == 'dc':
        v = _noise(12, (2, 66000))
        v[1] = 0.5*v[0] + v[1]
        return (1.0e4*np.sqrt(1.0/3.0) + v).astype(np.float32)          # sigma = sqrt(1/3): an offset of 10^4 sigma
    if name == 'small':
        return _noise(13, (3, 700)).astype(np.float32)
    raise KeyError(name)


def _lengths(c, start, ns):
    return [(c, start, start + n) for n in ns]


# name -> (slab, regions, partners, L)
GPU_CASES = {
    # window lengths around a wave, a thread's step and the tile, against all channels (own channel, the delayed copy)
    'lengths': ('main', _lengths(0, 5001, [0, 1, 2, 7, 8, 9, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2*TILE + 1]),
                [0, 1, 2, 3, 4], 8),
    # ... and around the chunk
    'chunks': ('main', _lengths(0, 1001, [CHUNK - 1, CHUNK, CHUNK + 1, 2*CHUNK + 1]), [2], 1),
    'dc': ('dc', [(0, 101, 101 + CHUNK)], [1, 0], 2),
    # row edges: regions at and near both ends, x_pitch == frames with other rows on either side
    'edges': ('main', [(2, 0, 100), (2, 3, 203), (2, MAIN_FRAMES - 100, MAIN_FRAMES), (2, MAIN_FRAMES - 205, MAIN_FRAMES - 5),
                       (0, 0, MAIN_FRAMES), (4, 0, 1), (0, MAIN_FRAMES - 1, MAIN_FRAMES)], [0, 1, 2, 3, 4], 8),
    'const': ('const', [(0, 6000, 6100), (0, 6000, 6101), (1, 9100, 9300), (2, 9050, 9250)], [0, 2, 3], 60),
    'nonfinite': ('nonfinite', [(0, 6000, 6100), (0, 7000, 7100), (0, 8000, 8100), (1, 9100, 9160), (4, 9000, 9060),
                                (1, 20000, 20300)], [2, 3, 4, 1], 40),
    'small': ('small', [(0, 10, 310), (2, 0, 700), (1, 350, 355)], [1, 2], 300),
}
# the lags around a thread's nine and the extremes, on a window longer and one shorter than most of them
for _L in (0, 1, 4, 5, 7, 8, 9, 13, 255, MAX_LAG):
    GPU_CASES['lag%d' % _L] = ('main', [(0, 3000, 3300), (2, 3000, 3005), (3, 500, 500 + TILE + 1)], [1, 3], _L)


def case(name):
    s, regions, partners, L = GPU_CASES[name]
    return slab(s), np.array(regions, dtype=np.int64).reshape(-1, 3), list(partners), L
