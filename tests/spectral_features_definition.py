"""The definition of hipdsp_spectral_features (include/hip_dsp.h) and what a float64 implementation may miss it by.

``row_features`` writes every feature as plain loops in np.longdouble over one float32 row; ``slab_features`` is the
same arithmetic on whole slabs (np.longdouble array operations, rows in chunks), held to the loops by the host tests.
Both return the value V of every feature and the float64 term T of the bound; ``compare`` judges every element:

  bits 0, 2, 6, 7 (PEAK_BIN_FREQ, PEAK_POWER, FREQ_LOW, FREQ_HIGH): bit for bit -- np.float32(np.float64(scale)*k),
      P[kp]; the >= of the extents is evaluated in float64 exactly as the header states it.
  bits 1, 3, 4, 5 (PEAK_FREQ, CENTROID, BANDWIDTH, FLATNESS): |got - V| <= 2^-24 (|V| + T) + T + 2^-150, one float32
      rounding of a float64 result that is within T of V.

The term T, with u = 2^-53, n = k1 - k0 and g(m) = m u (1 + 2^-10) / (1 - m u), the error factor of a float64 sum of m
additions IN ANY ORDER (the 2^-10 pays for the longdouble reference's own sums, 2^-11 u per addition) -- the device's
order (a thread's share, a butterfly) and numpy's pairwise order are both covered:

  S  = sum P[k]                |dS|  <= g(n-1) S          (the terms are exact float64, all >= 0)
  M1 = sum (k-kp) P[k]         |dM1| <= g(n-1) A1,        A1 = sum |k-kp| P[k]   (the products are exact: 18 + 24 bits)
  M2 = sum (k-kp)^2 P[k]       |dM2| <= g(n) M2           (one rounding per product)
  m  = M1/S                    |dm|  <= e_m a1,           a1 = A1/S,  e_m = 2 g(n-1) + 2u
  CENTROID  scale (kp + m)     T = scale (|dm| + 3u |kp + m|)
  BANDWIDTH scale sqrt(var), var = q - m^2, q = M2/S.  a1^2 <= q (Cauchy-Schwarz), so 2 |m| |dm| <= e_m (q + m^2) and
            |dvar| <= (e_q + e_m + 2u)(q + m^2) + dm^2,   e_q = g(n) + g(n-1) + u
            which is var times the condition factor (q + m^2)/var times the roundoff: for var > 0
            T = value (|dvar|/var + (LOG_ULPS + 2) u)   while |dvar| < var/2  (|sqrt(1+x) - 1| <= |x| there),
            else, and for var = 0, T = scale (sqrt(var + |dvar|) (1 + 8u) - value) + value (the whole range down to 0).
  FLATNESS  exp(L/n)/(S/n), L = sum ln P[k]: a device log is taken to be within LOG_ULPS ulp (2 LOG_ULPS u relative);
            |dL| <= (g(n-1) + 2 LOG_ULPS u (1 + g(n-1))) B,  B = sum |ln P[k]|, the exponent is off by |dL|/n + u |L|/n =: x,
            T = value (expm1(x) + 2 LOG_ULPS u + g(n-1) + 4u).  A zero bin gives exactly 0: T = 0.
  PEAK_FREQ scale (kp + d), d = 0.5 (a - c)/den, den = (a - 2b) + c:  e_a = 2 LOG_ULPS u |a| etc.,
            |dnum| <= 0.5 (e_a + e_c) + u |a - c|,  |dden| <= e_a + 2 e_b + e_c + u (|a - 2b| + |den|),
            |dd| <= (|dnum| + |d| |dden|)/(|den| - |dden|) + u |d|     -- the factor 1/|den| --
            T = scale (|dd| + 3u |kp + d|); T = inf if |dden| >= |den| (the branch den < 0 itself is then undecided;
            no test input is like that, the host tests assert it).  d = 0 by rule: T = scale 3u kp.

ROCm's published accuracy table of the device math library is not at hand where these tests were written: LOG_ULPS = 4
is ASSUMED for log, exp and sqrt in float64.  The terms it enters sit decades under the float32 rounding (the host tests
assert T < 2^-30 of the value, or of one bin where a frequency is smaller than that), so the choice cannot hide an error.
"""

import numpy as np

LD = np.longdouble
U = 2.0**-53
LOG_ULPS = 4
NAMES = ('peak_bin_freq', 'peak_freq', 'peak_power', 'centroid', 'bandwidth', 'flatness', 'freq_low', 'freq_high')
EXACT_BITS = (0, 2, 6, 7)
ALL = 0xFF
T_LIMIT = 2.0**-30


def g(m):
    m = max(int(m), 0)
    return m*U*(1 + 2.0**-10)/(1 - m*U)


def drop_ratio(drop_db):
    return 10.0**(-float(drop_db)/10.0)


def row_features(P, k0, k1, scale=1.0, min_power=0.0, ratio=0.1):
    """(V, T): eight np.longdouble values and eight float64 terms for one float32 row `P` and the band [k0, k1)."""
    P = np.asarray(P, dtype=np.float32)
    V = [LD(np.nan)]*8
    T = [0.0]*8
    n = k1 - k0
    kp = -1
    for k in range(k0, k1):                                   # np.argmax: the first NaN, else the first of the largest
        if kp < 0:
            kp = k
        elif np.isnan(P[kp]):
            break
        elif np.isnan(P[k]) or P[k] > P[kp]:
            kp = k
    if kp < 0:
        return V, T
    peak = P[kp]
    V[2] = LD(peak)
    if not (np.isfinite(peak) and np.float64(peak) > np.float64(min_power)):
        return V, T
    s = LD(scale)
    V[0] = LD(np.float64(scale)*np.float64(kp))
    # the extents, in float64 as stated
    thr = np.float64(ratio)*np.float64(peak)
    klo = khi = -1
    for k in range(k0, k1):
        if np.float64(P[k]) >= thr:
            if klo < 0:
                klo = k
            khi = k
    V[6], V[7] = LD(np.float64(scale)*np.float64(klo)), LD(np.float64(scale)*np.float64(khi))
    # the interpolated peak
    d, td = LD(0), 0.0
    if kp - 1 >= k0 and kp + 1 < k1 and P[kp - 1] > 0 and P[kp + 1] > 0:
        a, b, c = np.log(LD(P[kp - 1])), np.log(LD(peak)), np.log(LD(P[kp + 1]))
        den = (a - 2*b) + c
        ea, eb, ec = (2*LOG_ULPS*U*abs(float(v)) for v in (a, b, c))
        dden = ea + 2*eb + ec + U*(abs(float(a - 2*b)) + abs(float(den)))
        if den < 0:
            d = LD(0.5)*(a - c)/den
            dnum = 0.5*(ea + ec) + U*abs(float(a - c))
            if dden < abs(float(den)):
                td = (dnum + abs(float(d))*dden)/(abs(float(den)) - dden) + U*abs(float(d))
            else:
                td = np.inf
        elif dden > 0 and abs(float(den)) <= dden and float(den) != 0.0:
            td = np.inf                                        # a float64 den could fall below 0
    V[1] = s*(LD(kp) + d)
    T[1] = abs(scale)*(td + 3*U*abs(float(kp + d)))
    # the moments about the peak and the logarithms
    S = M1 = M2 = A1 = L = B = LD(0)
    zero = False
    for k in range(k0, k1):
        p, dk = LD(P[k]), LD(k - kp)
        S += p
        M1 += dk*p
        A1 += abs(dk)*p
        M2 += dk*dk*p
        if P[k] == 0:
            zero = True
        else:
            lp = np.log(p)
            L += lp
            B += abs(lp)
    m, q, a1 = M1/S, M2/S, float(A1/S)
    e_m = 2*g(n - 1) + 2*U
    dm = e_m*a1
    V[3] = s*(LD(kp) + m)
    T[3] = abs(scale)*(dm + 3*U*abs(float(kp + m)))
    var = q - m*m
    var = var if var > 0 else LD(0)
    e_q = g(n) + g(n - 1) + U
    dvar = (e_q + e_m + 2*U)*float(q + m*m) + dm*dm
    V[4] = s*np.sqrt(var)
    if var > 0 and dvar < 0.5*float(var):
        T[4] = float(V[4])*(dvar/float(var) + (LOG_ULPS + 2)*U)
    else:
        T[4] = abs(scale)*np.sqrt(float(var) + dvar)*(1 + 8*U)
    if zero:
        V[5] = LD(0)
    else:
        V[5] = np.exp(L/n)/(S/n)
        x = (g(n - 1) + 2*LOG_ULPS*U*(1 + g(n - 1)))*float(B)/n + U*abs(float(L))/n
        T[5] = float(V[5])*(np.expm1(x) + 2*LOG_ULPS*U + g(n - 1) + 4*U)
    return V, T


def slab_features(spec, k0, k1, scale=1.0, min_power=0.0, ratio=0.1, chunk=1 << 21):
    """row_features of every row of `spec` (..., nfreq) float32: (V, T) of shape (8, ...), np.longdouble and float64."""
    spec = np.asarray(spec, dtype=np.float32)
    lead, n = spec.shape[:-1], k1 - k0
    rows = spec.reshape(-1, spec.shape[-1])[:, k0:k1]
    R = len(rows)
    V = np.full((8, R), np.nan, dtype=LD)
    T = np.zeros((8, R))
    step = max(1, chunk//max(n, 1))
    s = LD(scale)
    for r0 in range(0, R if n > 0 else 0, step):
        P = rows[r0:r0 + step]
        sl = slice(r0, r0 + len(P))
        with np.errstate(all='ignore'):
            j = np.argmax(P, axis=1)
            idx = np.arange(len(P))
            peak = P[idx, j]
            kp = j + k0
            V[2, sl] = peak
            valid = np.isfinite(peak) & (peak.astype(np.float64) > np.float64(min_power))
            V[0, sl] = np.float64(scale)*kp.astype(np.float64)
            above = P.astype(np.float64) >= (np.float64(ratio)*peak.astype(np.float64))[:, None]
            V[6, sl] = np.float64(scale)*(np.argmax(above, axis=1) + k0).astype(np.float64)
            V[7, sl] = np.float64(scale)*(k1 - 1 - np.argmax(above[:, ::-1], axis=1)).astype(np.float64)
            # the interpolated peak
            pa, pc = P[idx, np.clip(j - 1, 0, n - 1)], P[idx, np.clip(j + 1, 0, n - 1)]
            inside = (j - 1 >= 0) & (j + 1 < n) & (pa > 0) & (pc > 0) & valid
            a, b, c = (np.log(np.where(inside, v, 1).astype(LD)) for v in (pa, peak, pc))
            den = (a - 2*b) + c
            ea, eb, ec = (2*LOG_ULPS*U*np.abs(v.astype(np.float64)) for v in (a, b, c))
            dden = ea + 2*eb + ec + U*(np.abs((a - 2*b).astype(np.float64)) + np.abs(den.astype(np.float64)))
            aden = np.abs(den.astype(np.float64))
            use = inside & (den < 0)
            d = np.where(use, LD(0.5)*(a - c)/np.where(use, den, LD(1)), LD(0))
            dnum = 0.5*(ea + ec) + U*np.abs((a - c).astype(np.float64))
            td = np.where(dden < aden, (dnum + np.abs(d.astype(np.float64))*dden)/np.where(dden < aden, aden - dden, 1.0)
                          + U*np.abs(d.astype(np.float64)), np.inf)
            td = np.where(use, td, np.where(inside & (aden <= dden) & (aden != 0) & (dden > 0), np.inf, 0.0))
            V[1, sl] = s*(kp.astype(LD) + d)
            T[1, sl] = abs(scale)*(td + 3*U*np.abs((kp + d).astype(np.float64)))
            # the moments about the peak and the logarithms
            p = P.astype(LD)
            dk = (np.arange(k0, k1)[None, :] - kp[:, None]).astype(LD)
            S = p.sum(axis=1)
            M1, A1, M2 = (dk*p).sum(axis=1), (np.abs(dk)*p).sum(axis=1), (dk*dk*p).sum(axis=1)
            zero = np.any(P == 0, axis=1)
            lp = np.log(np.where(P > 0, p, LD(1)))
            L, B = lp.sum(axis=1), np.abs(lp).sum(axis=1).astype(np.float64)
            m, q, a1 = M1/S, M2/S, (A1/S).astype(np.float64)
            e_m = 2*g(n - 1) + 2*U
            dm = e_m*a1
            V[3, sl] = s*(kp.astype(LD) + m)
            T[3, sl] = abs(scale)*(dm + 3*U*np.abs((kp + m).astype(np.float64)))
            var = q - m*m
            var = np.where(var > 0, var, LD(0))
            var64 = var.astype(np.float64)
            dvar = (g(n) + g(n - 1) + U + e_m + 2*U)*(q + m*m).astype(np.float64) + dm*dm
            V[4, sl] = s*np.sqrt(var)
            bw = V[4, sl].astype(np.float64)
            good = (var64 > 0) & (dvar < 0.5*var64)
            T[4, sl] = np.where(good, bw*(dvar/np.where(good, var64, 1.0) + (LOG_ULPS + 2)*U),
                                abs(scale)*np.sqrt(var64 + dvar)*(1 + 8*U))
            flat = np.exp(L/n)/(S/n)
            V[5, sl] = np.where(zero, LD(0), flat)
            x = (g(n - 1) + 2*LOG_ULPS*U*(1 + g(n - 1)))*B/n + U*np.abs(L.astype(np.float64))/n
            T[5, sl] = np.where(zero, 0.0, flat.astype(np.float64)*(np.expm1(x) + 2*LOG_ULPS*U + g(n - 1) + 4*U))
            for bit in (0, 1, 3, 4, 5, 6, 7):
                V[bit, sl] = np.where(valid, V[bit, sl], LD(np.nan))
                T[bit, sl] = np.where(valid, T[bit, sl], 0.0)
    return V.reshape((8,) + lead), T.reshape((8,) + lead)


def bits_of(mask):
    return [b for b in range(8) if mask >> b & 1]


def compare(got, V, T, mask=ALL, what=''):
    """Judge every element of `got` (the rows of the features of `mask`, float32, in bit order) against (V, T) of
    slab_features; returns the worst |got - V| / allowed over the approximate features (0 when there is none)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (len(bits_of(mask)),) + V.shape[1:], (what, got.shape, V.shape)
    worst = 0.0
    for j, bit in enumerate(bits_of(mask)):
        v, t, x = V[bit], T[bit], got[j]
        nan = np.isnan(v)
        assert np.array_equal(np.isnan(x), nan), '%s %s: NaN where a value is due, or the reverse' % (what, NAMES[bit])
        ok = ~nan
        if bit in EXACT_BITS:
            with np.errstate(over='ignore'):
                want = v.astype(np.float64).astype(np.float32)
            same = x[ok].view(np.uint32) == want[ok].view(np.uint32)
            same |= (x[ok] == 0) & (want[ok] == 0)
            assert np.all(same), '%s %s: %d of %d differ, first got %r want %r' % (
                what, NAMES[bit], int((~same).sum()), same.size, x[ok][~same][0], want[ok][~same][0])
            continue
        inf = ok & np.isinf(v)
        assert np.array_equal(x[inf].astype(np.float64), v[inf].astype(np.float64)), (what, NAMES[bit])
        ok &= ~inf
        err = np.abs(x[ok].astype(LD) - v[ok]).astype(np.float64)
        allowed = 2.0**-24*(np.abs(v[ok]).astype(np.float64) + t[ok]) + t[ok] + 2.0**-150
        ratio = err/allowed
        if ratio.size:
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1.0, '%s %s: %d of %d outside the bound, worst got %r want %r allowed %r' % (
                what, NAMES[bit], int((ratio > 1).sum()), ratio.size, x[ok][i], float(v[ok][i]), allowed[i])
            worst = max(worst, float(ratio[i]))
    return worst


def term_scale(V, scale):
    """What T is measured against: |V|, but at least one bin for the frequency features (a frequency may be 0)."""
    ref = np.abs(V).astype(np.float64)
    for bit in (0, 1, 3, 4, 6, 7):
        ref[bit] = np.maximum(ref[bit], abs(scale))
    return ref


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------

def slab_random(rng, C, frames, F):
    """Non-negative float32 spanning 1e-12 ... 1e6 within every row."""
    u = rng.random((C, frames, F), dtype=np.float32)
    return np.power(np.float32(10.0), np.float32(18.0)*u - np.float32(12.0)).astype(np.float32)


def band_kinds(F):
    """name -> (k0, k1): every kind of band of the contract that fits into F bins."""
    kinds = {'one bin': (F//2, F//2 + 1), 'first bin': (0, 1), 'last bin': (F - 1, F), 'full': (0, F),
             'top 1/16': (F - max(F//16, 1), F), 'empty': (F//3, F//3), 'empty at F': (F, F)}
    for w in (63, 64, 65):
        for start in (1, 77):
            if start + w <= F:
                kinds['width %d at %d' % (w, start)] = (start, start + w)
    return kinds


FAMILIES = ('random', 'one bin', 'far line', 'two lines', 'equal', 'plateau 2', 'plateau 3', 'peak at k0',
            'peak at k1-1', 'peak at bin 0', 'peak at F-1', 'zero neighbour', 'zeros', 'denormals', 'nan at peak',
            'inf at peak', 'nan beside peak', 'inf elsewhere', 'nan outside', 'inf outside')


def family_row(name, F, k0, k1, rng):
    """One float32 row of the family `name`, shaped for the band [k0, k1) (n >= 1)."""
    n = k1 - k0
    floor = np.power(10.0, -9.0 + 3.0*rng.random(F)).astype(np.float32)           # 1e-9 ... 1e-6
    row = floor.copy()
    mid = k0 + min(n - 1, max(n//10, 1))                                          # far from the band's centre
    if name == 'random':
        row = np.power(10.0, 18.0*rng.random(F) - 12.0).astype(np.float32)
    elif name == 'one bin':
        row[k0:k1] = 0
        row[k0 + int(rng.integers(0, n))] = 3.5
    elif name == 'far line':
        for off, v in ((-1, 0.21), (0, 1.0), (1, 0.33)):
            if k0 <= mid + off < k1:
                row[mid + off] = v
    elif name == 'two lines':
        row[mid] = 1.0
        row[k1 - 1 - min(n - 1, n//7)] = 0.9
    elif name == 'equal':
        row[:] = 0.37
    elif name in ('plateau 2', 'plateau 3'):
        w = 2 if name == 'plateau 2' else 3
        row[mid:min(mid + w, k1)] = 2.0
        if mid + w < k1:
            row[mid + w] = 0.5
    elif name == 'peak at k0':
        row[k0] = 4.0
    elif name == 'peak at k1-1':
        row[k1 - 1] = 4.0
    elif name == 'peak at bin 0':
        row[0] = 9.0
    elif name == 'peak at F-1':
        row[F - 1] = 9.0
    elif name == 'zero neighbour':
        row[mid] = 1.0
        if mid + 1 < k1:
            row[mid + 1] = 0
    elif name == 'zeros':
        row[:] = 0
    elif name == 'denormals':
        row = (rng.integers(1, 2**22, F).astype(np.uint32)).view(np.float32).copy()
    elif name in ('nan at peak', 'inf at peak'):
        row[mid] = np.nan if name == 'nan at peak' else np.inf
    elif name == 'nan beside peak':
        row[mid] = 1.0
        row[min(mid + 1, k1 - 1)] = np.nan
    elif name == 'inf elsewhere':
        row[mid] = 1.0
        row[k1 - 1] = np.inf
    elif name in ('nan outside', 'inf outside'):
        row[mid] = 1.0
        bad = np.nan if name == 'nan outside' else np.inf
        if k0 > 0:
            row[k0 - 1] = bad
        if k1 < F:
            row[k1] = bad
        if k0 > 1:
            row[0] = bad
    else:
        raise ValueError(name)
    return row


def family_slab(F, frames, C, k0, k1, seed):
    """(C, frames, F) float32: row r = c*frames + t is of family FAMILIES[r % len(FAMILIES)], shaped for [k0, k1)."""
    rng = np.random.default_rng([F, frames, C, k0, k1, seed])
    spec = np.empty((C, frames, F), dtype=np.float32)
    for r in range(C*frames):
        spec[r//frames, r % frames] = family_row(FAMILIES[r % len(FAMILIES)], F, k0, k1, rng)
    return spec


# (nfreq, frames, channels): the issue's list; then the borders of the mapping -- nfreq 256 | 257 (8 lanes per row in
# an LDS tile | a wave per row), 1056 | 1057 (a wave | a workgroup per row), a band of 8448 | 8449 bins (held in LDS |
# read twice) -- and frame counts one below, at and above the short rows' tile of 32 frames
RANDOM_SLABS = [(5, 1, 1), (5, 100003, 3), (129, 65, 64), (257, 257, 3), (513, 63, 1), (1025, 1000, 64), (1025, 64, 3),
                (4097, 65, 3), (8193, 9, 1), (32769, 63, 3), (262145, 1, 3),
                (256, 33, 2), (1056, 5, 2), (1057, 5, 2), (8449, 3, 1), (129, 31, 1), (129, 32, 2), (33, 33, 2)]
# the slabs every family is laid into, one per mapping and one that is read twice
FAMILY_SLABS = [(129, 40, 2), (1025, 20, 2), (4097, 20, 1), (8449, 20, 1)]
SCALE = 46.875


def random_bands(F, frames, C):
    """The bands a random slab is judged on: all kinds, but only the narrow ones where the slab is large."""
    kinds = band_kinds(F)
    if C*frames*F > (1 << 24):
        return {k: v for k, v in kinds.items() if v[1] - v[0] <= 65}
    return kinds


def family_bands(F):
    kinds = band_kinds(F)
    return {k: kinds[k] for k in ('full', 'top 1/16', 'width 65 at 77', 'width 63 at 1', 'one bin') if k in kinds}


def random_spec(F, frames, C):
    return slab_random(np.random.default_rng([F, frames, C]), C, frames, F)


def gpu_cases():
    """(label, spec, k0, k1) of every slab and band the GPU tests judge against this file, min_power 0, ratio 0.1,
    scale SCALE."""
    for F, frames, C in RANDOM_SLABS:
        spec = random_spec(F, frames, C)
        for kind, (k0, k1) in random_bands(F, frames, C).items():
            yield 'random F %d frames %d C %d, %s' % (F, frames, C, kind), spec, k0, k1
    for F, frames, C in FAMILY_SLABS:
        for kind, (k0, k1) in family_bands(F).items():
            yield 'families F %d frames %d C %d, %s' % (F, frames, C, kind), family_slab(F, frames, C, k0, k1, 3), k0, k1
