"""Spectrogram template matching as include/hip_dsp.h defines it (hipdsp_template_prepare_host, hipdsp_template_match),
written out from the header's sentences in np.longdouble -- the comparator of tests/test_template_match_host.py and
tests/test_gpu_template_match.py, never the code under test.

The values v (after the dB transform and the floor) are taken as given: the GPU test obtains them from hipdsp_decibel
on the same slab and clamps them on the host; a host test makes them up.

The bound (u = 2^-24, e = 2^-53, n = Tt*Fb, m = n + 3, gamma = m u/(1 - m u)), derived here and quoted by the header:

  x = v - pivot is exact in float64, the matrix core sees fl(x) = x (1 + d), |d| <= u.  The accumulator G~ is a float32
  sum of the n products g fl(x) with one rounding per step in a fixed order, so with M = sum |g| |fl(x)|
      |G~ - sum g x| <= gamma_m M                                   (n roundings of the chain, one of fl(x), two spare).
  raw: out = fl32(G~ + pivot H0) formed in float64 (a product, a sum: 2e, H0's own error below e): 4 e |pivot H0|, and
  the float32 store u |s|; at pivot == 0 out = G~ itself.
  normalised: S1~ and S2~ are float64 sums of n terms in some order: |S2~ - S2| <= gamma64_(n+1) S2 (the squares are
  rounded too), |S1~ - S1| <= gamma64_n sum |x| <= gamma64_n sqrt(n S2).  D~ = S2~ - S1~^2/n: since S1^2 <= n S2,
      |D~ - D| <= (gamma64_(n+1) + 2 gamma64_n + 4e) S2 <= (3n + 6) e S2 =: eD S2.
  The numerator N~ = G~ - (S1~/n) H0 is off by gamma_m M + (n + 4) e sqrt(S2/n) |H0| + e |N|; the quotient
  N~/(sqrt(Q) sqrt(D~)) adds |r| (eD S2/D) for D (first order eD S2/(2D): the factor 2 covers the higher orders
  while eD S2/D < 1/2; beyond that the bound is infinite) and 8e |r| for the square roots, the product, the division
  and Q's rounding; the store u |r| (or a denormal, 2^-149).  Clamping to [-1, 1] moves out towards r.
  The mask compares D~ with fl(n min_std^2): a window is undecided where |D - n min_std^2| <= eD S2 + 4e n min_std^2.
"""

import numpy as np

LD = np.longdouble
U = 2.0**-24
E = 2.0**-53


def prepare(templates, normalize):
    """The header's preparation in plain longdouble loops: (taps float32 (K, Tt, Fb), H0 (K,) longdouble, Q (K,)
    longdouble).  ValueError for a non-finite template and, normalised, for one whose values are all equal."""
    t = np.asarray(templates, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    taps = np.zeros(t.shape, np.float32)
    h0, q = np.zeros(len(t), LD), np.zeros(len(t), LD)
    for k in range(len(t)):
        h = [LD(x) for x in t[k].ravel()]
        n = len(h)
        if not all(np.isfinite(x) for x in h):
            raise ValueError('non-finite template')
        if normalize:
            if max(h) == min(h):
                raise ValueError('constant template')
            s = LD(0)
            for x in h:
                s += x
            mean = s/LD(n)
            ss = LD(0)
            for x in h:
                ss += (x - mean)*(x - mean)
            norm = np.sqrt(ss)
            g = [np.float32((x - mean)/norm) for x in h]
        else:
            g = [np.float32(x) for x in h]
        s = LD(0)
        for x in g:
            s += LD(x)
        gm = s/LD(n)
        ss = LD(0)
        for x in g:
            ss += (LD(x) - gm)*(LD(x) - gm)
        taps[k] = np.array(g, np.float32).reshape(t.shape[1:])
        h0[k], q[k] = s, ss
    return taps, h0, q


def scores(v, taps, k0, first, n_out, normalize, min_std=0.0, pivot=0.0):
    """The scores of the rounded `taps` (K, Tt, Fb) float32 over the values v (C, frames, nfreq), band [k0, k0 + Fb),
    windows starting at first + i, i < n_out.  Returns a dict of
      value  (K, C, n_out) float64: s or r, NaN by the header's rules
      bound  (K, C, n_out) float64: the header's bound on |out - value| (0 where value is not finite); with a sequence of
             pivots (P, K, C, n_out), one per pivot -- the value does not depend on it
      near   (C, n_out) bool: normalised windows the mask cannot decide (see the module docstring)
      std    (C, n_out) float64: sqrt(D/n) of every window that lies inside the slab and is finite, else NaN."""
    v = np.asarray(v)
    taps = np.asarray(taps, np.float32)
    K, Tt, Fb = taps.shape
    C, frames, _ = v.shape
    n = Tt*Fb
    g = taps.reshape(K, n).astype(LD)
    ga = np.abs(g)
    h0 = np.array([sum(row, LD(0)) for row in g])
    q = np.array([np.sum((row - np.sum(row)/LD(n))**2) for row in g])
    gamma = (n + 3)*U/(1.0 - (n + 3)*U)
    e_d = (3*n + 6)*E
    pivots = [LD(np.float32(x)) for x in np.atleast_1d(pivot)]
    thr = LD(n)*LD(min_std)*LD(min_std)
    value = np.full((K, C, n_out), np.nan)
    bound = np.zeros((len(pivots), K, C, n_out))
    near = np.zeros((C, n_out), bool)
    std = np.full((C, n_out), np.nan)
    with np.errstate(all='ignore'):
        for c in range(C):
            for i in range(n_out):
                t = first + i
                if t < 0 or t + Tt > frames:
                    continue
                w = v[c, t:t + Tt, k0:k0 + Fb].reshape(n).astype(LD)
                M = [ga @ np.abs((w - p).astype(np.float32).astype(LD)) for p in pivots]
                if not normalize:
                    s = g @ w
                    value[:, c, i] = s.astype(np.float64)
                    for j, p in enumerate(pivots):
                        b = gamma*M[j] + 4*E*np.abs(p*h0) + (U*np.abs(s) if p != 0 else 0)
                        bound[j, :, c, i] = np.where(np.isfinite(s), b, 0).astype(np.float64)
                    continue
                if not np.all(np.isfinite(w)):
                    continue
                wm = np.sum(w)/LD(n)
                D = np.sum((w - wm)**2)
                S2 = [np.sum((w - p)**2) for p in pivots]
                std[c, i] = np.sqrt(D/LD(n))
                near[c, i] = abs(D - thr) <= e_d*max(S2) + 4*E*thr
                if D <= thr:
                    continue
                r = (g @ (w - wm))/np.sqrt(q*D)
                value[:, c, i] = r.astype(np.float64)
                for j in range(len(pivots)):
                    cond = e_d*S2[j]/D
                    b = (gamma*M[j] + (n + 4)*E*np.sqrt(S2[j]/LD(n))*np.abs(h0))/np.sqrt(q*D) + (cond + U + 8*E)*np.abs(r) \
                        + 2.0**-149
                    bound[j, :, c, i] = (b if cond < 0.5 else np.full(K, np.inf)).astype(np.float64)
    if np.ndim(pivot) == 0:
        bound = bound[0]
    return {'value': value, 'bound': bound, 'near': near, 'std': std}
