"""The definition of hipdsp_spec_adapt (include/hip_dsp.h) and of BufferedAdaptiveSpectrogram in numpy longdouble, the
sequential float64 evaluation that sets the pattern of non-finite values, and the per-element bounds the GPU and host
tests hold both to.  Pinned to scipy.signal.lfilter by tests/golden/adaptive_spectrogram.npz.

For one column (channel c, bin k) of a slab (channels, frames, nfreq), x_t = spec[c, t, k], s = smooth, a = 1 - s:
    M_0 = x_0,    M_t = a*M_(t-1) + s*x_t    (t >= 1)
The first nbefore rows are warm-up only; output row i belongs to t = nbefore + i and is float32 of
    background  M_t            divide  x_t/(eps + M_t)            subtract  max(x_t - M_t, 0)
    pcen        (x_t/(eps + M_t)**gain + bias)**power - bias**power

The bounds (u = 2^-24, w = 2^-53, P_t = max_(j <= t) |x_j| of the column, for finite columns):

Smoother.  The kernels keep M in float64 and take a = fl(1 - s) (relative error w).  One step a*M + s*x rounds three
times: fl(a*M) by at most w*a*P_t, fl(s*x) by w*s*P_t, the sum by w*P_t (|a*M + s*x| <= P_t), together 2*w*P_t since a
+ s = 1; a's own rounding moves a*M by another w*a*P_t: at most three roundings of magnitude <= P_t a step.  The error
obeys the same recursion, so a + s = 1 damps what a step adds geometrically: sum a^j = 1/s, at most (3/s)*w*P_t.  The
chunked hand-over M' = fl(fl(A*M) + v), A = a^n rounded once from long double, adds w*P_t*(1 + 2*A) at a chunk border
(the two roundings and A's), damped by A from border to border: w*P_t*(1 + 2*A)/(1 - A), which is <= (1/s)*w*P_t for
every 0 < s <= 1 at n = 256, as at any n >= 3: it tends to 3/n for small s and to 1 at s = 1 (handover_share() evaluates
it; the zero-state end value v is a run of the same steps and is counted with them).  Together
    dM_t = (4/s)*w*P_t
background  |out - M| <= u*|M| + dM_t + 2^-149
subtract    |out - y| <= u*|y| + dM_t + 2^-149             (x - M in float64: w*|y| more, inside u*|y|)
divide      |out - y| <= |y|*(u + 4*w + dM_t/(eps + M_t)) + 2^-149        (fl(eps + M), the quotient: 2 w; 4 w is room)
            the first-order term as it stands, without the 1/(1 - d) of the exact propagation
pcen        E = eps + M, D = E**gain, G = x/D, B = G + bias, y = B**power - bias**power.  With K = POW_W (below) the error
            of one pow() in units of w, and r(d) = d/(1 - d), the relative change of 1/E when E moves by the fraction d
            (infinite for d >= 1: the exact propagation, since dM_t/E is not small where a column has dropped):
              dE = dM_t/E + w                       relative, of fl(eps + M)
              dG = gain*r(dE) + (K + 1)*w           relative: pow, the quotient
              dB = G*r(dG)/B + w                    relative: what G's error is of B, the sum's rounding
              dP = power*r(dB) + K*w                relative, of B**power; for power > 1 (1 + d)^p - 1 <= p*d*(1 + d)^(p-1),
                                                    taken as power*r(dB)*(1 + r(dB))^(power - 1)
            |out - y| <= u*|y| + B**power*dP + bias**power*K*w + w*|y| + 2^-149
            The last subtraction makes the term absolute in B**power: where G << bias, y is a small difference of two
            numbers near bias**power and inherits their absolute error.  bias**power is the same device pow() (a zero
            frame, G = 0, gives exactly 0).

POW_W is the one constant that cannot be derived here: the error of the device library's float64 pow().  It was measured
on an MI355X by tools/adaptive_pow_sweep against powl() over every binade of the base that float32 inputs reach
(eps + M from 2^-149 to 2^128, G + bias up to 2^277) for the exponents 0.98, 0.5, 0.25, 1/3, 0.9, 2 and 1e-3
(profiles/adaptive_spectrogram_bound.log): worst 1.9978 w, about one ulp, at exponent 1; POW_W = 4.0 is twice the worst
error seen, because the sweep samples arguments and does not exhaust them."""

import numpy as np

LD = np.longdouble
U = LD(2.0)**-24
W = LD(2.0)**-53
TINY = LD(2.0)**-149
MODES = ('background', 'divide', 'subtract', 'pcen')
CHUNK = 256                                   # HIPDSP_ADAPT_CHUNK
DEFAULTS = dict(gain=0.98, bias=2.0, power=0.5, eps=1e-20)
POW_W = 4.0                                   # in units of w = 2^-53: twice the worst of the sweep (see the docstring)


def smooth_for(time_constant, frame_rate):
    """s = (sqrt(1 + 4 T^2) - 1)/(2 T^2), T = time_constant*frame_rate: librosa's pcen coefficient."""
    T = LD(time_constant)*LD(frame_rate)
    return float((np.sqrt(1 + 4*T*T) - 1)/(2*T*T))


def smoother(spec, smooth, dtype=LD):
    """M (channels, frames, nfreq) of the slab spec, sequentially in `dtype` (longdouble: the definition; float64: the
    pattern of non-finite values)."""
    x = np.asarray(spec, dtype=np.float32).astype(dtype)
    s = dtype(smooth)
    a = dtype(1) - s
    M = np.empty_like(x)
    with np.errstate(all='ignore'):
        if x.shape[1] > 0:
            M[:, 0] = x[:, 0]
        for t in range(1, x.shape[1]):
            M[:, t] = a*M[:, t - 1] + s*x[:, t]
    return M


def mode_value(x, M, mode, gain, bias, power, eps, dtype=LD):
    gain, bias, power, eps = dtype(gain), dtype(bias), dtype(power), dtype(eps)
    with np.errstate(all='ignore'):
        if mode == 'background':
            return M.copy()
        if mode == 'divide':
            return x/(eps + M)
        if mode == 'subtract':
            d = x - M
            return np.where(d < 0, dtype(0), d)
        if mode == 'pcen':
            return np.power(x/np.power(eps + M, gain) + bias, power) - np.power(bias, power)
    raise ValueError(mode)


def running_peak(spec):
    """P_t = max_(j <= t) |x_j| per column, longdouble."""
    return np.maximum.accumulate(np.abs(np.asarray(spec, dtype=np.float32).astype(LD)), axis=1)


def _r(d):
    with np.errstate(all='ignore'):
        return np.where(d < 1, d/np.where(d < 1, 1 - d, 1), LD(np.inf))


def handover_share(smooth, n=CHUNK):
    """s*(1 + 2 A)/(1 - A), A = a^n: the hand-over's part of the smoother bound in units of (1/s)*w*P_t (<= 1)."""
    s = LD(smooth)
    A = (1 - s)**n
    return float(s*(1 + 2*A)/(1 - A))


class Definition(object):
    """The definition of one slab (channels, frames, nfreq) under one `smooth`: the floor is computed once, every mode
    and its bound over ALL rows from it (output row i of a call with nbefore is row nbefore + i here)."""

    def __init__(self, spec, smooth):
        self.spec = np.asarray(spec, dtype=np.float32)
        self.smooth = float(smooth)
        self.x = self.spec.astype(LD)
        self.M = smoother(self.spec, smooth)
        self.P = running_peak(self.spec)

    def value(self, mode, gain=0.98, bias=2.0, power=0.5, eps=1e-20):
        return mode_value(self.x, self.M, mode, gain, bias, power, eps)

    def bound(self, mode, gain=0.98, bias=2.0, power=0.5, eps=1e-20):
        """The per-element bound on |out - y| of the module's docstring, longdouble, for a slab of finite values."""
        x, M = self.x, self.M
        dM = (4/LD(self.smooth))*W*self.P
        ay = np.abs(self.value(mode, gain, bias, power, eps))
        with np.errstate(all='ignore'):
            if mode == 'background':
                return U*np.abs(M) + dM + TINY
            if mode == 'subtract':
                return U*ay + dM + TINY
            E = LD(eps) + M
            if mode == 'divide':
                rel = U + 4*W + dM/np.abs(E)
                return np.where(ay == 0, 0, ay*rel) + TINY          # (x = 0 gives exactly 0 whatever the floor's error)
            gain, bias, power = LD(gain), LD(bias), LD(power)
            K = LD(POW_W)
            dE = dM/np.abs(E) + W
            dG = gain*_r(dE) + (K + 1)*W
            G = x/np.power(E, gain)
            B = G + bias
            dB = np.where((B > 0) & (G != 0), np.abs(G)*_r(dG)/np.where(B > 0, B, 1), 0) + W
            rB = _r(dB)
            grow = np.power(1 + rB, power - 1) if power > 1 else LD(1)
            dP = power*rB*grow + K*W
            return U*ay + np.power(B, power)*dP + np.power(bias, power)*K*W + W*ay + TINY

    def within(self, got, nbefore, mode, **kw):
        """(ok, worst ratio |got - y|/bound): every element of got (channels, frames - nbefore, nfreq) inside the bound."""
        y, b = self.value(mode, **kw)[:, nbefore:], self.bound(mode, **kw)[:, nbefore:]
        got = np.asarray(got, dtype=np.float32)
        assert got.shape == y.shape, (got.shape, y.shape)
        err = np.abs(got.astype(LD) - y)
        with np.errstate(all='ignore'):
            ratio = err/b
        worst = float(np.max(ratio)) if ratio.size else 0.0
        return bool(np.all(err <= b)), worst


def adapt(spec, nbefore, smooth, mode, gain=0.98, bias=2.0, power=0.5, eps=1e-20, dtype=LD):
    """The definition on a slab (channels, frames, nfreq): float32 (channels, frames - nbefore, nfreq); dtype float64
    is the sequential float64 evaluation that sets the pattern of non-finite values."""
    x = np.asarray(spec, dtype=np.float32).astype(dtype)
    y = mode_value(x, smoother(spec, smooth, dtype), mode, gain, bias, power, eps, dtype)[:, nbefore:]
    with np.errstate(all='ignore'):
        return y.astype(np.float32)


def chunked_model(spec, smooth, n=CHUNK):
    """numpy float64 model of the kernels' hand-over: per chunk of n frames the zero-state end value v (chunk 0: from
    M_0 = x_0), the scan M' = A*M + v with A = a^n rounded once from longdouble, then every chunk again from its true
    entering state.  Returns M (channels, frames, nfreq) float64."""
    x = np.asarray(spec, dtype=np.float32).astype(np.float64)
    s = np.float64(smooth)
    a = np.float64(1.0) - s
    A = np.float64(LD(a)**n)
    frames = x.shape[1]
    chunks = -(-frames//n)
    v = []
    for j in range(chunks - 1):
        m = x[:, 0].copy() if j == 0 else np.zeros_like(x[:, 0])
        for t in range(j*n + (1 if j == 0 else 0), (j + 1)*n):
            m = a*m + s*x[:, t]
        v.append(m)
    enter, m = [None], np.zeros_like(x[:, 0]) if frames else None
    for j in range(chunks - 1):
        m = A*m + v[j]
        enter.append(m)
    M = np.empty_like(x)
    for j in range(chunks):
        t0, t1 = j*n, min((j + 1)*n, frames)
        if j == 0:
            m = x[:, 0].copy()
            M[:, 0] = m
            t0 = 1
        else:
            m = enter[j]
        for t in range(t0, t1):
            m = a*m + s*x[:, t]
            M[:, t] = m
    return M


# ---- cases ------------------------------------------------------------------------------------------------------

def decades_slab(rng, channels, frames, nfreq, zero_tail=0):
    """x >= 0 float32: every column spans 12 decades (log-uniform around a column level), column 0 of every channel
    drops by 10^9 in the middle of the slab, the last zero_tail frames are zero."""
    level = np.power(10.0, rng.uniform(-14.0, -2.0, (channels, 1, nfreq)))
    x = level*np.power(10.0, rng.uniform(0.0, 12.0, (channels, frames, nfreq)))
    if nfreq > 0 and frames > 1:
        col = np.power(10.0, rng.uniform(0.0, 1.0, (channels, frames)))
        col[:, frames//2:] *= 1e-9
        x[:, :, 0] = col
    if zero_tail:
        x[:, frames - zero_tail:] = 0.0
    return x.astype(np.float32)


def same_pattern(got, want):
    """The NaN / +inf / -inf / finite pattern of two arrays is the same."""
    got, want = np.asarray(got), np.asarray(want)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


def exact_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float32).view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))
