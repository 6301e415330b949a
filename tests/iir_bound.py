"""A local accuracy bound for the IIR sweeps (hipdsp_sosfilt, the envelope sweeps, the fused forward sweep, the
multi-plan envelope), the test signals it is applied to and the reference it is measured against.

The suite's parity metric (conftest.rel_err) divides a channel's largest error by the channel's loudest sample and
allows 1e-4: an error that sits where the trace is quiet -- behind a loud passage, behind a segment border where a
warm-up or a state hand-over replaces history, at the ends of a sosfiltfilt -- passes.  The kernels' contract is
float64 coefficients and state with float32 I/O: one rounding.  Here every window of 64 consecutive samples
(aligned to sample 0 of the call's input, also when `skip` / `env_first` drop a prefix; the last may be short) is
held to that:

    r_w = max_w |ref|,  e_w = max_w |got - ref|,      e_w <= (1 + 16 q) 2^-24 r_w,      got == 0 where r_w == 0

* The 1 is derived: the kernels carry float64 and round once to float32, round-to-nearest is off by at most 2^-24
  relative.
* q belongs to the CASE (filter x input), not to the kernel: the largest e_w / (2^-24 r_w) of the SEQUENTIAL
  float64 recurrence (this module's code with np.float64) against the reference (the same code with np.longdouble,
  eps <= 2^-63), computed at run time from the same inputs.  The factor 16 is a margin over the reference's own
  float64 error, not a measurement of the kernel: the block-parallel form reaches an output through 32-term dot
  products (phase 1), a six-step scan over the lanes and hand-over sums over up to the filter's memory in tiles,
  none of which a running recurrence has; each adds a small multiple of the same (float64 rounding x noise gain)
  term, and 16 leaves an order of magnitude for that.  Cases are chosen with q <= Q_CAP = 2^-6, so the whole
  allowance is at most a quarter of one float32 rounding (tests/test_iir_bound.py holds the case list to the cap).
* The odd extensions need no term for a low-pass envelope: sos.hip, chain.hip and chain_fwd.h form the
  right one (and, where the envelope starts inside the trace, the left one) in float32, 2.f*r(T-1) - r(T-2-i), and
  test_iir_bound.py shows the float64 recurrence with those extensions inside the bound with the 16 replaced by 1.
* Two float32 roundings that the reference does not have and that sit in the sweeps' tile loops are held to DERIVED
  terms on top, per sample and only on the paths they reach: extension_term (the extension's rounding under an
  envelope with a high-pass) and between_term (the forward pass handed to the backward pass through the float32 tile:
  envelope plans of three and four sections, the frame-split backward sweep).  Each is the rounding's size times the
  absolute response of the linear pass behind it.
* hipdsp_envelope_multi runs a cascade plan by plan and writes float32 between the plans: 2P - 1 roundings for P plans,
  held to handover_term, derived the same way (and to extension_term on both sides where the cascade has a high-pass:
  odd_ext_kernel forms both extensions in float32).
* The clamp at zero is judged apart from the arithmetic (envelope_case), and a case's reference must stay in the
  range where the bound can be met at all (assert_in_range).

tests/test_iir_bound.py calibrates all of this on the CPU (the restatement against the C oracle, the cap, the
correct model inside the bound, wrong versions outside it); tests/test_gpu_iir_accuracy.py applies it, and
tests/test_gpu_sweep_matrix.py applies it to every instantiation of the fused sweeps.
Nothing here imports scipy: designs come from audian_amd.design.butter_sos.
"""

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0**-63, 'np.longdouble is no wider than float64 here: the reference would measure nothing'

ULP = 2.0**-24             # one float32 rounding, relative
MARGIN = 16.0
Q_CAP = 2.0**-6
WINDOW = 64
TILE = 2048
GAIN = np.pi/2             # the reference's envelope: sosfiltfilt(sos, (pi/2)*|x|)

FAMILIES = ('stepdown', 'stepup', 'offset', 'burst', 'onset')
ONSET = 5000


# ---- signal families ------------------------------------------------------------------------------------------

def family(name, T, rate, seed=0, level=None):
    """One float32 row of T samples; s = 0.5 uniform(-1, 1) + 0.5 sin(2 pi 1000 t):

    stepdown  amplitude 1 for the first quarter, then `level` (1e-4)
    stepup    `level` (1e-4) for the first half, then 1
    offset    1 + `level` (1e-3) * s
    burst     (`level` (1e-4) + a Gaussian of width 300 samples at T/2) * s
    onset     exact zeros for the first 5000 samples, then s
    """
    rng = np.random.default_rng([seed, FAMILIES.index(name), T])
    n = np.arange(T, dtype=np.float64)
    s = 0.5*rng.uniform(-1.0, 1.0, T) + 0.5*np.sin(2*np.pi*1000.0*n/rate)
    if name == 'stepdown':
        x = np.where(n < T//4, 1.0, 1e-4 if level is None else level)*s
    elif name == 'stepup':
        x = np.where(n < T//2, 1e-4 if level is None else level, 1.0)*s
    elif name == 'offset':
        x = 1.0 + (1e-3 if level is None else level)*s
    elif name == 'burst':
        x = ((1e-4 if level is None else level) + np.exp(-0.5*((n - T//2)/300.0)**2))*s
    elif name == 'onset':
        x = np.where(n < ONSET, 0.0, s)
    else:
        raise ValueError(name)
    return x.astype(np.float32)


def families(names, T, rate, seed=0):
    """(T, len(names)) float32: the families as the channels of one call; a name may be (name, level)."""
    pairs = [nm if isinstance(nm, tuple) else (nm, None) for nm in names]
    return np.ascontiguousarray(np.stack([family(nm, T, rate, seed, level) for nm, level in pairs], axis=1))


# ---- the reference: scipy's sosfilt / sosfiltfilt restated, one time loop over (T, lanes) in `dtype` ------------

def _coef(sos, dtype):
    sos = np.asarray(sos, dtype=np.float64)
    assert sos.ndim == 2 and sos.shape[1] == 6 and np.all(sos[:, 3] == 1.0)
    return [tuple(dtype(v) for v in (row[0], row[1], row[2], row[4], row[5])) for row in sos]


def sosfilt(sos, x, dtype=LD, zi=None, round_state_every=0):
    """scipy.signal.sosfilt along axis 0 of (T, lanes): direct form II transposed, samples outer, sections inner,
    zero initial state unless `zi` ((S, 2, lanes), consumed) is given.  round_state_every = n rounds the cascade's
    state to float32 at every multiple of n samples (a wrong version for the calibration, never a reference)."""
    coef = _coef(sos, dtype)
    x = np.asarray(x).astype(dtype)
    T, lanes = x.shape
    z = [[np.zeros(lanes, dtype), np.zeros(lanes, dtype)] for _ in coef] if zi is None else \
        [[np.array(zi[s][0], dtype), np.array(zi[s][1], dtype)] for s in range(len(coef))]
    y = np.empty((T, lanes), dtype)
    for i in range(T):
        if round_state_every and i and i % round_state_every == 0:
            z = [[v.astype(np.float32).astype(dtype) for v in zs] for zs in z]
        cur = x[i]
        for s, (b0, b1, b2, a1, a2) in enumerate(coef):
            zs = z[s]
            out = b0*cur + zs[0]
            zs[0] = b1*cur - a1*out + zs[1]
            zs[1] = b2*cur - a2*out
            cur = out
        y[i] = cur
    return y


def padlen(sos):
    """scipy's default sosfiltfilt pad length: 3 ntaps, ntaps reduced by the first-order sections."""
    sos = np.asarray(sos, dtype=np.float64)
    ntaps = 2*len(sos) + 1 - min(int(np.sum(sos[:, 2] == 0)), int(np.sum(sos[:, 5] == 0)))
    return 3*ntaps


def sosfilt_zi(sos, dtype=LD):
    """scipy.signal.sosfilt_zi, (S, 2): lfilter_zi of a biquad in closed form ((I - A) zi = B, B = b[1:] - a[1:] b0,
    I - A = [[1 + a1, -1], [a2, 1]]), scaled by the DC gain of the sections in front."""
    zi = np.zeros((len(sos), 2), dtype)
    scale = dtype(1)
    for s, (b0, b1, b2, a1, a2) in enumerate(_coef(sos, dtype)):
        B0, B1 = b1 - a1*b0, b2 - a2*b0
        det = (1 + a1) + a2
        zi[s, 0] = scale*(B0 + B1)/det
        zi[s, 1] = scale*((1 + a1)*B1 - a2*B0)/det
        scale = scale*(b0 + b1 + b2)/(1 + a1 + a2)
    return zi


def _filtfilt(sos, ext, dtype, between_f32=False):
    """Forward pass from zi ext[0], reversal, forward pass from zi y[-1], reversal (scipy's sosfiltfilt behind its
    extension; linear in ext).  between_f32: the forward pass's output is rounded to float32 on its way to the
    backward pass (a model of the sweeps that keep it in a float32 tile, never the reference)."""
    zi = sosfilt_zi(sos, dtype)
    y = sosfilt(sos, ext, dtype, zi=zi[:, :, None]*ext[0][None, None, :])
    if between_f32:
        y = y.astype(np.float32).astype(dtype)
    return sosfilt(sos, y[::-1], dtype, zi=zi[:, :, None]*y[-1][None, None, :])[::-1]


def _ext32(r, edge):
    """The odd extensions as the kernels form them, in float32 from the float32 trace r: (left, right), (edge, lanes)."""
    r32 = r.astype(np.float32)
    assert np.array_equal(r32, r)
    return np.float32(2)*r32[0] - r32[edge:0:-1], np.float32(2)*r32[-1] - r32[-2:-(edge + 2):-1]


def sosfiltfilt(sos, x, dtype=LD, gain=GAIN, rectify=True, clamp=True, right_ext_f32=False, left_ext_f32=False,
                between_f32=False):
    """The envelope as the reference forms it, along axis 0 of (T, lanes): u = gain |x| (or gain x), scipy's
    sosfiltfilt(sos, u) -- odd extension by padlen on both sides, forward pass from zi u_ext[0], reversal, forward
    pass from zi y[-1], reversal, trim -- and optionally the clamp at zero.  right_ext_f32 / left_ext_f32: that
    extension is formed from the float32 trace in float32 before the gain, as the kernels do (the right one always,
    the left one where the envelope starts inside the trace: a model for the calibration, never the reference)."""
    x = np.asarray(x)
    T = len(x)
    edge = padlen(sos)
    if T <= edge:
        raise ValueError('The length of the input vector x must be greater than padlen, which is %d.' % edge)
    r = np.abs(x) if rectify else x
    u = dtype(gain)*r.astype(dtype)
    left, right = 2*u[0] - u[edge:0:-1], 2*u[-1] - u[-2:-(edge + 2):-1]
    if left_ext_f32:
        left = dtype(gain)*_ext32(r, edge)[0].astype(dtype)
    if right_ext_f32:
        right = dtype(gain)*_ext32(r, edge)[1].astype(dtype)
    y = _filtfilt(sos, np.concatenate([left, u, right]), dtype, between_f32)[edge:edge + T]
    if clamp:
        y = np.where(y < 0, dtype(0), y)
    return y


# ---- the float32 odd extension, where it shows ----------------------------------------------------------------------
# A low-pass envelope follows the level of the rectified trace, the extension's rounding (2^-24 of that level) is
# 2^-24 of the answer, and the correct model stays inside the bound (test_iir_bound.py).  An envelope WITH A
# HIGH-PASS (DC gain zero) takes the level out: next to the end of the trace its answer can be orders of magnitude
# under the rectified trace's level, and the rounding of the extension's samples -- in a float32 tile, where the
# kernels keep them -- shows against it (the model misses the bound by up to 3000 on `offset`).  Moving it to
# float64 would put a second, float64 tile into the sweeps' tile loops; instead such envelopes are held to the
# derived term below, which decays with the filter's impulse response away from the end.

def extension_response(sos, T, left=False):
    """|G|, (T, edge) float64: the answer of the (linear) forward-backward pass at the trace's T samples to a unit
    pulse at sample i of the right (or left) extension.  Depends on the filter and T only."""
    def make():
        edge = padlen(sos)
        ext = np.zeros((T + 2*edge, edge))
        ext[np.arange(edge) + (0 if left else edge + T), np.arange(edge)] = 1.0
        if left:
            return np.abs(_filtfilt(sos, ext, np.float64)[edge:edge + T])
        y = ext                                         # (the forward pass answers nothing in front of the pulses)
        y[edge + T:] = sosfilt(sos, ext[edge + T:], np.float64)
        zi = sosfilt_zi(sos, np.float64)
        return np.abs(sosfilt(sos, y[::-1], np.float64, zi=zi[:, :, None]*y[-1][None, None, :])[::-1][edge:edge + T])
    return _cached((np.asarray(sos, dtype=np.float64).tobytes(), T, bool(left), 'G'), make)


def extension_term(sos, x, gain=GAIN, rectify=True, left=False):
    """(T, lanes) float64, per sample: what the float32 rounding of the right (and, with `left`, the left) extension
    can add to the envelope of x.  Sample i of the extension is e_i = 2 r(T-1) - r(T-2-i) rounded once to float32:
    off by at most 2^-24 |fl(e_i)|; the pass is linear, so the answer at sample n is off by at most
    gain sum_i |G(n, i)| 2^-24 |fl(e_i)|."""
    x = np.asarray(x)
    r = np.abs(x) if rectify else x
    edge = padlen(sos)
    e_left, e_right = _ext32(r, edge)
    term = extension_response(sos, len(x)) @ (ULP*np.abs(e_right.astype(np.float64)))
    if left:
        term = term + extension_response(sos, len(x), left=True) @ (ULP*np.abs(e_left.astype(np.float64)))
    return (gain if rectify else 1.0)*term


# ---- the float32 tile between the two passes -----------------------------------------------------------------------
# env_bwd_kernel for plans of three and four sections (REGW false) and the backward sweep of "chain_split_frames"
# (chain.hip) write the recomputed forward pass into the float32 tile and run the backward cascade from there: one
# float32 rounding of the forward output that the reference does not have (the one- and two-section sweeps of sos.hip
# keep it in float64 registers).  It sits in the tile loop -- the registers are what the three- and four-section plans
# lack -- so those two paths are held to the term below instead.

def _responses(sos, N):
    """(|h|, |s|), (N,) float64 each: the absolute impulse response of a run of sections from zero state, and (where the
    run starts the cascade) its absolute answer to the state zi alone."""
    def make():
        pulse = np.zeros((N, 1))
        pulse[0] = 1.0
        zi = sosfilt_zi(sos, np.float64)
        return (np.abs(sosfilt(sos, pulse, np.float64)[:, 0]),
                np.abs(sosfilt(sos, np.zeros((N, 1)), np.float64, zi=zi[:, :, None]*np.ones((1, 1, 1)))[:, 0]))
    return _cached((np.asarray(sos, dtype=np.float64).tobytes(), N, 'h'), make)


def _conv(h, w):
    """sum_(m <= n) h(n - m) w(m, lane), (N, lanes), h and w non-negative, by FFT (negative round-off clipped)."""
    N = len(w)
    n = 1 << int(np.ceil(np.log2(2*N)))
    return np.maximum(np.fft.irfft(np.fft.rfft(h, n)[:, None]*np.fft.rfft(w, n, axis=0), n, axis=0)[:N], 0.0)


def between_term(sos, x, gain=GAIN, rectify=True):
    """(T, lanes) float64, per sample: what rounding the forward pass's output y_f to float32 can add to the envelope
    of x.  Sample m of it is off by at most 2^-24 |fl(y_f(m))|; the backward pass is linear with impulse response h and
    starts from zi fl(y_f(last)), so the answer at sample n is off by at most
    2^-24 (sum_(m >= n) |h(m - n)| |fl(y_f(m))| + |s(last - n)| |fl(y_f(last))|), s the answer to the state zi alone."""
    x = np.asarray(x)
    T = len(x)
    edge = padlen(sos)
    r = np.abs(x) if rectify else x
    u = (gain if rectify else 1.0)*r.astype(np.float64)
    left, right = 2*u[0] - u[edge:0:-1], (gain if rectify else 1.0)*_ext32(r, edge)[1].astype(np.float64)
    ext = np.concatenate([left, u, right])
    zi = sosfilt_zi(sos, np.float64)
    yf = sosfilt(sos, ext, np.float64, zi=zi[:, :, None]*ext[0][None, None, :])
    w = (ULP*np.abs(yf.astype(np.float32)).astype(np.float64))[::-1]            # in the backward pass's order
    h, s = _responses(sos, len(w))
    p = _conv(h, w) + s[:, None]*w[0][None, :]
    return p[::-1][edge:edge + T]


# ---- two wrong versions, for the teeth check ---------------------------------------------------------------------

def wrong_f32_handover(sos, x):
    """The float64 run with the cascade's state rounded to float32 at every tile border."""
    return sosfilt(sos, x, np.float64, round_state_every=TILE)


def wrong_one_tile_warmup(sos, x, tiles=8):
    """The float64 run cut into 8-tile segments, each started from zero state one tile before its range."""
    x = np.asarray(x)
    y = np.empty(x.shape, np.float64)
    for lo in range(0, len(x), tiles*TILE):
        start = max(lo - TILE, 0)
        y[lo:lo + tiles*TILE] = sosfilt(sos, x[start:lo + tiles*TILE], np.float64)[lo - start:]
    return y


# ---- warm-ups that start inside the trace -----------------------------------------------------------------------------
# A segment of a sweep starts from zero state `warm` samples before its range (sos_plan.hip: the smallest multiple of the
# tile with ||A^warm|| < 2^-60): 26 tiles for the 20 Hz low-pass, 15 for the 100 Hz high-pass at 192 kHz.  At T_LONG (17
# tiles) every such warm-up is clipped at the start of the trace, which is exact.  The rows below are long enough for a
# segment to start from zero state in mid-trace: the third of three segments of 64 tiles starts at tile 44 and warms up
# from tile 18.  The forward sweep of a band-pass (hipdsp_sosfilt, the fused sweeps) cuts off the past, and `stepdown`
# shows it (quiet windows behind a loud passage); the backward sweep of an envelope cuts off the future, and `stepup`
# shows it.  (The envelope's forward sweep hands its states over exactly and has no warm-up.)

WARM_FAMILIES = ('stepdown', 'stepup', 'offset', 'burst')
WARM_BANDPASS = 'hp3 100 Hz @ 192 kHz'          # BANDPASSES; 2 sections, warm-up 15 tiles; q at most 2.2e-3 at T_WARM
WARM_ENVELOPE = 'lp2 20 Hz @ 96 kHz'            # ENVELOPES; 1 section, warm-up 26 tiles; q at most 5.3e-3 (forward pass)
WARM_FUSED = 'bp2 300-3000 Hz @ 96 kHz'         # the band-pass in front of WARM_ENVELOPE in the fused launches
T_WARM = {WARM_BANDPASS: 48*TILE + 5, WARM_ENVELOPE: 64*TILE + 5}
WARM_TILES = {WARM_BANDPASS: 15, WARM_ENVELOPE: 26}       # what hipdsp_sos_plan_host gives (test_iir_bound.py asserts it)


def segment_starts(n_tiles, seg_tiles):
    """The first tile of every segment of a sweep over n_tiles tiles in segments of seg_tiles (in the sweep's order: a
    backward sweep counts its tiles from the end of the extended trace)."""
    return list(range(0, n_tiles, seg_tiles))


def cut_warmups(n_tiles, seg_tiles, warm_tiles):
    """The segments (first tile, first tile of the warm-up) whose warm-up starts inside the trace, at least one tile
    from its start: the ones that run from zero state in place of history."""
    return [(t, t - warm_tiles) for t in segment_starts(n_tiles, seg_tiles) if t - warm_tiles >= 1]


def segmented_sosfilt(sos, x, warm_tiles, segments=3, zi=None, lead=0):
    """The float64 run of sosfilt(sos, x) cut into `segments` segments of whole tiles, every one started from zero state
    warm_tiles tiles before its range (from `zi` where that is the start of x).  `lead`: the tile grid starts that many
    samples in front of x (a backward sweep's ragged first tile).  A model for the calibration, never a reference."""
    x = np.asarray(x)
    n_tiles = -(-(len(x) + lead)//TILE)
    seg = -(-n_tiles//segments)*TILE
    y = np.empty(x.shape, np.float64)
    for lo in range(0, n_tiles*TILE, seg):
        a, b = max(lo - lead, 0), min(lo + seg - lead, len(x))
        start = max(lo - warm_tiles*TILE - lead, 0)
        y[a:b] = sosfilt(sos, x[start:b], np.float64, zi=zi if start == 0 else None)[a - start:]
    return y


def segmented_envelope(sos, x, warm_tiles, segments=3, gain=GAIN):
    """The float64 envelope of x, unclamped, as the sweeps cut it: the right extension formed in float32, the forward
    pass whole (its states are handed over exactly), the backward pass over the trace and its right extension in
    `segments` segments of whole tiles counted from the end, every one started from zero state warm_tiles tiles behind
    its range.  A model for the calibration, never a reference."""
    x = np.asarray(x)
    T, edge = len(x), padlen(sos)
    r = np.abs(x)
    u = gain*r.astype(np.float64)
    ext = np.concatenate([2*u[0] - u[edge:0:-1], u, gain*_ext32(r, edge)[1].astype(np.float64)])
    zi = sosfilt_zi(sos, np.float64)
    y = sosfilt(sos, ext, np.float64, zi=zi[:, :, None]*ext[0][None, None, :])
    back = segmented_sosfilt(sos, y[::-1], warm_tiles, segments, zi=zi[:, :, None]*y[-1][None, None, :], lead=-(T + edge) % TILE)
    return back[::-1][edge:edge + T]


# ---- the metric -------------------------------------------------------------------------------------------------

def window_stats(got, ref, first=0):
    """(e_w, r_w), each (windows, lanes) longdouble, of (n, lanes) arrays that hold samples first ... first + n - 1
    of the call; windows sit on the grid of the call's sample 0."""
    ref = np.asarray(ref, dtype=LD)
    got = np.asarray(got).astype(LD)
    assert got.shape == ref.shape and ref.ndim == 2 and len(ref) > 0, (got.shape, ref.shape)
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err)
    pos = np.arange(len(ref)) + first
    starts = np.concatenate([[0], np.nonzero(pos[1:] % WINDOW == 0)[0] + 1])
    return np.maximum.reduceat(err, starts, axis=0), np.maximum.reduceat(np.abs(ref), starts, axis=0)


def ratios(got, ref, first=0):
    """e_w / (2^-24 r_w), (windows, lanes) float64; where r_w == 0: 0 if the result is exactly zero there, inf if
    not."""
    e, r = window_stats(got, ref, first)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(r == 0, np.where(e == 0, 0.0, np.inf), e/(ULP*r)).astype(np.float64)


def allowance(run64, ref, first=0):
    """q of a case, per lane: the worst ratio of the sequential float64 run against the reference."""
    return np.max(ratios(run64, ref, first), axis=0)


def assert_within(got, ref, q, what, first=0, margin=MARGIN, term=None):
    """Assert e_w <= (1 + margin q) 2^-24 r_w for every window and lane (q a scalar or one value per lane), exact
    zeros where the reference is all zero; `what` names the case.  `term` ((n, lanes), extension_term) is a
    per-sample absolute allowance on top: its largest value in the window joins the right-hand side.  Returns the
    worst ratio e_w / (2^-24 r_w) (with a term: of what is left of e_w beyond it)."""
    e, r = window_stats(got, ref, first)
    if term is not None:
        _, t = window_stats(term, term, first)
        e = np.where(r == 0, e, np.maximum(e - t, 0))
    with np.errstate(divide='ignore', invalid='ignore'):
        rho = np.where(r == 0, np.where(e == 0, 0.0, np.inf), e/(ULP*r)).astype(np.float64)
    bound = 1.0 + margin*np.broadcast_to(np.asarray(q, dtype=np.float64), rho.shape[1:])
    over = rho/bound[None, :]
    w, lane = np.unravel_index(int(np.argmax(over)), over.shape)
    assert rho[w, lane] <= bound[lane], \
        '%s: lane %d, window %d of the call (samples from %d): e_w / (2^-24 r_w) = %.6g, allowed %.6g (q %.3g)' % (
            what, lane, w + first//WINDOW, (w + first//WINDOW)*WINDOW, rho[w, lane], bound[lane],
            (bound[lane] - 1)/margin if margin else 0.0)
    return float(np.max(rho))


def allowance_share(got, ref, q, term=None, first=0, margin=MARGIN):
    """Per lane, the largest e_w / ((1 + margin q) 2^-24 r_w + the term's largest value in the window): the share of the
    whole allowance that a result uses (above 1 where assert_within fails; inf for a non-zero result where nothing is
    allowed).  A figure to report next to assert_within, never in its place."""
    e, r = window_stats(got, ref, first)
    allowed = (1.0 + margin*np.broadcast_to(np.asarray(q, dtype=np.float64), r.shape))*ULP*r
    if term is not None:
        allowed = allowed + np.where(r == 0, 0, window_stats(term, term, first)[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.max(np.where(allowed > 0, e/allowed, np.where(e > 0, np.inf, 0.0)), axis=0).astype(np.float64)


# ---- the cases: filter x families, shared by the CPU calibration and the GPU tests ---------------------------------
# Every (filter, family) pair below meets q <= Q_CAP (test_iir_bound.py asserts it; measured q in the comments, at
# T_LONG) and keeps its reference where the bound can be met at all (assert_in_range): `onset` rides only where the
# sweep's answer in front of the onset is exactly zero (sosfilt) or decays slowly enough (the 20 Hz and 60 Hz
# low-passes, the envelopes with a high-pass).

T_LONG = 16*TILE + 5          # 17 tiles with a ragged tail, above the fused sweep's minimum, shorter than the memory of
#                               the 20 Hz low-pass (a state is a sum over every hand-over)
T_SKIP = 3*TILE + 17
SKIPS = (0, 1, 2047, 2049)
ENV_FIRST = (0, 12345)

# the 5-3000 Hz band-pass at 96 kHz (the slowest-decaying band-pass the suite uses) exceeds the cap behind an 80 dB
# step (q 0.45 stepdown, 0.21 offset, 0.05 burst at the default levels): it takes stepup as is (4e-4) and steps of
# 40 / 20 / 40 dB for the others (stepdown to 1e-2: 6e-3, offset + 1e-1 s: 8e-3, burst over 1e-2: 2e-3)
SLOW_FAMILIES = ('stepup', ('stepdown', 1e-2), ('offset', 1e-1), ('burst', 1e-2), 'onset')

# label: (order, Wn, btype, rate, families)                                    sections, largest q
BANDPASSES = {
    'lp1 4000 Hz @ 48 kHz': (1, 4000.0, 'lowpass', 48000.0, FAMILIES),                   # 1, 6e-9
    'bp1 300-3000 Hz @ 96 kHz': (1, (300.0, 3000.0), 'bandpass', 96000.0, FAMILIES),     # 1, 2e-5
    'bp2 300-3000 Hz @ 96 kHz': (2, (300.0, 3000.0), 'bandpass', 96000.0, FAMILIES),     # 2, 2e-3
    'bp2 5-3000 Hz @ 96 kHz': (2, (5.0, 3000.0), 'bandpass', 96000.0, SLOW_FAMILIES),    # 2, 8e-3
    'hp3 100 Hz @ 192 kHz': (3, 100.0, 'highpass', 192000.0, FAMILIES),                  # 2, 8e-4
    'bp3 300-3000 Hz @ 48 kHz': (3, (300.0, 3000.0), 'bandpass', 48000.0, FAMILIES),     # 3, 5e-5
    'bp4 300-3000 Hz @ 48 kHz': (4, (300.0, 3000.0), 'bandpass', 48000.0, FAMILIES),     # 4, 4e-4
}
GENERAL = 'bp3 300-3000 Hz @ 48 kHz'          # also run with its gain spread over the sections (general phase 3)
SKIP_BANDPASSES = ('bp2 300-3000 Hz @ 96 kHz', 'hp3 100 Hz @ 192 kHz')      # the cases run with `skip` at T_SKIP

# Envelopes (sosfiltfilt of pi/2 |x|).  In front of 5000 exact zeros the backward pass of a fast low-pass decays to
# 1e-32 (200 Hz), 1e-33 (300 Hz), 1e-100 (500 Hz) of the trace's level: below float32's range, or below what a sweep in
# time segments keeps of the history it cuts off (the planner's warm-up: ||A^n|| < 2^-60 of the state -- against a
# window more than 2^-36 under the loudest, more than a float32 rounding; measured 4-8 roundings there).  No `onset`
# for those (assert_in_range is the precondition).  Envelopes with a high-pass exceed the cap on `offset` as it
# stands (q 0.59 / 0.17 / 0.03 for the three below): 1 + 1e-1 s meets it (8e-3); they are the ones that take
# extension_term.
NO_ONSET = FAMILIES[:4]
HP_FAMILIES = ('stepdown', 'stepup', ('offset', 1e-1), 'burst', 'onset')
# label: (order, Wn, btype, rate, families)                                    sections, largest q
ENVELOPES = {
    'lp2 20 Hz @ 96 kHz': (2, 20.0, 'lowpass', 96000.0, FAMILIES),                       # 1, 6e-3
    'lp2 500 Hz @ 48 kHz': (2, 500.0, 'lowpass', 48000.0, NO_ONSET),                     # 1, 7e-7
    'lp3 200 Hz @ 44.1 kHz': (3, 200.0, 'lowpass', 44100.0, NO_ONSET),                   # 2, 4e-6
    'lp4 300 Hz @ 48 kHz': (4, 300.0, 'lowpass', 48000.0, NO_ONSET),                     # 2, 5e-6
    'bp2 10-500 Hz @ 48 kHz': (2, (10.0, 500.0), 'bandpass', 48000.0, HP_FAMILIES),      # 2, 8e-3
    'bp3 20-300 Hz @ 48 kHz': (3, (20.0, 300.0), 'bandpass', 48000.0, HP_FAMILIES),      # 3, 1.5e-3
    'lp8 60 Hz @ 48 kHz': (8, 60.0, 'lowpass', 48000.0, FAMILIES),                       # 4, 9e-4
    'bp4 50-800 Hz @ 48 kHz': (4, (50.0, 800.0), 'bandpass', 48000.0, HP_FAMILIES),      # 4, 3e-4
}
SKIP_ENVELOPES = ('lp2 500 Hz @ 48 kHz', 'bp2 10-500 Hz @ 48 kHz')
PLAYBACK = 'lp4 300 Hz @ 48 kHz'               # run once with rectify 0 (the playback low-pass: sosfiltfilt of x itself)

# band-pass and envelope of the fused launches (at most four and two sections); the envelope is that of the
# launch's own float32 band-pass output, of the families of the band-pass that the envelope's list names too
SOSFILT_ENVELOPE = (('bp2 300-3000 Hz @ 96 kHz', 'lp2 20 Hz @ 96 kHz'), ('bp4 300-3000 Hz @ 48 kHz', 'lp4 300 Hz @ 48 kHz'),
                    ('bp1 300-3000 Hz @ 96 kHz', 'bp2 10-500 Hz @ 48 kHz'))
CHAIN = {(2048, 1024): ('bp2 300-3000 Hz @ 96 kHz', 'lp2 20 Hz @ 96 kHz'),
         (2048, 512): ('bp1 300-3000 Hz @ 96 kHz', 'lp4 300 Hz @ 48 kHz'),
         (1024, 512): ('bp4 300-3000 Hz @ 48 kHz', 'lp2 500 Hz @ 48 kHz'),
         (1024, 256): ('bp3 300-3000 Hz @ 48 kHz', 'lp3 200 Hz @ 44.1 kHz'),
         (512, 256): ('hp3 100 Hz @ 192 kHz', 'lp2 20 Hz @ 96 kHz'),
         (256, 128): ('bp2 5-3000 Hz @ 96 kHz', 'lp4 300 Hz @ 48 kHz')}
SPLIT_FRAMES = (('bp2 300-3000 Hz @ 96 kHz', 'lp2 20 Hz @ 96 kHz'), ('bp2 300-3000 Hz @ 96 kHz', 'lp4 300 Hz @ 48 kHz'))

# The sweep matrix (tests/test_gpu_sweep_matrix.py) runs EVERY instantiation of the fused sweeps, so it needs one band-pass
# and one envelope per section count, every band-pass in front of every envelope: section count -> label.  q of the 16
# pairs at T_LONG (the float64 band-pass run rounded to float32 in front of the envelope) is at most 1.2e-2
# (bp4 + lp2 20 Hz); test_iir_bound.py holds every pair to the cap, from sample 0 and, for the pairs the matrix runs on
# the shifted grid (MATRIX_SHIFTED: the fused forward sweep takes envelopes of at most two sections), from ENV_FIRST[1].
MATRIX_BANDPASS = {1: 'bp1 300-3000 Hz @ 96 kHz', 2: 'bp2 300-3000 Hz @ 96 kHz', 3: 'bp3 300-3000 Hz @ 48 kHz',
                   4: 'bp4 300-3000 Hz @ 48 kHz'}
MATRIX_ENVELOPE = {1: 'lp2 20 Hz @ 96 kHz', 2: 'lp4 300 Hz @ 48 kHz', 3: 'bp3 20-300 Hz @ 48 kHz', 4: 'lp8 60 Hz @ 48 kHz'}
# One pair misses a precondition: from ENV_FIRST[1] the 20 Hz low-pass behind bp3 starts 4152 samples behind the step of
# `stepdown`, and the correct model with the left extension formed in float32 is off by 1.23 roundings in window 2 (1 + q
# allows 1.0001; the three other band-passes stay inside).  Behind bp3 the one-section envelope is the 500 Hz low-pass.
MATRIX_ENVELOPE_BEHIND = {(3, 1): 'lp2 500 Hz @ 48 kHz'}


def matrix_pair(sf, se):
    """(band-pass, envelope) labels of the sweep matrix for a band-pass of sf and an envelope of se sections."""
    return MATRIX_BANDPASS[sf], MATRIX_ENVELOPE_BEHIND.get((sf, se), MATRIX_ENVELOPE[se])


MATRIX_PAIRS = tuple(matrix_pair(sf, se) for sf in sorted(MATRIX_BANDPASS) for se in sorted(MATRIX_ENVELOPE))
MATRIX_SHIFTED = tuple(matrix_pair(sf, se) for sf in sorted(MATRIX_BANDPASS) for se in (1, 2))
# The fused forward sweep's PSD is judged per bin on stationary lanes of tests/spectral_bound.py that ride behind the
# band-pass's own families: `tones` and `edges` at both levels for each of the four window lengths (`edges` puts a tone on
# bin 1 of ITS window), the same 16 lanes for every shape, so that one reference per band-pass serves all six.
MATRIX_SPECTRAL = ('tones', 'edges')
MATRIX_NFFT = (2048, 1024, 512, 256)


def matrix_spectral_lanes(T, rate):
    """(T, 16) float32: for every window length of MATRIX_NFFT the families MATRIX_SPECTRAL, two levels each."""
    import spectral_bound as sb
    return np.ascontiguousarray(np.concatenate([sb.family(name, T, nfft, rate, seed=nfft)
                                                for nfft in MATRIX_NFFT for name in MATRIX_SPECTRAL], axis=1))


def has_highpass(sos):
    """An envelope plan whose DC gain is zero: the one that takes extension_term."""
    sos = np.asarray(sos, dtype=np.float64)
    return bool(np.any(np.abs(np.sum(sos[:, :3], axis=1)) <= 1e-9*np.sum(np.abs(sos[:, :3]), axis=1)))


def envelope_lanes(bp_families, env_families):
    """The lanes of a fused launch whose envelope is judged: families the envelope's list names (at any level)."""
    base = {f[0] if isinstance(f, tuple) else f for f in env_families}
    return [i for i, f in enumerate(bp_families) if (f[0] if isinstance(f, tuple) else f) in base]


def design(case, table=None):
    """(sos, rate, families) of a case of BANDPASSES / ENVELOPES."""
    from audian_amd.design import butter_sos
    order, wn, btype, rate, fams = (table if table is not None else BANDPASSES)[case]
    return butter_sos(order, wn, btype, rate), rate, fams


def spread(sos):
    """The same filter with its gain moved between the sections: numerators that are not scipy's [1, +-2, 1]."""
    t = np.array(sos, dtype=np.float64)
    for i in range(1, len(t)):
        t[0, :3] *= 1.0/(1.5 + i)
        t[i, :3] *= 1.5 + i
    return t


def assert_in_range(ref, what):
    """A case's precondition: no window's r_w lies in (0, 2^-126), where float32 has fewer than 24 bits, nor more than
    2^-36 under the lane's loudest window, where the 2^-60 of the history that a sweep in time segments cuts off reaches
    a float32 rounding."""
    _, r = window_stats(ref, ref)
    assert not np.any((r > 0) & (r < 2.0**-126)), '%s: the reference leaves float32\'s normal range' % what
    assert not np.any((r > 0) & (r < 2.0**-36*np.max(r, axis=0)[None, :])), '%s: a window more than 2^-36 under the loudest' % what


# ---- cached references -------------------------------------------------------------------------------------------

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _key(sos, x, *more):
    import hashlib
    x = np.ascontiguousarray(x)
    return (np.asarray(sos, dtype=np.float64).tobytes(), x.shape, hashlib.sha1(x.tobytes()).hexdigest()) + more


def sosfilt_runs(sos, x):
    """(reference (T, lanes) longdouble, sequential float64 run) of sosfilt(sos, x), computed once per (filter, input)."""
    return _cached(_key(sos, x, 'sosfilt'), lambda: (sosfilt(sos, x, LD), sosfilt(sos, x, np.float64)))


def sosfilt_case(sos, x):
    """(reference, q per lane) of sosfilt(sos, x)."""
    ref, run = sosfilt_runs(sos, x)
    return ref, allowance(run, ref)


def envelope_runs(sos, x, rectify=True, gain=GAIN):
    """(reference, sequential float64 run) of the UNCLAMPED envelope of x, computed once per (filter, input)."""
    gain = gain if rectify else 1.0
    return _cached(_key(sos, x, 'envelope', bool(rectify), float(gain)),
                   lambda: (sosfiltfilt(sos, x, LD, gain, rectify, False), sosfiltfilt(sos, x, np.float64, gain, rectify, False)))


def envelope_case(sos, x, rectify=True, gain=GAIN):
    """(reference, q per lane) of the unclamped envelope of x.  The clamp is judged apart from the arithmetic (the
    clamped result must be the clamp of the unclamped one, bit for bit): next to a zero crossing it leaves a window
    whose largest value is arbitrarily far under the values the recurrence carries there, the sequential float64 run
    itself is off by 0.1 roundings of THAT (q 0.04-0.12 on the 20 Hz low-pass), and a result on the other side of
    zero by less than the bound would have to be exactly zero."""
    ref, run = envelope_runs(sos, x, rectify, gain)
    return ref, allowance(run, ref)


def clamped(y):
    """env[env < 0] = 0."""
    return np.where(y < 0, y.dtype.type(0), y)


# ---- hipdsp_envelope_multi: a cascade over several plans, float32 between them ------------------------------------------
# The call runs scipy's sosfiltfilt step by step: the odd extensions by the pad length of the WHOLE cascade, formed in
# float32 (odd_ext_kernel, both sides); one float64 sweep per plan, each from the whole table's zi for its sections
# (times the input gain in the first pass), each writing float32; a flip; the same sweeps from zi * y[-1]; a flip that
# trims.  With P plans that is 2P - 1 float32 roundings the reference does not have (after every plan of the forward
# pass, after every plan but the last of the backward pass; the last one is the bound's own 1), held to the derived
# handover_term below.  multi_model restates the call with exactly these roundings for the CPU calibration.

T_MULTI = 8*TILE + 5          # the smallest size at which one segment, three, the planner's choice and one-tile segments
#                               are four different cuts of N = T + 2 padlen

# label: (order, Wn, btype, rate, families, splits)                                       sections, largest q at T_MULTI
MULTI = {
    'lp10 800 Hz @ 48 kHz': (10, 800.0, 'lowpass', 48000.0, NO_ONSET, ((2, 2, 1), (4, 1))),              # 5, 9e-6
    'lp12 2000 Hz @ 48 kHz': (12, 2000.0, 'lowpass', 48000.0, NO_ONSET, ((3, 3),)),                      # 6, 1.2e-6
    'bp5 10-500 Hz @ 48 kHz': (5, (10.0, 500.0), 'bandpass', 48000.0, HP_FAMILIES, ((4, 1),)),           # 5, 1.3e-2
    'bp8 50-4000 Hz @ 48 kHz': (8, (50.0, 4000.0), 'bandpass', 48000.0, HP_FAMILIES, ((4, 4),)),         # 8, 2.8e-4
    'lp8 60 Hz @ 48 kHz': (8, 60.0, 'lowpass', 48000.0, FAMILIES, ((2, 2), (1, 1, 1, 1))),               # 4, 1.7e-3
}
MULTI_SINGLE = 'lp8 60 Hz @ 48 kHz'            # fits one plan too: also run through hipdsp_envelope, under the same reference
MULTI_SKIP = ('lp10 800 Hz @ 48 kHz', 'bp5 10-500 Hz @ 48 kHz')     # the cases run with `skip`
MULTI_EDGE = 'bp8 50-4000 Hz @ 48 kHz'         # eight sections: pad length 51
MULTI_PLAIN = 'lp12 2000 Hz @ 48 kHz'          # run once with rectify 0
MULTI_GAIN = ('lp10 800 Hz @ 48 kHz', 0.37)    # run once with another gain


def multi_design(case):
    """(sos, rate, families, splits) of a case of MULTI."""
    from audian_amd.design import butter_sos
    order, wn, btype, rate, fams, splits = MULTI[case]
    return butter_sos(order, wn, btype, rate), rate, fams, splits


def plan_slices(sos, split):
    """The sections of every plan of a cascade cut as `split`."""
    assert sum(split) == len(sos) and min(split) >= 1, (split, len(sos))
    lo = np.concatenate([[0], np.cumsum(split)])
    return [slice(int(a), int(b)) for a, b in zip(lo[:-1], lo[1:])]


MULTI_WRONG = ('pad length of the last plan', 'float32 state at tile borders', 'one-tile warm-up per segment',
               'input gain left out of the later plans\' zi', 'backward zi from the extension\'s first sample')


def _sweep(sos, x, zi, wrong):
    """One plan's sweep over the extended sequence in float64, as the kernel is meant to run it -- or as one of the
    wrong versions does."""
    if wrong == 'float32 state at tile borders':
        return sosfilt(sos, x, np.float64, zi=zi, round_state_every=TILE)
    if wrong == 'one-tile warm-up per segment':                  # two-tile segments, each from zero state one tile before
        y = np.empty(x.shape, np.float64)
        for lo in range(0, len(x), 2*TILE):
            start = max(lo - TILE, 0)
            y[lo:lo + 2*TILE] = sosfilt(sos, x[start:lo + 2*TILE], np.float64, zi=zi if lo == 0 else None)[lo - start:]
        return y
    return sosfilt(sos, x, np.float64, zi=zi)


def multi_model(sos, split, x, gain=GAIN, rectify=True, wrong=None):
    """hipdsp_envelope_multi restated with its roundings, (T, lanes) float32, unclamped: float32 extensions on both sides
    by the whole cascade's pad length, float64 sweeps, a float32 rounding after every plan of both passes, zi from the
    whole table.  `wrong`: one of MULTI_WRONG.  A model for the CPU calibration, never a reference."""
    assert wrong is None or wrong in MULTI_WRONG, wrong
    x = np.asarray(x)
    T = len(x)
    sos = np.asarray(sos, dtype=np.float64)
    parts = plan_slices(sos, split)
    edge = padlen(sos[parts[-1]]) if wrong == 'pad length of the last plan' else padlen(sos)
    r = (np.abs(x) if rectify else x).astype(np.float32)
    left, right = _ext32(r, edge)
    cur = np.concatenate([left, r, right]).astype(np.float64)
    g = float(gain) if rectify else 1.0
    zi = sosfilt_zi(sos, np.float64)
    first = cur[0].copy()
    for backward in (False, True):
        ref = cur[0].copy()
        if backward and wrong == 'backward zi from the extension\'s first sample':
            ref = first
        for p, part in enumerate(parts):
            scale = 1.0 if backward else g
            if p > 0 and wrong == 'input gain left out of the later plans\' zi':
                scale = 1.0
            feed = g*cur if (p == 0 and not backward) else cur
            cur = _sweep(sos[part], feed, zi[part][:, :, None]*(scale*ref)[None, None, :], wrong)
            cur = cur.astype(np.float32).astype(np.float64)
        cur = cur[::-1]
    return cur[edge:edge + T].astype(np.float32)


def handover_term(sos, split, x, gain=GAIN, rectify=True):
    """(T, lanes) float64, per sample: what the 2P - 1 float32 roundings between the plans of hipdsp_envelope_multi can
    add to the envelope of x.  Derived, not measured:

    * e is the extended sequence (float32-formed extensions, times the gain), v_k the float64 run of plans 1 ... k over
      it in the forward pass, u_k the same in the backward pass over the reversed v_P.  Rounding k writes fl(v) for a
      value v and is off by at most 2^-24 max(|v|, |fl(v)|).
    * Everything behind a rounding is linear.  A forward-pass rounding behind plan j reaches the point behind plan k
      through the sections of plans j+1 ... k, whose states start from zi e[0], which no rounding touches: it is bounded
      by the convolution with their absolute impulse response |h_(j,k]|.  What has gathered behind plan P, F(m), goes
      through the backward pass as in between_term: |h_all| of the whole cascade, plus |s_all(n)| F(last) for the states
      zi fl(v_P(last)) of EVERY plan of the backward pass (s_all the whole cascade's answer to zi alone).  A
      backward-pass rounding behind plan j < P reaches the answer through |h_(j,P]|.
    * The value a rounding sees is v_k plus what the earlier roundings have made of it, so its weight is
      2^-24 (|v_k| + that earlier term at this very point): this covers the products of two and more roundings
      exactly, nothing is dropped and no factor is fitted.
    * The float64 arithmetic of the sweeps is the case's q, as for every other path; the float32 extensions are
      extension_term's (added by the caller for cascades with a high-pass).
    Reversed and trimmed to the T samples."""
    def make():
        xx = np.asarray(x)
        T = len(xx)
        table = np.asarray(sos, dtype=np.float64)
        parts = plan_slices(table, split)
        P = len(parts)
        edge = padlen(table)
        r = (np.abs(xx) if rectify else xx).astype(np.float32)
        g = float(gain) if rectify else 1.0
        left, right = _ext32(r, edge)
        cur = g*np.concatenate([left, r, right]).astype(np.float64)
        N = len(cur)
        zi = sosfilt_zi(table, np.float64)

        pulse = np.zeros((N, 1))
        pulse[0] = 1.0
        signed = {}

        def response(j, k):                                     # h of plans j+1 ... k (0-based: parts[j] ... parts[k-1]), plan by plan
            if (j, k) not in signed:
                signed[j, k] = sosfilt(table[parts[k - 1]], pulse if k == j + 1 else response(j, k - 1), np.float64)
            return signed[j, k]

        def between(j, k):
            return np.abs(response(j, k)[:, 0])

        def rounding(v, earlier):
            return ULP*(np.maximum(np.abs(v), np.abs(v.astype(np.float32)).astype(np.float64)) + earlier)

        ref = cur[0].copy()
        weights = []                                            # W_j, the forward pass's roundings
        for k, part in enumerate(parts, 1):
            cur = sosfilt(table[part], cur, np.float64, zi=zi[part][:, :, None]*ref[None, None, :])
            earlier = sum((_conv(between(j, k), weights[j - 1]) for j in range(1, k)), np.zeros_like(cur))
            weights.append(rounding(cur, earlier))
            gathered = earlier + weights[-1]
        d = gathered[::-1]                                      # in the backward pass's order
        cur = cur[::-1]
        ref = cur[0].copy()
        h_all, s_all = _responses(table, N)
        weights = []                                            # V_j, the backward pass's roundings
        for k, part in enumerate(parts, 1):
            cur = sosfilt(table[part], cur, np.float64, zi=zi[part][:, :, None]*ref[None, None, :])
            h_k, s_k = (h_all, s_all) if k == P else _responses(table[:part.stop], N)
            earlier = _conv(h_k, d) + s_k[:, None]*d[0][None, :] + \
                sum((_conv(between(j, k), weights[j - 1]) for j in range(1, k)), np.zeros_like(cur))
            if k < P:
                weights.append(rounding(cur, earlier))
        return earlier[::-1][edge:edge + T]
    return _cached(_key(sos, x, 'handover', tuple(split), bool(rectify), float(gain)), make)


def multi_term(sos, split, x, gain=GAIN, rectify=True):
    """The whole per-sample allowance of a hipdsp_envelope_multi run on top of the window bound: handover_term, and for a
    cascade with a high-pass extension_term on both sides (odd_ext_kernel forms both extensions in float32).  A low-pass
    cascade takes no extension term: the calibration (test_iir_bound.py) shows the model inside the bound without."""
    term = handover_term(sos, split, x, gain, rectify)
    if has_highpass(sos):
        term = term + extension_term(sos, x, gain, rectify, left=True)
    return term
