"""A per-bin accuracy bound for spectrogram PSDs, and the test signals it is applied to.

The suite's parity metric (conftest.rel_err) divides a frame's largest bin error by the frame's peak, so a bin
60 dB under the peak may be entirely wrong and pass.  The display is a dB image over 60-100 dB, so every bin
matters.  Here a frame is held to what a faithful float32 transform achieves, per bin and normwise, in
amplitudes a_k = sqrt(P_ref[k]) and a^_k = sqrt(P_got[k]):

    rho  = ||a^ - a||_2 / (eps sqrt(L) ||a||_2)                   normwise, rho <= RHO_MAX
    beta = max_k |a^_k - a_k| / (eps (a_k + L r))                 per bin,  beta <= 4 L

with eps = 2^-23, L = log2(nfft), r = rms_k a_k.  A bin under the float32 floor of its frame (eps L r) is held to
that floor only, so no dB threshold needs picking.  (The floor is L r, not sqrt(L) r: see floor_growth.)  The
direct DFT (non powers of two) sums nfft fmaf terms one after another: there sqrt(L) and L become sqrt(nfft).  Frames whose reference is all zero must
be exactly zero.  tests/test_spectral_bound.py calibrates the bound on the CPU: a faithful float32 emulation
passes with margin, injected defects (twiddles, window, edge bins, detrend, a pivot carried over from an earlier frame)
fail.  FAMILIES are stationary; NONSTATIONARY move the level between frames (nonstationary()).
"""

import numpy as np

EPS = 2.0**-23
RHO_MAX = 2.0
FAMILIES = ('tones', 'bandpass', 'edges', 'offset', 'chirp', 'synth')
LEVELS = (1e-3, 1e3)


def growth(nfft, direct=False):
    """The error growth factor g: sqrt(log2 nfft) for an FFT, sqrt(nfft) for the sequential direct DFT."""
    return float(np.sqrt(nfft)) if direct else float(np.sqrt(np.log2(nfft)))


def floor_growth(nfft, direct=False):
    """The growth of the per-bin floor (relative to r): L for an FFT, sqrt(nfft) for the direct DFT.  A faithful
    float32 radix-2 FFT of a tone puts isolated spurs far above its rms error floor (eps sqrt(L) r / 5): at nfft
    2^19 beta reaches 25-34 with sqrt(L) r as the floor, under 2.5x margin to 4 L (test_spectral_bound.py)."""
    return float(np.sqrt(nfft)) if direct else float(np.log2(nfft))


def beta_max(nfft):
    return 4.0*float(np.log2(nfft))


def frame_stats(got, want, nfft, direct=False):
    """rho and beta of every frame: got, want are (..., F) PSDs (float32 / float64); returns two arrays of the
    leading shape.  All-zero reference frames give 0 when the result is all zero too, inf otherwise."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    g = growth(nfft, direct)
    gf = floor_growth(nfft, direct)
    a = np.sqrt(want)
    ah = np.sqrt(np.abs(got))*np.sign(got)                 # a negative power is an error of its own size
    d = np.abs(ah - a)
    d = np.where(np.isnan(d), np.inf, d)
    norm = np.sqrt(np.sum(a*a, axis=-1))
    r = norm/np.sqrt(a.shape[-1])
    zero = norm == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        rho = np.sqrt(np.sum(d*d, axis=-1))/(EPS*g*norm)
        beta = np.max(d/(EPS*(a + gf*r[..., None])), axis=-1)
    exact = np.all(got == 0, axis=-1)
    rho = np.where(zero, np.where(exact, 0.0, np.inf), rho)
    beta = np.where(zero, np.where(exact, 0.0, np.inf), beta)
    return rho, beta


def check_db(db_got, p_got, want, nfft, direct=False):
    """The dB image against decibel(P_ref): within the PSD bound where that bound is under a tenth of the bin
    (|ddB| <= 20 log10(1 + delta/a) + 1e-4), elsewhere no more energy than the bound allows (dB <= 20 log10(a +
    delta) + 1e-4); -inf exactly where the result's own power is at or below 1e-20, as decibel() has it.  Returns
    a list of (index, message) for the first failures (empty when the image passes)."""
    db_got = np.asarray(db_got, dtype=np.float64)
    p_got = np.asarray(p_got, dtype=np.float64)
    a = np.sqrt(np.asarray(want, dtype=np.float64))
    r = np.sqrt(np.mean(a*a, axis=-1, keepdims=True))
    delta = beta_max(nfft)*EPS*(a + floor_growth(nfft, direct)*r)
    bad = []
    inf_want = p_got <= 1e-20
    pattern = (np.isneginf(db_got) != inf_want) | np.isnan(db_got) | np.isposinf(db_got)
    for idx in zip(*np.nonzero(pattern)[:3]):
        bad.append((idx, 'dB -inf pattern: dB %r at power %r' % (db_got[idx], p_got[idx])))
        break
    fin = np.isfinite(db_got)
    close = fin & (delta <= a/10)
    with np.errstate(divide='ignore', invalid='ignore'):
        want_db = 20.0*np.log10(a)
        tol = 20.0*np.log10(1.0 + delta/a) + 1e-4
        ceiling = 20.0*np.log10(a + delta) + 1e-4
        over = close & ~(np.abs(db_got - want_db) <= tol)
    for idx in zip(*np.nonzero(over)):
        bad.append((idx, 'dB %.6f, oracle %.6f, allowed +-%.2e' % (db_got[idx], want_db[idx], tol[idx])))
        break
    loud = fin & ~close & ~(db_got <= ceiling)
    for idx in zip(*np.nonzero(loud)):
        bad.append((idx, 'dB %.6f above the ceiling %.6f (oracle %.6f)' % (db_got[idx], ceiling[idx],
                                                                            want_db[idx])))
        break
    return bad


def assert_within(got, want, nfft, what, direct=False, db=None, rho_max=RHO_MAX, b_max=None):
    """Assert the bound on (C, frames, F) / (frames, C, F) arrays laid out alike; `what` names the case (path,
    nfft, hop, family) in the message, which gives the worst frame, rho and beta.  Returns (worst rho, worst beta)."""
    b_max = beta_max(nfft) if b_max is None else b_max
    rho, beta = frame_stats(got, want, nfft, direct)
    wr = np.unravel_index(int(np.argmax(rho)), rho.shape)
    wb = np.unravel_index(int(np.argmax(beta)), beta.shape)
    msg = '%s: worst rho %.3g at frame %s (bound %g), worst beta %.3g at frame %s (bound %g)' % (
        what, rho[wr], tuple(int(i) for i in wr), rho_max, beta[wb], tuple(int(i) for i in wb), b_max)
    assert rho[wr] <= rho_max and beta[wb] <= b_max, msg
    if db is not None:
        bad = check_db(db, got, want, nfft, direct)
        assert not bad, '%s: %s' % (what, bad)
    return float(rho[wr]), float(beta[wb])


# ---- signal families: seeded, float32, (T, C) with the channels at the absolute levels LEVELS ----------------

def bandpass_noise(rng, n, rate):
    """Gaussian noise through a fourth-order Butterworth band-pass (0.3-0.35 fs): the bilinear zeros at DC and fs/2
    put the stopband far more than 100 dB down.  Filtered in float64 by the C oracle, after a warm-up that is
    discarded."""
    from audian_amd.design import butter_sos
    from oracle import oracle as orc
    sos = butter_sos(4, (0.3*rate, 0.35*rate), 'bandpass', rate)
    warm = 4096
    y = orc.sosfilt(sos, rng.standard_normal(n + warm))[warm:]
    return y/np.sqrt(np.mean(y*y))


def family(name, n, nfft, rate=48000.0, seed=0, levels=LEVELS):
    """A test signal of `n` samples for windows of `nfft`, float32 (n, len(levels)), each channel scaled to its
    level (the loudest component at about that amplitude):

    tones     a tone off bin centre at full scale, one at -80 dB, Gaussian noise at -120 dB
    bandpass  band-passed noise (stopband beyond -100 dB)
    edges     (-1)^n at -60 dB, a tone exactly on bin 1 of `nfft`, a tone off bin centre
    offset    noise and a tone under a constant offset of 1e4 times their level (the detrend path)
    chirp     a linear chirp from 0 to fs/2 over the signal, noise at -120 dB
    synth     test_gpu_parity.synth: uniform noise at 0.5 plus a tone at 0.5
    """
    rng = np.random.default_rng([seed, FAMILIES.index(name), n, nfft])
    t = np.arange(n, dtype=np.float64)
    C = len(levels)
    x = np.zeros((n, C))
    for c in range(C):
        f1 = rng.uniform(0.05, 0.45)                        # cycles per sample, off bin centre for any nfft
        ph = rng.uniform(0, 2*np.pi, size=3)
        if name == 'tones':
            f2 = rng.uniform(0.05, 0.45)
            s = np.sin(2*np.pi*f1*t + ph[0]) + 1e-4*np.sin(2*np.pi*f2*t + ph[1]) + 1e-6*rng.standard_normal(n)
        elif name == 'bandpass':
            s = 0.25*bandpass_noise(rng, n, rate)
        elif name == 'edges':
            s = (1e-3*(1.0 - 2.0*(np.arange(n) % 2)) + 0.5*np.cos(2*np.pi*t/nfft + ph[0])
                 + 0.5*np.sin(2*np.pi*f1*t + ph[1]))
        elif name == 'offset':
            s = 0.5*rng.standard_normal(n) + 0.5*np.sin(2*np.pi*f1*t + ph[0])
            s = s + 1e4*np.sign(rng.uniform(-1, 1))
        elif name == 'chirp':
            s = np.cos(np.pi*0.5*t*t/max(n - 1, 1) + ph[0]) + 1e-6*rng.standard_normal(n)
        elif name == 'synth':
            s = 0.5*rng.uniform(-1.0, 1.0, n) + 0.5*np.sin(2*np.pi*1000.0*(1 + c/C)*t/rate)
        else:
            raise ValueError(name)
        x[:, c] = levels[c]*s
    return x.astype(np.float32)


# ---- non-stationary families: the 'tones' base with an event in the level ------------------------------------

NONSTATIONARY = ('fall', 'rise', 'staircase', 'burst', 'silence', 'pulses', 'transient')
STEPS = (1e2, 1e4, 1e6)                    # S: the size of an event in units of the level (1e6: full scale / 24-bit LSB)
PLACES = ('border', 'middle', 'before')    # the event sample: a frame border, a frame's middle, one sample before a border


def event_sample(frame, nfft, hop, place):
    return {'border': frame*hop, 'middle': frame*hop + nfft//2, 'before': frame*hop - 1}[place]


def nonstationary(name, n, nfft, hop, rate=48000.0, seed=0, levels=LEVELS, S=1e4, place='border', frame=None,
                  floor=0.0):
    """A non-stationary test signal of `n` samples for windows of `nfft` every `hop`, float32 (n, len(levels)): the
    'tones' base (120 dB inside a frame) at each channel's level, with an event at the sample `place` puts into
    frame `frame` (default: the middle one of the frames that fit):

    fall       raised by S times the level until the event sample, the baseline from there
    rise       the baseline first, raised by S from the event sample
    staircase  rises and falls of different sizes (S times 1, .25, .75, .1, .5, .05 ...) every third frame (every
               frame where fewer than seven fit), the last one back to the baseline; `place` moves them all
    burst      the base times 1e6 for three hops from the event sample: 120 dB between neighbours, no offset
    silence    exact zeros over three whole frames from `frame` (one where fewer than seven fit) and over the
               last frame; with `floor`, Gaussian noise at `floor` times the level in their place (see below)
    pulses     a pulse of 1e3 levels on every frame's first sample (channel 0) / on the sample before it (channel 1)
    transient  S exp(-t/tau) times the level added from the event sample, tau two hops: a filter's transient

    `floor` is for traces that pass an IIR filter on their way to the transform.  Behind exact zeros the filter's
    output decays through every magnitude down to the smallest float32, and the frames it crosses on the way have
    reference powers under 1e-38: no float32 PSD holds them (they come out as denormals or zeros), which says
    nothing about the transform.  A floor of 1e-9 levels keeps such frames 180 dB down and representable."""
    i = NONSTATIONARY.index(name)
    rng = np.random.default_rng([seed, i + len(FAMILIES), n, nfft])
    t = np.arange(n, dtype=np.float64)
    nseg = (n - nfft)//hop + 1
    frame = nseg//2 if frame is None else frame
    e = event_sample(frame, nfft, hop, place)
    C = len(levels)
    x = np.zeros((n, C), dtype=np.float32)
    for c in range(C):
        f1, f2 = rng.uniform(0.05, 0.45, size=2)
        ph = rng.uniform(0, 2*np.pi, size=2)
        s = np.sin(2*np.pi*f1*t + ph[0]) + 1e-4*np.sin(2*np.pi*f2*t + ph[1]) + 1e-6*rng.standard_normal(n)
        if name == 'fall':
            s[:e] += S
        elif name == 'rise':
            s[e:] += S
        elif name == 'staircase':
            every = 3 if nseg >= 7 else 1
            at = [event_sample(j, nfft, hop, place) for j in range(every, nseg, every)]
            sizes = [S*(1.0, 0.25, 0.75, 0.1, 0.5, 0.05)[k % 6] for k in range(len(at))]
            sizes[-1] = 0.0
            for k, a in enumerate(at):
                s[a:at[k + 1] if k + 1 < len(at) else n] += sizes[k]
        elif name == 'burst':
            s[e:e + 3*hop] *= 1e6
        elif name == 'silence':
            nz = 3 if nseg >= 7 else 1
            for a, b in ((frame*hop, (frame + nz - 1)*hop + nfft), ((nseg - 1)*hop, n)):
                s[a:b] = floor*rng.standard_normal(max(min(b, n) - a, 0)) if floor else 0.0
        elif name == 'pulses':
            s[(0 if c % 2 == 0 else hop - 1)::hop] += 1e3
        elif name == 'transient':
            s[e:] += S*np.exp(-(t[e:] - e)/(2.0*hop))
        else:
            raise ValueError(name)
        x[:, c] = (levels[c]*s).astype(np.float32)
    return x
