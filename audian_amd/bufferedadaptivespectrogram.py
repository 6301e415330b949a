"""The spectrogram normalised by a RUNNING noise floor, on the fly: a spectrogram-shaped trace whose SOURCE is a
spectrogram (or any spectrogram-shaped trace, 'equalized' included).  Per channel and bin a first-order smoother along
time follows the background -- wind and rain that come and go, a passing car, a chorus that swells over minutes, where
one fixed profile (``BufferedEqualizedSpectrogram``) is either raised by them or lies below them -- and the frame is
divided by it, reduced by it, or compressed as per-channel energy normalisation (PCEN, the front end of bioacoustic
detectors: automatic gain control by the smoother, then root compression).

Everything that takes a spectrogram by name takes this trace as it is.  ``process()`` is one ``hipdsp_spec_adapt`` call
from the source's device mirror into this trace's; on a host-only graph ``host_adapt`` computes the same values in numpy
float64.  The contract is in ``include/hip_dsp.h``."""

from math import ceil, sqrt

import numpy as np

from .buffereddata import BufferedData
from .bufferedequalizedspectrogram import BufferedFollowingSpectrogram

MODES = ('background', 'divide', 'subtract', 'pcen')


def smooth_for(time_constant, frame_rate):
    """The smoother's coefficient s = (sqrt(1 + 4 T^2) - 1)/(2 T^2), T = time_constant*frame_rate (librosa's pcen)."""
    T = float(time_constant)*float(frame_rate)
    if not (T > 0 and T < float('inf')):
        raise ValueError(f'time_constant*frame_rate must be a positive finite number, got {T}')
    return 2.0/(sqrt(1.0 + 4.0*T*T) + 1.0)          # the same number without the cancellation of small T


def check_parameters(mode, smooth, gain, bias, power, eps):
    """ValueError for what hipdsp_spec_adapt refuses: an unknown mode, smooth outside (0, 1], eps <= 0 ('divide' and
    'pcen'), gain outside [0, 1], bias < 0 or power <= 0 ('pcen'); NaN and infinities included."""
    if mode not in MODES:
        raise ValueError(f'unknown adaptive mode {mode!r}: one of {", ".join(MODES)}')
    huge = np.finfo(np.float64).max
    if not 0.0 < float(smooth) <= 1.0:
        raise ValueError(f'smooth must lie in (0, 1], got {smooth}')
    if mode in ('divide', 'pcen') and not 0.0 < float(eps) <= huge:
        raise ValueError(f'eps must be a positive finite number, got {eps}')
    if mode == 'pcen':
        if not 0.0 <= float(gain) <= 1.0:
            raise ValueError(f'gain must lie in [0, 1], got {gain}')
        if not 0.0 <= float(bias) <= huge:
            raise ValueError(f'bias must be >= 0 and finite, got {bias}')
        if not 0.0 < float(power) <= huge:
            raise ValueError(f'power must be > 0 and finite, got {power} (the logarithmic power -> 0 variant is not served)')


def host_adapt(slab, nbefore, smooth, mode, gain=0.98, bias=2.0, power=0.5, eps=1e-20):
    """hipdsp_spec_adapt on a host slab (frames, channels, nfreq), taken as float32: the rows from nbefore on of the
    slab normalised by its running floor M_0 = x_0, M_t = (1 - smooth) M_(t-1) + smooth x_t, sequentially in float64,
    rounded to float32 once."""
    check_parameters(mode, smooth, gain, bias, power, eps)
    x = np.asarray(slab, dtype=np.float32).astype(np.float64)
    nbefore = int(nbefore)
    if not 0 <= nbefore <= len(x):
        raise ValueError(f'nbefore {nbefore} not inside [0, {len(x)}]')
    s = float(smooth)
    a = 1.0 - s
    M = np.empty_like(x)
    with np.errstate(all='ignore'):
        if len(x):
            M[0] = x[0]
        for t in range(1, len(x)):
            M[t] = a*M[t - 1] + s*x[t]
        x, M = x[nbefore:], M[nbefore:]
        if mode == 'background':
            y = M
        elif mode == 'divide':
            y = x/(eps + M)
        elif mode == 'subtract':
            d = x - M
            y = np.where(d < 0, 0.0, d)
        else:
            y = np.power(x/np.power(eps + M, gain) + bias, power) - np.power(float(bias), float(power))
        return y.astype(np.float32)


class BufferedAdaptiveSpectrogram(BufferedFollowingSpectrogram):
    """The source normalised by its running noise floor M (per channel and bin, M_0 = x_0, M_t = (1 - s) M_(t-1) + s x_t
    along the frames, s = smooth_for(time_constant, frame rate)), frame by frame, shape and step of the source:
        'background'  M itself                        'divide'  x/(eps + M)          'subtract'  max(x - M, 0)
        'pcen'        (x/(eps + M)**gain + bias)**power - bias**power
    The defaults time_constant 0.4 s, gain 0.98, bias 2, power 0.5 are librosa's.  eps = 1e-20 is this project's
    `min_power`: a choice for PSD units (a floor far below any recording's noise, which keeps the spectrogram's zero tail
    frames at 0 instead of 0/0), NOT calibrated on recordings.  The unit is '' for 'pcen' and 'divide', the source's
    else.

    Warm-up.  A scroll loads strips, and a recursion that restarted at every strip would show a seam.  A strip therefore
    asks for up to ceil(warmup*time_constant*rate) source frames ahead of it (`warmup` time constants: 10 by default),
    as many as the source's buffer holds, and the recursion starts at the first of them: `lead` is what the last
    process() call got.  What remains of that start state after the lead is a^lead (a = 1 - s) of its distance to the
    floor -- e^-10 after ten time constants -- so values that stay in the buffer change by that much, not more, when a
    scroll recomputes them.  At the recording's start there is nothing ahead and M_0 = x_0 is the definition's own.
    After a jump, and after any recompute of the whole buffer in mid-recording (update(), a new window of the source),
    the buffer lies exactly over the source's: there is nothing ahead either, the lead is 0, and the recursion starts
    from M_0 = x_0 of the BUFFER's first frame, not the recording's -- the first warmup*time_constant seconds of the
    buffer (4 s at the defaults) are still settling towards the floor a longer history would give.

    update(mode=..., time_constant=..., gain=..., bias=..., power=..., eps=...) recomputes this trace and what hangs
    below it, never the source; bad values are a ValueError before anything is launched, with nothing changed."""

    def __init__(self, name='adaptive', source='spectrogram', panel='spectrogram', mode='pcen', time_constant=0.4,
                 gain=0.98, bias=2.0, power=0.5, eps=1e-20, warmup=10.0):
        BufferedFollowingSpectrogram.__init__(self, name, source, panel=panel)
        self._check(mode, time_constant, gain, bias, power, eps, warmup)
        self.mode, self.time_constant, self.warmup = mode, float(time_constant), float(warmup)
        self.gain, self.bias, self.power, self.eps = float(gain), float(bias), float(power), float(eps)
        self.lead = 0

    @staticmethod
    def _check(mode, time_constant, gain, bias, power, eps, warmup):
        if not 0.0 < float(time_constant) < float('inf'):
            raise ValueError(f'time_constant must be a positive finite number of seconds, got {time_constant}')
        if not 0.0 <= float(warmup) < float('inf'):
            raise ValueError(f'warmup must be a finite number of time constants >= 0, got {warmup}')
        check_parameters(mode, 1.0, gain, bias, power, eps)

    @property
    def smooth(self):
        return smooth_for(self.time_constant, self.rate)

    def warmup_frames(self):
        """Source frames a strip asks for ahead of it."""
        return int(ceil(self.warmup*self.time_constant*self.rate))

    def open(self, source):
        self._open_following(source)
        self._set_unit()

    def _set_unit(self):
        self.unit = '' if self.mode in ('pcen', 'divide') else self.source.unit

    def update(self, mode=None, time_constant=None, gain=None, bias=None, power=None, eps=None, warmup=None):
        new = dict(mode=self.mode, time_constant=self.time_constant, gain=self.gain, bias=self.bias, power=self.power,
                   eps=self.eps, warmup=self.warmup)
        given = dict(mode=mode, time_constant=time_constant, gain=gain, bias=bias, power=power, eps=eps, warmup=warmup)
        new.update({k: v for k, v in given.items() if v is not None})
        self._check(**new)
        self.mode = new.pop('mode')
        for k, v in new.items():
            setattr(self, k, float(v))
        self._set_unit()
        self.init = True
        self.recompute_all()

    def recompute(self):
        """Take over the source's current geometry, then allocate and compute as the base class does."""
        self._follow_geometry()
        BufferedData.recompute(self)

    def _load_geometry(self, offset, nframes):
        """The base class's slab with the warm-up ahead of it: up to warmup_frames() more source frames, as many as the
        source's buffer holds in front of the strip (the reference's /rate quirk gives this trace no lead of its own)."""
        first, count, lead = BufferedData._load_geometry(self, offset, nframes)
        extra = max(0, min(self.warmup_frames(), first))
        return first - extra, count + extra, lead + extra

    def process(self, source, dest, nbefore):
        """dest[i, c, k] = source[nbefore + i, c, k] normalised by the floor that started at source[0]."""
        n = len(dest)
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        self.lead = nbefore
        if n > 0:
            self._adapt(source, dest, nbefore, n, call)
        self._set_spec_rect()

    def _adapt(self, source, dest, nbefore, n, call):
        on_mirror = self._source_mirror(call)
        if on_mirror is not None:
            from . import hipdsp
            spec, spitch = on_mirror
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            hipdsp.spec_adapt(self.ctx, spec, spitch, ddst, dpitch, self.channels, nbefore + n, self._inner(), nbefore,
                              self.smooth, self.mode, self.gain, self.bias, self.power, self.eps)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float64
        dest[...] = host_adapt(np.asarray(source[:nbefore + n]), nbefore, self.smooth, self.mode, self.gain, self.bias,
                               self.power, self.eps)
        self._host_wrote(call)
