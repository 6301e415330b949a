"""The spectrogram equalised by a noise profile, on the fly: a second spectrogram-shaped trace whose SOURCE is the
spectrogram -- divided by the per-bin profile (a whitened image: 0 dB is the noise) or reduced by it (spectral
subtraction).

Everything that takes a spectrogram by name (``BufferedBandPower``, ``BufferedSpectralFeature``,
``BufferedTemplateMatch``, ``TraceGraph.cut_template / match_templates / detect_calls / event_contours``) takes this trace
as it is: it is a ``BufferedSpectrogram`` of its source's window, hop and frames, with the image and reduction methods of
one (the one thing a consumer must not do is take the sample rate from ``spec.source.rate``: ``spec.sample_rate`` is the
same for both spectrogram-shaped traces, and ``TraceGraph.region_contours`` was changed to read it).  ``process()`` is one ``hipdsp_spec_equalize`` launch from the spectrogram's device mirror into this trace's, and a
new profile or mode recomputes this trace and what hangs below it, never the spectrogram."""

import numpy as np

from .buffereddata import BufferedData
from .bufferedspectrogram import BufferedSpectrogram
from .noiseprofile import MODES, NoiseProfile, host_equalize


class BufferedFollowingSpectrogram(BufferedSpectrogram):
    """A spectrogram-shaped trace computed from a spectrogram-shaped SOURCE, one frame per source frame: it takes over the
    source's window, hop, frequency axis and sample rate at open() and at every recompute(), its buffer lies exactly over
    the source's, set_hop() is not its to call and the fused forward sweep never writes it.  The base of
    BufferedEqualizedSpectrogram and BufferedAdaptiveSpectrogram."""

    def __init__(self, name, source, panel='spectrogram'):
        BufferedSpectrogram.__init__(self, name, source, panel=panel)
        # window and hop are the source's from open() on (set_hop() is not this trace's to call), and a frame needs
        # nothing of its source but the same frame: none of the spectrogram's margin
        self.hop = 128
        self.source_tbefore = self.source_tafter = 0

    def _follow(self):
        """Take over the source's window, hop and frequency axis."""
        src = self.source
        self.nfft, self.hop, self.overlap_frac = src.nfft, src.hop, src.overlap_frac
        self.fresolution, self.tresolution = src.fresolution, src.tresolution
        self.frequencies = src.frequencies
        self.ampl_min, self.ampl_max = src.ampl_min, src.ampl_max

    @property
    def sample_rate(self):
        return self.source.sample_rate

    def _recording_samples(self):
        return self.source._recording_samples()

    def _open_following(self, source):
        if len(getattr(source, 'shape', ())) != 3 or not hasattr(source, 'nfft'):
            raise ValueError(f'{self.name}: the source must be a spectrogram (frames, channels, bins)')
        BufferedData.open(self, source, 1, more_shape=(int(source.shape[2]),))
        self._follow()
        self.spec_rect, self.use_spec = [], True

    def _follow_geometry(self):
        """The source's current geometry: one frame per source frame, the buffer exactly over the source's."""
        src = self.source
        self.update_step(1, more_shape=(int(src.shape[2]),))
        self.offset, self.bufferframes = src.offset, self._source_len()
        self._follow()

    def _fusable_with(self, filt):
        return None              # the fused forward sweep writes spectrograms of the filtered trace, never this one

    def set_hop(self):
        return False

    def _set_spec_rect(self):
        self.spec_rect = [self.offset/self.rate, 0, len(self._hostbuf)/self.rate,
                          getattr(self.source, 'ampl_max', 0) + self.fresolution]


class BufferedEqualizedSpectrogram(BufferedFollowingSpectrogram):
    """``source / profile`` (`mode` 'divide') or ``max(source - profile, 0)`` ('subtract') in float32, frame by frame:
    shape (frames, channels, bins) and step of the source.  `profile` is a noiseprofile.NoiseProfile
    (BufferedSpectrogram.noise_profile, TraceGraph.estimate_noise_profile); with None the trace is a copy of its source.

    A value depends only on the source's value at the same frame, channel and bin and on the profile: a scroll never
    changes a value that stays in the buffer.  The geometry follows the source as BufferedBandPower's does.  A profile
    that does not fit the source (another bin or channel count, another frequency resolution) is a ValueError from
    set_profile() and open(), before anything is launched; when a later BufferedSpectrogram.update(nfft, ...) makes the
    profile stale, the trace fills with NaN and `stale` is True until a fitting profile (or None) is set."""

    def __init__(self, name='equalized', source='spectrogram', panel='spectrogram', mode='divide', profile=None):
        BufferedFollowingSpectrogram.__init__(self, name, source, panel=panel)
        self.mode = self._checked_mode(mode)
        self.profile = self._checked(profile)
        self.stale = False
        self._dev_profile = None
        self._dev_profile_key = None

    @staticmethod
    def _checked_mode(mode):
        if mode not in MODES:
            raise ValueError(f'unknown equalisation mode {mode!r}: one of {", ".join(MODES)}')
        return mode

    @staticmethod
    def _checked(profile):
        if profile is not None and not isinstance(profile, NoiseProfile):
            raise ValueError('profile must be a noiseprofile.NoiseProfile (BufferedSpectrogram.noise_profile, '
                             'NoiseProfile.load)')
        return profile

    def _require_fit(self, profile, source):
        if profile is not None and not profile.fits(source):
            raise ValueError(f'{self.name}: the profile ({profile.channels} channels x {profile.nfreq} bins of '
                             f'{profile.fresolution!r} Hz) does not fit {source.name} ({source.channels} x '
                             f'{int(source.shape[2])} of {float(source.fresolution)!r} Hz)')

    def open(self, source):
        if len(getattr(source, 'shape', ())) == 3 and hasattr(source, 'nfft'):
            self._require_fit(self.profile, source)
        self._open_following(source)
        self._set_unit()
        self.stale = False

    def _set_unit(self):
        src = self.source
        self.unit = '' if self.mode == 'divide' and self.profile is not None else src.unit

    def set_profile(self, profile):
        """Another profile (None: none, the trace copies its source): recomputes this trace and what hangs below it,
        never the spectrogram.  ValueError, with nothing changed or launched, for one that does not fit."""
        profile = self._checked(profile)
        if self.source is not None:
            self._require_fit(profile, self.source)
        self.profile = profile
        if profile is None:
            self._drop_device_profile()
        self._set_unit()
        self.init = True
        self.recompute_all()

    def update(self, mode=None):
        """The other mode; recomputes this trace and what hangs below it, never the spectrogram."""
        if mode is not None:
            self.mode = self._checked_mode(mode)
        self._set_unit()
        self.init = True
        self.recompute_all()

    def recompute(self):
        """Take over the source's current geometry (one frame per source frame, the buffer exactly over the source's),
        see whether the profile still fits, then allocate and compute as the base class does."""
        self._follow_geometry()
        self.stale = self.profile is not None and not self.profile.fits(self)
        BufferedData.recompute(self)

    def _device_profile(self):
        """The profile's values on the device, uploaded again whenever their bytes differ from what was uploaded last (a
        new profile, or one edited in place): keyed by content, as BufferedTemplateMatch's plan is -- an object's
        identity is reused as soon as the object before is gone."""
        from . import hipdsp
        key = (self.profile.values.shape, self.profile.values.tobytes())
        if key != self._dev_profile_key:
            self._drop_device_profile()
            self._dev_profile = hipdsp.DeviceArray.from_host(self.ctx, self.profile.values)
            self._dev_profile_key = key
        return self._dev_profile

    def _drop_device_profile(self):
        """Free the device copy (after the launches that read it): with the profile gone, before another takes its place;
        a trace that goes away itself leaves it to the DeviceArray's own release."""
        if self._dev_profile is not None:
            self.ctx.synchronize()
            self._dev_profile.free()
        self._dev_profile, self._dev_profile_key = None, None

    def process(self, source, dest, nbefore):
        """dest[t, c, k] = source[nbefore + t, c, k] equalised by profile[c, k]."""
        n = len(dest)
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if n > 0:
            self._equalize(source, dest, nbefore, n, call)
        self._set_spec_rect()

    def _equalize(self, source, dest, nbefore, n, call):
        if self.stale:
            dest[...] = np.nan
            self._host_wrote(call)
            return
        on_mirror = self._source_mirror(call, nbefore)
        if on_mirror is not None:
            from . import hipdsp
            spec, spitch = on_mirror
            F = self._inner()
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            if self.profile is None:
                hipdsp.memcpy2d(self.ctx, ddst, 4*dpitch, spec, 4*spitch, 4*n*F, self.channels)
            else:
                hipdsp.spec_equalize(self.ctx, spec, spitch, ddst, dpitch, self.channels, n, F, self._device_profile(), 0,
                                     self.mode)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            return
        # no mirror to read (a plain host array, a host-only graph): numpy in float32
        slab = np.asarray(source[nbefore:nbefore + n])
        dest[...] = slab if self.profile is None else host_equalize(slab, self.profile.values, self.mode)
        self._host_wrote(call)
