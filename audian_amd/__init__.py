"""audian_amd -- MI355X-native (gfx950) implementation of audian's BufferedData DSP
hot path: Butterworth SOS band-pass (BufferedFilter), rectified zero-phase envelope
(BufferedEnvelope) and Hann STFT power spectrogram + dB (BufferedSpectrogram),
as hand-written HIP kernels behind the C ABI of ``include/hip_dsp.h``.

Importing this package does not touch the GPU; ``audian_amd.hipdsp`` (and anything
that computes) loads ``libhip_dsp.so`` and fails loudly if it is missing.
"""

__version__ = '0.1.0'

# names resolved on first use, so that importing the package stays free of side effects
_EXPORTS = {'NoiseProfile': 'noiseprofile', 'host_bin_quantiles': 'noiseprofile', 'host_equalize': 'noiseprofile',
            'BufferedEqualizedSpectrogram': 'bufferedequalizedspectrogram',
            'BufferedAdaptiveSpectrogram': 'bufferedadaptivespectrogram', 'host_adapt': 'bufferedadaptivespectrogram',
            'smooth_for': 'bufferedadaptivespectrogram'}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        from importlib import import_module
        return getattr(import_module('.' + _EXPORTS[name], __name__), name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
