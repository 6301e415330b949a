"""The streaming cache policies of the sweeps (sos_device.h: HD_NT_X, HD_NT_YF_ST, HD_NT_PSD, HD_NT_YF_LD, HD_NT_ENV) change
no value: the shipped library and the build with every stream on the default policy (libhip_dsp_plain.so, built next to
it by csrc/Makefile) must agree bit for bit.  A hinted access can only go wrong on addressing and on the counted waits of
the prefetches, so the shapes are the smallest that reach every path: eight tiles of 2048 samples give the prefetch loops
interior iterations on both sides of a segment border, the 777 samples behind them a border tile.

Both builds are loaded into this process through bare ctypes handles and run the same calls on their own buffers, which
are filled with 0x7f bytes first: what a build does not write differs from nothing, what it writes elsewhere does.
max_segments 3 cuts the forward sweeps (band-pass warm-up: one tile) and, with the 500 Hz envelope, the backward sweeps
of these traces into three segments of three tiles (hipdsp_sos_segments_host); max_segments 1 keeps them whole."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048
RATE = 48000.0
vp = ctypes.c_void_p


class Build:
    """One build of the library with a context of its own; device buffers as raw pointers."""

    def __init__(self, path):
        from audian_amd import _lib
        from audian_amd.design import butter_sos
        self.L = ctypes.CDLL(path)
        for name, (args, res) in _lib._SIGNATURES.items():
            fn = getattr(self.L, name)
            fn.argtypes = args
            fn.restype = res
        self.ctx = vp()
        self.ok(self.L.hipdsp_ctx_create(0, None, ctypes.byref(self.ctx)))
        self.fplan = self.plan(butter_sos(2, (300.0, 3000.0), 'bandpass', RATE))
        # the envelope's low-pass: 20 Hz, the product's (its warm-up of 26624 samples keeps these short traces in one
        # segment), and 500 Hz (2048 samples) for the runs that are to be cut into segments
        self.eplans = {hz: self.plan(butter_sos(2, hz, 'lowpass', RATE)) for hz in (20.0, 500.0)}
        self.bufs = []

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.hipdsp_last_error().decode())

    def plan(self, sos):
        h = vp()
        self.ok(self.L.hipdsp_sosplan_create(self.ctx, ctypes.byref(h)))
        tab = np.ascontiguousarray(sos, dtype=np.float64)
        self.ok(self.L.hipdsp_sosplan_set(self.ctx, h, vp(tab.ctypes.data), len(tab)))
        return h

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        p = self.new(a.size)
        self.ok(self.L.hipdsp_memcpy_h2d(self.ctx, p, vp(a.ctypes.data), a.nbytes))
        return p

    def new(self, n):
        p = vp()
        self.ok(self.L.hipdsp_malloc(self.ctx, 4*n, ctypes.byref(p)))
        self.ok(self.L.hipdsp_memset(self.ctx, p, 0x7f, 4*n))
        self.bufs.append(p)
        return p

    def down(self, p, n):
        out = np.empty(n, dtype=np.float32)
        self.ok(self.L.hipdsp_ctx_synchronize(self.ctx))
        self.ok(self.L.hipdsp_memcpy_d2h(self.ctx, vp(out.ctypes.data), p, 4*n))
        return out

    def release(self):
        self.ok(self.L.hipdsp_ctx_synchronize(self.ctx))
        for p in self.bufs:
            self.ok(self.L.hipdsp_free(self.ctx, p))
        self.bufs = []

    # ---- the entry points under test; every output comes back as a flat float32 array, pitch padding included
    def fused(self, x, T, pitch, nfft, hop, max_segments=0, spec_first=0, env_first=0, db=False):
        """hipdsp_chain_forward + hipdsp_sosfilt_envelope(phase 2): yf, env, psd (, dB)"""
        C = x.shape[0]
        L, c = self.L, self.ctx
        F = nfft//2 + 1
        nd = (T - spec_first + hop - 1)//hop
        ne = T - env_first
        epitch = ne + (pitch - T)
        self.eplan = self.eplans[500.0 if max_segments >= 3 else 20.0]
        self.ok(L.hipdsp_ctx_set_max_segments(c, max_segments))
        try:
            seg_len, n_seg = ctypes.c_int64(), ctypes.c_int()
            self.ok(L.hipdsp_chain_plan(c, self.fplan, self.eplan, C, T, ctypes.byref(seg_len), ctypes.byref(n_seg)))
            assert (n_seg.value == 1) if max_segments == 1 else (n_seg.value >= 3), (n_seg.value, max_segments)
            dx = self.up(pad_rows(x, pitch))
            yf, env, psd = self.new(C*pitch), self.new(C*epitch), self.new(C*nd*F)
            dbp = self.new(C*nd*F) if db else None
            self.ok(L.hipdsp_chain_forward(c, self.fplan, self.eplan, dx, pitch, yf, pitch, C, T, 1, np.pi/2, nfft, hop, RATE,
                                           psd, dbp, nd, 0, 0, spec_first, env_first))
            self.ok(L.hipdsp_sosfilt_envelope(c, self.fplan, self.eplan, dx, pitch, yf, pitch, env, epitch, C, T, 1, np.pi/2,
                                              1, 2, env_first))
            out = {'yf': self.down(yf, C*pitch), 'env': self.down(env, C*epitch), 'psd': self.down(psd, C*nd*F)}
            if db:
                out['db'] = self.down(dbp, C*nd*F)
            return out
        finally:
            self.ok(L.hipdsp_ctx_set_max_segments(c, 0))
            self.release()

    def separate(self, x, T, max_segments=0):
        """hipdsp_sosfilt_envelope phases 1 + 2 (sos_ckpt_kernel, env_bwd_kernel) and hipdsp_envelope of the filtered trace"""
        C = x.shape[0]
        L, c = self.L, self.ctx
        self.eplan = self.eplans[500.0 if max_segments >= 3 else 20.0]
        self.ok(L.hipdsp_ctx_set_max_segments(c, max_segments))
        try:
            dx = self.up(x)
            yf, env, env2 = self.new(C*T), self.new(C*T), self.new(C*T)
            for phase in (1, 2):
                self.ok(L.hipdsp_sosfilt_envelope(c, self.fplan, self.eplan, dx, T, yf, T, env, T, C, T, 1, np.pi/2, 1, phase, 0))
            self.ok(L.hipdsp_envelope(c, self.eplan, yf, T, env2, T, C, T, 0, 1, np.pi/2, 1))
            return {'yf': self.down(yf, C*T), 'env': self.down(env, C*T), 'envelope': self.down(env2, C*T)}
        finally:
            self.ok(L.hipdsp_ctx_set_max_segments(c, 0))
            self.release()


def pad_rows(x, pitch):
    out = np.zeros((x.shape[0], pitch), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def trace(C, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)/RATE
    x = np.stack([np.sin(2*np.pi*(700.0 + 350.0*c)*t)*(1.0 + 0.5*np.sin(2*np.pi*3.0*t)) for c in range(C)])
    return (x + 0.1*rng.standard_normal((C, T)) + 0.05).astype(np.float32)


@pytest.fixture(scope='module')
def builds():
    from audian_amd import _lib
    plain = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libhip_dsp_plain.so')
    assert os.path.exists(plain), f'{plain} is missing: build() makes it next to the shipped library'
    return Build(_lib.LIB_PATH), Build(plain)


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        ua, ub = a[k].view(np.uint32), b[k].view(np.uint32)
        assert ua.shape == ub.shape
        bad = np.flatnonzero(ua != ub)
        assert bad.size == 0, f'{what}: {k} differs in {bad.size} of {ua.size} values, first at {bad[0]}'


T8 = 8*TILE + 777


@pytest.mark.parametrize('max_segments', [1, 3])
def test_fused_sweep_unshifted_grid(builds, max_segments):
    """3 channels x (8 tiles + 777 samples) at 2048/1024, in one segment and in three."""
    x = trace(3, T8, 1)
    a, b = (B.fused(x, T8, T8, 2048, 1024, max_segments=max_segments, db=True) for B in builds)
    assert np.isfinite(a['env'][:T8]).all() and np.abs(a['psd']).max() > 0
    same_bits(a, b, f'fused sweep, max_segments {max_segments}')


@pytest.mark.parametrize('max_segments', [1, 3])
def test_fused_sweep_shifted_grid(builds, max_segments):
    """spec_first 300 puts the tile grid 724 samples in front of the trace (lead > 0), the envelope starts at sample 5000;
    every row has five floats of padding behind it."""
    x = trace(3, T8, 2)
    a, b = (B.fused(x, T8, T8 + 5, 2048, 1024, max_segments=max_segments, spec_first=300, env_first=5000) for B in builds)
    same_bits(a, b, f'fused sweep on a shifted grid, max_segments {max_segments}')


@pytest.mark.parametrize('max_segments', [1, 3])
def test_separate_launches(builds, max_segments):
    """sos_ckpt_kernel + env_bwd_kernel through both phases of hipdsp_sosfilt_envelope, and hipdsp_envelope, 2 channels x 8 tiles"""
    x = trace(2, 8*TILE, 3)
    a, b = (B.separate(x, 8*TILE, max_segments=max_segments) for B in builds)
    same_bits(a, b, f'separate launches, max_segments {max_segments}')


def test_fused_sweep_256_128(builds):
    """256-sample windows: the IIR wave keeps the stores of the filtered trace"""
    x = trace(2, T8, 4)
    a, b = (B.fused(x, T8, T8, 256, 128, db=True) for B in builds)
    same_bits(a, b, 'fused sweep 256/128')


@pytest.mark.parametrize('max_segments', [1, 3])
def test_nan_channel(builds, max_segments):
    """a NaN in the middle channel: the flood and fill paths run beside the hinted stores of its neighbours"""
    x = trace(3, T8, 5)
    x[1, 3*TILE + 100] = np.nan
    a, b = (B.fused(x, T8, T8, 2048, 1024, max_segments=max_segments, db=True) for B in builds)
    assert np.isnan(a['env'][T8:2*T8]).all() and np.isfinite(a['env'][:T8]).all() and np.isfinite(a['env'][2*T8:]).all()
    same_bits(a, b, f'NaN channel, max_segments {max_segments}')
    a, b = (B.separate(x, T8, max_segments=max_segments) for B in builds)
    same_bits(a, b, f'NaN channel, separate launches, max_segments {max_segments}')
