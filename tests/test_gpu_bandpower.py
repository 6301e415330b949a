"""hipdsp_band_power and BufferedBandPower on the GPU.  The comparator is numpy in float64 -- on random slabs, on the
slab the device itself produced (the kernel's 1-ulp contract), and on the CPU checker's float64 spectrogram (end to
end, under the per-bin bound of tests/spectral_bound.py) -- never the code under test."""

import ctypes

import numpy as np
import pytest

import gpu_helpers as gh
import spectral_bound as sb
from conftest import rel_err

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.5)          # no band power of non-negative bins is negative


def slab_random(rng, C, frames, F):
    """Non-negative float32 spanning 1e-12 ... 1e6 within every row."""
    u = rng.random((C, frames, F), dtype=np.float32)
    return np.power(np.float32(10.0), np.float32(18.0)*u - np.float32(12.0)).astype(np.float32)


def want_f32(spec, bands, scale):
    """float32(scale * sum in float64) per band: (nb, C, frames).  numpy's pairwise float64 sum is within 2^-40 of
    exact, far inside the contract."""
    out = np.empty((len(bands),) + spec.shape[:2], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for b, (k0, k1) in enumerate(bands):
            out[b] = (scale*np.sum(spec[:, :, k0:k1], axis=2, dtype=np.float64)).astype(np.float32)
    return out


def assert_one_ulp(got, want, what):
    got64, want64 = got.astype(np.float64), want.astype(np.float64)
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got64), nan), what
    inf = np.isinf(want64)
    assert np.array_equal(got64[inf], want64[inf]), what
    ok = ~(nan | inf)
    err = np.abs(got64[ok] - want64[ok])
    tol = np.spacing(np.abs(want[ok])).astype(np.float64)
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, '%s: %d of %d beyond 1 ulp, first got %r want %r' % (
        what, bad.size, err.size, got64[ok][bad[0]], want64[ok][bad[0]])


def run(spec, bands, scale, db=False, ref_power=1.0, min_power=1e-20, strided=False):
    """hipdsp_band_power on a host slab (C, frames, F): returns (nb, C, frames) float32.  The output block is filled
    with a sentinel first: every value must be written and nothing else touched.  strided: odd base offsets and
    non-compact spec_pitch, out_pitch, out_band_pitch."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, frames, F = spec.shape
    nb = len(bands)
    s_off, s_pitch = (3, frames*F + 7) if strided else (0, frames*F)
    o_off, o_pitch = (5, frames + 5) if strided else (0, frames)
    o_band = C*o_pitch + (11 if strided else 0)
    host = np.zeros(s_off + C*s_pitch, dtype=np.float32)
    for ch in range(C):
        host[s_off + ch*s_pitch:s_off + ch*s_pitch + frames*F] = spec[ch].ravel()
    dspec = hipdsp.DeviceArray.from_host(c, host)
    n_out = o_off + nb*o_band + 3
    dout = hipdsp.DeviceArray.from_host(c, np.full(n_out, SENTINEL, dtype=np.float32))
    hipdsp.band_power(c, dspec.view(s_off, (1,)), s_pitch if strided else 0, C, frames, F, bands, scale,
                      dout.view(o_off, (1,)), db=db, ref_power=ref_power, min_power=min_power,
                      out_pitch=o_pitch if strided else 0, out_band_pitch=o_band if strided else 0)
    flat = dout.to_host()
    dspec.free()
    dout.free()
    written = np.zeros(n_out, dtype=bool)
    out = np.empty((nb, C, frames), dtype=np.float32)
    for b in range(nb):
        for ch in range(C):
            a = o_off + b*o_band + ch*o_pitch
            out[b, ch] = flat[a:a + frames]
            written[a:a + frames] = True
    assert np.all(flat[~written] == SENTINEL), 'written outside the rows'
    assert not np.any(out == SENTINEL), 'values left unwritten'
    return out


def band_kinds(F):
    """name -> list of bands (one call each): every kind of the contract that fits into F bins."""
    kinds = {'one bin': [(F//2, F//2 + 1)], 'first bin': [(0, 1)], 'last bin': [(F - 1, F)], 'full': [(0, F)],
             'top 1/16': [(F - max(F//16, 1), F)], 'empty': [(F//3, F//3)], 'empty at F': [(F, F)]}
    for w in (63, 64, 65):
        for start in (1, 77):
            if start + w <= F:
                kinds['width %d at %d' % (w, start)] = [(start, start + w)]
    kinds['overlapping pair'] = [(F//4, F//2 + 1), (F//3, min(F, F//2 + F//4 + 1))]
    kinds['nested pair'] = [(0, F), (F//3, F//3 + max(1, F//5))]
    rng = np.random.default_rng(F)
    sixteen = [(0, F), (F//2, F//2), (F - 1, F), (1, min(F, 65))]
    while len(sixteen) < 16:
        k0 = int(rng.integers(0, F))
        sixteen.append((k0, int(rng.integers(k0, F + 1))))
    kinds['16 bands'] = sixteen
    kinds['4 disjoint'] = [(j*F//4 + 1, j*F//4 + 1 + max(1, F//9)) for j in range(4)]
    return kinds


# nfreq of all three mappings (<= 256: lanes along time; < 8192: a wave per row; beyond: a workgroup per row); every frame
# count and channel count of the contract at least once; the largest slab is 64 x 1000 x 1025 (262 MB)
SLABS = [(5, 100003, 3), (5, 1, 1), (129, 100000, 1), (129, 65, 64), (513, 1000, 3), (513, 63, 1), (1025, 1000, 64),
         (1025, 64, 3), (4097, 65, 3), (4097, 1000, 1), (32769, 63, 3), (32769, 1, 1), (262145, 64, 1), (262145, 1, 3)]


@pytest.mark.parametrize('F, frames, C', SLABS)
def test_kernel_is_within_one_ulp_on_random_slabs(F, frames, C):
    rng = np.random.default_rng([F, frames, C])
    spec = slab_random(rng, C, frames, F)
    scale = 46.875
    strided = frames <= 1000 and C <= 3            # the padded layout for the slabs that are cheap to re-pack
    for name, bands in band_kinds(F).items():
        got = run(spec, bands, scale, strided=strided)
        assert_one_ulp(got, want_f32(spec, bands, scale), 'F %d frames %d C %d %s' % (F, frames, C, name))
        for b, (k0, k1) in enumerate(bands):
            if k0 == k1:
                assert np.all(got[b] == 0)


@pytest.mark.parametrize('F, frames, C', [(129, 300, 3), (1025, 65, 3), (8193, 9, 1)])
def test_strided_and_compact_layouts_agree(F, frames, C):
    rng = np.random.default_rng(F)
    spec = slab_random(rng, C, frames, F)
    for name, bands in band_kinds(F).items():
        a = run(spec, bands, 2.0, strided=False)
        b = run(spec, bands, 2.0, strided=True)
        assert np.array_equal(a, b), name


@pytest.mark.parametrize('nfft, hop, C', [(256, 128, 3), (1024, 512, 3), (16384, 8192, 1)])
def test_kernel_on_real_spectrogram_output(nfft, hop, C):
    """The slab hipdsp_spectrogram wrote (tones over noise, zero tail frames), summed on the device where it lies."""
    from audian_amd import hipdsp
    c = gh.ctx()
    rate, F = 96000.0, nfft//2 + 1
    T = 40*hop + nfft
    nd = 45                                           # the last frames do not fit: zero
    dx = hipdsp.DeviceArray(c, (C, T), np.float32)
    hipdsp.synth(c, dx, T, C, T, rate, 7)
    ds = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
    hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, rate, ds, nd)
    spec = ds.to_host()
    assert np.all(spec[:, -1] == 0) and np.all(spec[:, 0].max(axis=1) > 0)
    fres = rate/nfft
    for name, bands in band_kinds(F).items():
        out = hipdsp.DeviceArray.from_host(c, np.full((len(bands), C, nd), SENTINEL, dtype=np.float32))
        hipdsp.band_power(c, ds, 0, C, nd, F, bands, fres, out)
        got = out.to_host()
        assert not np.any(got == SENTINEL)
        assert_one_ulp(got, want_f32(spec, bands, fres), 'nfft %d %s' % (nfft, name))
        assert np.all(got[:, :, -1] == 0)


@pytest.mark.parametrize('F, frames, C', [(129, 700, 3), (1025, 200, 3), (32769, 5, 1)])
def test_db_is_bit_identical_to_decibel_of_the_linear_result(F, frames, C):
    from audian_amd import hipdsp
    c = gh.ctx()
    rng = np.random.default_rng(F + 1)
    spec = slab_random(rng, C, frames, F)
    bands = [(F//2, F//2 + 1), (0, F), (F//3, F//3), (1, min(F, 66))]
    for ref_power, min_power, scale in [(1.0, 1e-20, 1.0), (2.5, 1e-7, 1e-3), (1e-6, 3.0, 46.875)]:
        lin = run(spec, bands, scale)
        db = run(spec, bands, scale, db=True, ref_power=ref_power, min_power=min_power, strided=True)
        dlin = hipdsp.DeviceArray.from_host(c, lin)
        ddb = hipdsp.DeviceArray(c, lin.shape, np.float32)
        hipdsp.decibel(c, dlin, ddb, lin.size, ref_power, min_power)
        want = ddb.to_host()
        assert np.array_equal(db.view(np.uint32), want.view(np.uint32))
        assert np.all(np.isneginf(db[2]))                              # the empty band
        assert np.any(np.isneginf(db[0])) == bool(np.any(lin[0] <= np.float32(min_power)))


@pytest.mark.parametrize('F, frames, C', [(129, 400, 2), (1025, 70, 2), (32769, 6, 1)])
def test_nan_and_inf_reach_their_own_frame_only(F, frames, C):
    rng = np.random.default_rng(F + 2)
    spec = slab_random(rng, C, frames, F)
    bands = [(F//4, F//2), (0, F), (F//2, F)]
    clean = run(spec, bands, 1.0)
    t_nan, t_inf, t_out = frames//3, frames//2, frames - 1
    spec[0, t_nan, F//4] = np.nan                   # first bin of band 0
    spec[C - 1, t_inf, F//2 - 1] = np.inf           # last bin of band 0
    spec[0, t_out, F - 1] = np.nan                  # outside band 0, inside the others
    got = run(spec, bands, 1.0)
    assert np.isnan(got[0, 0, t_nan]) and np.isnan(got[1, 0, t_nan]) and not np.isnan(got[2, 0, t_nan])
    assert np.isposinf(got[0, C - 1, t_inf]) and np.isposinf(got[1, C - 1, t_inf]) and np.isfinite(got[2, C - 1, t_inf])
    assert np.isfinite(got[0, 0, t_out]) and np.isnan(got[1, 0, t_out]) and np.isnan(got[2, 0, t_out])
    touched = np.zeros(got.shape, dtype=bool)
    touched[:, 0, t_nan] = touched[:, C - 1, t_inf] = touched[:, 0, t_out] = True
    assert np.array_equal(got[~touched], clean[~touched])           # every neighbour bit for bit as before
    assert_one_ulp(got, want_f32(spec, bands, 1.0), 'non-finite input')


def test_argument_errors():
    from audian_amd import hipdsp, _lib
    c = gh.ctx()
    C, frames, F = 2, 10, 33
    ds = hipdsp.DeviceArray.from_host(c, np.ones((C, frames, F), dtype=np.float32))
    out = hipdsp.DeviceArray.from_host(c, np.full((17, C, frames), SENTINEL, dtype=np.float32))

    def call(k0s, k1s, n=None, channels=C, nframes=frames, spec=ds, dst=out, spec_pitch=0, out_pitch=0):
        n = len(k0s) if n is None else n
        a0 = (ctypes.c_int64*max(1, len(k0s)))(*k0s)
        a1 = (ctypes.c_int64*max(1, len(k1s)))(*k1s)
        return _lib.lib.hipdsp_band_power(c.handle, hipdsp._p(spec), spec_pitch, channels, nframes, F, a0, a1, n, 1.0, 0,
                                          1.0, 1e-20, hipdsp._p(dst), out_pitch, 0)

    for k0s, k1s in [([-1], [3]), ([5], [4]), ([0], [F + 1]), ([0, 7], [F, 6])]:
        assert call(k0s, k1s) == _lib.ERR_INVALID
        assert 'band' in _lib.last_error()
    assert call([], [], n=0) == _lib.ERR_INVALID and _lib.last_error()
    assert call([0], [F], spec_pitch=frames*F - 1) == _lib.ERR_INVALID and 'spec_pitch' in _lib.last_error()
    assert call([0], [F], out_pitch=frames - 1) == _lib.ERR_INVALID and 'out_pitch' in _lib.last_error()
    assert call([0], [F], spec=None) == _lib.ERR_INVALID and _lib.last_error()
    assert call([0]*17, [F]*17) == _lib.ERR_UNSUPPORTED and '16' in _lib.last_error()
    with pytest.raises(NotImplementedError):
        hipdsp.band_power(c, ds, 0, C, frames, F, [(0, F)]*17, 1.0, out)
    with pytest.raises(ValueError):
        hipdsp.band_power(c, ds, 0, C, frames, F, [(3, 2)], 1.0, out)
    assert np.all(out.to_host() == SENTINEL)                         # none of these wrote anything
    assert call([0], [F], nframes=0) == _lib.OK and call([0], [F], channels=0) == _lib.OK
    assert np.all(out.to_host() == SENTINEL)
    assert call([0]*16, [F]*16) == _lib.OK
    got = out.to_host()
    assert np.all(got[:16] == np.float32(F)) and np.all(got[16] == SENTINEL)


# ---- end to end against the float64 checker ---------------------------------------------------------------------

RATE = 48000.0


def band_bound(want_psd, bands, nfft, fres, direct):
    """What the per-bin bound of spectral_bound.py allows a band sum: with a_k = sqrt(P_ref[k]), r the rms of a over
    the frame's bins, delta_k = beta_max*EPS*(a_k + floor_growth*r), a spectrogram inside its bound has
    |P^_k - P_k| <= 2 a_k delta_k + delta_k^2 in every bin; the float32 result of the sum adds 2^-23 of it."""
    a = np.sqrt(want_psd)
    r = np.sqrt(np.mean(a*a, axis=-1, keepdims=True))
    delta = sb.beta_max(nfft)*sb.EPS*(a + sb.floor_growth(nfft, direct)*r)
    per_bin = 2*a*delta + delta*delta
    want = np.stack([fres*np.sum(want_psd[..., k0:k1], axis=-1) for k0, k1 in bands])
    tol = np.stack([fres*np.sum(per_bin[..., k0:k1], axis=-1) for k0, k1 in bands]) + 2.0**-23*want
    return want, tol


def check_end_to_end(oracle, name, nfft, hop, frames, direct=False):
    from audian_amd import hipdsp
    c = gh.ctx()
    F, fres = nfft//2 + 1, RATE/nfft
    x = sb.family(name, (frames - 1)*hop + nfft, nfft, RATE, seed=nfft + hop)
    T, C = x.shape
    nd = frames + 1                                                    # one frame past the input: zero
    dx = gh.to_planar(c, x)
    ds = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
    hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, RATE, ds, nd)
    ref = np.zeros((nd, C, F))
    oracle.spectrogram_process(x.astype(np.float64), ref, RATE, nfft, hop)
    ref = ref.transpose(1, 0, 2)
    w = min(64, F)
    quiet = int(np.argmin(np.convolve(ref[0, 0], np.ones(max(1, F//16)), 'valid')))
    bands = [(0, F), (F - max(F//16, 1), F), (min(3, F - w), min(3, F - w) + w), (F//3, F//3 + 1),
             (quiet, quiet + max(1, F//16)), (F//2, F//2)]
    out = hipdsp.DeviceArray(c, (len(bands), C, nd), np.float32)
    hipdsp.band_power(c, ds, 0, C, nd, F, bands, fres, out)
    got = out.to_host().astype(np.float64)
    want, tol = band_bound(ref, bands, nfft, fres, direct)
    over = np.abs(got - want) > tol
    worst = np.unravel_index(int(np.argmax(np.abs(got - want) - tol)), got.shape)
    assert not np.any(over), 'nfft %d hop %d family %s: band %s channel %d frame %d: got %r want %r allowed %r' % (
        nfft, hop, name, bands[worst[0]], worst[1], worst[2], got[worst], want[worst], tol[worst])
    assert np.all(got[:, :, frames] == 0) and np.all(got[len(bands) - 1] == 0)


@pytest.mark.parametrize('nfft', [2**k for k in range(3, 20)])
def test_end_to_end_power_of_two_windows(oracle, nfft):
    names = sb.FAMILIES if nfft <= 65536 else ('tones', 'edges', 'offset')
    for name in names:
        check_end_to_end(oracle, name, nfft, nfft//2, 3 if nfft <= 16384 else 2)


@pytest.mark.parametrize('nfft', [24, 1000, 3000, 12000])
def test_end_to_end_direct_dft_windows(oracle, nfft):
    names = sb.FAMILIES if nfft <= 3000 else ('tones', 'edges')
    for i, name in enumerate(names):
        check_end_to_end(oracle, name, nfft, nfft//2 + (i % 2), 2 if nfft <= 3000 else 1, direct=True)


# ---- the facade ---------------------------------------------------------------------------------------------------

class Item:
    def isVisible(self):
        return True


def recording(rate, seconds, channels, seed=11):
    rng = np.random.default_rng(seed)
    n = int(rate*seconds)
    t = np.arange(n)/rate
    x = rng.uniform(-1, 1, size=(n, channels))
    for ch in range(channels):
        x[:, ch] = 0.5*x[:, ch] + 0.5*np.sin(2*np.pi*(700.0 + 300*ch)*t)*(1 + np.sin(2*np.pi*3*t))/2
    return x.astype(np.float32).astype(np.float64)


def graph_of(F, S, E, B, x, rate, buffer_time, back_time, nfft, **band):
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(buffer_time, back_time)
    for t in (F(), S(nfft=nfft), B(**band), E(envelope_cutoff=200.0)):
        g.add_trace(t)
    g.setup_traces()
    g.open(x, rate)
    for t in g.traces:
        t.plot_items = [Item() for _ in range(t.channels)]
    g.set_need_update()
    return g


def test_facade_walk_against_checker_twins(oracle, monkeypatch):
    """filter -> spectrogram -> band power with device mirrors, driven like the browser drives it, against twins that
    compute with the CPU checker and the host formula; what a move of the band costs is counted."""
    from audian_amd import hipdsp, bufferedfilter
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedbandpower import BufferedBandPower
    from test_gpu_facade import oracle_twins
    OF, OE, OS = oracle_twins(oracle)

    class HostBand(BufferedBandPower):
        def process(self, source, dest, nbefore):
            self._pending = None
            n = len(dest)
            p = self.scale*np.sum(np.asarray(source[nbefore:nbefore + n], dtype=np.float64)[:, :, self.k0:self.k1], axis=2)
            with np.errstate(divide='ignore'):
                dest[...] = np.where(p > self.min_power, 10*np.log10(np.maximum(p, 1e-300)), -np.inf) if self.log else p

    rate = 16000.0
    x = recording(rate, 90.0, 2)
    g = graph_of(BufferedFilter, BufferedSpectrogram, BufferedEnvelope, BufferedBandPower, x, rate, 4.0, 1.0, 512,
                 fmin=500.0, fmax=2500.0)
    o = graph_of(OF, OS, OE, HostBand, x, rate, 4.0, 1.0, 512, fmin=500.0, fmax=2500.0)
    assert [t.name for t in g.traces[1:]] == ['filtered', 'spectrogram', 'bandpower', 'envelope']
    for twin in (g, o):
        twin['filtered'].highpass_cutoff, twin['filtered'].lowpass_cutoff = 300.0, 3000.0
        twin['filtered'].update()

    counts = {}
    for name in ('spectrogram', 'chain_forward', 'unpack_spectrum', 'pack', 'band_power'):
        real = getattr(hipdsp, name)
        counts[name] = 0

        def wrapped(*a, _real=real, _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(hipdsp, name, wrapped)

    calls = []
    real_process = BufferedBandPower.process

    def counted_process(self, source, dest, nbefore):
        calls.append(len(dest))
        return real_process(self, source, dest, nbefore)
    monkeypatch.setattr(BufferedBandPower, 'process', counted_process)

    def compare(read_spectrogram=True):
        a, b, s = g['bandpower'], o['bandpower'], g['spectrogram']
        assert (a.offset, a.rate, a.frames, a.shape) == (b.offset, b.rate, b.frames, b.shape)
        assert (a.offset, a.rate, a.frames, len(a.buffer)) == (s.offset, s.rate, s.frames, len(s.buffer))
        assert (a.k0, a.k1, a.scale, a.unit) == (b.k0, b.k1, b.scale, b.unit)
        got, want = np.array(a.buffer), np.array(b.buffer)
        assert got.shape == want.shape
        if a.log:
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), fin)
            got, want = np.where(fin, 10**(got/10), 0.0), np.where(fin, 10**(want/10), 0.0)
        for ch in range(a.channels):
            assert rel_err(got[:, ch], want[:, ch]) < 1e-4, ch       # the project's parity metric, per channel
        if read_spectrogram and not a.log:
            # and to the ulp against the same formula on the device's own spectrogram (bookkeeping: offsets, bins)
            own = a.scale*np.sum(np.array(s.buffer)[:, :, a.k0:a.k1], axis=2)
            assert_one_ulp(got.astype(np.float32), own.astype(np.float32), 'own spectrogram')

    # the raw buffer holds 25 s: it moves once the window (plus the margins) leaves it; small steps forward then keep most
    # of every derived buffer and load the rest (doffset > 0), jumps load everything
    for t0, t1 in [(0.0, 2.0), (1.0, 3.0), (14.0, 17.0), (29.0, 31.0), (30.0, 32.0), (31.5, 33.5), (88.0, 90.0), (86.5, 88.0)]:
        g.update_times(t0, t1)
        o.update_times(t0, t1)
        compare()
    # every load went through the kernel (no host fallback), whole buffers and partial loads
    assert counts['band_power'] == len(calls) and all(n > 0 for n in calls)
    assert len(calls) >= 5 and min(calls) < 100 < max(calls)
    # scrolls with nothing read in between: partial loads into a recycled mirror, what is stale travels with it
    before = len(calls)
    for t0, t1 in [(50.0, 52.0), (51.0, 53.0), (52.5, 55.0), (56.0, 57.0)]:
        g.update_times(t0, t1)
        o.update_times(t0, t1)
    assert g['bandpower']._stale and g['spectrogram']._stale
    assert counts['band_power'] == len(calls) == before + 4 and max(calls[before + 1:]) < len(g['bandpower'].buffer)
    compare(read_spectrogram=False)
    # the whole graph recomputed by the filter, once through the fused launch (its spectrogram only marks its mirror)
    monkeypatch.setattr(bufferedfilter, 'FUSION_MARGIN', 100.0)
    before = dict(counts)
    for twin in (g, o):
        twin['filtered'].highpass_cutoff = 400.0
        twin['filtered'].update()
    assert counts['chain_forward'] == before['chain_forward'] + 1 and counts['spectrogram'] == before['spectrogram']
    assert counts['band_power'] == before['band_power'] + 1
    compare(read_spectrogram=False)
    # moving the band: exactly one launch, no spectrogram work, no spectrogram frame read back
    s, a = g['spectrogram'], g['bandpower']
    assert s._stale
    for fmin, fmax in [(1000.0, 1200.0), (0.0, None), (1010.0, 1020.0), (2000.0, 1000.0), (700.0, 3900.0)]:
        stale, before = [list(r) for r in s._stale], dict(counts)
        a.set_band(fmin, fmax)
        o['bandpower'].set_band(fmin, fmax)
        after = dict(counts)
        assert after['band_power'] == before['band_power'] + 1
        assert all(after[k] == before[k] for k in ('spectrogram', 'chain_forward', 'unpack_spectrum', 'pack'))
        assert s._stale == stale
        compare(read_spectrogram=False)
        assert all(counts[k] == before[k] for k in ('spectrogram', 'chain_forward', 'unpack_spectrum', 'pack'))
    # screen decimation of the result: an ordinary 2-D trace
    i0, i1 = a.offset + 3, a.offset + len(a.buffer) - 2
    mm = a.minmax_decimate(i0, i1, 7, channel=1)
    col = np.array(a.buffer)[3:len(a.buffer) - 2, 1]
    seg = np.arange(0, len(col), 7)
    assert np.array_equal(mm[0::2], np.minimum.reduceat(col, seg)) and np.array_equal(mm[1::2], np.maximum.reduceat(col, seg))
    compare()
    # dB, and back
    before = dict(counts)
    a.update(log=True)
    o['bandpower'].update(log=True)
    assert counts['band_power'] == before['band_power'] + 1 and counts['spectrogram'] == before['spectrogram']
    assert a.unit == 'dB' and abs(a.ampl_min + 200.0) < 1e-9 and a.ampl_max == 0.0
    compare()
    for t0, t1 in [(41.0, 43.0), (42.0, 44.5)]:                      # a jump and a partial load in dB
        g.update_times(t0, t1)
        o.update_times(t0, t1)
        compare()
    a.update(log=False)
    o['bandpower'].update(log=False)
    assert (a.unit, a.ampl_min, a.ampl_max) == ('a.u.^2', 0, 1.0)
    # another window: hop, rate, frames, offset and bins follow the spectrogram
    for nfft, overlap in [(1024, 0.75), (256, 0.5), (4096, 0.5)]:
        for twin in (g, o):
            twin['spectrogram'].update(nfft=nfft, overlap_frac=overlap)
        assert a.rate == rate/g['spectrogram'].hop and a.scale == rate/nfft
        compare()
        g.update_times(8.0, 10.0)
        o.update_times(8.0, 10.0)
        compare()


def test_band_powers_of_the_spectrogram(oracle):
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedenvelope import BufferedEnvelope
    from audian_amd.bufferedspectrogram import BufferedSpectrogram, band_bins
    from audian_amd.bufferedbandpower import BufferedBandPower
    rate = 16000.0
    x = recording(rate, 20.0, 3, seed=5)
    g = graph_of(BufferedFilter, BufferedSpectrogram, BufferedEnvelope, BufferedBandPower, x, rate, 4.0, 1.0, 1024)
    g['filtered'].highpass_cutoff, g['filtered'].lowpass_cutoff = 300.0, 3000.0
    g['filtered'].update()
    g.update_times(6.0, 8.0)
    s = g['spectrogram']
    n = len(s.buffer)
    assert s._stale == [[0, n]]
    bands = [(500.0, 2500.0), (0.0, None), (1000.0, 1200.0), (1000.0, 1000.0), (3000.0, 2000.0), (900.0, 4000.0),
             (7000.0, 1e9)] + [(100.0*j, 100.0*j + 450.0) for j in range(12)]          # 19: two launches
    i0, i1 = s.offset + 2, s.offset + n - 1
    for log in (False, True):
        got = s.band_powers(bands, i0, i1, log=log)
        assert got.shape == (len(bands), 3, i1 - i0) and got.dtype == np.float32
        assert s._stale == [[0, n]]                                   # nothing of the spectrogram was read back
        for j, band in enumerate(bands):
            one = s.band_powers([band], i0, i1, log=log)
            assert np.array_equal(one[0].view(np.uint32), got[j].view(np.uint32)), band
    lin = s.band_powers(bands, i0, i1)
    host = np.array(s.buffer)                                          # now the host copy is current ...
    want = np.stack([(s.fresolution*np.sum(host[i0 - s.offset:i1 - s.offset, :, k0:k1], axis=2)).T
                     for k0, k1 in (band_bins(f0, f1, s.fresolution, 513) for f0, f1 in bands)]).astype(np.float32)
    assert_one_ulp(lin, want, 'device against the host formula')
    s._dev_valid = []                                                   # ... and without a mirror numpy serves
    fallback = s.band_powers(bands, i0, i1)
    assert np.array_equal(fallback, want)
    fdb = s.band_powers(bands, i0, i1, log=True)
    fin = want > 1e-20
    assert np.all(np.isneginf(fdb[~fin])) and np.allclose(fdb[fin], 10*np.log10(want[fin].astype(np.float64)), atol=1e-4)
    assert s.band_powers(bands, i0, i0).shape == (len(bands), 3, 0)
    with pytest.raises(IndexError):
        s.band_powers(bands, s.offset - 1, i1)
    with pytest.raises(IndexError):
        s.band_powers(bands, i0, s.offset + n + 1)


def test_graph_capture_of_spectrogram_and_band_power():
    from audian_amd import hipdsp
    rate, C, T, nfft, hop = 96000.0, 3, 96000, 1024, 512
    F, nd = nfft//2 + 1, (T + hop - 1)//hop
    ctx = hipdsp.Context(0)
    stream = ctx.create_stream()
    ctx.set_stream(stream)
    dx = hipdsp.DeviceArray(ctx, (C, T), np.float32)
    hipdsp.synth(ctx, dx, T, C, T, rate, 3)
    ds = hipdsp.DeviceArray(ctx, (C, nd, F), np.float32)
    bands = [(40, 60), (0, F), (50, 51)]
    out = hipdsp.DeviceArray(ctx, (len(bands), C, nd), np.float32)

    def chain():
        hipdsp.spectrogram(ctx, dx, T, C, T, nfft, hop, rate, ds, nd)
        hipdsp.band_power(ctx, ds, 0, C, nd, F, bands, rate/nfft, out)

    chain()
    ctx.synchronize()
    ctx.graph_begin()
    chain()
    graph = ctx.graph_end()
    seen = []
    for seed in (11, 12):
        hipdsp.synth(ctx, dx, T, C, T, rate, seed)
        out.zero_()
        ctx.graph_launch(graph)
        ctx.synchronize()
        got = out.to_host()
        assert_one_ulp(got, want_f32(ds.to_host(), bands, rate/nfft), 'replay %d' % seed)
        assert np.all(got[1, :, :nd - 2] > 0)
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])                        # the result followed the input
    ctx.graph_destroy(graph)
    ctx.set_stream(None)
    ctx.destroy_stream(stream)


def test_full_size_slab_once():
    """BASELINE configs[2]'s spectrogram (64 x 56 250 x 1025: 3.69 G elements, past 32-bit indices) built on the device;
    the full band and a 64-bin band; sampled rows against the host sum of the same row."""
    from audian_amd import hipdsp
    c = gh.ctx()
    rate, C, nfft, hop = 96000.0, 64, 2048, 1024
    T = int(600*rate)
    F, nd = nfft//2 + 1, (T + hop - 1)//hop
    assert (nd, F) == (56250, 1025) and C*nd*F > 2**31
    dx = hipdsp.DeviceArray(c, (C, T), np.float32)
    hipdsp.synth(c, dx, T, C, T, rate, 1)
    ds = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
    hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, rate, ds, nd)
    dx.free()
    bands = [(0, F), (333, 397)]
    out = hipdsp.DeviceArray.from_host(c, np.full((2, C, nd), SENTINEL, dtype=np.float32))
    hipdsp.band_power(c, ds, 0, C, nd, F, bands, rate/nfft, out)
    got = out.to_host()
    assert not np.any(got == SENTINEL)
    rng = np.random.default_rng(0)
    rows = []
    for ch in (0, C//2, C - 1):
        picks = {0, 1, nd - 2, nd - 1} | {int(f) for f in rng.integers(0, nd, 28)}
        rows += [(ch, f) for f in sorted(picks)]
    edge = 2**31//F                                                     # the row that holds element 2^31
    rows += [(r//nd, r % nd) for r in (edge - 1, edge, edge + 1)]
    assert (edge*F) < 2**31 < (edge + 1)*F
    for ch, f in rows:
        row = ds.view((ch*nd + f)*F, (F,)).to_host()[None, None, :]
        want = want_f32(row, bands, rate/nfft)[:, 0, 0]
        assert_one_ulp(got[:, ch, f], want, 'channel %d frame %d' % (ch, f))
        assert (f < nd - 1) == bool(got[0, ch, f] > 0)
    ds.free()
