"""hipdsp_spectral_features on the GPU.  The comparator is always tests/spectral_features_definition.py (np.longdouble
and the bounds derived there), never the package's numpy path: bits 0, 2, 6, 7 bit for bit, bits 1, 3, 4, 5 inside one
float32 rounding plus the float64 term, every element judged."""

import numpy as np
import pytest

import gpu_helpers as gh
import spectral_features_definition as sd

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.5)          # no feature of non-negative bins is negative


def run(spec, k0, k1, mask=sd.ALL, scale=sd.SCALE, min_power=0.0, drop_db=10.0, strided=False, nframes=None, first=0):
    """hipdsp_spectral_features on a host slab (C, frames, F): returns (n_features, C, frames) float32.  The output block
    is filled with a sentinel first: every value must be written and nothing else touched.  strided: odd base offsets
    and non-compact pitches.  first / nframes: the call sees only that frame range, as a view with the slab's pitch."""
    from audian_amd import hipdsp
    c = gh.ctx()
    C, frames, F = spec.shape
    m = frames - first if nframes is None else nframes
    nb = len(sd.bits_of(mask))
    s_off, s_pitch = (3, frames*F + 7) if strided else (0, frames*F)
    o_off, o_pitch = (5, m + 5) if strided else (0, m)
    o_feat = C*o_pitch + (11 if strided else 0)
    host = np.zeros(s_off + C*s_pitch, dtype=np.float32)
    for ch in range(C):
        host[s_off + ch*s_pitch:s_off + ch*s_pitch + frames*F] = spec[ch].ravel()
    dspec = hipdsp.DeviceArray.from_host(c, host)
    n_out = o_off + nb*o_feat + 3
    dout = hipdsp.DeviceArray.from_host(c, np.full(n_out, SENTINEL, dtype=np.float32))
    view = strided or first > 0 or m != frames
    hipdsp.spectral_features(c, dspec.view(s_off + first*F, (1,)), s_pitch if view else 0, C, m, F, k0, k1, mask, scale,
                             dout.view(o_off, (1,)), min_power=min_power, drop_db=drop_db,
                             out_pitch=o_pitch if strided else 0, out_feature_pitch=o_feat if strided else 0)
    flat = dout.to_host()
    dspec.free()
    dout.free()
    written = np.zeros(n_out, dtype=bool)
    out = np.empty((nb, C, m), dtype=np.float32)
    for b in range(nb):
        for ch in range(C):
            a = o_off + b*o_feat + ch*o_pitch
            out[b, ch] = flat[a:a + m]
            written[a:a + m] = True
    assert np.all(flat[~written] == SENTINEL), 'written outside the rows'
    assert not np.any(out == SENTINEL), 'values left unwritten'
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('F, frames, C', sd.RANDOM_SLABS)
def test_random_slabs_against_the_definition(F, frames, C):
    spec = sd.random_spec(F, frames, C)
    strided = frames <= 1000 and C <= 3            # the padded layout for the slabs that are cheap to re-pack
    for kind, (k0, k1) in sd.random_bands(F, frames, C).items():
        what = 'F %d frames %d C %d %s' % (F, frames, C, kind)
        got = run(spec, k0, k1, strided=strided)
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, 0.0, 0.1)
        sd.compare(got, V, T, sd.ALL, what)
        if k0 == k1:
            assert np.all(np.isnan(got))            # an empty band: NaN, PEAK_POWER included


def rows_of(name, C, frames):
    r = np.arange(C*frames)
    r = r[r % len(sd.FAMILIES) == sd.FAMILIES.index(name)]
    return r//frames, r % frames


@pytest.mark.parametrize('F, frames, C', sd.FAMILY_SLABS)
def test_input_families_against_the_definition(F, frames, C):
    B = {name: b for b, name in enumerate(sd.NAMES)}
    for kind, (k0, k1) in sd.family_bands(F).items():
        what = 'F %d %s' % (F, kind)
        n = k1 - k0
        spec = sd.family_slab(F, frames, C, k0, k1, 3)
        got = run(spec, k0, k1, strided=True)
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, 0.0, 0.1)
        sd.compare(got, V, T, sd.ALL, what)
        at = {name: rows_of(name, C, frames) for name in sd.FAMILIES}
        # one nonzero bin: no width, no flatness; all bins equal: the first wins, no shift
        assert np.all(got[B['bandwidth']][at['one bin']] == 0) and (n == 1 or np.all(got[B['flatness']][at['one bin']] == 0))
        eq = at['equal']
        assert np.all(got[B['peak_bin_freq']][eq] == np.float32(sd.SCALE*k0))
        assert same_bits(got[B['peak_freq']][eq], got[B['peak_bin_freq']][eq])
        want_bw = sd.SCALE*np.sqrt((n*n - 1)/12.0)
        assert np.all(np.abs(got[B['bandwidth']][eq] - want_bw) <= 2.0**-22*want_bw)
        assert np.all(np.abs(got[B['flatness']][eq] - 1) <= 2.0**-22)
        assert np.all(got[B['freq_low']][eq] == np.float32(sd.SCALE*k0))
        assert np.all(got[B['freq_high']][eq] == np.float32(sd.SCALE*(k1 - 1)))
        # plateaus: the first of the equal maxima (the formula then puts the peak half a bin towards its equal neighbour)
        mid = k0 + min(n - 1, max(n//10, 1))
        for name in ('plateau 2', 'plateau 3'):
            assert np.all(got[B['peak_bin_freq']][at[name]] == np.float32(sd.SCALE*mid)), (what, name)
            if mid + 2 <= k1 and mid > k0:
                assert np.all(got[B['peak_freq']][at[name]] == np.float32(sd.SCALE*(mid + 0.5))), (what, name)
        # the peak at the band's edges and next to a zero: no shift
        for name in ('peak at k0', 'peak at k1-1', 'zero neighbour'):
            if name != 'zero neighbour' or mid + 1 < k1:
                assert same_bits(got[B['peak_freq']][at[name]], got[B['peak_bin_freq']][at[name]]), (what, name)
        assert np.all(got[B['peak_bin_freq']][at['peak at k1-1']] == np.float32(sd.SCALE*(k1 - 1)))
        # silent rows and non-finite bins in the band: masked, the peak power as it is
        for name, power in (('zeros', 0.0), ('nan at peak', np.nan), ('inf at peak', np.inf), ('nan beside peak', np.nan)):
            rows = at[name]
            if name == 'nan beside peak' and n == 1:
                continue
            assert np.all(np.isnan(np.delete(got, 2, axis=0)[(slice(None),) + rows])), (what, name)
            p = got[2][rows]
            assert np.all(np.isnan(p)) if np.isnan(power) else np.all(p == power), (what, name)
        if n > 1:
            assert np.all(np.isposinf(got[2][at['inf elsewhere']]))
        # NaN and +inf OUTSIDE the band do not matter: the same bytes as without them
        clean = spec.copy()
        for name in ('nan outside', 'inf outside'):
            rows = at[name]
            assert np.all(np.isfinite(got[(slice(None),) + rows]))
            block = clean[rows]
            block[:, :k0] = 1.0
            block[:, k1:] = 1.0
            clean[rows] = block
        assert same_bits(run(clean, k0, k1), got), what


@pytest.mark.parametrize('F, frames, C', [(129, 70, 3), (1025, 33, 3), (4097, 9, 2), (8449, 5, 1)])
def test_layouts_masks_repeats_channels_and_views(F, frames, C):
    """Strided against compact layouts, every single-bit mask and a few others against the all-bits call, the same
    call twice, a channel alone against the same channel among others, a frame range as a view: all bit for bit."""
    spec = sd.family_slab(F, frames, C, 1, F - 1, 9)
    spec[:, ::3] = sd.random_spec(F, frames, C)[:, ::3]
    for k0, k1 in ((0, F), (1, F - 1), (F//3, F//3 + 65)):
        full = run(spec, k0, k1)
        assert same_bits(run(spec, k0, k1), full)
        assert same_bits(run(spec, k0, k1, strided=True), full)
        for mask in [1 << b for b in range(8)] + [0x07, 0x2A, 0xD5, 0xF8]:
            assert same_bits(run(spec, k0, k1, mask=mask, strided=bool(mask & 0x55)), full[sd.bits_of(mask)]), hex(mask)
        for ch in (0, C - 1):
            assert same_bits(run(spec[ch:ch + 1], k0, k1), full[:, ch:ch + 1])
        for first, m in ((0, 1), (3, frames - 4), (frames - 1, 1), (2, 0)):
            assert same_bits(run(spec, k0, k1, first=first, nframes=m), full[:, :, first:first + m])


def test_floor_and_drop():
    """min_power at, below and above a row's peak; drop_ratio 1.0 and 1e-6."""
    F, frames, C = 300, 37, 2
    spec = sd.random_spec(F, frames, C)
    k0, k1 = 20, 280
    peak = spec[:, :, k0:k1].max(axis=2).astype(np.float64)
    p = float(peak[1, 5])
    for floor in (p, np.nextafter(p, 0.0), np.nextafter(p, np.inf), 1e3):
        got = run(spec, k0, k1, min_power=floor)
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, floor, 0.1)
        sd.compare(got, V, T, sd.ALL, 'min_power %r' % floor)
        assert np.array_equal(np.isnan(got[0]), ~(peak > floor))
    assert np.isnan(run(spec, k0, k1, min_power=p)[0, 1, 5]) and not np.isnan(run(spec, k0, k1, min_power=np.nextafter(p, 0))[0, 1, 5])
    for drop_db in (0.0, 60.0):
        got = run(spec, k0, k1, drop_db=drop_db)
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, 0.0, sd.drop_ratio(drop_db))
        sd.compare(got, V, T, sd.ALL, 'drop_db %r' % drop_db)
    assert sd.drop_ratio(0.0) == 1.0 and sd.drop_ratio(60.0) == 1e-6
    got = run(spec, k0, k1, drop_db=0.0)
    assert same_bits(got[6], got[0]) and np.all(got[7] >= got[0])        # ratio 1: from the peak to the last bin equal to it


def test_refusals_leave_nothing_behind():
    from audian_amd import hipdsp, _lib
    c = gh.ctx()
    C, frames, F = 2, 10, 33
    spec = sd.random_spec(F, frames, C)
    ds = hipdsp.DeviceArray.from_host(c, spec)
    out = hipdsp.DeviceArray.from_host(c, np.full((8, C, frames), SENTINEL, dtype=np.float32))
    good = dict(spec=ds, spec_pitch=0, channels=C, nframes=frames, nfreq=F, k0=3, k1=30, features=0xFF, ratio=0.1, dst=out,
                out_pitch=0, out_feature_pitch=0, handle=c.handle)

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib.hipdsp_spectral_features(a['handle'], hipdsp._p(a['spec']), a['spec_pitch'], a['channels'],
                                                 a['nframes'], a['nfreq'], a['k0'], a['k1'], a['features'], sd.SCALE, 0.0,
                                                 a['ratio'], hipdsp._p(a['dst']), a['out_pitch'], a['out_feature_pitch'])

    assert call() == _lib.OK
    want = out.to_host()
    V, T = sd.slab_features(spec, 3, 30, sd.SCALE, 0.0, 0.1)
    sd.compare(want, V, T, sd.ALL, 'the valid call')
    refused = [(dict(handle=None), 'ctx'), (dict(spec=None), 'NULL'), (dict(dst=None), 'NULL'), (dict(channels=-1), 'negative'),
               (dict(nframes=-1), 'negative'), (dict(nfreq=-1), 'negative'), (dict(k0=-1), 'band'), (dict(k0=31), 'band'),
               (dict(k1=F + 1), 'band'), (dict(features=0), 'features'), (dict(features=0x100), 'features'),
               (dict(ratio=0.0), 'drop_ratio'), (dict(ratio=1.5), 'drop_ratio'), (dict(ratio=float('nan')), 'drop_ratio'),
               (dict(spec_pitch=frames*F - 1), 'spec_pitch'), (dict(out_pitch=frames - 1), 'out_pitch'),
               (dict(out_feature_pitch=C*frames - 1), 'out_feature_pitch'), (dict(spec_pitch=-1), 'pitch')]
    for kw, word in refused:
        out.copy_from_host(np.full((8, C, frames), SENTINEL, dtype=np.float32))
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
        assert np.all(out.to_host() == SENTINEL), kw                    # nothing was written
        assert call() == _lib.OK
        assert same_bits(out.to_host(), want), kw                       # and the next valid call gives its bytes again
    out.copy_from_host(np.full((8, C, frames), SENTINEL, dtype=np.float32))
    assert call(nframes=0) == _lib.OK and call(channels=0) == _lib.OK
    assert call(nframes=0, spec=None, dst=None) == _lib.OK
    assert np.all(out.to_host() == SENTINEL)
    for bad in (('peak',), (), 0, 256):
        with pytest.raises(ValueError):
            hipdsp.spectral_features(c, ds, 0, C, frames, F, 3, 30, bad, 1.0, out)
    with pytest.raises(ValueError):
        hipdsp.spectral_features(c, ds, 0, C, frames, F, 3, 30, ('peak_freq',), 1.0, out, drop_db=-1.0)
    assert np.all(out.to_host() == SENTINEL)


def test_graph_capture_and_replay_on_a_changed_slab():
    from audian_amd import hipdsp
    C, frames, F, k0, k1 = 3, 70, 1025, 100, 900
    ctx = hipdsp.Context(0)
    stream = ctx.create_stream()
    ctx.set_stream(stream)
    ds = hipdsp.DeviceArray.from_host(ctx, sd.random_spec(F, frames, C))
    out = hipdsp.DeviceArray(ctx, (8, C, frames), np.float32)
    before = dict(hipdsp.launches)
    hipdsp.spectral_features(ctx, ds, 0, C, frames, F, k0, k1, sd.ALL, sd.SCALE, out)
    assert hipdsp.launches['spectral_features'] == before.get('spectral_features', 0) + 1
    ctx.synchronize()
    ctx.graph_begin()
    hipdsp.spectral_features(ctx, ds, 0, C, frames, F, k0, k1, sd.ALL, sd.SCALE, out)
    graph = ctx.graph_end()
    seen = []
    for seed in (11, 12):
        spec = sd.slab_random(np.random.default_rng(seed), C, frames, F)
        ds.copy_from_host(spec)
        out.zero_()
        ctx.graph_launch(graph)
        ctx.synchronize()
        got = out.to_host()
        V, T = sd.slab_features(spec, k0, k1, sd.SCALE, 0.0, 0.1)
        sd.compare(got, V, T, sd.ALL, 'replay %d' % seed)
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])                        # the result followed the input
    ctx.graph_destroy(graph)
    ctx.set_stream(None)
    ctx.destroy_stream(stream)


def test_rows_past_element_2_to_the_31():
    """A spectrogram of 64 x 32800 x 1025 float32 (2.15 G elements) built on the device: the rows around element 2^31 and
    the slab's first and last rows, all features, against the definition -- the slab index arithmetic is 64-bit."""
    from audian_amd import hipdsp
    c = gh.ctx()
    rate, C, nfft, hop, nd = 96000.0, 64, 2048, 1024, 32800
    F, T = nfft//2 + 1, nd*hop
    assert C*nd*F > 2**31
    dx = hipdsp.DeviceArray(c, (C, T), np.float32)
    hipdsp.synth(c, dx, T, C, T, rate, 5)
    ds = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
    hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, rate, ds, nd)
    dx.free()
    edge = 2**31//F                                                     # the row that holds element 2^31
    assert edge*F < 2**31 < (edge + 1)*F
    rows = [(r//nd, r % nd) for r in (0, 1, edge - 1, edge, edge + 1, C*nd - 3, C*nd - 1)]
    k0, k1 = 10, 1000
    out = hipdsp.DeviceArray.from_host(c, np.full((8, C, nd), SENTINEL, dtype=np.float32))
    hipdsp.spectral_features(c, ds, 0, C, nd, F, k0, k1, sd.ALL, sd.SCALE, out)
    got = out.to_host()
    assert not np.any(got == SENTINEL)
    for ch, f in rows:
        row = ds.view((ch*nd + f)*F, (F,)).to_host()
        V, T_ = sd.slab_features(row[None, None, :], k0, k1, sd.SCALE, 0.0, 0.1)
        sd.compare(got[:, ch:ch + 1, f:f + 1], V, T_, sd.ALL, 'channel %d frame %d' % (ch, f))
        assert (f < nd - 1) == bool(got[0, ch, f] >= 0)                  # the zero tail frame is masked
    ds.free()
    out.free()
