"""Full-trace overview on the device: hipdsp_pcm_minmax against float64 NumPy (bit-exact), its unwrap against
oracle.unwrap + oracle.minmax_decimate per block, and CompressedData on WavLoader / ArrayLoader recordings."""

import ctypes
import threading
import time
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hd():
    from audian_amd import hipdsp
    return hipdsp


@pytest.fixture(scope='module')
def ctx(hd):
    return hd.default_context()


def pcm_bytes(ints, sample_bytes):
    u = np.asarray(ints, dtype=np.int64) & ((1 << (8*sample_bytes)) - 1)
    return np.stack([(u >> (8*k)) & 0xff for k in range(sample_bytes)], axis=-1).astype(np.uint8).reshape(-1)


def write_pcm_wav(path, ints, sample_bytes, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(ints.shape[1])
        w.setsampwidth(sample_bytes)
        w.setframerate(int(rate))
        w.writeframes(pcm_bytes(ints, sample_bytes).tobytes())


def random_ints(frames, channels, sample_bytes, seed):
    lo, hi = -(1 << (8*sample_bytes - 1)), (1 << (8*sample_bytes - 1)) - 1
    rng = np.random.default_rng(seed)
    ints = rng.integers(lo, hi, size=(frames, channels), endpoint=True, dtype=np.int64)
    ints[rng.integers(0, frames), :] = lo                    # full-scale extremes
    ints[rng.integers(0, frames), :] = hi
    ints[-1, 0] = hi
    ints[0, -1] = lo
    return ints


def ref_minmax(values, step):
    seg = np.arange(0, len(values), step)
    out = np.zeros((2*len(seg), values.shape[1]))
    np.minimum.reduceat(values, seg, out=out[0::2])
    np.maximum.reduceat(values, seg, out=out[1::2])
    return out


def run_kernel(hd, ctx, ints, sample_bytes, step, scale, byte_offset=0, **kw):
    frames, channels = ints.shape
    raw = pcm_bytes(ints, sample_bytes)
    dev = hd.DeviceArray(ctx, (len(raw) + 16,), np.uint8)
    src = dev.view(byte_offset, (len(raw),))
    src.copy_from_host(raw)
    nseg = (frames + step - 1)//step
    pitch = channels + 1
    out = hd.DeviceArray(ctx, (2*nseg, pitch), np.float64)
    hd.pcm_minmax(ctx, src, sample_bytes, frames, channels, step, scale, out, pitch, **kw)
    res = out.to_host()[:, :channels]
    dev.free()
    out.free()
    return res


@pytest.mark.parametrize('sample_bytes', [2, 3, 4])
@pytest.mark.parametrize('channels', [1, 2, 3, 5, 64])
def test_kernel_bit_exact_against_float64(hd, ctx, sample_bytes, channels):
    frames = 9001 if channels < 64 else 4099
    ints = random_ints(frames, channels, sample_bytes, 10*sample_bytes + channels)
    scale = 1.0/float(1 << (8*sample_bytes - 1))
    for step in (1, 7, 512, 4096, frames + 3):
        want = ref_minmax(ints*scale, step)
        got = run_kernel(hd, ctx, ints, sample_bytes, step, scale)
        assert np.array_equal(got, want), (sample_bytes, channels, step)


@pytest.mark.parametrize('sample_bytes', [2, 4])
def test_kernel_generic_path_on_unaligned_bytes(hd, ctx, sample_bytes):
    """The same numbers from a source pointer off a 16-byte boundary, and from an odd scale (negative too)."""
    ints = random_ints(5003, 8, sample_bytes, 7)
    for off, scale in ((1, 1.0/(1 << (8*sample_bytes - 1))), (3, 0.37), (0, -1e-3)):
        want = ref_minmax(ints*scale, 33)
        assert np.array_equal(run_kernel(hd, ctx, ints, sample_bytes, 33, scale, byte_offset=off), want)


def wrapped_ints(frames, channels, sample_bytes, seed, boundaries=()):
    """A signal that leaves [-1, 1) and wraps around, quantised to the file's integers; `boundaries` get a wrap
    right there (a jump of almost full range between frame b-1 and b)."""
    bits = 8*sample_bytes - 1
    t = np.arange(frames)[:, None]
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.002, 0.01, size=channels)
    x = 1.7*np.sin(2*np.pi*f*t + rng.uniform(0, 6, size=channels)) + 0.01*rng.standard_normal((frames, channels))
    x = ((x + 1.0) % 2.0) - 1.0
    ints = np.clip(np.round(x*(1 << bits)), -(1 << bits), (1 << bits) - 1).astype(np.int64)
    for b in boundaries:
        if 0 < b < frames:
            ints[b - 1, :] = (1 << bits) - 2
            ints[b, :] = -(1 << bits) + 1
    return ints


@pytest.mark.parametrize('sample_bytes', [2, 3, 4])
@pytest.mark.parametrize('clips,down_scale', [(False, False), (True, False), (False, True), (True, True)])
def test_kernel_unwrap_bit_exact_per_block(hd, ctx, oracle, sample_bytes, clips, down_scale):
    frames, channels, step, nblock = 5*1024 + 517, 3, 64, 1024
    bounds = [64*5, 64*7 + 13, 1024, 2047, 2048, 3072 - 1]        # at a segment boundary, inside one, block edges
    ints = wrapped_ints(frames, channels, sample_bytes, sample_bytes, bounds)
    scale = 1.0/float(1 << (8*sample_bytes - 1))
    thresh = 1.5
    nblocks = 0
    for index in range(0, frames, nblock):
        blk = ints[index:index + nblock]
        x = (blk*scale).astype(np.float32)
        y = oracle.unwrap(x, thresh, 1.0, clips=clips, down_scale=down_scale)
        want = oracle.minmax_decimate(y.astype(np.float64), 0, len(blk), step)
        got = run_kernel(hd, ctx, blk, sample_bytes, step, scale, unwrap_thresh=thresh, ampl_max=1.0, clips=clips,
                         down_scale=down_scale)
        assert np.array_equal(got, want), (index, clips, down_scale)
        nblocks += 1
    assert nblocks >= 5 and frames % nblock


def test_kernel_unwrap_long_runs(hd, ctx, oracle):
    """One call whose parts and slices cross many times: the carried event count must be exact."""
    ints = wrapped_ints(200003, 2, 2, 11)
    scale = 1.0/32768
    y = oracle.unwrap((ints*scale).astype(np.float32), 1.5, 1.0, clips=False, down_scale=False)
    for step in (1, 1000, 200003):
        want = oracle.minmax_decimate(y.astype(np.float64), 0, len(y), step)
        got = run_kernel(hd, ctx, ints, 2, step, scale, unwrap_thresh=1.5, ampl_max=1.0)
        assert np.array_equal(got, want), step


def test_argument_errors_do_not_launch(hd, ctx):
    from audian_amd._lib import lib
    raw = hd.DeviceArray(ctx, (64,), np.uint8)
    out = hd.DeviceArray(ctx, (8, 4), np.float64)
    out.copy_from_host(np.full((8, 4), 7.0))
    h, rp, op = ctx.handle, ctypes.c_void_p(raw.ptr), ctypes.c_void_p(out.ptr)
    bad = [
        (h, None, 2, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 2, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, None, 4),
        (None, rp, 2, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 1, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 5, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 2, 16, 2, 0, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 2, 16, 2, -3, 1.0, 0.0, 1.0, 0, 0, op, 4),
        (h, rp, 2, 16, 2, 4, 1.0, 0.0, 1.0, 0, 0, op, 1),
    ]
    for args in bad:
        rc = lib.hipdsp_pcm_minmax(*args)
        assert rc == 1, args
        assert lib.hipdsp_last_error()
    with pytest.raises(ValueError):
        hd.pcm_minmax(ctx, raw, 2, 16, 2, 0, 1.0, out, 4)
    ctx.synchronize()
    assert np.all(out.to_host() == 7.0)
    raw.free()
    out.free()


def test_host_staging_round_trip(hd, ctx):
    buf = hd.HostBuffer(ctx, 4096 + 3)
    buf.array[:] = np.arange(len(buf.array)) % 251
    dev = hd.DeviceArray(ctx, (len(buf.array),), np.uint8)
    hd.memcpy_h2d_async(ctx, dev, buf, buf.nbytes)
    ctx.synchronize()
    assert np.array_equal(dev.to_host(), buf.array)
    dev.free()
    buf.free()


# ---- CompressedData ------------------------------------------------------------------------------

def host_overview(ints, scale, lay, unwrap=None, oracle=None):
    """The reference's workers restated on the host: every block on its own (unwrapped from zero at its first
    frame), rows at 2*index//step of a zeroed (len(times), channels) array."""
    datas = np.zeros((lay['long_rows'], ints.shape[1]))
    for index, n, row in lay['blocks']:
        v = ints[index:index + n]*scale
        if unwrap is not None:
            v = oracle.unwrap(v.astype(np.float32), unwrap[0], 1.0, clips=unwrap[1], down_scale=False)
            v = v.astype(np.float64)
        r = ref_minmax(v, lay['step'])
        datas[row:row + len(r)] = r
    return datas


def synchronous_overview(loader, lay):
    """down_sample_worker's loop run on the loader itself, one block after the other."""
    datas = np.zeros((lay['long_rows'], loader.channels))
    for index, n, row in lay['blocks']:
        buf = np.zeros((n, loader.channels))
        loader.load_buffer(index, n, buf)
        seg = np.arange(0, n, lay['step'])
        np.minimum.reduceat(buf, seg, out=datas[row:row + 2*len(seg):2])
        np.maximum.reduceat(buf, seg, out=datas[row + 1:row + 1 + 2*len(seg):2])
    return datas


def overview_threads():
    return [t for t in threading.enumerate() if t.name.startswith('overview-')]


@pytest.mark.parametrize('sample_bytes,channels,unwrap', [(2, 64, None), (3, 3, None), (4, 5, None),
                                                          (2, 2, (1.5, False)), (3, 3, (1.2, True))])
def test_compressed_wavloader_long_path(tmp_path, oracle, sample_bytes, channels, unwrap, monkeypatch):
    from audian_amd.bufferedarray import WavLoader
    from audian_amd import compresseddata as cd
    rate, frames = 100.0, 5*2992 + 1234                             # nblock 2992 at step 16: 6 blocks, the last partial
    if unwrap is None:
        ints = random_ints(frames, channels, sample_bytes, channels)
    else:
        ints = wrapped_ints(frames, channels, sample_bytes, 3, [2992, 2*2992 - 1, 16*40])
    path = tmp_path/'rec.wav'
    write_pcm_wav(path, ints, sample_bytes, rate)
    loader = WavLoader(str(path), buffer_time=10.0, back_time=0.0)
    try:
        if unwrap is not None:
            loader.set_unwrap(unwrap[0], unwrap[1], False, loader.unit)
        lay = cd.overview_layout(frames, rate, 1000)
        assert lay['step'] == 16 and lay['nblock'] == 2992 and len(lay['blocks']) == 6
        scale = 1.0/float(1 << (8*sample_bytes - 1))
        # hold the readers until is_busy() has been seen
        gate = threading.Event()
        read = cd._Source.read

        def gated(self, fd, index, n, slot):
            gate.wait(10.0)
            return read(self, fd, index, n, slot)
        monkeypatch.setattr(cd._Source, 'read', gated)
        c = cd.CompressedData(loader, cache_dir=tmp_path/'cache')
        t0 = time.perf_counter()
        c.start(1000, {})
        assert time.perf_counter() - t0 < 5.0
        assert c.is_busy() and not c.short_data
        gate.set()
        c.wait()
        assert not c.is_busy() and not overview_threads()
        want = host_overview(ints, scale, lay, unwrap, oracle)
        assert np.array_equal(c.times, lay['times'])
        assert np.array_equal(c.datas, want)
        assert np.array_equal(c.datas, synchronous_overview(loader, lay))
        # the cache next to the recording gives the same arrays back
        c.save_data_local()
        d = cd.CompressedData(loader, cache_dir=tmp_path/'cache')
        d.load_data()
        assert np.array_equal(d.datas, c.datas)
        assert np.allclose(d.times, c.times[:len(d.times)], rtol=1e-12, atol=0) and len(d.times) == len(c.times)
        d.start(1000, {})                  # found in the cache: nothing to compute
        assert not d.is_busy() and d.datas is not None
        c.close()
    finally:
        loader.close()


def test_compressed_short_path(tmp_path):
    from audian_amd.bufferedarray import WavLoader
    from audian_amd import compresseddata as cd
    rate, frames = 1000.0, 7001
    ints = random_ints(frames, 5, 2, 5)
    path = tmp_path/'short.wav'
    write_pcm_wav(path, ints, 2, rate)
    loader = WavLoader(str(path))
    try:
        assert len(loader.buffer) == frames
        c = cd.CompressedData(loader, cache_dir=tmp_path/'cache')
        c.start(1000, {})
        assert c.short_data and not c.is_busy()
        lay = cd.overview_layout(frames, rate, 1000)
        assert c.datas.shape == (1 + 2*lay['nseg'], 5) != (len(c.times), 5)
        want = ref_minmax(ints/32768.0, lay['step'])
        assert np.array_equal(c.datas[:-1], want) and np.all(c.datas[-1] == 0)
        c.save_data_local()
        assert not (tmp_path/'short-fulltrace.wav').exists()
    finally:
        loader.close()


def test_close_mid_run_joins_every_thread(tmp_path, monkeypatch):
    from audian_amd.bufferedarray import WavLoader
    from audian_amd import compresseddata as cd
    rate, frames = 100.0, 8*3000
    path = tmp_path/'rec.wav'
    write_pcm_wav(path, random_ints(frames, 4, 2, 1), 2, rate)
    loader = WavLoader(str(path), buffer_time=5.0, back_time=0.0)
    c = cd.CompressedData(loader, cache_dir=tmp_path/'cache')
    first = threading.Event()
    read = cd._Source.read

    def slow(self, fd, index, n, slot):
        first.set()
        time.sleep(0.05)
        return read(self, fd, index, n, slot)
    monkeypatch.setattr(cd._Source, 'read', slow)
    try:
        c.start(1000, {})
        assert first.wait(10.0) and c.is_busy()
        c.close()
        assert not c.is_busy() and not overview_threads()
    finally:
        loader.close()


def test_compressed_arrayloader_is_float32_rounding(tmp_path):
    from audian_amd.bufferedarray import ArrayLoader
    from audian_amd import compresseddata as cd
    rate, frames, channels = 100.0, 4*2992 + 77, 3
    x = np.random.default_rng(2).standard_normal((frames, channels))
    loader = ArrayLoader(x, rate, buffer_time=5.0, back_time=0.0)
    c = cd.CompressedData(loader)
    c.start(1000, {})
    c.wait()
    lay = cd.overview_layout(frames, rate, 1000)
    want = np.zeros((lay['long_rows'], channels))
    for index, n, row in lay['blocks']:
        r = ref_minmax(x[index:index + n], lay['step'])
        want[row:row + len(r)] = r
    assert np.array_equal(c.datas, want.astype(np.float32).astype(np.float64))
    assert np.array_equal(c.datas, synchronous_overview(loader, lay).astype(np.float32).astype(np.float64))
    c.save_data()                          # no file behind the recording: nothing to cache
    c.close()
