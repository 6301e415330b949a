"""Full-trace overview (audian_amd.compresseddata), host side: the reference's layout arithmetic, the float64 WAV
cache files, the user-cache index and the command line.  No GPU."""

import json
import os
import struct
import wave

import numpy as np
import pytest

from audian_amd import compresseddata as cd


def ref_layout(frames, rate, max_pixel):
    """CompressedData.start's arithmetic as the reference writes it (src/audian/compresseddata.py:80-96, 31-52)."""
    step = max(1, frames//max_pixel)
    nblock = max(step, int(30.0*rate//step)*step)
    times = np.arange(0, frames + step - 1, step/2)/rate
    segments = np.arange(0, frames, step)
    rows = {}
    for index in range(0, frames, nblock):
        n = min(nblock, frames - index)
        rows[index] = (2*index//step, 2*len(np.arange(0, n, step)))
    return step, nblock, times, 1 + 2*len(segments), rows


@pytest.mark.parametrize('frames', [1, 5, 999, 1000, 1001, 44100*7 + 13, 96000*95 + 1, 48000*61])
@pytest.mark.parametrize('rate', [1000.0, 44100.0, 96000.0])
@pytest.mark.parametrize('max_pixel', [1000, 1919, 6000])
def test_layout_matches_reference_formulas(frames, rate, max_pixel):
    step, nblock, times, short_rows, rows = ref_layout(frames, rate, max_pixel)
    lay = cd.overview_layout(frames, rate, max_pixel)
    assert lay['step'] == step and lay['nblock'] == nblock
    assert np.array_equal(lay['times'], times)
    assert lay['short_rows'] == short_rows
    assert lay['long_rows'] == len(times)
    assert lay['nseg'] == (frames + step - 1)//step
    assert [(i, r) for i, _, r in lay['blocks']] == [(i, r[0]) for i, r in rows.items()]
    # every block's rows fit the long path's array, and the blocks tile the segments without a gap
    end = 0
    for index, n, row in lay['blocks']:
        assert row == end
        end = row + rows[index][1]
    assert end == 2*lay['nseg'] <= lay['long_rows']


def test_layout_grid_covers_both_row_counts_and_odd_steps():
    cases = [cd.overview_layout(f, 44100.0, 1000) for f in (999, 7*1000 + 3, 2001, 10000)]
    assert cases[0]['step'] == 1                                   # frames < max_pixel
    assert any(c['step'] % 2 == 1 for c in cases)                  # odd step
    assert any(c['short_rows'] != c['long_rows'] for c in cases)   # the two paths' row counts differ
    assert any(c['short_rows'] == c['long_rows'] for c in cases)


@pytest.mark.parametrize('channels', [1, 3, 64])
def test_f64_wav_round_trip(tmp_path, channels):
    rng = np.random.default_rng(channels)
    data = rng.standard_normal((257, channels))
    data[0, 0] = np.finfo(np.float64).max
    data[1, 0] = np.finfo(np.float64).tiny
    p = tmp_path/'x-fulltrace.wav'
    cd.write_wav_f64(p, data, 200000000.0)
    back, rate = cd.read_wav_float(p)
    assert rate == 200000000.0
    assert back.dtype == np.float64 and np.array_equal(back, data)


def test_f64_wav_against_scipy(tmp_path):
    wavfile = pytest.importorskip('scipy.io.wavfile')
    data = np.random.default_rng(1).standard_normal((100, 5))
    p = tmp_path/'ours.wav'
    cd.write_wav_f64(p, data, 12345)
    rate, theirs = wavfile.read(p)
    assert rate == 12345 and np.array_equal(theirs, data)
    q = tmp_path/'theirs.wav'
    wavfile.write(q, 4321, data)
    back, rate = cd.read_wav_float(q)
    assert rate == 4321 and np.array_equal(back, data)


def test_reads_extensible_float_wav(tmp_path):
    data = np.arange(12, dtype='<f8').reshape(6, 2)
    guid_tail = b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'
    fmt = struct.pack('<HHIIHHHHI', 0xFFFE, 2, 1000, 16000, 16, 64, 22, 64, 3) + struct.pack('<H', 3) + guid_tail
    raw = data.tobytes()
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'data' + struct.pack('<I', len(raw)) + raw
    p = tmp_path/'ext.wav'
    p.write_bytes(b'RIFF' + struct.pack('<I', len(body)) + body)
    back, rate = cd.read_wav_float(p)
    assert rate == 1000 and np.array_equal(back, data)


@pytest.mark.parametrize('step,rate', [(960, 96000.0), (7, 44100.0), (1, 48000.0), (3, 20000.0)])
def test_cache_rate_and_inference(step, rate):
    frames = 6000*step + 11
    times = cd.overview_layout(frames, rate, 6000)['times']
    assert cd.overview_layout(frames, rate, 6000)['step'] == step
    r = 1/(times[1] - times[0])
    stored = cd.cache_rate(times)
    want = r*1e6
    while want > 2**31:
        want /= 1e3
    assert stored == want and stored <= 2**31
    nrows = len(times)
    got = cd.infer_rate(float(int(round(stored))), nrows, frames, rate)
    assert abs(got - r)/r < 1e-6


class FakeWav:
    """The attributes CompressedData's cache methods read from a loader."""

    def __init__(self, path, frames=96000*120, rate=96000.0, channels=2):
        self.filepath = path
        self.file_paths = [path]
        self.frames, self.rate, self.channels = frames, rate, channels


def test_save_local_then_load(tmp_path):
    path = tmp_path/'rec.wav'
    path.write_bytes(b'')
    data = FakeWav(str(path))
    lay = cd.overview_layout(data.frames, data.rate, 6000)
    c = cd.CompressedData(data, cache_dir=tmp_path/'cache')
    c.times, c.datas, c.short_data = lay['times'], np.random.default_rng(0).standard_normal((lay['long_rows'], 2)), False
    c.save_data_local()
    assert (tmp_path/'rec-fulltrace.wav').is_file()
    d = cd.CompressedData(data, cache_dir=tmp_path/'cache')
    d.load_data()
    assert np.array_equal(d.datas, c.datas)
    assert np.allclose(d.times, np.arange(len(c.datas))*(c.times[1] - c.times[0]), rtol=1e-12, atol=0)


def test_user_cache_index(tmp_path, monkeypatch):
    cache = tmp_path/'cache'
    monkeypatch.setattr(cd.CompressedData, 'max_files', 3)
    names = []
    stamps = iter(f'2026-01-01T00:00:{s:02d}' for s in range(60))

    class Clock:
        @staticmethod
        def now():
            class T:
                @staticmethod
                def isoformat():
                    return next(stamps)
            return T

    monkeypatch.setattr(cd, 'datetime', Clock)
    for k in range(3):
        p = tmp_path/f'rec{k}.wav'
        p.write_bytes(b'')
        data = FakeWav(str(p))
        lay = cd.overview_layout(data.frames, data.rate, 6000)
        c = cd.CompressedData(data, cache_dir=cache)
        c.times, c.datas, c.short_data = lay['times'], np.full((lay['long_rows'], 2), float(k)), False
        c.save_data()
        names.append(f'{k + 1:08X}-fulltrace.wav')
    index = json.loads((cache/'fulltraces.json').read_text())
    assert sorted(index) == names
    e = index[names[0]]
    assert set(e) == {'first', 'last', 'rate', 'created', 'used'}
    assert e['first'] == e['last'] == os.fspath((tmp_path/'rec0.wav').absolute())
    assert e['rate'] == 1/(lay['times'][1] - lay['times'][0])
    # loading rec0 from the user cache refreshes its `used` stamp ...
    d = cd.CompressedData(FakeWav(str(tmp_path/'rec0.wav')), cache_dir=cache)
    d.load_data()
    assert np.all(d.datas == 0.0) and d.times[1] == 1/e['rate']
    index = json.loads((cache/'fulltraces.json').read_text())
    assert index[names[0]]['used'] > index[names[0]]['created']
    # ... so a fourth file evicts rec1, the least recently used
    p = tmp_path/'rec3.wav'
    p.write_bytes(b'')
    data = FakeWav(str(p))
    lay = cd.overview_layout(data.frames, data.rate, 6000)
    c = cd.CompressedData(data, cache_dir=cache)
    c.times, c.datas, c.short_data = lay['times'], np.full((lay['long_rows'], 2), 3.0), False
    c.save_data()
    index = json.loads((cache/'fulltraces.json').read_text())
    assert names[1] not in index and not (cache/names[1]).exists()
    assert len(index) == 3 and names[0] in index
    new = [n for n in index if index[n]['first'].endswith('rec3.wav')]
    assert new == [f'{4:08X}-fulltrace.wav']     # (named before the eviction, as the reference does)
    # an entry whose file is empty is dropped on load
    (cache/names[2]).write_bytes(b'')
    d = cd.CompressedData(FakeWav(str(tmp_path/'rec2.wav')), cache_dir=cache)
    d.load_data()
    assert d.datas is None and d.times is None
    index = json.loads((cache/'fulltraces.json').read_text())
    assert names[2] not in index


def test_short_data_saves_nothing(tmp_path):
    data = FakeWav(str(tmp_path/'r.wav'))
    c = cd.CompressedData(data, cache_dir=tmp_path/'cache')
    c.times, c.datas = np.arange(3.0), np.zeros((3, 2))
    c.save_data_local()
    c.save_data()
    assert not (tmp_path/'r-fulltrace.wav').exists() and not (tmp_path/'cache').exists()


def test_default_cache_dir_is_audians():
    platformdirs = pytest.importorskip('platformdirs')
    assert cd.default_cache_dir() == platformdirs.PlatformDirs('audian', 'janscience').user_cache_path


@pytest.mark.parametrize('argv,unwrap,clip', [
    (['f.wav'], 0.0, False),
    (['f.wav', '-u'], 1.5, False),
    (['-u', '0.8', 'f.wav'], 0.8, False),
    (['f.wav', '-U'], 1.5, True),
    (['-U', '1.2', 'f.wav'], 1.2, True),
    (['-u', '0.5', '-U', '1.1', 'f.wav'], 1.1, True),
    (['-U', '0', 'f.wav'], 0.0, False),
])
def test_cli_arguments(argv, unwrap, clip):
    args = cd.parse_args(argv)
    assert args.unwrap == unwrap and args.unwrap_clip is clip and args.files == ['f.wav']


def test_lock_takes_multiprocessing_keyword():
    lock = cd.CompressedData(None).get_lock()
    assert lock.acquire(block=False)
    assert not lock.acquire(block=False)
    lock.release()
    with lock:
        assert lock.locked()


def write_pcm_wav(path, ints, sample_bytes, rate=8000):
    ints = np.asarray(ints, dtype=np.int64)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(ints.shape[1])
        w.setsampwidth(sample_bytes)
        w.setframerate(rate)
        u = ints.astype(np.int64) & ((1 << (8*sample_bytes)) - 1)
        b = np.stack([(u >> (8*k)) & 0xff for k in range(sample_bytes)], axis=-1).astype(np.uint8)
        w.writeframes(b.tobytes())


@pytest.mark.parametrize('sample_bytes', [2, 3, 4])
def test_wavloader_exposes_file_paths_and_pcm_layout(tmp_path, sample_bytes):
    from audian_amd.bufferedarray import WavLoader
    ints = np.arange(-30, 30).reshape(20, 3)
    p = tmp_path/'r.wav'
    write_pcm_wav(p, ints, sample_bytes)
    w = WavLoader(str(p))
    try:
        assert w.file_paths == [str(p)] and w.filepath == str(p)
        off, nb, ch, frames = cd.pcm_wav_info(w.filepath)
        assert (nb, ch, frames) == (sample_bytes, 3, 20)
        raw = open(p, 'rb').read()[off:off + frames*ch*nb]
        assert raw == w.pcm_slab(0, frames).tobytes()
    finally:
        w.close()


def test_several_files_are_refused():
    class Multi:
        channels, frames, rate = 1, 10, 1000.0
        file_paths = ['a.wav', 'b.wav']
    with pytest.raises(NotImplementedError):
        cd._Source(Multi())
