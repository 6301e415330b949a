"""CompressedData: the full-trace overview (FullTracePlot's min/max envelope of the whole recording) on the GPU.

A drop-in for audian's ``CompressedData`` (src/audian/compresseddata.py): the same surface and attributes
(``start``, ``wait``, ``is_busy``, ``close``, ``get_lock``, ``save_data_local``, ``save_data``, ``load_data``,
``times``, ``datas``, ``short_data``, ``fulltraces_file``, ``max_files``), the same arithmetic and the same cache
files.  What differs is where the work runs:

- the reference starts ``os.cpu_count() - 1`` processes that reopen the file, convert 30 s blocks to float64,
  unwrap them and reduce them with ``np.minimum/maximum.reduceat``;
- here a few reader threads read the blocks' raw PCM bytes with file descriptors of their own (``os.preadv``) into
  page-locked staging slots, and one worker thread, with a ``hipdsp.Context`` and stream of its own, copies each
  block to the device and reduces it with one kernel (``hipdsp_pcm_minmax``).  Nothing is forked: the process holds
  the GPU.

Sources: a ``WavLoader`` (one PCM WAV file) goes through the fused PCM kernel, bit-exact with the reference's
float64 arithmetic (unwrap off: ``int * scale``; unwrap on: the float32 unwrap every slab of the loader gets).  A
loader without a PCM file behind it but with its recording in memory (``ArrayLoader``: ``.data``) goes through the
existing kernels block by block -- ``pack`` -> ``unwrap`` -> ``minmax_decimate`` -- whose results are the float32
rounding of the reference's float64 values.  Recordings split over several files are not covered.

Like the reference's workers, every block is loaded on its own: an armed unwrap starts again at every block
boundary (``WavLoader.load_buffer`` does the same per slab), with the loader's ``unwrap_thresh`` and
``unwrap_clips`` and ``down_scale=False`` (``set_unwrap(thresh, clips, False, unit)``).

Cache files: ``<stem>-fulltrace.wav`` next to the recording (``save_data_local``) or ``{k:08X}-fulltrace.wav`` in
the user cache with the ``fulltraces.json`` index (``save_data``), float64 IEEE WAV, read and written here with
``struct`` (audioio is not a dependency).  Whether cache files that audian itself wrote through audioio open here
is not pinned by a test.

Command line: ``python -m audian_amd.compresseddata [-u [T]] [-U [T]] file.wav`` (the reference's
``audian-compress``).
"""

import argparse
import json
import os
import queue
import struct
import sys
import threading
import time
from datetime import datetime
from pathlib import Path

import numpy as np


# ---- the reference's arithmetic ------------------------------------------------------------------

def overview_layout(frames, rate, max_pixel):
    """Step, block size, time axis and row counts of the overview, as CompressedData.start computes them
    (src/audian/compresseddata.py:80-96):

    - ``step = max(1, frames//max_pixel)`` frames per min/max pair;
    - ``nblock = max(step, int(30.0*rate//step)*step)`` frames per block (a multiple of step);
    - ``times = np.arange(0, frames + step - 1, step/2)/rate``;
    - ``nseg = len(np.arange(0, frames, step))`` = ceil(frames/step) segments;
    - ``long_rows = len(times)``: the rows of ``datas`` on the background path (rows past ``2*nseg`` stay zero);
    - ``short_rows = 1 + 2*nseg``: the rows of ``datas`` on the short path.  That is one row more than the
      segments fill (the last stays zero), and it can differ from ``len(times)``: the reference does this.
    - ``blocks``: (first frame, frames, first row) of every block; a block's rows start at ``2*index//step``.
    """
    frames = int(frames)
    step = max(1, frames//int(max_pixel))
    nblock = max(step, int(30.0*rate//step)*step)
    times = np.arange(0, frames + step - 1, step/2)/rate
    nseg = len(np.arange(0, frames, step))
    blocks = [(index, min(nblock, frames - index), 2*index//step) for index in range(0, frames, nblock)]
    return dict(step=step, nblock=nblock, times=times, nseg=nseg, long_rows=len(times),
                short_rows=1 + 2*nseg, blocks=blocks)


def cache_rate(times):
    """The rate a cache file is written with: 1/(times[1] - times[0]) * 1e6, divided by 1e3 while above 2**31."""
    rate = 1/(times[1] - times[0])
    rate *= 1e6
    while rate > 2**31:
        rate /= 1e3
    return rate


def infer_rate(rate, nrows, frames, data_rate):
    """Which of rate/1e6, rate/1e3 and rate a cache file of `nrows` rows was written with: the one whose duration
    comes closest to the recording's (CompressedData.load_data)."""
    rates = np.array([rate/1e6, rate/1e3, rate])
    durations = nrows/rates
    return rates[np.argmin(np.abs(durations - frames/data_rate))]


# ---- float64 WAV files ---------------------------------------------------------------------------

_WAVE_FORMAT_PCM = 1
_WAVE_FORMAT_IEEE_FLOAT = 3
_WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def write_wav_f64(path, data, rate):
    """A (frames, channels) array as a float64 IEEE WAV file (format tag 3) with an integer rate."""
    data = np.asarray(data, dtype='<f8')
    if data.ndim == 1:
        data = data[:, None]
    frames, channels = data.shape
    raw = np.ascontiguousarray(data).tobytes()
    irate = int(round(rate))
    fmt = struct.pack('<HHIIHHH', _WAVE_FORMAT_IEEE_FLOAT, channels, irate,
                      min(irate*channels*8, 0xFFFFFFFF), channels*8, 64, 0)   # (byte rate: informative only)
    fact = struct.pack('<I', frames)
    body = (b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'fact' + struct.pack('<I', len(fact)) + fact +
            b'data' + struct.pack('<I', len(raw)) + raw)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def _wav_chunks(f):
    """(chunk id, offset of its payload, payload size) of a RIFF/WAVE file."""
    head = f.read(12)
    if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        raise ValueError('not a RIFF/WAVE file')
    pos = 12
    while True:
        f.seek(pos)
        h = f.read(8)
        if len(h) < 8:
            return
        cid, size = h[:4], struct.unpack('<I', h[4:])[0]
        yield cid, pos + 8, size
        pos += 8 + size + (size & 1)


def read_wav_float(path):
    """(data as float64 (frames, channels), rate) of a float WAV file: format tag 3, or WAVE_FORMAT_EXTENSIBLE with
    the IEEE-float sub-format; 32- or 64-bit samples."""
    with open(path, 'rb') as f:
        fmt = None
        for cid, off, size in _wav_chunks(f):
            if cid == b'fmt ':
                f.seek(off)
                fmt = f.read(size)
            elif cid == b'data':
                if fmt is None:
                    raise ValueError('data chunk before fmt chunk')
                tag, channels, rate, _, _, bits = struct.unpack('<HHIIHH', fmt[:16])
                if tag == _WAVE_FORMAT_EXTENSIBLE and len(fmt) >= 26:
                    tag = struct.unpack('<H', fmt[24:26])[0]
                if tag != _WAVE_FORMAT_IEEE_FLOAT or bits not in (32, 64):
                    raise ValueError(f'{path}: not a float WAV file (format {tag}, {bits} bits)')
                f.seek(off)
                raw = f.read(size)
                dt = '<f8' if bits == 64 else '<f4'
                n = len(raw)//(bits//8)//channels*channels
                data = np.frombuffer(raw[:n*(bits//8)], dtype=dt).astype(np.float64).reshape(-1, channels)
                return data, float(rate)
    raise ValueError(f'{path}: no data chunk')


def pcm_wav_info(path):
    """(byte offset of the samples, sample bytes, channels, frames) of a PCM WAV file (format tag 1, or
    WAVE_FORMAT_EXTENSIBLE with the PCM sub-format)."""
    with open(path, 'rb') as f:
        fmt = None
        for cid, off, size in _wav_chunks(f):
            if cid == b'fmt ':
                f.seek(off)
                fmt = f.read(size)
            elif cid == b'data':
                if fmt is None:
                    raise ValueError('data chunk before fmt chunk')
                tag, channels, _, _, align, bits = struct.unpack('<HHIIHH', fmt[:16])
                if tag == _WAVE_FORMAT_EXTENSIBLE and len(fmt) >= 26:
                    tag = struct.unpack('<H', fmt[24:26])[0]
                if tag != _WAVE_FORMAT_PCM:
                    raise ValueError(f'{path}: not a PCM WAV file')
                nbytes = (bits + 7)//8
                return off, nbytes, channels, size//(nbytes*channels)
    raise ValueError(f'{path}: no data chunk')


def default_cache_dir():
    """audian's own user cache directory (audian_dirs.user_cache_path)."""
    from platformdirs import PlatformDirs
    return Path(PlatformDirs('audian', 'janscience').user_cache_path)


class _Lock:
    """A threading.Lock whose acquire() also takes multiprocessing's keyword: FullTracePlot.plot_data calls
    ``get_lock().acquire(block=False)``."""

    def __init__(self):
        self._lock = threading.Lock()

    def acquire(self, block=True, timeout=None):
        if timeout is None:
            return self._lock.acquire(block)
        return self._lock.acquire(block, timeout)

    def release(self):
        self._lock.release()

    def locked(self):
        return self._lock.locked()

    def __enter__(self):
        self._lock.acquire()
        return self

    def __exit__(self, *exc):
        self._lock.release()


# ---- the device side -----------------------------------------------------------------------------

class _Source:
    """Where the blocks come from: a PCM WAV file (read with own descriptors) or an in-memory recording."""

    def __init__(self, data):
        self.channels = int(data.channels)
        self.frames = int(data.frames)
        paths = getattr(data, 'file_paths', None)
        if paths is not None and len(paths) > 1:
            raise NotImplementedError('CompressedData: recordings split over several files are not supported')
        self.path = None
        path = getattr(data, 'filepath', None)
        if path is not None and getattr(data, 'sample_bytes', None) in (2, 3, 4):
            offset, nbytes, channels, frames = pcm_wav_info(path)
            if nbytes != data.sample_bytes or channels != self.channels or frames < self.frames:
                raise ValueError(f'{path}: the file does not match its loader')
            self.path = os.fspath(path)
            self.offset = offset
            self.sample_bytes = nbytes
            self.scale = float(data.scale)
            self.frame_bytes = nbytes*self.channels
        else:
            array = getattr(data, 'data', None)
            if not isinstance(array, np.ndarray):
                raise NotImplementedError('CompressedData: the loader has neither a PCM WAV file nor its recording '
                                          'in memory (.data)')
            self.array = array.reshape(len(array), -1)
            self.dtype = np.float32 if self.array.dtype == np.float32 else np.float64
            self.frame_bytes = np.dtype(self.dtype).itemsize*self.channels
        self.unwrap_thresh = float(getattr(data, 'unwrap_thresh', 0.0))
        self.unwrap_clips = bool(getattr(data, 'unwrap_clips', False))
        self.unwrap_ampl = float(getattr(data, 'unwrap_ampl', getattr(data, 'ampl_max', 1.0)))

    @property
    def is_pcm(self):
        return self.path is not None

    def open(self):
        """A read handle of the calling reader thread's own."""
        return os.open(self.path, os.O_RDONLY) if self.is_pcm else None

    def close(self, fd):
        if fd is not None:
            os.close(fd)

    def read(self, fd, index, n, slot):
        """Frames [index, index + n) into the staging slot (a uint8 array)."""
        nbytes = n*self.frame_bytes
        view = memoryview(slot)[:nbytes]
        if self.is_pcm:
            pos, done = self.offset + index*self.frame_bytes, 0
            while done < nbytes:
                got = os.preadv(fd, [view[done:]], pos + done)
                if got <= 0:
                    raise IOError(f'{self.path}: short read at frame {index}')
                done += got
        else:
            dst = np.frombuffer(view, dtype=self.dtype).reshape(n, self.channels)
            dst[:, :] = self.array[index:index + n]


class _Engine:
    """A context and stream of the calling thread's own, device buffers for one block, and the block reduction."""

    def __init__(self, source, nblock, step):
        from . import hipdsp
        self.hd = hipdsp
        self.src = source
        self.step = step
        self.nblock = nblock
        self.ctx = hipdsp.Context(int(os.environ.get('LOCAL_RANK', '0')))
        self.stream = None
        self.bufs = []
        try:
            self.stream = self.ctx.create_stream()
            self.ctx.set_stream(self.stream)
            C = source.channels
            nseg = (nblock + step - 1)//step
            self.raw = self._dev((nblock*source.frame_bytes + 15)//16*16, np.uint8)
            if source.is_pcm:
                self.out = self._dev((2*nseg, C), np.float64)
            else:
                self.planar = self._dev((C, nblock), np.float32)
                if source.unwrap_thresh > 1e-3:
                    self.unwrapped = self._dev((C, nblock), np.float32)
                self.out = self._dev((C, 2*nseg), np.float32)
        except BaseException:
            self.close()
            raise

    def _dev(self, shape, dtype):
        d = self.hd.DeviceArray(self.ctx, shape, dtype)
        self.bufs.append(d)
        return d

    def host_slot(self, frames):
        return self.hd.HostBuffer(self.ctx, frames*self.src.frame_bytes)

    def stage(self, slot, frame0, n):
        """Frames [frame0, frame0 + n) of the block, staged in `slot` (a HostBuffer), to the device; returns when
        the copy is done and the slot is free again."""
        fb = self.src.frame_bytes
        self.hd.memcpy_h2d_async(self.ctx, self.raw.ptr + frame0*fb, slot, n*fb)
        self.ctx.synchronize()

    def reduce(self, n):
        """min/max rows of the block of n frames on the device: float64 (2*ceil(n/step), C)."""
        hd, src, ctx = self.hd, self.src, self.ctx
        C = src.channels
        nseg = (n + self.step - 1)//self.step
        wrap = src.unwrap_thresh > 1e-3
        if src.is_pcm:
            hd.pcm_minmax(ctx, self.raw, src.sample_bytes, n, C, self.step, src.scale, self.out, C,
                          unwrap_thresh=src.unwrap_thresh if wrap else 0.0, ampl_max=src.unwrap_ampl,
                          clips=src.unwrap_clips, down_scale=False)
            return self.out.view(0, (2*nseg, C)).to_host()
        hd.pack(ctx, self.raw, self.planar, self.nblock, n, C, src_dtype=src.dtype)
        x = self.planar
        if wrap:
            hd.unwrap(ctx, self.planar, self.nblock, C, n, src.unwrap_thresh, self.unwrapped, self.nblock,
                      ampl_max=src.unwrap_ampl, clips=src.unwrap_clips, down_scale=False)
            x = self.unwrapped
        hd.minmax_decimate(ctx, x, self.nblock, C, 0, n, self.step, self.out, 2*nseg)
        return self.out.view(0, (C, 2*nseg)).to_host().T.astype(np.float64)

    def close(self):
        if self.ctx is None:
            return
        try:
            self.ctx.synchronize()
        finally:
            for d in self.bufs:
                d.free()
            self.bufs = []
            if self.stream is not None:
                self.ctx.set_stream(None)
                self.ctx.destroy_stream(self.stream)
                self.stream = None
            self.ctx.close()
            self.ctx = None


class CompressedData:

    fulltraces_file = 'fulltraces.json'
    max_files = 1000
    readers = 2              # reader threads of the background path
    chunk_bytes = 16 << 20   # bytes of a page-locked staging slot (readers + 2 of them)

    def __init__(self, data, cache_dir=None):
        self.data = data
        self.cache_dir = Path(cache_dir) if cache_dir is not None else None
        self.times = None
        self.datas = None
        self.short_data = True
        self._lock = _Lock()
        self._threads = []
        self._stop = threading.Event()
        self._error = None
        self.setup_seconds = None   # background path: context, buffers and threads up, before the first chunk

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def user_cache_path(self):
        if self.cache_dir is None:
            self.cache_dir = default_cache_dir()
        return self.cache_dir

    # -- computing ------------------------------------------------------------------------------
    def close(self):
        """Stop the background work, join every thread, free the device and host memory."""
        self._stop.set()
        for t in self._threads:
            t.join()
        self._threads = []

    def start(self, max_pixel, load_kwargs, do_short=True):
        if self.times is not None and self.datas is not None:
            return
        self.close()
        self._stop = threading.Event()
        self._error = None
        source = _Source(self.data)
        lay = overview_layout(self.data.frames, self.data.rate, max_pixel)
        step, nblock = lay['step'], lay['nblock']
        self.times = lay['times']
        if len(self.data.buffer) == self.data.frames:
            # short file, do not compress in background: the whole recording as one block, right here
            self.short_data = True
            if do_short:
                # one row more than the segments need (the reference's arithmetic, kept)
                self.datas = np.zeros((lay['short_rows'], self.data.channels))
                n = self.data.frames
                eng = _Engine(source, max(n, 1), step)
                try:
                    slot = eng.host_slot(n)
                    fd = source.open()
                    try:
                        source.read(fd, 0, n, slot.array)
                    finally:
                        source.close(fd)
                    eng.stage(slot, 0, n)
                    slot.free()
                    self.datas[:2*lay['nseg']] = eng.reduce(n)
                finally:
                    eng.close()
            return
        # compress in background:
        self.short_data = False
        self.datas = np.zeros((lay['long_rows'], self.data.channels))
        worker = threading.Thread(target=self._worker, args=(source, lay), name='overview-worker', daemon=True)
        self._threads = [worker]
        worker.start()

    def _worker(self, source, lay):
        """Readers fill page-locked slots of `chunk_bytes` with consecutive chunks of the blocks, in order; this
        thread copies each chunk into the block's device buffer as soon as it is there (the slot goes back to the
        readers), reduces a block once its last chunk is in, and puts its rows into `datas` under the lock."""
        blocks, step, nblock = lay['blocks'], lay['step'], lay['nblock']
        eng = None
        slots = []
        readers = []
        try:
            t0 = time.perf_counter()
            eng = _Engine(source, nblock, step)
            cf = max(1, min(nblock, self.chunk_bytes//source.frame_bytes))      # frames per chunk
            items = [(k, j0, min(cf, n - j0)) for k, (index, n, row) in enumerate(blocks) for j0 in range(0, n, cf)]
            nread = max(1, min(self.readers, len(items)))
            slots = [eng.host_slot(cf) for _ in range(min(nread + 2, len(items)))]
            free, filled = queue.Queue(), queue.Queue()
            for s in slots:
                free.put(s)
            todo = iter(range(len(items)))
            todo_lock = threading.Lock()

            def reader():
                fd = source.open()
                try:
                    while not self._stop.is_set():
                        slot = None
                        while slot is None:
                            if self._stop.is_set():
                                return
                            try:
                                slot = free.get(timeout=0.05)
                            except queue.Empty:
                                pass
                        with todo_lock:
                            i = next(todo, None)
                        if i is None:
                            return
                        k, j0, m = items[i]
                        source.read(fd, blocks[k][0] + j0, m, slot.array)
                        filled.put((i, slot))
                except BaseException as e:
                    self._error = e
                    self._stop.set()
                finally:
                    source.close(fd)

            readers = [threading.Thread(target=reader, name=f'overview-reader{i}', daemon=True) for i in range(nread)]
            for t in readers:
                t.start()
            self.setup_seconds = time.perf_counter() - t0
            arrived = {}
            for i, (k, j0, m) in enumerate(items):
                while i not in arrived:
                    if self._stop.is_set():
                        return
                    try:
                        got, slot = filled.get(timeout=0.05)
                        arrived[got] = slot
                    except queue.Empty:
                        pass
                slot = arrived.pop(i)
                eng.stage(slot, j0, m)
                free.put(slot)
                index, n, row = blocks[k]
                if j0 + m == n:
                    rows = eng.reduce(n)
                    with self._lock:
                        self.datas[row:row + len(rows)] = rows
        except BaseException as e:
            if self._error is None:
                self._error = e
            self._stop.set()
        finally:
            self._stop.set()
            for t in readers:
                t.join()
            for s in slots:
                s.free()
            if eng is not None:
                eng.close()

    def wait(self):
        for t in self._threads:
            t.join()
        self._threads = []
        if self._error is not None:
            err, self._error = self._error, None
            raise RuntimeError('CompressedData: computing the overview failed') from err

    def is_busy(self):
        return any(t.is_alive() for t in self._threads)

    def get_lock(self):
        return self._lock

    # -- caches -----------------------------------------------------------------------------------
    def _local_path(self):
        fp = Path(self.data.filepath)
        return fp.with_name(fp.stem + '-fulltrace.wav')

    def _first_last(self):
        paths = getattr(self.data, 'file_paths', None) or [self.data.filepath]
        return os.fspath(Path(paths[0]).absolute()), os.fspath(Path(paths[-1]).absolute())

    def save_data_local(self):
        if self.short_data or getattr(self.data, 'filepath', None) is None:
            return
        write_wav_f64(self._local_path(), self.datas, cache_rate(self.times))

    def save_data(self):
        if self.short_data or getattr(self.data, 'filepath', None) is None:
            return
        cache = self.user_cache_path
        cache.mkdir(parents=True, exist_ok=True)
        files = {}
        ft_path = cache / self.fulltraces_file
        if ft_path.exists():
            with ft_path.open() as sf:
                files = json.load(sf)
        # new filename:
        ft_name = f'{1:08X}-fulltrace.wav'
        for k in range(1, self.max_files + 10):
            ft_name = f'{k:08X}-fulltrace.wav'
            if ft_name not in files.keys():
                break
        first_file, last_file = self._first_last()
        timestamp = datetime.now().isoformat()
        rate = 1/(self.times[1] - self.times[0])
        files[ft_name] = dict(first=first_file, last=last_file, rate=rate, created=timestamp, used=timestamp)
        # remove the least recently used files:
        if len(files) > self.max_files:
            ft_files = list(files)
            timestamps = [files[ftf]['used'] for ftf in ft_files]
            idx = np.argsort(timestamps)
            for i in idx[:len(ft_files) - self.max_files]:
                try:
                    (cache / ft_files[i]).unlink()
                except Exception as e:
                    print(e)
                files.pop(ft_files[i])
        with ft_path.open('w') as df:
            json.dump(files, df, indent=4)
        write_wav_f64(cache / ft_name, self.datas, cache_rate(self.times))

    def load_data(self):
        self.times = None
        self.datas = None
        if getattr(self.data, 'filepath', None) is None:
            return
        # load from folder of data file:
        ft_path = self._local_path()
        if ft_path.exists():
            self.datas, rate = read_wav_float(ft_path)
            rate = infer_rate(rate, len(self.datas), self.data.frames, self.data.rate)
            self.times = np.arange(len(self.datas))/rate
            return
        # load from user cache:
        cache = self.user_cache_path
        ft_path = cache / self.fulltraces_file
        if cache.exists() and ft_path.exists():
            with ft_path.open() as sf:
                files = json.load(sf)
            first_file, last_file = self._first_last()
            for ft_file in files.keys():
                ft_props = files[ft_file]
                if ft_props['first'] == first_file and ft_props['last'] == last_file:
                    ft_file_path = cache / ft_file
                    if not ft_file_path.is_file() or ft_file_path.stat().st_size == 0:
                        # remove file from json file:
                        del files[ft_file]
                        with ft_path.open('w') as df:
                            json.dump(files, df, indent=4)
                        break
                    self.datas, _ = read_wav_float(ft_file_path)
                    rate = ft_props['rate']
                    self.times = np.arange(len(self.datas))/rate
                    ft_props['used'] = datetime.now().isoformat()
                    with ft_path.open('w') as df:
                        json.dump(files, df, indent=4)
                    break


# ---- command line --------------------------------------------------------------------------------

def parse_args(cargs):
    """audian-compress's arguments and its -u / -U rule: with -U T (T > 1e-3) unwrap = T and clip."""
    parser = argparse.ArgumentParser(description='Compress timeseries data for audian (full-trace overview on '
                                     'the GPU).')
    parser.add_argument('-u', dest='unwrap', default=0, type=float, metavar='UNWRAP', const=1.5, nargs='?',
                        help='unwrap clipped data with threshold relative to maximum input range')
    parser.add_argument('-U', dest='unwrap_clip', default=0, type=float, metavar='UNWRAP', const=1.5, nargs='?',
                        help='unwrap clipped data with threshold relative to maximum input range and clip')
    parser.add_argument('files', nargs='+', default=[], type=str,
                        help='name of files with the time series data')
    args = parser.parse_args(cargs)
    if args.unwrap_clip > 1e-3:
        args.unwrap = args.unwrap_clip
        args.unwrap_clip = True
    else:
        args.unwrap_clip = False
    return args


def main(cargs):
    from .bufferedarray import WavLoader
    args = parse_args(cargs)
    if len(args.files) > 1:
        raise NotImplementedError('recordings split over several files are not supported')
    data = WavLoader(args.files[0], buffer_time=1.0, back_time=0.0)
    try:
        data.set_unwrap(args.unwrap, args.unwrap_clip, False, data.unit)
        compress = CompressedData(data)
        compress.start(6000, {})
        compress.wait()
        compress.save_data_local()
        compress.close()
    finally:
        data.close()


def run():
    main(sys.argv[1:])
    return 0


if __name__ == '__main__':
    run()
