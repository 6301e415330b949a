"""Full-trace overview (audian_amd.compresseddata): what the GPU path costs, on a synthetic PCM WAV file.

  python tools/overview_bench.py [--seconds 60] [--rate 96000] [--channels 64] [--bits 16 24 32] [--dir DIR]
  python tools/overview_bench.py --cpu-baseline [same options]

(a) hipdsp_pcm_minmax against hipdsp_pcm_unpack + hipdsp_minmax_decimate on one 30 s block already on the device,
    timed with device events; GB/s counts the PCM bytes only (the algorithmic volume of both paths' input);
(b) CompressedData.start() -> wait() wall time next to the time the same reader threads take just to read the file
    into page-locked staging slots (no device work);
(c) --cpu-baseline, in a separate invocation that opens no GPU: the reference's method on the same file -- float64
    blocks of 30 s, np.minimum/maximum.reduceat, a pool of at most 15 worker processes.

The file is written first (random samples, 30 s of them repeated) and so is read from the page cache.  One JSON
line per sample width; nothing here is part of bench.py.
"""

import argparse
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from audian_amd import compresseddata as cd      # noqa: E402  (opens no GPU by itself)


def write_wav(path, seconds, rate, channels, sample_bytes, seed=1):
    """A PCM WAV file of `seconds` of random samples: one 30 s block of random bytes, written repeatedly."""
    import struct
    frames = int(seconds*rate)
    fb = channels*sample_bytes
    block = min(frames, int(30*rate))
    raw = np.frombuffer(np.random.default_rng(seed).bytes(block*fb), dtype=np.uint8)
    nbytes = frames*fb
    fmt = struct.pack('<HHIIHH', 1, channels, int(rate), int(rate)*fb, fb, 8*sample_bytes)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', (36 + nbytes) & 0xFFFFFFFF) + b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt +
                b'data' + struct.pack('<I', nbytes & 0xFFFFFFFF))
        done = 0
        while done < frames:
            n = min(block, frames - done)
            f.write(raw[:n*fb].tobytes())
            done += n
    return frames


class RawWav:
    """The loader attributes CompressedData reads, for a file too long for wave's 32-bit sizes to matter."""

    def __init__(self, path, frames, rate, channels, sample_bytes):
        self.filepath = path
        self.file_paths = [path]
        self.frames, self.rate, self.channels = frames, float(rate), channels
        self.sample_bytes = sample_bytes
        self.scale = 1.0/float(1 << (8*sample_bytes - 1))
        self.buffer = np.zeros((0, channels))
        self.unwrap_thresh, self.unwrap_clips, self.unwrap_ampl = 0.0, False, 1.0


def kernel_ab(hd, ctx, path, frames, rate, channels, sample_bytes, reps):
    """(a): one 30 s block on the device, the fused kernel against the two-kernel path."""
    lay = cd.overview_layout(frames, rate, 6000)
    n, step = lay['blocks'][0][1], lay['step']
    off, _, _, _ = cd.pcm_wav_info(path)
    fb = channels*sample_bytes
    with open(path, 'rb') as f:
        f.seek(off)
        raw = np.frombuffer(f.read(n*fb), dtype=np.uint8)
    scale = 1.0/float(1 << (8*sample_bytes - 1))
    nseg = (n + step - 1)//step
    pcm = hd.DeviceArray.from_host(ctx, raw)
    out64 = hd.DeviceArray(ctx, (2*nseg, channels), np.float64)
    planar = hd.DeviceArray(ctx, (channels, n), np.float32)
    out32 = hd.DeviceArray(ctx, (channels, 2*nseg), np.float32)

    def fused():
        hd.pcm_minmax(ctx, pcm, sample_bytes, n, channels, step, scale, out64, channels)

    def two():
        hd.pcm_unpack(ctx, pcm, sample_bytes, n, channels, scale, planar, n)
        hd.minmax_decimate(ctx, planar, n, channels, 0, n, step, out32, 2*nseg)

    res = {}
    e0, e1 = ctx.event(), ctx.event()
    for name, fn in (('fused', fused), ('two_kernel', two), ('fused_again', fused)):
        for _ in range(3):
            fn()
        ctx.synchronize()
        ms = []
        for _ in range(reps):
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ctx.synchronize()
            ms.append(ctx.elapsed_ms(e0, e1))
        res[name] = float(np.median(ms))
    # the two paths agree (float32 rounding of the exact values)
    a = out64.to_host()
    b = out32.to_host().T.astype(np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), b), 'fused and two-kernel results differ'
    ctx.destroy_event(e0)
    ctx.destroy_event(e1)
    for d in (pcm, out64, planar, out32):
        d.free()
    gb = n*fb/1e9
    fused_ms = min(res['fused'], res['fused_again'])
    return dict(block_frames=n, step=step, pcm_GB=round(gb, 4), fused_ms=round(fused_ms, 4),
                two_kernel_ms=round(res['two_kernel'], 4), fused_GBps=round(gb/fused_ms*1e3, 1),
                two_kernel_GBps=round(gb/res['two_kernel']*1e3, 1), speedup=round(res['two_kernel']/fused_ms, 2))


def read_only(path, frames, rate, channels, sample_bytes, hd, ctx, readers):
    """(b)'s yardstick: the same reader threads reading the same chunks into page-locked slots of the same size,
    no device work."""
    loader = RawWav(path, frames, rate, channels, sample_bytes)
    src = cd._Source(loader)
    lay = cd.overview_layout(frames, rate, 6000)
    cf = max(1, min(lay['nblock'], cd.CompressedData.chunk_bytes//src.frame_bytes))
    items = [(index + j0, min(cf, n - j0)) for index, n, _ in lay['blocks'] for j0 in range(0, n, cf)]
    slots = [hd.HostBuffer(ctx, cf*src.frame_bytes) for _ in range(readers)]
    todo = iter(items)
    lock = threading.Lock()

    def reader(slot):
        fd = src.open()
        try:
            while True:
                with lock:
                    item = next(todo, None)
                if item is None:
                    return
                src.read(fd, item[0], item[1], slot.array)
        finally:
            src.close(fd)

    t0 = time.perf_counter()
    ts = [threading.Thread(target=reader, args=(s,)) for s in slots]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    for s in slots:
        s.free()
    return dt


def end_to_end(path, frames, rate, channels, sample_bytes):
    loader = RawWav(path, frames, rate, channels, sample_bytes)
    c = cd.CompressedData(loader)
    t0 = time.perf_counter()
    c.start(6000, {})
    c.wait()
    dt = time.perf_counter() - t0
    c.close()
    return dt, c.setup_seconds


def _cpu_worker(args):
    """The reference's down_sample_worker for one block: float64, reduceat."""
    path, off, index, n, channels, sample_bytes, step = args
    fb = channels*sample_bytes
    with open(path, 'rb') as f:
        f.seek(off + index*fb)
        raw = np.frombuffer(f.read(n*fb), dtype=np.uint8)
    if sample_bytes == 2:
        ints = raw.view('<i2').astype(np.int64)
    elif sample_bytes == 4:
        ints = raw.view('<i4').astype(np.int64)
    else:
        b = raw.reshape(-1, 3).astype(np.int64)
        ints = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        ints = np.where(ints >= 1 << 23, ints - (1 << 24), ints)
    buf = ints.reshape(-1, channels)*(1.0/float(1 << (8*sample_bytes - 1)))
    seg = np.arange(0, n, step)
    out = np.empty((2*len(seg), channels))
    np.minimum.reduceat(buf, seg, out=out[0::2])
    np.maximum.reduceat(buf, seg, out=out[1::2])
    return index, out


def cpu_baseline(path, frames, rate, channels, sample_bytes):
    import multiprocessing as mp
    lay = cd.overview_layout(frames, rate, 6000)
    off, _, _, _ = cd.pcm_wav_info(path)
    nproc = max(1, min(15, (os.cpu_count() or 2) - 1))
    jobs = [(path, off, index, n, channels, sample_bytes, lay['step']) for index, n, _ in lay['blocks']]
    datas = np.zeros((lay['long_rows'], channels))
    t0 = time.perf_counter()
    with mp.get_context('fork').Pool(nproc) as pool:
        for index, out in pool.imap_unordered(_cpu_worker, jobs):
            row = 2*index//lay['step']
            datas[row:row + len(out)] = out
    return time.perf_counter() - t0, nproc, datas


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--rate', type=float, default=96000.0)
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--bits', type=int, nargs='+', default=[16, 24, 32])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--dir', default=None, help='where the synthetic file goes (default: a temporary directory)')
    ap.add_argument('--cpu-baseline', action='store_true', help='(c) only: the reference method, no GPU')
    args = ap.parse_args()
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    hd = ctx = None
    if not args.cpu_baseline:
        from audian_amd import hipdsp as hd
        ctx = hd.default_context()
    try:
        for bits in args.bits:
            sb = bits//8
            path = os.path.join(tmp.name, f'synthetic_{bits}bit.wav')
            frames = write_wav(path, args.seconds, args.rate, args.channels, sb)
            res = dict(bits=bits, channels=args.channels, seconds=args.seconds, rate=args.rate,
                       file_GB=round(frames*args.channels*sb/1e9, 3))
            if args.cpu_baseline:
                dt, nproc, _ = cpu_baseline(path, frames, args.rate, args.channels, sb)
                res['cpu_pool'] = dict(processes=nproc, wall_s=round(dt, 3))
            else:
                res['kernel'] = kernel_ab(hd, ctx, path, frames, args.rate, args.channels, sb, args.reps)
                ro = [read_only(path, frames, args.rate, args.channels, sb, hd, ctx, cd.CompressedData.readers)
                      for _ in range(3)]
                e2e, setup = [], []
                for _ in range(3):
                    dt, st = end_to_end(path, frames, args.rate, args.channels, sb)
                    e2e.append(dt)
                    setup.append(st)
                res['end_to_end'] = dict(readers=cd.CompressedData.readers, read_only_s=round(min(ro), 3),
                                         overview_s=round(min(e2e), 3),
                                         setup_s=round(setup[int(np.argmin(e2e))], 4),
                                         ratio=round(min(e2e)/min(ro), 3), read_GBps=round(res['file_GB']/min(ro), 2))
            os.unlink(path)
            print(json.dumps(res), flush=True)
    finally:
        tmp.cleanup()


if __name__ == '__main__':
    main()
