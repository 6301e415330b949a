"""hipdsp_band_power, device resident, at BASELINE configs[2]'s sample count (64 ch x 600 s x 96 kHz) for the slabs of
three windows -- 2048/1024 (64 x 56 250 x 1025, configs[2]'s own), 256/128 and 8192/4096 -- and five band sets: the full
band, the top 1/16, a 64-bin band, one bin, four disjoint bands in one call.
    python tools/band_power_bench.py [seconds=600] [--host-route] [--pmc]
Per line: median of 10 launches after 3 warm-ups (hipdsp_event_*), GB/s over the ALGORITHMIC bytes (band bins x 4 B +
output x 4 B); behind it the bytes of the 128-B lines those bins lie in (what HBM has to deliver at least), the rate over
them, and the same run's hipdsp_copy_probe rate (read + write).  The lines are in the format tools/entry_points_gate.py
reads.  --host-route: what the same numbers cost without the kernel -- np.sum(spec.buffer[:, :, k0:k1], axis=2) through the
lazy read-back of the spectrogram's mirror -- at configs[2]'s shape with a TENTH of its duration (the host copy is
float64: 3 GB for 60 s), next to BufferedBandPower.set_band() on the same graph.  --pmc: nothing but three launches of the
64-bin band on configs[2]'s slab, for a counter run of its own (rocprofv3 --pmc FETCH_SIZE, then WRITE_SIZE, the program
after `--`): per launch the band's 64 x 56 250 rows of 256 B at 4-byte alignment lie in 2-3 lines of 128 B each."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

args = [a for a in sys.argv[1:] if not a.startswith('--')]
host_route = '--host-route' in sys.argv
pmc = '--pmc' in sys.argv
C, rate = 64, 96000.0
T = int((float(args[0]) if args else 600.0)*rate)
WINDOWS = ((2048, 1024),) if pmc else ((2048, 1024), (256, 128), (8192, 4096))
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()


def median_ms(f, n=10, warm=3):
    if pmc:
        n, warm = 3, 0
    for _ in range(warm):
        f()
    times = []
    for _ in range(n):
        ctx.record(e0)
        f()
        ctx.record(e1)
        ctx.synchronize()
        times.append(ctx.elapsed_ms(e0, e1))
    return float(np.median(times))


def line_bytes(nd, F, bands):
    """Bytes of the distinct 128-B lines the bands' bins of all rows lie in (compact slab, base 128-B aligned)."""
    rows = np.arange(C*nd, dtype=np.int64)
    lines = 0
    segs = []
    for k0, k1 in sorted(b for b in bands if b[1] > b[0]):
        if segs and k0 <= segs[-1][1]:
            segs[-1][1] = max(segs[-1][1], k1)
        else:
            segs.append([k0, k1])
    last = None
    for k0, k1 in segs:
        first_line = (rows*F + k0)*4//128
        last_line = ((rows*F + k1)*4 - 1)//128
        lines += int(np.sum(last_line - first_line + 1))
        if last is not None:
            lines -= int(np.sum(first_line == last))          # a line two segments share counts once
        last = last_line
    return 128.0*lines


nbytes = 1 << (20 if pmc else 31)
a, b = h.DeviceArray(ctx, (nbytes,), np.uint8), h.DeviceArray(ctx, (nbytes,), np.uint8)
a.zero_()
copy_ms = median_ms(lambda: h.check(h.lib.hipdsp_copy_probe(ctx.handle, h._p(b), h._p(a), nbytes)))
copy_rate = 2.0*nbytes/copy_ms/1e6
a.free()
b.free()
print(f'{"hipdsp_copy_probe, %d MiB (read + write)" % (nbytes >> 20):78s} {copy_ms:8.3f} ms {copy_rate:7.0f} GB/s', flush=True)

dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
ds = h.DeviceArray(ctx, (max(C*((T + hp - 1)//hp)*(n//2 + 1) for n, hp in WINDOWS),), np.float32)
for nfft, hop in WINDOWS:
    F, nd = nfft//2 + 1, (T + hop - 1)//hop
    h.spectrogram(ctx, dx, T, C, T, nfft, hop, rate, ds, nd)
    ctx.synchronize()
    w = max(F//16, 1)
    sets = [('full band', [(0, F)]), ('top 1/16', [(F - w, F)]), ('64-bin band', [(F//3, F//3 + 64)]),
            ('one bin', [(F//3, F//3 + 1)]), ('4 disjoint bands of 1/16', [(j*F//4 + 1, j*F//4 + 1 + w) for j in range(4)])]
    if pmc:
        sets = sets[2:3]
    out = h.DeviceArray(ctx, (4, C, nd), np.float32)
    for name, bands in sets:
        ms = median_ms(lambda: h.band_power(ctx, ds, 0, C, nd, F, bands, rate/nfft, out))
        bins = sum(k1 - k0 for k0, k1 in bands)
        algo = 4.0*C*nd*(bins + len(bands))
        touched = line_bytes(nd, F, bands) + 4.0*C*nd*len(bands)
        print(f'{f"hipdsp_band_power {nfft}/{hop} slab (64 x {nd} x {F}), {name}":78s} {ms:8.3f} ms {algo/ms/1e6:7.0f} GB/s', flush=True)
        print(f'    algorithmic {algo/1e9:.3f} GB; in 128-B lines {touched/1e9:.3f} GB = {touched/ms/1e6:.0f} GB/s; '
              f'copy probe {copy_rate:.0f} GB/s', flush=True)
    out.free()
ds.free()
dx.free()

if host_route:
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedbandpower import BufferedBandPower
    from audian_amd.tracegraph import TraceGraph
    h._default_ctx = ctx
    Th = T//10
    rng = np.random.default_rng(1)
    host = rng.uniform(-1, 1, size=(Th, C)).astype(np.float32)

    class Shown:
        def isVisible(self):
            return True

    g = TraceGraph(Th/rate, 0.0)
    filt, spec, band = BufferedFilter(), BufferedSpectrogram(nfft=2048), BufferedBandPower()
    for t in (filt, spec, band):
        g.add_trace(t)
    g.setup_traces()
    g.open(host, rate, view=True)
    for t in g.traces:
        t.plot_items = [Shown() for _ in range(t.channels)]
    g.set_need_update()
    g.update_times(0.0, Th/rate)
    filt.update()
    ctx.synchronize()
    nd, F = len(spec._hostbuf), spec.shape[2]
    times = []
    for fmin in (100.0, 200.0, 0.0):
        t0 = time.perf_counter()
        band.set_band(fmin, None)
        _ = band.buffer[:, 0]                                   # what a plot item reads: one channel, from the mirror
        times.append((time.perf_counter() - t0)*1e3)
    dev = np.array(band.buffer)
    t0 = time.perf_counter()
    res = spec.fresolution*np.sum(spec.buffer[:, :, 0:F], axis=2)
    first = (time.perf_counter() - t0)*1e3
    t0 = time.perf_counter()
    res = spec.fresolution*np.sum(spec.buffer[:, :, 0:F], axis=2)
    again = (time.perf_counter() - t0)*1e3
    err = float(np.max(np.abs(dev - res)/np.maximum(res, 1e-300)))
    print(f'host route at a tenth of the duration (64 x {nd} x {F}, full band): np.sum over the lazy read-back {first:.0f} ms '
          f'the first time ({8e-9*C*nd*F:.2f} GB over PCIe, the read-back is float64), {again:.0f} ms once the host copy '
          f'is current; BufferedBandPower.set_band() + one channel read {min(times):.2f} ms (wall clock); '
          f'largest relative difference {err:.2e}', flush=True)
