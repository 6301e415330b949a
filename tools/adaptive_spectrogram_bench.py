"""hipdsp_spec_adapt, device resident, on the PSD slab of BASELINE configs[2] (64 ch x 600 s x 96 kHz, window 2048/1024:
64 x 56 250 x 1025 float32, 14.76 GB), all four modes, out of place, with the default parameters of
BufferedAdaptiveSpectrogram (time constant 0.4 s at 93.75 frames/s).
    python tools/adaptive_spectrogram_bench.py [seconds=600]
Per line: median of 10 calls after 3 warm-ups (hipdsp_event_*), GB/s over the bytes the shape has to move: the slab read
twice and written once (2 R + 1 W; the carries add 1/128 of a read and of a write).  The yardsticks of the same process:
hipdsp_spec_equalize (1 R + 1 W) and hipdsp_memcpy_d2d of the same slab.  The ratios at the end are reported, not gated.
The lines are in the format tools/entry_points_gate.py reads."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.bufferedadaptivespectrogram import smooth_for

args = [a for a in sys.argv[1:] if not a.startswith('--')]
C, rate, nfft, hop = 64, 96000.0, 2048, 1024
T = int((float(args[0]) if args else 600.0)*rate)
F, nd = nfft//2 + 1, (T + hop - 1)//hop
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()


def median_ms(f, n=10, warm=3):
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


def report(name, ms, nbytes, note=''):
    print(f'{name:86s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s{note}', flush=True)


slab_bytes = 4.0*C*nd*F
dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
ds = h.DeviceArray(ctx, (C, nd, F), np.float32)
h.spectrogram(ctx, dx, T, C, T, nfft, hop, rate, ds, nd)
ctx.synchronize()
dx.free()
do = h.DeviceArray(ctx, (C, nd, F), np.float32)
shape = f'(64 x {nd} x {F})'
ctx.reserve(h.adapt_scratch_bytes(C, nd, F))

copy_ms = median_ms(lambda: h.check(h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(do), h._p(ds), int(slab_bytes))))
report(f'hipdsp_memcpy_d2d of the slab {shape} (read + write)', copy_ms, 2.0*slab_bytes)
prof = h.DeviceArray.from_host(ctx, np.full((C, F), 1e-9, dtype=np.float32))
eq_ms = median_ms(lambda: h.spec_equalize(ctx, ds, 0, do, 0, C, nd, F, prof, 0, 'divide'))
report(f'hipdsp_spec_equalize {shape}, divide, out of place (read + write)', eq_ms, 2.0*slab_bytes)

smooth = smooth_for(0.4, rate/hop)
ms = {}
for mode in ('background', 'divide', 'subtract', 'pcen'):
    ms[mode] = median_ms(lambda: h.spec_adapt(ctx, ds, 0, do, 0, C, nd, F, 0, smooth, mode))
    report(f'hipdsp_spec_adapt {shape}, {mode}, out of place (2 reads + write)', ms[mode], 3.0*slab_bytes)
floor_ms = 1.5*copy_ms
print('ratios to the slab copy (2 R + 1 W floor: 1.5): ' + ', '.join(f'{m} {ms[m]/copy_ms:.2f}' for m in ms) +
      '; to that floor: ' + ', '.join(f'{m} {ms[m]/floor_ms:.2f}' for m in ms) +
      f'; spec_equalize / slab copy {eq_ms/copy_ms:.2f}', flush=True)
