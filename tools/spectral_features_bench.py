"""hipdsp_spectral_features, device resident, on BASELINE configs[2]'s PSD slab (64 ch x 600 s x 96 kHz at 2048/1024:
64 x 56 250 x 1025), next to hipdsp_band_power over the same band of the same slab in the same process:
    python tools/spectral_features_bench.py [seconds=600]
three calls -- the peak alone (bits 0-2) and all eight features over the full band, all eight over a 1/8 band -- each
followed by the band-power pass over the same bins.  Per line: median of 10 launches after 3 warm-ups (hipdsp_event_*),
GB/s over the band's bytes (band bins x 4 B + output x 4 B), in the format tools/entry_points_gate.py reads; behind
each pair the ratio of the two times."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

C, rate, nfft, hop = 64, 96000.0, 2048, 1024
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
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


dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
ds = h.DeviceArray(ctx, (C, nd, F), np.float32)
h.spectrogram(ctx, dx, T, C, T, nfft, hop, rate, ds, nd)
ctx.synchronize()
dx.free()
out = h.DeviceArray(ctx, (8, C, nd), np.float32)
where = f'{nfft}/{hop} slab (64 x {nd} x {F})'
for name, mask, (k0, k1) in (('peak only (bits 0-2), full band', 0x07, (0, F)), ('all eight features, full band', 0xFF, (0, F)),
                             ('all eight features, 1/8 band', 0xFF, (F//3, F//3 + F//8))):
    ms = median_ms(lambda: h.spectral_features(ctx, ds, 0, C, nd, F, k0, k1, mask, rate/nfft, out, min_power=1e-20))
    nbytes = 4.0*C*nd*(k1 - k0 + bin(mask).count('1'))
    print(f'{f"hipdsp_spectral_features {where}, {name}":78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s', flush=True)
    bp = median_ms(lambda: h.band_power(ctx, ds, 0, C, nd, F, [(k0, k1)], rate/nfft, out))
    nbytes = 4.0*C*nd*(k1 - k0 + 1)
    print(f'{f"hipdsp_band_power {where}, bins [{k0}, {k1})":78s} {bp:8.3f} ms {nbytes/bp/1e6:7.0f} GB/s', flush=True)
    print(f'    spectral features / band power over the same bins: {ms/bp:.2f}', flush=True)
out.free()
ds.free()
