"""hipdsp_bin_quantiles and hipdsp_spec_equalize, device resident, on the PSD slab of BASELINE configs[2] (64 ch x 600 s x
96 kHz, window 2048/1024: 64 x 56 250 x 1025 float32, 14.76 GB).
    python tools/noise_profile_bench.py [seconds=600]
Per line: median of 10 launches after 3 warm-ups (hipdsp_event_*), GB/s over the bytes the call actually reads (and
writes).  hipdsp_bin_quantiles at q = 0.5 reads the slab four times (one pass per 8-bit digit): on the noise slab as
hipdsp_spectrogram wrote it, and on the same slab quantised to 256 levels per channel (heavy ties: every column's values
meet in a few LDS counters; channel 0's values in every channel).  hipdsp_spec_equalize in both modes, out of place and
in place, reads and writes the slab once.  The yardsticks of the same process: one full-band hipdsp_band_power pass (the slab read once), one
device-to-device copy of the slab (hipdsp_memcpy_d2d) and hipdsp_copy_probe.  The ratios at the end are reported, not
gated.  The lines are in the format tools/entry_points_gate.py reads."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

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

nbytes = 1 << 31
a, b = h.DeviceArray(ctx, (nbytes,), np.uint8), h.DeviceArray(ctx, (nbytes,), np.uint8)
a.zero_()
probe_ms = median_ms(lambda: h.check(h.lib.hipdsp_copy_probe(ctx.handle, h._p(b), h._p(a), nbytes)))
report('hipdsp_copy_probe, 2048 MiB (read + write)', probe_ms, 2.0*nbytes)
a.free()
b.free()
copy_ms = median_ms(lambda: h.check(h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(do), h._p(ds), int(slab_bytes))))
report(f'hipdsp_memcpy_d2d of the slab {shape} (read + write)', copy_ms, 2.0*slab_bytes)
band = h.DeviceArray(ctx, (C, nd), np.float32)
band_ms = median_ms(lambda: h.band_power(ctx, ds, 0, C, nd, F, [(0, F)], rate/nfft, band))
report(f'hipdsp_band_power {shape}, full band (the slab read once)', band_ms, slab_bytes + 4.0*C*nd)
band.free()

lo_hi = h.DeviceArray(ctx, (C, F, 2), np.float32)
count = h.DeviceArray(ctx, (C, F), np.int32)
out_bytes = 12.0*C*F


def quantiles(spec, n_frames=nd, step=1):
    h.bin_quantiles(ctx, spec, 0, C, nd, F, 0, n_frames, step, 0, F, 0.5, lo_hi, count)


q_ms = median_ms(lambda: quantiles(ds))
report(f'hipdsp_bin_quantiles {shape}, q 0.5, noise slab (4 passes)', q_ms, 4.0*slab_bytes + out_bytes)
median = lo_hi.to_host()[:, :, 0]
assert np.all(count.to_host() == nd) and np.all(median >= 0)
q8_ms = median_ms(lambda: quantiles(ds, nd//8, 8))
report(f'hipdsp_bin_quantiles {shape}, q 0.5, every 8th frame (4 passes of rows 8 apart)', q8_ms,
       4.0*slab_bytes/8 + out_bytes)

# a slab quantised to 256 levels: channel 0's dB values over 100 dB, rounded on the host, as floats again, in every channel
h.decibel(ctx, ds, do, nd*F, 1.0, 1e-20)
ctx.synchronize()
one = do.view(0, (nd, F))
host = one.to_host()
host = np.clip(np.rint((host + 160.0)*(255.0/100.0)), 0, 255).astype(np.float32)
one.copy_from_host(host)
for c in range(1, C):
    h.check(h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(do.view(c*nd*F, (1,))), h._p(do), 4*nd*F))
ctx.synchronize()
levels = len(np.unique(host))
del host
t_ms = median_ms(lambda: quantiles(do))
report(f'hipdsp_bin_quantiles {shape}, q 0.5, quantised to 256 levels ({levels} in use; ties)', t_ms,
       4.0*slab_bytes + out_bytes)

prof = h.DeviceArray.from_host(ctx, np.maximum(median, np.float32(1e-20)).astype(np.float32))
eq = {}
for mode in ('divide', 'subtract'):
    eq[mode] = median_ms(lambda: h.spec_equalize(ctx, ds, 0, do, 0, C, nd, F, prof, 0, mode))
    report(f'hipdsp_spec_equalize {shape}, {mode}, out of place (read + write)', eq[mode], 2.0*slab_bytes)
h.check(h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(do), h._p(ds), int(slab_bytes)))
for mode in ('subtract', 'divide'):           # (subtract first: in place it leaves non-negative powers for the division)
    ms = median_ms(lambda: h.spec_equalize(ctx, do, 0, do, 0, C, nd, F, prof, 0, mode))
    report(f'hipdsp_spec_equalize {shape}, {mode}, in place (read + write)', ms, 2.0*slab_bytes)
    eq[mode + ' in place'] = ms

print(f'ratios: bin_quantiles / band_power pass {q_ms/band_ms:.2f} (floor 4: four reads of the slab), with ties '
      f'{t_ms/band_ms:.2f}; bin_quantiles / slab copy {q_ms/copy_ms:.2f}; spec_equalize divide / slab copy '
      f'{eq["divide"]/copy_ms:.2f}, subtract {eq["subtract"]/copy_ms:.2f}; in place {eq["divide in place"]/copy_ms:.2f}, '
      f'{eq["subtract in place"]/copy_ms:.2f}', flush=True)
