"""hipdsp_fir_bank, device resident: L in {9, 65, 257, 1025, 4097} taps x K in {1, 16} kernels x step in {1, 96} at
64 ch x 60 s x 96 kHz, and one line at BASELINE configs[2]'s full length (64 ch x 600 s x 96 kHz) for L = 257, K = 16,
step = 96.
    python tools/fir_bank_bench.py [seconds=60] [full_seconds=600]
Per line: median of the timed launches after the warm-ups (hipdsp_event_*; 10 after 3, 3 after 1 once a launch takes more
than 100 ms), TFLOP/s over the work the matrix core does (2 * 16 * L per output and channel: the kernel axis is always
padded to 16) and over the useful part of it (the true K), GB/s over the algorithmic bytes (every sample read once, every
output written once: 4 B + 4 K / step B per sample), next to the same run's hipdsp_copy_probe rate.  The lines are in
the format tools/entry_points_gate.py reads.  --pmc: nothing but one launch each of (L, step) = (9, 1), (257, 1), (257, 96),
(257, 1000) with 16 kernels on 64 ch x 10 s, for a counter run of its own (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT
SQ_LDS_IDX_ACTIVE, the program after `--`): the LDS layouts of the three mappings."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

args = [a for a in sys.argv[1:] if not a.startswith('--')]
C, rate = 64, 96000.0
T = int((float(args[0]) if args else 60.0)*rate)
T_full = int((float(args[1]) if len(args) > 1 else 600.0)*rate)
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()


def once(f):
    ctx.record(e0)
    f()
    ctx.record(e1)
    ctx.synchronize()
    return ctx.elapsed_ms(e0, e1)


def median_ms(f):
    first = once(f)
    n, warm = (3, 0) if first > 100.0 else (10, 2)
    for _ in range(warm):
        f()
    return float(np.median([once(f) for _ in range(n)]))


if '--pmc' in sys.argv:
    Tp = int(10*rate)
    dx = h.DeviceArray(ctx, (C, Tp), np.float32)
    h.synth(ctx, dx, Tp, C, Tp, rate, 1)
    out = h.DeviceArray(ctx, (16, C, Tp), np.float32)
    for L, step in ((9, 1), (257, 1), (257, 96), (257, 1000)):
        plan = h.FirPlan(ctx, np.random.default_rng(1).standard_normal((16, L)))
        h.fir_bank(ctx, plan, dx, Tp, C, Tp, 0, step, -(-Tp//step), out)
        ctx.synchronize()
        plan.close()
    sys.exit(0)

nbytes = 1 << 31
a, b = h.DeviceArray(ctx, (nbytes,), np.uint8), h.DeviceArray(ctx, (nbytes,), np.uint8)
a.zero_()
copy_ms = median_ms(lambda: h.check(h.lib.hipdsp_copy_probe(ctx.handle, h._p(b), h._p(a), nbytes)))
copy_rate = 2.0*nbytes/copy_ms/1e6
a.free()
b.free()
print(f'{"hipdsp_copy_probe, %d MiB (read + write)" % (nbytes >> 20):78s} {copy_ms:8.3f} ms {copy_rate:7.0f} GB/s', flush=True)

rng = np.random.default_rng(7)


def bench(frames, L, K, step, dx, out):
    n_out = -(-frames//step)
    plan = h.FirPlan(ctx, rng.standard_normal((K, L))/np.sqrt(L))
    ms = median_ms(lambda: h.fir_bank(ctx, plan, dx, frames, C, frames, 0, step, n_out, out))
    plan.close()
    padded = 2.0*16*L*C*n_out
    moved = 4.0*C*frames + 4.0*K*C*n_out
    name = f'hipdsp_fir_bank 64 x {frames}, L {L}, K {K}, step {step}'
    print(f'{name:78s} {ms:8.3f} ms {moved/ms/1e6:7.0f} GB/s', flush=True)
    print(f'    matrix core {padded/ms/1e9:.1f} TFLOP/s (16 columns), useful {padded*K/16/ms/1e9:.1f} TFLOP/s (K = {K}); '
          f'{moved/1e9:.3f} GB algorithmic; copy probe {copy_rate:.0f} GB/s', flush=True)


dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
out = h.DeviceArray(ctx, (16, C, T), np.float32)
for step in (1, 96):
    for L in (9, 65, 257, 1025, 4097):
        for K in (1, 16):
            bench(T, L, K, step, dx, out)
out.free()
dx.free()
if T_full > 0:
    dx = h.DeviceArray(ctx, (C, T_full), np.float32)
    h.synth(ctx, dx, T_full, C, T_full, rate, 1236)
    out = h.DeviceArray(ctx, (16, C, -(-T_full//96)), np.float32)
    bench(T_full, 257, 16, 96, dx, out)
