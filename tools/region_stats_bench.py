"""hipdsp_region_stats at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz = 57.6 M samples per channel):
the whole buffer as one region, 16 regions of 1 s, and one channel x 1 s -- next to hipdsp_minmax_decimate over the
same ranges (the other read-once reduction over a trace: screen decimation to 2000 points) and hipdsp_copy_probe, all
in this one process on the same device buffer.  Every figure: the fastest of ROUNDS rounds of N timed calls between
two device events (and the slowest round, the spread), in microseconds and in GB/s of bytes READ (the copy: read +
written).
    python tools/region_stats_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '5'))
sec = int(rate)
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
ncopy = (C*T//4)//4*4
dcopy = h.DeviceArray(ctx, (ncopy,), np.float32)
stats = h.DeviceArray(ctx, (16, C, 8), np.float64)
mm = h.DeviceArray(ctx, (C, 2*2000 + 2), np.float32)
ctx.synchronize()
lines = []


def timed(f, n):
    f(); f()
    rounds = []
    for _ in range(ROUNDS):
        ctx.record(e0)
        for _ in range(n):
            f()
        ctx.record(e1)
        ctx.synchronize()
        rounds.append(ctx.elapsed_ms(e0, e1)/n*1e3)
    return min(rounds), max(rounds)


def report(name, f, nbytes, n):
    best, worst = timed(f, n)
    lines.append(f'{name:86s} {best:11.1f} us (slowest round {worst:11.1f}) {nbytes/best/1e3:7.0f} GB/s')
    print(lines[-1], flush=True)


def minmax(channels, spans):
    for a, b in spans:
        step = max(1, (b - a)//2000)
        h.minmax_decimate(ctx, dx, T, channels, a, b, step, mm, 2*2000 + 2)


whole = [(0, T)]
sixteen = [(k*(T - sec)//15, k*(T - sec)//15 + sec) for k in range(16)]     # spread over the buffer, any 4-byte phase
one = [(T//3 + 1, T//3 + 1 + sec)]
report('hipdsp_region_stats, the whole buffer as one region, 64 ch', lambda: h.region_stats(ctx, dx, T, C, T, whole, out=stats), 4.0*C*T, 5)
report('hipdsp_minmax_decimate, the whole buffer to 2000 points, 64 ch', lambda: minmax(C, whole), 4.0*C*T, 5)
report('hipdsp_region_stats, 16 regions of 1 s in one call, 64 ch', lambda: h.region_stats(ctx, dx, T, C, T, sixteen, out=stats), 4.0*C*16*sec, 50)
report('hipdsp_minmax_decimate, the same 16 ranges to 2000 points each (16 calls), 64 ch', lambda: minmax(C, sixteen), 4.0*C*16*sec, 50)
report('hipdsp_region_stats, one region of 1 s, 64 ch', lambda: h.region_stats(ctx, dx, T, C, T, one, out=stats), 4.0*C*sec, 200)
report('hipdsp_minmax_decimate, the same range to 2000 points, 64 ch', lambda: minmax(C, one), 4.0*C*sec, 200)
report('hipdsp_region_stats, one region of 1 s, 1 ch', lambda: h.region_stats(ctx, dx, T, 1, T, one, out=stats), 4.0*sec, 200)
report('hipdsp_minmax_decimate, the same range to 2000 points, 1 ch', lambda: minmax(1, one), 4.0*sec, 200)
report('hipdsp_copy_probe over a quarter of the buffer (bytes read + written)', lambda: h.lib.hipdsp_copy_probe(ctx.handle, h._p(dcopy), h._p(dx), 4*ncopy), 8.0*ncopy, 10)
# what the user waits for: the call with its 64 B per region and channel read back
import time
t0 = time.perf_counter()
for _ in range(20):
    res = h.region_stats(ctx, dx, T, C, T, one)
us = (time.perf_counter() - t0)/20*1e6
lines.append(f'{"hipdsp.region_stats with the read-back of (1, 64, 8) doubles, host clock, one region of 1 s":86s} {us:11.1f} us')
print(lines[-1], flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/region_stats_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
