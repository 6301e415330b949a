"""hipdsp_find_peaks at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz = 57.6 M samples per channel), next
to ONE hipdsp_region_stats pass (the project's read-once reduction: the yardstick) and ONE hipdsp_detect_events pass over
the same slab, measured on the same card in the same minute.  Three cases:
  (a) the envelope of the synthetic recording's band-passed trace, a height border (mean + std per channel, from the
      region_stats call) and a prominence border (std): the smooth trace a detector looks at;
  (b) white noise, all borders open, counts only (capacity 0): the pure scan -- a peak at every third sample, no search,
      no min/max table;
  (c) white noise with a closed prominence border and no wlen: the worst realistic search load, a search for every
      third sample (counts only: the positions of 64 x 19 M peaks would be 10 GB).
Every figure: the fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in
milliseconds, in effective GB/s = 4 B x samples / time and as a multiple of the region_stats pass.
    python tools/peaks_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.design import butter_sos

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '5'))
CAP = 1 << 16
INF = np.inf
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
df = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.sosfilt_envelope(ctx, h.SosPlan(ctx, butter_sos(2, (300.0, 3000.0), 'bandpass', rate)),
                   h.SosPlan(ctx, butter_sos(2, 200.0, 'lowpass', rate)), dx, T, df, T, de, T, C, T)
df.free()
stats = h.DeviceArray(ctx, (1, C, 8), np.float64)
host = h.region_stats(ctx, de, T, C, T, [(0, T)])[0]
dthr = h.DeviceArray.from_host(ctx, (host[:, 1] + host[:, 2]).astype(np.float32))
borders = np.tile(np.array([-INF, INF]*3), (C, 1))
borders[:, 0], borders[:, 4] = host[:, 1] + host[:, 2], host[:, 2]
dborders = h.DeviceArray.from_host(ctx, borders)
peaks = h.DeviceArray(ctx, (C, CAP), np.int64)
props = h.DeviceArray(ctx, (C, CAP, 4), np.float64)
events = h.DeviceArray(ctx, (C, CAP, 2), np.int64)
counts = h.DeviceArray(ctx, (C,), np.int64)
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
        rounds.append(ctx.elapsed_ms(e0, e1)/n)
    return min(rounds), max(rounds)


def report(name, f, n, note='', base=None):
    best, worst = timed(f, n)
    lines.append(f'{name:78s} {best:9.3f} ms (slowest round {worst:9.3f}) {4.0*C*T/best/1e6:7.0f} GB/s{note}')
    print(lines[-1], flush=True)
    if base:
        lines.append(f'    = {best/base:.2f} region_stats passes')
        print(lines[-1], flush=True)
    return best


def find(x, b, wlen, cap):
    h.find_peaks_into(ctx, x, T, C, 0, T, b, wlen, cap, peaks if cap else None, props if cap else None, counts)


def found():
    n = counts.to_host()
    return f'  {int(n.sum())} peaks, at most {int(n.max())} per channel'


base = report('hipdsp_region_stats, the whole buffer as one region (the yardstick)',
              lambda: h.region_stats(ctx, de, T, C, T, [(0, T)], out=stats), 5)
report('hipdsp_detect_events, envelope > mean + std, min_gap 0.1 s, min_len 0.01 s',
       lambda: h.detect_events_into(ctx, de, T, C, 0, T, dthr, 9600, 960, CAP, events, counts), 5, base=base)
find(de, dborders, 0, CAP)
report('(a) hipdsp_find_peaks, envelope, height >= mean + std, prominence >= std', lambda: find(de, dborders, 0, CAP), 5,
       found(), base)
find(de, dborders, 0, 0)
report('(a) the same, counts only (capacity 0)', lambda: find(de, dborders, 0, 0), 5, found(), base)
# white noise: 4 M normal samples uploaded once and copied along every row, each row at a shift of its own
rng = np.random.default_rng(5)
de.free()
block = 1 << 22
dnoise = h.DeviceArray.from_host(ctx, rng.standard_normal(block + C).astype(np.float32))
for c in range(C):
    for k in range(0, T, block):
        n = min(block, T - k)
        h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(dx.view(c*T + k, (1,))), h._p(dnoise.view(c, (1,))), 4*n)
ctx.synchronize()
open6 = [-INF, INF]*3
find(dx, open6, 0, 0)
report('(b) hipdsp_find_peaks, white noise, all borders open, counts only: the scan', lambda: find(dx, open6, 0, 0), 5,
       found(), base)
closed = [-INF, INF, -INF, INF, 1.0, INF]
find(dx, closed, 0, 0)
report('(c) hipdsp_find_peaks, white noise, prominence >= 1, no wlen, counts only', lambda: find(dx, closed, 0, 0), 3,
       found(), base)
find(dx, closed, 9600, 0)
report('(c) the same with wlen 0.1 s', lambda: find(dx, closed, 9600, 0), 3, found(), base)
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/peaks_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
