"""hipdsp_detect_events at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz = 57.6 M samples per channel):
the envelope of the synthetic recording's band-passed trace against mean + std per channel (thresholds from one
hipdsp_region_stats call), min_gap 0 and 0.1 s, min_len 0 and 0.01 s -- next to ONE hipdsp_region_stats pass over the
same slab (the project's read-once reduction: the yardstick, measured on the same card in the same minute) and, for the
worst case of the later passes, a trace of alternating samples (every second sample an event).  Every figure: the
fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in milliseconds and in
effective GB/s = 4 B x samples / time.
    python tools/events_bench.py [seconds=600] [log file]"""
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
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
df = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.sosfilt_envelope(ctx, h.SosPlan(ctx, butter_sos(2, (300.0, 3000.0), 'bandpass', rate)),
                   h.SosPlan(ctx, butter_sos(2, 200.0, 'lowpass', rate)), dx, T, df, T, de, T, C, T)
stats = h.DeviceArray(ctx, (1, C, 8), np.float64)
host = h.region_stats(ctx, de, T, C, T, [(0, T)])[0]
dthr = h.DeviceArray.from_host(ctx, (host[:, 1] + host[:, 2]).astype(np.float32))
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


def report(name, f, n, note=''):
    best, worst = timed(f, n)
    lines.append(f'{name:78s} {best:9.3f} ms (slowest round {worst:9.3f}) {4.0*C*T/best/1e6:7.0f} GB/s{note}')
    print(lines[-1], flush=True)
    return best


def detect(x, thr, gap, length, cap=CAP):
    h.detect_events_into(ctx, x, T, C, 0, T, thr, gap, length, cap, events if cap else None, counts)


base = report('hipdsp_region_stats, the whole buffer as one region (the yardstick)',
              lambda: h.region_stats(ctx, de, T, C, T, [(0, T)], out=stats), 5)
for gap_s, len_s in ((0.0, 0.0), (0.1, 0.0), (0.1, 0.01)):
    gap, length = int(gap_s*rate), int(len_s*rate)
    detect(de, dthr, gap, length)
    found = counts.to_host()
    ms = report(f'hipdsp_detect_events, envelope > mean + std, min_gap {gap_s} s, min_len {len_s} s', lambda: detect(de, dthr, gap, length), 5,
                f'  {int(found.sum())} events, at most {int(found.max())} per channel')
    lines.append(f'    = {ms/base:.2f} region_stats passes')
    print(lines[-1], flush=True)
ms = report('hipdsp_detect_events, the same with min_gap 0.1 s, counts only (capacity 0)', lambda: detect(de, dthr, int(0.1*rate), 0, 0), 5)
# the worst case of the passes over the bits: every second sample above, 32 events per 64-bit word (counts only: the
# pairs of 64 x 28.8 M events would be 29 GB)
df.free()
alt = np.zeros(2, dtype=np.float32)
alt[0] = 1.0
dalt = h.DeviceArray.from_host(ctx, np.tile(alt, 1 << 20))
for c in range(C):
    for k in range(0, T, 1 << 21):
        n = min(1 << 21, T - k)
        h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(dx.view(c*T + k, (1,))), h._p(dalt), 4*n)
ctx.synchronize()
report('hipdsp_detect_events, alternating samples, min_gap 0, counts only', lambda: detect(dx, 0.5, 0, 0, 0), 3)
report('hipdsp_detect_events, alternating samples, min_gap 0.1 s (one event), counts only', lambda: detect(dx, 0.5, int(0.1*rate), 0, 0), 3)
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/events_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
