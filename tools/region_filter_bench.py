"""hipdsp_region_filtfilt and hipdsp_region_crossings at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz)
with ten events of 5 s per channel, each widened by 1 s on both sides (640 regions of 7 s, each at a position and with a
first-order low-pass of its own, cut-offs 40 ... 400 Hz), next to the only routes the library had before, measured in
the same process on the same buffers:
  filter     ONE hipdsp_sosplan_set plus ONE one-channel hipdsp_envelope(rectify = 0) per event -- 640 plans, 640 calls;
  crossings  hipdsp_region_stats over the same windows, 16 regions per call, every region on every channel -- 40 calls
             (it has no count and no first / last sample above: the maxima are all it can give).
Every figure: the fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in
milliseconds per call (all 640 regions) and in GB/s over the bytes of the regions (4 B x their samples).  The outputs of
the two filter routes are compared before they are timed (largest difference over largest value).
    python tools/region_filter_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.design import butter_sos

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '3'))
EVENTS = 10
LENGTH = min(int(7*rate), T//EVENTS)                   # 5 s widened by 1 s on both sides
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
dy = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.envelope(ctx, h.SosPlan(ctx, butter_sos(2, 500.0, 'lowpass', rate)), dx, T, de, T, C, T)
dx.free()
rng = np.random.default_rng(7)
# region k of a channel somewhere in the k-th tenth of the recording, at a start of its own
table = np.array([(c, k*(T//EVENTS) + int(rng.integers(0, T//EVENTS - LENGTH + 1)), 0) for c in range(C)
                  for k in range(EVENTS)], dtype=np.int64)
table[:, 2] = table[:, 1] + LENGTH
cuts = np.linspace(40.0, 400.0, len(table))
sos = np.array([butter_sos(1, f, 'lowpass', rate) for f in cuts])
nbytes = 4.0*len(table)*LENGTH
ctx.synchronize()
lines = []


def timed(f, n):
    f()
    rounds = []
    for _ in range(ROUNDS):
        ctx.record(e0)
        for _ in range(n):
            f()
        ctx.record(e1)
        ctx.synchronize()
        rounds.append(ctx.elapsed_ms(e0, e1)/n)
    return min(rounds), max(rounds)


def report(name, f, n, base=None):
    best, worst = timed(f, n)
    lines.append(f'{name:96s} {best:9.3f} ms (slowest round {worst:9.3f}) {nbytes/best/1e6:7.0f} GB/s')
    if base:
        lines[-1] += f'  = {best/base:.1f} x the one call'
    print(lines[-1], flush=True)
    return best


def one_call():
    h.region_filtfilt(ctx, de, T, dy, T, C, T, table, sos)


plan = h.SosPlan(ctx, sos[0])


def old_route():
    for (c, a, b), s in zip(table.tolist(), sos):
        plan.set(s)
        h.envelope(ctx, plan, de.view(c*T + a, (LENGTH,)), LENGTH, dy.view(c*T + a, (LENGTH,)), LENGTH, 1, LENGTH,
                   rectify=False, clamp=False)


one_call()
new = [dy.view(c*T + a, (LENGTH,)).to_host() for c, a, b in table[::97].tolist()]
old_route()
old = [dy.view(c*T + a, (LENGTH,)).to_host() for c, a, b in table[::97].tolist()]
worst = max(float(np.max(np.abs(p - q))/np.max(np.abs(q))) for p, q in zip(new, old))
lines.append(f'outputs of the two filter routes, {len(new)} regions: largest difference {worst:.3g} of the largest value')
print(lines[-1], flush=True)
one = report(f'hipdsp_region_filtfilt, {len(table)} regions of {LENGTH} samples, order 1, 40-400 Hz', one_call, 3)
report('the same regions one by one, hipdsp_sosplan_set + one-channel hipdsp_envelope(rectify = 0)', old_route, 1, one)

thr = np.full(len(table), 0.5)
out = h.DeviceArray(ctx, (len(table), 8), np.float64)
one = report(f'hipdsp_region_crossings, the same {len(table)} regions, one threshold each',
             lambda: h.region_crossings(ctx, de, T, C, T, table, thr, out=out), 5)
stats = h.DeviceArray(ctx, (16, C, 8), np.float64)


def stats_route():
    for k in range(0, len(table), 16):
        h.region_stats(ctx, de, T, C, T, [(a, b) for c, a, b in table[k:k + 16].tolist()], out=stats)


report('hipdsp_region_stats over the same windows, 16 per call, every window on all 64 channels', stats_route, 1, one)
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/region_filter_bench.py: {C} ch x {T} samples, {EVENTS} regions of {LENGTH} samples per channel, '
                f'ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
