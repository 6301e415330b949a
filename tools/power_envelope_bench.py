"""hipdsp_power_envelope at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz): the song detector's envelope
(first-order low-pass of the squares at 500 Hz, every 19th sample, clamp and root) in one call, next to the only route
the library had for an envelope at the envelope rate, measured in the same process on the same buffers: ONE
hipdsp_envelope(rectify = 1) over the slab into a full-rate buffer plus ONE hipdsp_stride_copy per channel.  (That route
computes another quantity -- pi/2 |x| filtered, no root -- it is what a user had to substitute; the comparison is of the
work, not of the values.)
Every figure: the fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in
milliseconds per call and GB/s over the algorithmic bytes (new: 12 B per sample read, 4 B per output written; old: 12 B
per sample for the envelope, then 4 B read and 4 B written per output), and the context scratch the new call takes.
    python tools/power_envelope_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.bufferedpowerenvelope import power_envelope_step
from audian_amd.design import butter_sos

C, rate, cutoff = 64, 96000.0, 500.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '3'))
step = power_envelope_step(rate, cutoff)
n_out = -(-T//step)
S = C*T
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
dy = h.DeviceArray(ctx, (C, n_out), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
lp1 = h.SosPlan(ctx, butter_sos(1, cutoff, 'lowpass', rate))
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


def report(name, f, n, nbytes, base=None):
    best, worst = timed(f, n)
    lines.append(f'{name:96s} {best:9.3f} ms (slowest round {worst:9.3f}) {nbytes/best/1e6:7.0f} GB/s')
    if base:
        lines[-1] += f'  = {best/base:.2f} x the one call'
    print(lines[-1], flush=True)
    return best


def one_call():
    h.power_envelope(ctx, lp1, dx, T, C, T, dy, n_out, 0, step, n_out, 4.0, True)


def old_route():
    h.envelope(ctx, lp1, dx, T, de, T, C, T, 0, rectify=True)
    for c in range(C):
        h.stride_copy(ctx, de.view(c*T, (T,)), T, step, dy.view(c*n_out, (n_out,)))


new = report(f'hipdsp_power_envelope, {C} ch x {T} samples, low-pass of 1 section at {cutoff:g} Hz, step {step}, root',
             one_call, 3, 12.0*S + 4.0*C*n_out)
report(f'hipdsp_envelope(rectify = 1) into a full-rate buffer + {C} x hipdsp_stride_copy, step {step}', old_route, 3,
       12.0*S + 8.0*C*n_out, new)
scratch = h.power_envelope_scratch(C, T, 1, 6)
lines.append(f'context scratch of the new call: {scratch/1e6:.1f} MB = {scratch/S:.3f} B per sample; written: {4.0*C*n_out/1e9:.2f} GB '
             f'instead of {4.0*S/1e9:.2f} GB at full rate')
print(lines[-1], flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/power_envelope_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
