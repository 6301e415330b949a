"""hipdsp_common_reference at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz = 57.6 M samples per
channel): mean and median, one group of 64 channels and four groups of 16, out of place and in place -- next to a
device-to-device copy of the same bytes and next to one hipdsp_unwrap pass over the same buffers (the project's
element-wise sweep along time: it reads the trace in its count pass and reads and writes it in its apply pass), both
measured in the same process on the same buffers.  Every figure: the fastest of ROUNDS rounds of N timed calls between two
device events (and the slowest round), in milliseconds and in effective GB/s over the 8 B per sample (4 read, 4
written) that a re-reference has to move.
    python tools/common_reference_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '5'))
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
dy = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
ctx.synchronize()
lines = []


def say(text):
    lines.append(text)
    print(text, flush=True)


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


def report(name, f, n=5):
    best, worst = timed(f, n)
    say(f'{name:78s} {best:9.3f} ms (slowest round {worst:9.3f}) {8.0*C*T/best/1e6:7.0f} GB/s')
    return best, worst


copy = report('device-to-device copy of the same bytes (hipdsp_memcpy_d2d; the yardstick)',
              lambda: h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(dy), h._p(dx), 4*C*T))
unwrap = report('hipdsp_unwrap, threshold 1.5: count pass + apply pass (the yardstick)',
                lambda: h.unwrap(ctx, dx, T, C, T, 1.5, dy, T))
one = [0]*C
four = [c//16 for c in range(C)]
results = {}
for mode in ('mean', 'median'):
    for gname, group in (('one group of 64', one), ('four groups of 16', four)):
        results[mode, gname, 'out of place'] = report(
            f'hipdsp_common_reference, {mode}, {gname}, out of place',
            lambda: h.common_reference(ctx, dx, T, dy, T, C, T, group, None, mode))
        # in place on the copy (a re-referenced trace re-referenced again: the same work)
        h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(dy), h._p(dx), 4*C*T)
        results[mode, gname, 'in place'] = report(
            f'hipdsp_common_reference, {mode}, {gname}, in place',
            lambda: h.common_reference(ctx, dy, T, dy, T, C, T, group, None, mode))
spread = max(worst/best for best, worst in [copy, unwrap] + list(results.values())) - 1.0
say(f'round-to-round spread: the slowest round of a line is up to {100*spread:.1f} % over its fastest')
for key, (best, worst) in results.items():
    say(f'    {", ".join(key):52s} = {best/copy[0]:.2f} copies = {best/unwrap[0]:.2f} unwrap passes')
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/common_reference_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
