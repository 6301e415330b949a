"""hipdsp_histogram (49 bins) and hipdsp_masked_stats at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz =
57.6 M samples per channel), on two slabs: uniform samples in [0, 1) (every bin equally full: the lanes of a wave
spread over the bins) and the envelope of the synthetic recording's band-passed trace (the noise floor puts most
samples into one or two bins: the contention case the ballot rounds of hg_count_kernel are for) -- next to ONE
hipdsp_region_stats pass over the same slab (the project's read-once reduction: the yardstick, measured on the same card
in the same process) and next to the whole four-pass BufferedData.threshold_estimates on the envelope (region_stats,
histogram, two masked_stats, with their read-backs and the host bookkeeping: wall time).  Every kernel figure: the
fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in milliseconds and in
effective GB/s = 4 B x samples / time.
    python tools/histogram_bench.py [seconds=600] [log file]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.buffereddata import BufferedData
from audian_amd.design import butter_sos

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '5'))
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
df = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.sosfilt_envelope(ctx, h.SosPlan(ctx, butter_sos(2, (300.0, 3000.0), 'bandpass', rate)),
                   h.SosPlan(ctx, butter_sos(2, 200.0, 'lowpass', rate)), dx, T, df, T, de, T, C, T)
ctx.synchronize()
df.free()
# the uniform slab: one tile of 2^21 uniform samples, repeated along every channel (over the raw recording)
tile = h.DeviceArray.from_host(ctx, np.random.default_rng(5).random(1 << 21, dtype=np.float32))
for c in range(C):
    for k in range(0, T, 1 << 21):
        n = min(1 << 21, T - k)
        h.lib.hipdsp_memcpy_d2d(ctx.handle, h._p(dx.view(c*T + k, (1,))), h._p(tile), 4*n)
ctx.synchronize()
du = dx
stats = h.DeviceArray(ctx, (1, C, 8), np.float64)
counts = h.DeviceArray(ctx, (C, 52), np.int64)
moments = h.DeviceArray(ctx, (C, 4), np.float64)
env = h.region_stats(ctx, de, T, C, T, [(0, T)])[0]
maxe = float(env[:, 4].max())
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


def report(name, f, n, base=None):
    best, worst = timed(f, n)
    ratio = '' if base is None else f'  = {best/base:.2f} region_stats passes'
    say(f'{name:78s} {best:9.3f} ms (slowest round {worst:9.3f}) {4.0*C*T/best/1e6:7.0f} GB/s{ratio}')
    return best


def bounds_of(lo, hi, pivot):
    return h.DeviceArray.from_host(ctx, np.tile([lo, hi, pivot], (C, 1)))


results = {}
for slab, x, top in (('uniform samples', du, 1.0), ('the envelope', de, maxe)):
    edges = np.linspace(0.0, top, 50)
    base = report(f'hipdsp_region_stats, {slab}, the whole buffer as one region (the yardstick)',
                  lambda: h.region_stats(ctx, x, T, C, T, [(0, T)], out=stats), 5)
    hist = h.histogram(ctx, x, T, C, 0, T, edges)
    full = hist[:, :49].max(axis=1)/float(T)
    say(f'    {slab}: the fullest of the 49 bins holds {100*full.min():.1f} ... {100*full.max():.1f} % of a channel\'s samples')
    cut = float(edges[min(2*int(np.argmax(hist[0, :49])) + 2, 49)])       # a cut as threshold_estimates places it
    below, above = bounds_of(-np.inf, cut, cut), bounds_of(cut, np.inf, cut)
    results[slab] = (
        base,
        report(f'hipdsp_histogram, {slab}, 49 bins', lambda: h.histogram(ctx, x, T, C, 0, T, edges, out=counts), 5, base),
        report(f'hipdsp_masked_stats, {slab}, the samples below {cut:.4g}',
               lambda: h.masked_stats(ctx, x, T, C, 0, T, below, out=moments), 5, base),
        report(f'hipdsp_masked_stats, {slab}, the samples above {cut:.4g}',
               lambda: h.masked_stats(ctx, x, T, C, 0, T, above, out=moments), 5, base))
say(f'hipdsp_histogram, the envelope against uniform samples: {results["the envelope"][1]/results["uniform samples"][1]:.2f} x')


class Resident(BufferedData):
    """The envelope slab as a trace whose device mirror is valid everywhere and whose host copy was never filled."""

    def __init__(self, dev):
        super().__init__('envelope', 'data')
        self.channels, self.rate, self.frames, self.shape, self.offset = C, rate, T, (T, C), 0
        self._hostbuf = np.broadcast_to(np.zeros((1, C)), (T, C))
        self._dev, self._alias_pitch, self._dev_valid, self._stale, self._ctx = dev, T, [[0, T]], [[0, T]], ctx


trace = Resident(de)
trace.threshold_estimates()
walls = []
for _ in range(ROUNDS):
    ctx.synchronize()
    t0 = time.perf_counter()
    thr = trace.threshold_estimates()
    walls.append((time.perf_counter() - t0)*1e3)
base = results['the envelope'][0]
say(f'{"BufferedData.threshold_estimates, the envelope, four passes with read-backs (wall)":78s} {min(walls):9.3f} ms '
    f'(slowest round {max(walls):9.3f})  = {min(walls)/base:.2f} region_stats passes')
say(f'    thresholds {thr.min():.4g} ... {thr.max():.4g} of a maximum of {maxe:.4g}')
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/histogram_bench.py: {C} ch x {T} samples, ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
