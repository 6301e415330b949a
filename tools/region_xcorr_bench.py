"""hipdsp_region_xcorr at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz) with ten events of 7 s per
channel (640 events, each at a position of its own) against 63 partner channels in ONE call.  The partner list belongs to
the call, not to the event, so it is channels 1 ... 63 for every event: the events of channel 0 meet the 63 other
channels, those of any other channel 62 others and themselves -- the same cost.  Three cases:
  (a) the band-passed trace at max_lag 96 (+-1 ms);
  (b) the power envelope at the envelope rate (step 19: 96 kHz / (10 x 500 Hz), songdetector.py:63-66) at max_lag 253
      (+-50 ms), the events' frames divided by 19;
  (c) case (a) at max_lag 0: what is left when the lags are gone (the fixed work per tile).
Next to them ONE hipdsp_region_stats pass over the same slab (the scale of a read-once reduction) and the chip's float64
FMA rate, measured in this process by a plain loop of independent FMAs (tools/fma_f64_probe.hip, built on first use).
Every figure: the fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in
milliseconds per call, in multiply-adds per second -- n (2 max_lag + 1) per event and partner, the definition's count; the
kernel's three sums per lag make three FMAs of each -- the share of the measured FMA rate those FMAs take, and the bytes the
call reads (each event window once per partner, each partner window once per tile of 2048 samples and its 2 max_lag more).
A table whose partial rows would not fit MAX_SCRATCH bytes of context scratch is split into calls, as
BufferedData.region_xcorr splits it; the time is that of all of them.
    python tools/region_xcorr_bench.py [seconds=600] [log file]"""
import ctypes, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.design import butter_sos

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '2'))
MAX_SCRATCH = int(os.environ.get('MAX_SCRATCH', str(4 << 30)))
EVENTS, LENGTH, STEP = 10, min(int(7*rate), T//10), 19
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
lines = []


def say(line):
    lines.append(line)
    print(line, flush=True)


def fma_rate():
    """float64 FMAs per second of this chip, or None when the probe cannot be built."""
    so = os.path.join(ROOT, 'tools', '_ab', 'libfma_f64_probe.so')
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
        if subprocess.call([hipcc, '-O3', '--offload-arch=gfx950', '-shared', '-fPIC',
                            os.path.join(ROOT, 'tools', 'fma_f64_probe.hip'), '-o', so]) != 0:
            return None
    lib = ctypes.CDLL(so)
    lib.fma_f64_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    got = ctypes.c_double(0.0)
    return got.value if lib.fma_f64_probe(4096, 32768, 5, ctypes.byref(got)) == 0 else None


peak = fma_rate()
say('float64 FMA rate of this chip, 16 independent v_fma_f64 per thread in a loop (tools/fma_f64_probe.hip): '
    + (f'{peak/1e12:.2f} T FMA/s' if peak else 'not run: no figure'))

dx = h.DeviceArray(ctx, (C, T), np.float32)
df = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.sosfilt(ctx, h.SosPlan(ctx, butter_sos(2, (300.0, 3000.0), 'bandpass', rate)), dx, T, df, T, C, T, 0)
n_env = -(-T//STEP)
de = h.DeviceArray(ctx, (C, n_env), np.float32)
h.power_envelope(ctx, h.SosPlan(ctx, butter_sos(1, 500.0, 'lowpass', rate)), df, T, C, T, de, n_env, 0, STEP, n_env, 4.0, True)
dx.free()
rng = np.random.default_rng(7)
# event k of a channel somewhere in the k-th tenth of the recording, at a start of its own
table = np.array([(c, k*(T//EVENTS) + int(rng.integers(0, T//EVENTS - LENGTH + 1)), 0) for c in range(C)
                  for k in range(EVENTS)], dtype=np.int64)
table[:, 2] = table[:, 1] + LENGTH
env_table = table.copy()
env_table[:, 1] = table[:, 1]//STEP
env_table[:, 2] = np.minimum(env_table[:, 1] + -(-LENGTH//STEP), n_env)
partners = list(range(1, C))
ctx.synchronize()


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


def groups(tab, L):
    """The table cut, in its order, into calls whose scratch stays under MAX_SCRATCH."""
    out, first = [], 0
    for i in range(1, len(tab) + 1):
        if i == len(tab) or h.region_xcorr_scratch(tab[first:i + 1], len(partners), L) > MAX_SCRATCH:
            out.append((first, i))
            first = i
    return out


for what, x, frames, tab, L in (('(a) band-passed trace, +-1 ms', df, T, table, 96),
                                ('(b) power envelope at step 19, +-50 ms', de, n_env, env_table, 253),
                                ('(c) band-passed trace, lag 0 only', df, T, table, 0)):
    W, P = 2*L + 1, len(partners)
    rows = h.DeviceArray(ctx, (len(tab), P, W), np.float32)
    info = h.DeviceArray(ctx, (len(tab), P, 4), np.float64)
    calls = groups(tab, L)

    def run():
        for a, b in calls:
            h.region_xcorr_into(ctx, x, frames, C, frames, tab[a:b], partners, L, rows.view(a*P*W, (1,)), info.view(a*P*4, (1,)))

    n = (tab[:, 2] - tab[:, 1]).astype(np.float64)
    macs = float(n.sum())*P*W
    tiles = np.ceil(n/h.XCORR_TILE)
    nbytes = 4.0*P*float((2*n + tiles*(W - 1)).sum())
    best, worst = timed(run, 1)
    share = f'{100.0*3*macs/(best*1e-3)/peak:5.1f} % of the FMA rate in 3 operations each' if peak else 'no FMA rate: no share'
    say(f'{what}: {len(tab)} events of {int(n[0])} samples x {P} partners, max_lag {L}, {len(calls)} call(s)'.ljust(104)
        + f' {best:10.3f} ms (slowest round {worst:10.3f}) {macs/(best*1e-3)/1e12:7.3f} T multiply-adds/s, {share}, '
        f'{nbytes/1e9:.2f} GB read = {nbytes/best/1e6:.0f} GB/s')
    rows.free()
    info.free()

stats = h.DeviceArray(ctx, (1, C, 8), np.float64)
best, worst = timed(lambda: h.region_stats(ctx, df, T, C, T, [(0, T)], out=stats), 5)
say(f'hipdsp_region_stats, the whole band-passed buffer as one region'.ljust(104)
    + f' {best:10.3f} ms (slowest round {worst:10.3f}) {4.0*C*T/best/1e6:7.0f} GB/s')
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/region_xcorr_bench.py: {C} ch x {T} samples, {EVENTS} events of {LENGTH} samples per channel, '
                f'{len(partners)} partners, ROUNDS={ROUNDS}, MAX_SCRATCH={MAX_SCRATCH}\n' + '\n'.join(lines) + '\n')
