"""hipdsp_region_spectra at BASELINE configs[2]'s resident buffer (64 ch x 600 s x 96 kHz) with ten events of 5 s per
channel (640 events, each at a position of its own), next to the only route the library had for the spectrum of an event
before: ONE hipdsp_spectrogram over the event's samples (every frame's spectrum written to HBM) plus ONE
hipdsp_mean_spectrum_db (which reads them back) per event and channel -- 1280 launches -- measured in the same process on
the same buffers.  Two cases:
  (a) nfft 1024 / hop 512, step 1 on the band-passed trace: the carrier of every call;
  (b) nfft 4096 / hop 2048, step 19 on the envelope (96 kHz / (10 x 500 Hz cut-off) = 19, the reference's envrate,
      songdetector.py:63-66): the pulse rate of every song.  The old route has no step: it gets the event decimated by
      hipdsp_stride_copy first, one more launch per event and channel.
Every figure: the fastest of ROUNDS rounds of N timed calls between two device events (and the slowest round), in
milliseconds per call (all 640 events) and in GB/s over the bytes of the regions (4 B x their samples, whatever the step).
    python tools/region_spectra_bench.py [seconds=600] [log file]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h
from audian_amd.design import butter_sos

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
ROUNDS = int(os.environ.get('ROUNDS', '3'))
EVENTS, LENGTH = 10, min(int(5*rate), T//10)
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
dx = h.DeviceArray(ctx, (C, T), np.float32)
df = h.DeviceArray(ctx, (C, T), np.float32)
de = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
h.sosfilt_envelope(ctx, h.SosPlan(ctx, butter_sos(2, (300.0, 3000.0), 'bandpass', rate)),
                   h.SosPlan(ctx, butter_sos(2, 500.0, 'lowpass', rate)), dx, T, df, T, de, T, C, T)
dx.free()
rng = np.random.default_rng(7)
# event k of a channel somewhere in the k-th tenth of the recording, at a start of its own
table = np.array([(c, k*(T//EVENTS) + int(rng.integers(0, T//EVENTS - LENGTH + 1)), 0) for c in range(C)
                  for k in range(EVENTS)], dtype=np.int64)
table[:, 2] = table[:, 1] + LENGTH
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
    lines.append(f'{name:88s} {best:9.3f} ms (slowest round {worst:9.3f}) {nbytes/best/1e6:7.0f} GB/s')
    if base:
        lines[-1] += f'  = {best/base:.1f} x the one call'
    print(lines[-1], flush=True)
    return best


for what, x, nfft, hop, step in (('(a) band-passed trace', df, 1024, 512, 1), ('(b) envelope', de, 4096, 2048, 19)):
    F = nfft//2 + 1
    rows = h.DeviceArray(ctx, (len(table), F), np.float32)
    info = h.DeviceArray(ctx, (len(table), 2), np.int64)
    one = report(f'{what}: hipdsp_region_spectra, {len(table)} events of {LENGTH} samples, {nfft}/{hop}, step {step}',
                 lambda: h.region_spectra_into(ctx, x, T, C, T, table, nfft, hop, step, rate/step, rows, info), 5)
    n_dec = -(-LENGTH//step)
    frames = (n_dec - nfft)//hop + 1
    spec = h.DeviceArray(ctx, (frames, F), np.float32)
    dec = h.DeviceArray(ctx, (n_dec,), np.float32)
    mean_db = h.DeviceArray(ctx, (len(table), F), np.float32)

    def old_route():
        for i, (c, a, b) in enumerate(table.tolist()):
            src = x.view(c*T + a, (LENGTH,))
            if step > 1:
                h.stride_copy(ctx, src, LENGTH, step, dec)
                src = dec
            h.spectrogram(ctx, src, n_dec, 1, n_dec, nfft, hop, rate/step, spec, frames)
            h.mean_spectrum_db(ctx, spec, F, 0, frames, mean_db.view(i*F, (F,)))

    report(f'{what}: the same events one by one, hipdsp_spectrogram + hipdsp_mean_spectrum_db'
           + (' behind hipdsp_stride_copy' if step > 1 else ''), old_route, 1, one)
    for d in (rows, info, spec, dec, mean_db):
        d.free()
if len(sys.argv) > 2:
    with open(sys.argv[2], 'w') as f:
        f.write(f'# tools/region_spectra_bench.py: {C} ch x {T} samples, {EVENTS} events of {LENGTH} samples per channel, '
                f'ROUNDS={ROUNDS}\n' + '\n'.join(lines) + '\n')
