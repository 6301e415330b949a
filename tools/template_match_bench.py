"""hipdsp_template_match, device resident, over the PSD slab of BASELINE configs[2] (64 ch x 600 s x 96 kHz) at 256/128
(450000 frames x 129 bins) and 2048/1024 (56250 x 1025): templates of 16 x 64, 32 x 128 and 64 x 256 (frames x bins; a
band that does not fit into 129 bins is skipped), K in {1, 16}, dB on and off, normalised, and one raw line per shape;
in the same process hipdsp_fir_bank at the same tap count per output (the flattened slab as a trace at step = nfreq,
where the 4097-tap limit allows it) and hipdsp_band_power over the same bins.
    python tools/template_match_bench.py [seconds=600] [log=profiles/template_match_bench.log]
Per line: median of the timed launches after the warm-ups (hipdsp_event_*), TFLOP/s over the work the matrix core does
(2 * 16 * Tt * Fb per window and channel: all 16 template columns are always computed), GB/s over the algorithmic bytes
(the band read once, every score written once).  The share of the staging work (the logarithm) is the dB-on minus the
dB-off time of the same line.  The lines are in the format tools/entry_points_gate.py reads."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audian_amd import hipdsp as h

C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'template_match_bench.log')
ctx = h.Context(0)
e0, e1 = ctx.event(), ctx.event()
log = open(LOG, 'w')


def say(line):
    print(line, flush=True)
    log.write(line + '\n')
    log.flush()


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


rng = np.random.default_rng(7)
dx = h.DeviceArray(ctx, (C, T), np.float32)
h.synth(ctx, dx, T, C, T, rate, 1236)
say(f'# 64 ch x {T} samples; TFLOP/s count all 16 template columns; every figure below is measured in this run')
for nfft, hop in ((256, 128), (2048, 1024)):
    F, nd = nfft//2 + 1, (T + hop - 1)//hop
    ds = h.DeviceArray(ctx, (C, nd, F), np.float32)
    out = h.DeviceArray(ctx, (16, C, nd), np.float32)
    h.spectrogram(ctx, dx, T, C, T, nfft, hop, rate, ds, nd)
    ctx.synchronize()
    for Tt, Fb in ((16, 64), (32, 128), (64, 256)):
        if Fb > F:
            say(f'# {nfft}/{hop}: a band of {Fb} bins does not fit into {F}')
            continue
        k0 = (F - Fb)//3
        taps = Tt*Fb
        flops = 2.0*16*taps*C*nd
        took = {}
        for K in (1, 16):
            for mode, normalize, db in (('normalised, dB', True, True), ('normalised, linear', True, False), ('raw, dB', False, True)):
                plan = h.TmplPlan(ctx, rng.uniform(-100.0, -40.0, (K, Tt, Fb)), normalize)
                ms = median_ms(lambda: h.template_match(ctx, plan, ds, 0, C, nd, F, k0, 0, nd, out, db=db, floor=-120.0 if db else -np.inf,
                                                        pivot=-90.0 if db else 0.0, min_std=0.1 if db else 0.0))
                plan.close()
                took[K, mode] = ms
                moved = 4.0*C*nd*(Fb + K)
                name = f'hipdsp_template_match {nfft}/{hop}, {Tt} x {Fb}, K {K}, {mode}'
                say(f'{name:78s} {ms:8.3f} ms {moved/ms/1e6:7.0f} GB/s')
                say(f'    matrix core {flops/ms/1e9:.1f} TFLOP/s (16 columns), useful {flops*K/16/ms/1e9:.1f} TFLOP/s (K = {K})')
            d = took[K, 'normalised, dB'] - took[K, 'normalised, linear']
            say(f'    staging share of the logarithm, K {K}: {d:.3f} ms = {100.0*d/took[K, "normalised, dB"]:.0f} % of the dB line')
        if taps <= 4097:
            for K in (1, 16):
                fir = h.FirPlan(ctx, rng.standard_normal((K, taps))/np.sqrt(taps))
                ms = median_ms(lambda: h.fir_bank(ctx, fir, ds, nd*F, C, nd*F, taps//2, F, nd, out))
                fir.close()
                name = f'hipdsp_fir_bank on the flattened slab {nfft}/{hop}, L {taps}, K {K}, step {F}'
                say(f'{name:78s} {ms:8.3f} ms {4.0*C*nd*(F + K)/ms/1e6:7.0f} GB/s')
                say(f'    matrix core {flops/ms/1e9:.1f} TFLOP/s (16 columns); hipdsp_template_match normalised, dB takes '
                    f'{took[K, "normalised, dB"]/ms:.2f} times as long, raw {took[K, "raw, dB"]/ms:.2f} times')
        else:
            say(f'# hipdsp_fir_bank holds at most 4097 taps: no line for {taps}')
        ms = median_ms(lambda: h.band_power(ctx, ds, 0, C, nd, F, [(k0, k0 + Fb)], rate/nfft, out))
        name = f'hipdsp_band_power over the same {Fb} bins, {nfft}/{hop}'
        say(f'{name:78s} {ms:8.3f} ms {4.0*C*nd*(Fb + 1)/ms/1e6:7.0f} GB/s')
    ds.free()
    out.free()
log.close()
