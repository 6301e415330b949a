"""One line per compute entry point of the C ABI at BASELINE configs[2]'s shape (64 ch x 600 s x 96 kHz): time and
algorithmic GB/s -- so that a change to a shared piece (the segment planner, the cascade include, the block cache)
shows up wherever it lands, not only in the chain bench.py times.  (tools/next_rows_bench.py has the SURVEY 8f rows.)
    python tools/entry_points_bench.py [seconds=600]
    LIBS=tools/_ab/libr04.so,tree OUT_PREFIX=gpurun_out/r05_entry_points python tools/entry_points_bench.py
LIBS: several BUILDS of the library in this ONE process on the SAME device buffers, every entry point timed for each of
them in turn (ROUNDS times, the fastest counts), one log per build (<OUT_PREFIX>_<name>.log; "tree" = the tree's build,
also printed) -- what tools/entry_points_gate.py compares.  Separate processes place their buffers differently in HBM,
and the envelope's backward sweep and the PSD kernels with the dB image move by 5-12 % with that alone (identical machine
code: profiles/r05x_*, r05y_*); a box moves by 5 % against the next one."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


sys.path.insert(0, os.path.join(ROOT, 'tools'))
from _builds import load_build, build_name

libs = [s for s in os.environ.get('LIBS', 'tree').split(',') if s]
rounds = int(os.environ.get('ROUNDS', '2' if len(libs) > 1 else '1'))
C, rate = 64, 96000.0
T = int((float(sys.argv[1]) if len(sys.argv) > 1 else 600.0)*rate)
S = C*T
WINDOWS = ((2048, 1024), (1024, 256), (256, 128), (8192, 4096), (65536, 32768))
FUSED = ((2048, 1024), (1024, 256), (256, 128))

builds = []
for i, lib in enumerate(libs):
    name = build_name(lib)
    h, d = load_build(lib)
    ctx = h.Context(0)
    builds.append({'name': name, 'h': h, 'design': d, 'ctx': ctx, 'e0': ctx.event(), 'e1': ctx.event()})

# the buffers: allocated once (by the first build's context), every build sees the same pointers
b0 = builds[0]
shapes = {'dx': (C, T), 'df': (C, T), 'de': (C, T),
          'ds': (max(C*((T + hp - 1)//hp)*(n//2 + 1) for n, hp in WINDOWS),), 'db': (max(C*((T + hp - 1)//hp)*(n//2 + 1) for n, hp in FUSED),)}
owned = {k: b0['h'].DeviceArray(b0['ctx'], shp, np.float32) for k, shp in shapes.items()}
b0['h'].synth(b0['ctx'], owned['dx'], T, C, T, rate, 1236)
b0['ctx'].synchronize()
for b in builds:
    h, ctx, bs = b['h'], b['ctx'], b['design'].butter_sos
    b['buf'] = {k: (a if b is b0 else h.DeviceArray(ctx, a.shape, np.float32, ptr=a.ptr, owner=a)) for k, a in owned.items()}
    b['bp2'] = h.SosPlan(ctx, bs(2, (300.0, 3000.0), 'bandpass', rate))
    b['bp4'] = h.SosPlan(ctx, bs(4, (300.0, 3000.0), 'bandpass', rate))
    b['lp1'] = h.SosPlan(ctx, bs(2, 20.0, 'lowpass', rate))
    b['lp2'] = h.SosPlan(ctx, bs(4, 20.0, 'lowpass', rate))
    b['lp6'] = [h.SosPlan(ctx, bs(12, 500.0, 'lowpass', rate)[i:i + 3]) for i in (0, 3)]


def entries(b):
    """(name, callable, algorithmic bytes, timed calls, preparation) per entry point, for one build"""
    h, ctx = b['h'], b['ctx']
    dx, df, de, ds, db = (b['buf'][k] for k in ('dx', 'df', 'de', 'ds', 'db'))
    bp2, bp4, lp1, lp2, lp6 = b['bp2'], b['bp4'], b['lp1'], b['lp2'], b['lp6']
    filt = lambda: h.sosfilt(ctx, bp2, dx, T, df, T, C, T, 0)              # (what the envelope and the PSD lines read)
    out = [
        ('hipdsp_sosfilt, band-pass of 2 sections (BufferedFilter alone)', filt, 8.0*S, 5, None),
        ('hipdsp_sosfilt, band-pass of 4 sections', lambda: h.sosfilt(ctx, bp4, dx, T, df, T, C, T, 0), 8.0*S, 5, None),
        ('hipdsp_sosfilt, no filter (copy)', lambda: h.sosfilt(ctx, None, dx, T, df, T, C, T, 0), 8.0*S, 5, None),
        ('hipdsp_envelope, low-pass of 1 section (BufferedEnvelope alone)', lambda: h.envelope(ctx, lp1, df, T, de, T, C, T, 0), 12.0*S, 5, filt),
        ('hipdsp_envelope, low-pass of 2 sections', lambda: h.envelope(ctx, lp2, df, T, de, T, C, T, 0), 12.0*S, 5, filt),
        ('hipdsp_envelope_multi, low-pass of 6 sections as 3 + 3 (default options; temporaries in the context scratch)',
         lambda: h.envelope_multi(ctx, lp6, df, T, de, T, C, T, 0), 12.0*S, 3, filt),
        ('hipdsp_sosfilt_envelope, both sweeps (filter + envelope, unfused spectrogram)',
         lambda: h.sosfilt_envelope(ctx, bp2, lp1, dx, T, df, T, de, T, C, T), 16.0*S, 5, None),
    ]
    for nfft, hop in WINDOWS:
        F, nd = nfft//2 + 1, (T + hop - 1)//hop
        out.append((f'hipdsp_spectrogram {nfft}/{hop} (BufferedSpectrogram alone)',
                    lambda nfft=nfft, hop=hop, nd=nd: h.spectrogram(ctx, df, T, C, T, nfft, hop, rate, ds, nd), 4.0*S + 4.0*C*nd*F, 5, filt))
        if (nfft, hop) in FUSED:
            fwd = lambda nfft=nfft, hop=hop, nd=nd: h.chain_forward(ctx, bp2, lp1, dx, T, df, T, C, T, nfft, hop, rate, ds, nd)
            out += [
                (f'hipdsp_spectrogram {nfft}/{hop} with the dB image',
                 lambda nfft=nfft, hop=hop, nd=nd: h.spectrogram(ctx, df, T, C, T, nfft, hop, rate, ds, nd, db_out=db), 4.0*S + 8.0*C*nd*F, 5, filt),
                (f'hipdsp_chain_forward {nfft}/{hop}, 2 + 1 sections', fwd, 8.0*S + 4.0*C*nd*F, 5, None),
                (f'hipdsp_chain_forward {nfft}/{hop}, 2 + 1 sections, with the dB image',
                 lambda nfft=nfft, hop=hop, nd=nd: h.chain_forward(ctx, bp2, lp1, dx, T, df, T, C, T, nfft, hop, rate, ds, nd, db_out=db), 8.0*S + 8.0*C*nd*F, 5, None),
                (f'hipdsp_chain_forward {nfft}/{hop}, 2 sections, no envelope',
                 lambda nfft=nfft, hop=hop, nd=nd: h.chain_forward(ctx, bp2, None, dx, T, df, T, C, T, nfft, hop, rate, ds, nd), 8.0*S + 4.0*C*nd*F, 5, None),
                (f'hipdsp_chain_forward {nfft}/{hop}, 4 + 2 sections',
                 lambda nfft=nfft, hop=hop, nd=nd: h.chain_forward(ctx, bp4, lp2, dx, T, df, T, C, T, nfft, hop, rate, ds, nd), 8.0*S + 4.0*C*nd*F, 5, None),
            ]
        if (nfft, hop) == (2048, 1024):
            out += [
                ('hipdsp_sosfilt_envelope phase 2 (backward sweep behind the fused forward sweep)',
                 lambda: h.sosfilt_envelope(ctx, bp2, lp1, dx, T, df, T, de, T, C, T, phase=2), 8.0*S, 5, fwd),
                ('hipdsp_decibel over the PSD', lambda nd=nd, F=F: h.decibel(ctx, ds, db, C*nd*F), 8.0*C*nd*F, 5, None),
            ]
    return out


def timed(b, f, n):
    ctx = b['ctx']
    f(); f()
    ctx.record(b['e0'])
    for _ in range(n):
        f()
    ctx.record(b['e1'])
    return ctx.elapsed_ms(b['e0'], b['e1'])/n


tables = [entries(b) for b in builds]
logs = {b['name']: [] for b in builds}
for row in zip(*tables):
    best = {b['name']: 1e30 for b in builds}
    for _ in range(rounds):
        for b, (name, f, nbytes, n, prep) in zip(builds, row):
            if prep is not None:
                prep()                                   # (leaves what this entry point reads: the filtered trace, the tile states)
                b['ctx'].synchronize()
            best[b['name']] = min(best[b['name']], timed(b, f, n))
            b['ctx'].synchronize()
    name, nbytes = row[0][0], row[0][2]
    for b in builds:
        ms = best[b['name']]
        logs[b['name']].append(f'{name:78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
    print(logs[builds[-1]['name']][-1] + ('' if len(builds) == 1 else '    | ' + '  '.join(f"{b['name']} {best[b['name']]:.3f}" for b in builds[:-1])), flush=True)
# ---- hipdsp_band_power over configs[2]'s PSD slab (tools/band_power_bench.py has the other slabs and band sets).  A build
# from before the entry point existed has no such lines: the gate lists them as new.
nfft, hop = 2048, 1024
F, nd = nfft//2 + 1, (T + hop - 1)//hop
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_band_power'):
        continue
    df, ds, de = b['buf']['df'], b['buf']['ds'], b['buf']['de']
    h.sosfilt(ctx, b['bp2'], b['buf']['dx'], T, df, T, C, T, 0)
    h.spectrogram(ctx, df, T, C, T, nfft, hop, rate, ds, nd)
    ctx.synchronize()
    for name, bands in (('the full band', [(0, F)]), ('a 64-bin band', [(341, 405)]),
                        ('4 disjoint bands of 64 bins in one call', [(j*256 + 1, j*256 + 65) for j in range(4)])):
        nbytes = 4.0*C*nd*(sum(k1 - k0 for k0, k1 in bands) + len(bands))
        ms = min(timed(b, lambda: h.band_power(ctx, ds, 0, C, nd, F, bands, rate/nfft, de), 5) for _ in range(rounds))
        ctx.synchronize()
        logs[b['name']].append(f'{"hipdsp_band_power over the PSD 2048/1024, " + name:78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
# ---- hipdsp_spectral_features over the same PSD slab (the loop above has just written it; tools/spectral_features_bench.py has
# the 1/8 band and hipdsp_band_power next to every line): the peak alone, and all eight features
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_spectral_features'):
        continue
    ds, out = b['buf']['ds'], b['buf']['db']            # (nothing below reads the dB image's buffer)
    for name, mask in (('peak bin, peak and peak power', 0x07), ('all eight features', 0xFF)):
        nbytes = 4.0*C*nd*(F + bin(mask).count('1'))
        ms = min(timed(b, lambda: h.spectral_features(ctx, ds, 0, C, nd, F, 0, F, mask, rate/nfft, out), 5) for _ in range(rounds))
        ctx.synchronize()
        logs[b['name']].append(f'{"hipdsp_spectral_features over the PSD 2048/1024, full band, " + name:78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
# ---- hipdsp_template_match over the same PSD slab: 16 normalised templates of 32 frames x 128 bins on the dB values
# (tools/template_match_bench.py has the other shapes, the raw mode and hipdsp_fir_bank at the same tap count)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_template_match'):
        continue
    ds, out = b['buf']['ds'], b['buf']['db']
    plan = h.TmplPlan(ctx, np.random.default_rng(7).uniform(-100.0, -40.0, (16, 32, 128)), True)
    nbytes = 4.0*C*nd*(128 + 16)
    ms = min(timed(b, lambda: h.template_match(ctx, plan, ds, 0, C, nd, F, 341, 0, nd, out, db=True, floor=-120.0, pivot=-90.0,
                                               min_std=0.1), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_template_match over the PSD 2048/1024, 16 templates of 32 x 128, dB":78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
    plan.close()
# ---- hipdsp_bin_quantiles / hipdsp_spec_equalize over the same PSD slab: the per-bin median, and the slab divided by it
# (tools/noise_profile_bench.py has the slab with ties, the other mode, in place, and the copy of the slab as a yardstick)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_bin_quantiles'):
        continue
    ds, out = b['buf']['ds'], b['buf']['db']
    lo_hi, count = h.DeviceArray(ctx, (C, F, 2), np.float32), h.DeviceArray(ctx, (C, F), np.int32)
    ms = min(timed(b, lambda: h.bin_quantiles(ctx, ds, 0, C, nd, F, 0, nd, 1, 0, F, 0.5, lo_hi, count), 3) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_bin_quantiles over the PSD 2048/1024, q 0.5 (four reads of the slab)":78s} {ms:8.3f} ms {16.0*C*nd*F/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
    prof = h.DeviceArray.from_host(ctx, np.maximum(lo_hi.to_host()[:, :, 0], np.float32(1e-20)))
    ms = min(timed(b, lambda: h.spec_equalize(ctx, ds, 0, out, 0, C, nd, F, prof, 0, 'divide'), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_spec_equalize over the PSD 2048/1024, divide, out of place":78s} {ms:8.3f} ms {8.0*C*nd*F/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
    if hasattr(h.lib, 'hipdsp_spec_adapt'):            # (tools/adaptive_spectrogram_bench.py has the other modes and the slab copy)
        ms = min(timed(b, lambda: h.spec_adapt(ctx, ds, 0, out, 0, C, nd, F, 0, 0.0263, 'pcen'), 3) for _ in range(rounds))
        ctx.synchronize()
        logs[b['name']].append(f'{"hipdsp_spec_adapt over the PSD 2048/1024, pcen, out of place (two reads, one write)":78s} {ms:8.3f} ms {12.0*C*nd*F/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
    for d in (lo_hi, count, prof):
        d.free()
# ---- hipdsp_fir_bank: 16 kernels of 257 taps over the envelope, one frame per millisecond (tools/fir_bank_bench.py has the
# other kernel lengths and steps)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_fir_bank'):
        continue
    n_out = -(-T//96)
    plan = h.FirPlan(ctx, np.random.default_rng(7).standard_normal((16, 257))/16.0)
    nbytes = 4.0*S + 4.0*16*C*n_out
    ms = min(timed(b, lambda: h.fir_bank(ctx, plan, b['buf']['df'], T, C, T, 0, 96, n_out, b['buf']['ds']), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_fir_bank, 16 kernels of 257 taps, step 96":78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_region_stats: the whole filtered buffer as one region, every channel (tools/region_stats_bench.py has the short
# regions and hipdsp_minmax_decimate over the same ranges)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_region_stats'):
        continue
    stats = h.DeviceArray(ctx, (1, C, 8), np.float64)
    ms = min(timed(b, lambda: h.region_stats(ctx, b['buf']['df'], T, C, T, [(0, T)], out=stats), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_region_stats, the whole buffer as one region":78s} {ms:8.3f} ms {4.0*S/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_detect_events: the envelope of the whole buffer against one threshold, gaps up to 0.1 s merged (tools/events_bench.py
# has the other gaps and hipdsp_region_stats over the same slab)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_detect_events'):
        continue
    ev, cnt = h.DeviceArray(ctx, (C, 65536, 2), np.int64), h.DeviceArray(ctx, (C,), np.int64)
    ms = min(timed(b, lambda: h.detect_events_into(ctx, b['buf']['de'], T, C, 0, T, 0.25, 9600, 960, 65536, ev, cnt), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_detect_events, the whole envelope, min_gap 0.1 s, min_len 0.01 s":78s} {ms:8.3f} ms {4.0*S/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_histogram and hipdsp_masked_stats: the whole envelope, the reference's 49 bins / the samples below a cut
# (tools/histogram_bench.py has the concentrated envelope, the ratios to hipdsp_region_stats and the whole threshold estimate)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_histogram'):
        continue
    counts = h.DeviceArray(ctx, (C, 52), np.int64)
    bounds = h.DeviceArray.from_host(ctx, np.tile([-np.inf, 0.25, 0.25], (C, 1)))
    moments = h.DeviceArray(ctx, (C, 4), np.float64)
    edges = np.linspace(0.0, 1.0, 50)
    for name, f in (('hipdsp_histogram, the whole envelope, 49 bins', lambda: h.histogram(ctx, b['buf']['de'], T, C, 0, T, edges, out=counts)),
                    ('hipdsp_masked_stats, the whole envelope, the samples below 0.25',
                     lambda: h.masked_stats(ctx, b['buf']['de'], T, C, 0, T, bounds, out=moments))):
        ms = min(timed(b, f, 5) for _ in range(rounds))
        ctx.synchronize()
        logs[b['name']].append(f'{name:78s} {ms:8.3f} ms {4.0*S/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
# ---- hipdsp_find_peaks: the peaks of the whole envelope above 0.25 with a prominence of at least 0.1 (tools/peaks_bench.py has
# white noise, the pure scan and hipdsp_region_stats over the same slab)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_find_peaks'):
        continue
    pk, pr, cnt = h.DeviceArray(ctx, (C, 65536), np.int64), h.DeviceArray(ctx, (C, 65536, 4), np.float64), h.DeviceArray(ctx, (C,), np.int64)
    borders = [0.25, np.inf, -np.inf, np.inf, 0.1, np.inf]
    ms = min(timed(b, lambda: h.find_peaks_into(ctx, b['buf']['de'], T, C, 0, T, borders, 0, 65536, pk, pr, cnt), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_find_peaks, the whole envelope, height 0.25, prominence 0.1":78s} {ms:8.3f} ms {4.0*S/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_region_spectra: ten 5 s events per channel of the filtered buffer, Welch 1024 / 512 (tools/region_spectra_bench.py
# has the decimated envelope and the per-event route through hipdsp_spectrogram + hipdsp_mean_spectrum_db)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_region_spectra'):
        continue
    n5 = min(int(5*rate), T//10)
    table = np.array([(c, k*(T//10), k*(T//10) + n5) for c in range(C) for k in range(10)], dtype=np.int64)
    rows, info = h.DeviceArray(ctx, (len(table), 513), np.float32), h.DeviceArray(ctx, (len(table), 2), np.int64)
    ms = min(timed(b, lambda: h.region_spectra_into(ctx, b['buf']['df'], T, C, T, table, 1024, 512, 1, rate, rows, info), 5)
             for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_region_spectra, 10 events of 5 s per channel, 1024/512":78s} {ms:8.3f} ms {4.0*len(table)*n5/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_region_filtfilt / hipdsp_region_crossings: the same ten events per channel widened by 1 s on both sides (7 s
# regions of the envelope), every region with a first-order low-pass of its own, 40 ... 400 Hz (tools/region_filter_bench.py
# has the per-event routes they replace)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_region_filtfilt'):
        continue
    n7 = min(int(7*rate), T//10)
    table = np.array([(c, k*(T//10), k*(T//10) + n7) for c in range(C) for k in range(10)], dtype=np.int64)
    sos = np.array([b['design'].butter_sos(1, f, 'lowpass', rate) for f in np.linspace(40.0, 400.0, len(table))])
    ms = min(timed(b, lambda: h.region_filtfilt(ctx, b['buf']['de'], T, b['buf']['ds'], T, C, T, table, sos), 3)
             for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_region_filtfilt, 10 regions of 7 s per channel, order 1":78s} {ms:8.3f} ms {8.0*len(table)*n7/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
    out = h.DeviceArray(ctx, (len(table), 8), np.float64)
    ms = min(timed(b, lambda: h.region_crossings(ctx, b['buf']['de'], T, C, T, table, 0.5, out=out), 5) for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_region_crossings, 10 regions of 7 s per channel":78s} {ms:8.3f} ms {4.0*len(table)*n7/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_power_envelope: the filtered buffer to the song detector's envelope at the envelope rate, first-order low-pass at
# 500 Hz, every 19th sample, with the root (tools/power_envelope_bench.py has the route through hipdsp_envelope + hipdsp_stride_copy)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_power_envelope'):
        continue
    n_out = -(-T//19)
    plan = h.SosPlan(ctx, b['design'].butter_sos(1, 500.0, 'lowpass', rate))
    ms = min(timed(b, lambda: h.power_envelope(ctx, plan, b['buf']['df'], T, C, T, b['buf']['ds'], n_out, 0, 19, n_out, 4.0, True), 3)
             for _ in range(rounds))
    ctx.synchronize()
    logs[b['name']].append(f'{"hipdsp_power_envelope, low-pass of 1 section at 500 Hz, step 19, root":78s} {ms:8.3f} ms {(12.0*S + 4.0*C*n_out)/ms/1e6:7.0f} GB/s')
    if b is builds[-1]:
        print(logs[b['name']][-1], flush=True)
# ---- hipdsp_common_reference: the raw buffer minus the mean / the median of its 64 channels (tools/common_reference_bench.py
# has the groups of 16, in place, and the copy and hipdsp_unwrap over the same buffers)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_common_reference'):
        continue
    for mode in ('mean', 'median'):
        ms = min(timed(b, lambda: h.common_reference(ctx, b['buf']['dx'], T, b['buf']['df'], T, C, T, [0]*C, None, mode), 5)
                 for _ in range(rounds))
        ctx.synchronize()
        logs[b['name']].append(f'{"hipdsp_common_reference, " + mode + ", one group of 64 channels":78s} {ms:8.3f} ms {8.0*S/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
# ---- hipdsp_region_xcorr: the same ten 7 s events per channel of the filtered buffer against 8 partner channels over +-1 ms
# (tools/region_xcorr_bench.py has all 63 partners, the envelope at +-50 ms, lag 0 alone and the measured float64 FMA rate)
for b in builds:
    h, ctx = b['h'], b['ctx']
    if not hasattr(h.lib, 'hipdsp_region_xcorr'):
        continue
    n7 = min(int(7*rate), T//10)
    table = np.array([(c, k*(T//10), k*(T//10) + n7) for c in range(C) for k in range(10)], dtype=np.int64)
    for L in (96, 0):
        rows, info = h.DeviceArray(ctx, (len(table), 8, 2*L + 1), np.float32), h.DeviceArray(ctx, (len(table), 8, 4), np.float64)
        ms = min(timed(b, lambda: h.region_xcorr_into(ctx, b['buf']['df'], T, C, T, table, list(range(8)), L, rows, info), 1)
                 for _ in range(rounds))
        ctx.synchronize()
        nbytes = 4.0*len(table)*8*(2*n7 + -(-n7//2048)*2*L)
        logs[b['name']].append(f'{"hipdsp_region_xcorr, 10 events of 7 s per channel, 8 partners, max_lag " + str(L):78s} {ms:8.3f} ms {nbytes/ms/1e6:7.0f} GB/s')
        if b is builds[-1]:
            print(logs[b['name']][-1], flush=True)
        rows.free()
        info.free()
prefix = os.environ.get('OUT_PREFIX')
if prefix:
    for name, lines in logs.items():
        with open(f'{prefix}_{name}.log', 'w') as f:
            f.write('\n'.join(lines) + '\n')

# ---- the reference's DEFAULT session through the plug-in surface: no filter set (bufferedfilter.py:40-42) + spectrogram
# 256 / 128 (plugins.py:11-13, bufferedspectrogram.py:14-16), whole recording resident: BufferedFilter.update() ->
# recompute_all().  The filtered trace's mirror is a view of the raw slab's device copy (no launch), the spectrogram is
# the only launch.  (The tree's build alone: the facade is the package, not a library.)
if os.environ.get('FACADE', '1') == '1' and libs == ['tree']:
    import time
    from audian_amd import hipdsp
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.tracegraph import TraceGraph
    h, ctx = b0['h'], b0['ctx']
    dx = owned['dx']
    for k in ('df', 'de', 'ds', 'db'):
        owned[k].free()
    host = np.empty((T, C), dtype=np.float32)
    chunk = 1 << 20
    tmp = h.DeviceArray(ctx, (chunk, C), np.float64)
    for a in range(0, T, chunk):
        n = min(chunk, T - a)
        h.unpack(ctx, dx.view(a, (1,)), T, tmp, n, C)
        host[a:a + n] = tmp.to_host().reshape(-1)[:n*C].reshape(n, C)
    tmp.free()
    dx.free()
    ctx2 = hipdsp.Context(0)
    hipdsp._default_ctx = ctx2

    class Shown:
        def isVisible(self):
            return True

    g = TraceGraph(T/rate, 0.0)
    filt, spec = BufferedFilter(), BufferedSpectrogram()          # the defaults: 256, 50 % overlap
    g.add_trace(filt)
    g.add_trace(spec)
    g.setup_traces()
    g.open(host, rate, view=True)
    for t in g.traces:
        t.plot_items = [Shown() for _ in range(t.channels)]
    g.set_need_update()
    g.update_times(0.0, T/rate)
    filt.update()
    ctx2.synchronize()
    before = dict(hipdsp.launches)
    t0 = time.perf_counter()
    for _ in range(5):
        filt.update()
    ctx2.synchronize()
    ms = (time.perf_counter() - t0)/5*1e3
    per = {k: (v - before.get(k, 0))//5 for k, v in hipdsp.launches.items() if v != before.get(k, 0)}
    nd = len(spec._hostbuf)
    print(f'{"default session (no filter + 256/128) through BufferedFilter.update(), launches " + str(per):78s} {ms:8.3f} ms {(4.0*S + 4.0*C*nd*129)/ms/1e6:7.0f} GB/s', flush=True)
