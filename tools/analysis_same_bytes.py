"""Do two BUILDS of the library give the same bytes from the analysis entry points?  hipdsp_region_stats,
hipdsp_histogram, hipdsp_masked_stats, hipdsp_detect_events, hipdsp_find_peaks, hipdsp_region_spectra,
hipdsp_region_filtfilt and hipdsp_region_crossings of BASE.so and of the tree's build run in this one process on the
same seeded device buffers (tools/_builds.load_build), every output buffer starts from the same sentinel bytes and is
compared whole -- counts, info and the padding of pitched outputs included.  No tolerance: the check of a change that
moves code between these units without reordering an addition.
    python tools/analysis_same_bytes.py tools/_ab/libbase.so
Exits 1 at the first difference, naming the entry point and the shape.

The shapes: 3 channels of odd pitch -- noise on a coarse grid (flat peaks) with NaN, +inf and -inf sprinkled in, a
constant row, a row above the event threshold throughout; start 0 ... 3 (the four 16-byte phases of a chunk's head);
lengths around the borders of a word (64), of the 4096- and 16384-sample chunks, and 262144 + 4097 (the third level of
the peaks table, 65 chunks: every slice of the 256-thread scans empty or not); capacities ample and too small; tables
of 70 regions (two 64-lane groups of rc_finish) with empty, one-sample, overlapping and repeated regions."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _builds import load_build, build_name

LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 2*16384 + 5, 262144 + 4097)
STARTS = (0, 1, 2, 3)
C, PITCH, RATE = 3, 3 + LENGTHS[-1] + 5, 96000.0        # 266249: odd
SENTINEL = 0xA5


class Build:
    def __init__(self, lib):
        self.name = build_name(lib)
        self.h, self.design = load_build(lib)
        self.ctx = self.h.Context(0)

    def arr(self, a):
        """this build's handle on a device array of the first build"""
        return self.h.DeviceArray(self.ctx, a.shape, a.dtype, ptr=a.ptr, owner=a)


def rows():
    rng = np.random.default_rng(20261019)
    x = np.empty((C, PITCH), dtype=np.float32)
    walk = np.cumsum(rng.standard_normal(PITCH))
    x[0] = np.round(8.0*(np.abs(rng.standard_normal(PITCH))*(1.2 + np.sin(walk/40.0))))/16.0     # runs of equal samples
    for at, v in ((3000, np.nan), (9000, np.inf), (20001, -np.inf), (70000, np.nan), (140000, np.inf), (263000, -np.inf)):
        x[0, at] = v
    x[1] = 0.375
    x[2] = 1.0 + 0.25*rng.random(PITCH)
    return x


def main():
    base, tree = Build(sys.argv[1]), Build('tree')
    builds = (base, tree)
    h0, ctx0 = base.h, base.ctx
    x = rows()
    dx = h0.DeviceArray.from_host(ctx0, x)
    n = {'calls': 0, 'buffers': 0, 'bytes': 0, 'events': 0, 'peaks': 0}

    def same(what, shape, outs, call):
        """outs: name -> (shape, dtype), allocated once per case; call(build, {name: array of that build})"""
        dev = {k: h0.DeviceArray(ctx0, s, t) for k, (s, t) in outs.items()}
        got = []
        for b in builds:
            for d in dev.values():
                d.copy_from_host(np.full(d.nbytes, SENTINEL, dtype=np.uint8).view(d.dtype).reshape(d.shape))
            call(b, {k: b.arr(d) for k, d in dev.items()})
            b.ctx.synchronize()
            got.append({k: d.to_host() for k, d in dev.items()})
        for k in dev:
            if got[0][k].tobytes() != got[1][k].tobytes():
                where = np.flatnonzero(got[0][k].view(np.uint8).reshape(-1) != got[1][k].view(np.uint8).reshape(-1))
                print(f'analysis_same_bytes: DIFFERENT: {what}, {shape}: buffer `{k}` differs in {len(where)} bytes, the '
                      f'first at byte {where[0]} ({base.name} vs {tree.name})', flush=True)
                sys.exit(1)
            n['buffers'] += 1
            n['bytes'] += got[0][k].nbytes
        n['calls'] += 1
        for d in dev.values():
            d.free()
        return got[1]

    edges49, edges5 = np.linspace(0.0, 2.0, 50), np.array([-1.0, 0.0, 0.1, 0.1, 0.7, 3.0])
    bounds = np.array([[-np.inf, 0.5, 0.25], [0.0, 1.0, 0.375], [1.1, 1.2, 1.0]])
    dbounds = h0.DeviceArray.from_host(ctx0, bounds)
    dthr = h0.DeviceArray.from_host(ctx0, np.array([0.5, 0.25, 0.75], dtype=np.float32))
    borders = [0.5, np.inf, -np.inf, np.inf, 0.25, np.inf]
    dborders = h0.DeviceArray.from_host(ctx0, np.array([borders, [-np.inf, np.inf]*3, [-np.inf, np.inf, 0.0, np.inf, -np.inf, 1.0]]))
    for start in STARTS:
        for length in LENGTHS:
            stop = start + length
            shape = f'start {start}, length {length}'
            for edges, pitch in ((edges49, 0), (edges5, 11)):
                B = len(edges) - 1
                same('hipdsp_histogram', f'{shape}, {B} bins, out_pitch {pitch}', {'out': ((C, pitch or B + 3), np.int64)},
                     lambda b, o: b.h.histogram(b.ctx, b.arr(dx), PITCH, C, start, stop, edges, out=o['out'], out_pitch=pitch))
            same('hipdsp_masked_stats', shape, {'out': ((C, 4), np.float64)},
                 lambda b, o: b.h.masked_stats(b.ctx, b.arr(dx), PITCH, C, start, stop, b.arr(dbounds), out=o['out']))
            regions = [(start, stop), (start, start + length//2), (start + length//3, stop), (stop, stop), (start, stop)]
            same('hipdsp_region_stats', f'{shape}, {len(regions)} regions', {'out': ((len(regions), C, 8), np.float64)},
                 lambda b, o: b.h.region_stats(b.ctx, b.arr(dx), PITCH, C, PITCH, regions, out=o['out']))
            ample = length//2 + 16                      # no more events or peaks than that
            for cap, pitch in ((ample, 0), (3, 7)):
                for thr, gap, mlen in ((b'dev', 5, 2), (0.5, 0, 0), (0.5, 300, 40)):
                    got = same('hipdsp_detect_events', f'{shape}, capacity {cap}, events_pitch {pitch}, min_gap {gap}, min_len {mlen}',
                               {'events': ((C, pitch or 2*cap), np.int64), 'counts': ((C,), np.int64)},
                               lambda b, o: b.h.detect_events_into(b.ctx, b.arr(dx), PITCH, C, start, stop, b.arr(dthr) if thr == b'dev' else thr,
                                                                   gap, mlen, cap, o['events'], o['counts'], events_pitch=pitch))
                    n['events'] += int(got['counts'].sum())
            for cap, pp, qp in ((ample, 0, 0), (3, 5, 13)):
                for bd, wlen, props in ((borders, 0, True), (b'dev', 0, True), (borders, 100, True), ([-np.inf, np.inf]*3, 0, False)):
                    outs = {'peaks': ((C, pp or cap), np.int64), 'counts': ((C,), np.int64)}
                    if props:
                        outs['props'] = ((C, qp or 4*cap), np.float64)
                    got = same('hipdsp_find_peaks', f'{shape}, capacity {cap}, pitches {pp}/{qp}, wlen {wlen}, borders {bd}, props {props}', outs,
                               lambda b, o: b.h.find_peaks_into(b.ctx, b.arr(dx), PITCH, C, start, stop, b.arr(dborders) if bd == b'dev' else bd, wlen,
                                                                cap, o['peaks'], o.get('props'), o['counts'], peaks_pitch=pp, props_pitch=qp))
                    n['peaks'] += int(got['counts'].sum())

    # ---- the calls over a (channel, start, stop) table: 70 regions
    rng = np.random.default_rng(7)
    table = [(0, 0, 0), (1, 5, 5), (2, PITCH, PITCH), (0, 7, 8), (2, 1, 2), (0, 100, 5000), (0, 100, 5000), (0, 2000, 9500),
             (1, 3, 4096 + 3), (1, 2, 4097 + 2), (2, 1, 4095 + 1), (0, 0, PITCH), (2, 3, 3 + LENGTHS[-1]), (0, 2990, 3010), (0, 8999, 9001)]
    while len(table) < 70:
        c, a = int(rng.integers(C)), int(rng.integers(PITCH - 1))
        table.append((c, a, min(PITCH, a + int(rng.integers(1, 40000)))))
    table = np.array(table, dtype=np.int64)
    R = len(table)
    same('hipdsp_region_crossings', f'{R} regions', {'out': ((R, 8), np.float64)},
         lambda b, o: b.h.region_crossings(b.ctx, b.arr(dx), PITCH, C, PITCH, table, np.linspace(0.1, 1.3, R), out=o['out']))
    for nfft, hop, step, pitch in ((64, 32, 1, 0), (256, 100, 3, 131), (8192, 4096, 1, 0)):
        F = nfft//2 + 1
        same('hipdsp_region_spectra', f'{R} regions, nfft {nfft}, hop {hop}, step {step}, out_pitch {pitch}',
             {'out': ((R, pitch or F), np.float32), 'info': ((R, 2), np.int64)},
             lambda b, o: b.h.region_spectra_into(b.ctx, b.arr(dx), PITCH, C, PITCH, table, nfft, hop, step, RATE, o['out'], o['info'], out_pitch=pitch))
    # hipdsp_region_filtfilt: regions longer than the padlen that do not overlap within a channel -- 70 in a row per channel
    # pattern, their lengths around the 64-sample chunk and the 4096-sample tile of the extended region
    lens = [16, 17, 40, 63, 64, 65, 100, 4065, 4077, 4078, 4079, 4096, 4097, 8200, 20000]
    ftab, at = [], [1, 2, 3]
    for i in range(R):
        c, ln = i % C, lens[i % len(lens)]
        ftab.append((c, at[c], at[c] + ln))
        at[c] += ln + (i % 2)                            # neighbours touch or leave one sample
    ftab = np.array(ftab, dtype=np.int64)
    for S in (1, 2):
        sos = np.array([base.design.butter_sos(S if S == 1 else 4, f, 'lowpass', RATE)[:S] for f in np.linspace(40.0, 4000.0, R)])
        for clamp in (False, True):
            same('hipdsp_region_filtfilt', f'{R} regions, {S} sections, clamp {clamp}', {'y': ((C, PITCH), np.float32)},
                 lambda b, o: b.h.region_filtfilt(b.ctx, b.arr(dx), PITCH, o['y'], PITCH, C, PITCH, ftab, sos, clamp=clamp))
    if n['events'] == 0 or n['peaks'] == 0:
        print('analysis_same_bytes: the inputs gave no event or no peak: nothing was compared', flush=True)
        sys.exit(2)
    print(f"analysis_same_bytes: {base.name} vs {tree.name}: {n['calls']} calls of the 8 analysis entry points, "
          f"{n['buffers']} output buffers, {n['bytes']} bytes, {n['events']} events and {n['peaks']} peaks counted: all equal", flush=True)


if __name__ == '__main__':
    main()
