"""The two launches of the flagship step for several BUILDS of the library in ONE process on the SAME device buffers,
round-robin: hipdsp_chain_forward 2048/1024 (2 + 1 sections) and hipdsp_sosfilt_envelope phase 2 at BASELINE configs[2]'s
size.  Made for the per-stream cache-policy builds (csrc/Makefile: V / VHINTS; sos_device.h: HD_NT_*), like
tools/libs_sweep.py with the backward sweep added and every build writing the SAME output buffers (where a buffer lies
in HBM moves a sweep by several per cent).
    python tools/stream_hints_ab.py base.so other.so ...          (ROUNDS, default 9; REPS, default 4; SECONDS_, default 600)
Prints per build the median of each launch and of their sum with the ratio to the FIRST build, and the spread
(max - min) / median of the rounds; name the same build twice (or a rebuild of it) to see what identical code differs by."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from audian_amd import hipdsp, _lib
from audian_amd.design import butter_sos

libs = sys.argv[1:]
C, secs, rate = 64, float(os.environ.get('SECONDS_', '600')), 96000.0
nfft, hop = 2048, 1024
T = int(secs*rate)
nd = (T + hop - 1)//hop
rounds, reps = int(os.environ.get('ROUNDS', '9')), int(os.environ.get('REPS', '4'))
ctx = hipdsp.Context(0)
dx, df, de = (hipdsp.DeviceArray(ctx, (C, T), np.float32) for _ in range(3))
ds = hipdsp.DeviceArray(ctx, (C*nd*(nfft//2 + 1),), np.float32)
hipdsp.synth(ctx, dx, T, C, T, rate, 7)
ctx.synchronize()
sos, esos = butter_sos(2, (300.0, 3000.0), 'bandpass', rate), butter_sos(2, 20.0, 'lowpass', rate)
vp = ctypes.c_void_p
P = lambda a: vp(a.ptr)
builds = []
for i, path in enumerate(libs):
    B = ctypes.CDLL(path if os.path.isabs(path) else os.path.join(ROOT, path))
    for name, (args, res) in _lib._SIGNATURES.items():
        fn = getattr(B, name); fn.argtypes = args; fn.restype = res

    def ok(rc, B=B):
        if rc:
            raise RuntimeError(B.hipdsp_last_error().decode())
    cb = vp(); ok(B.hipdsp_ctx_create(0, None, ctypes.byref(cb)))
    pf, pe = vp(), vp()
    for h, tab in ((pf, sos), (pe, esos)):
        ok(B.hipdsp_sosplan_create(cb, ctypes.byref(h)))
        tab = np.ascontiguousarray(tab, dtype=np.float64)
        ok(B.hipdsp_sosplan_set(cb, h, vp(tab.ctypes.data), len(tab)))
    e0, e1 = vp(), vp()
    ok(B.hipdsp_event_create(cb, ctypes.byref(e0))); ok(B.hipdsp_event_create(cb, ctypes.byref(e1)))
    builds.append(('%d:%s' % (i, os.path.basename(path)), B, ok, cb, pf, pe, e0, e1))


def launches(b):
    name, B, ok, cb, pf, pe, e0, e1 = b
    fwd = lambda: ok(B.hipdsp_chain_forward(cb, pf, pe, P(dx), T, P(df), T, C, T, 1, np.pi/2, nfft, hop, rate, P(ds), None, nd, 0, 0, 0, 0))
    bwd = lambda: ok(B.hipdsp_sosfilt_envelope(cb, pf, pe, P(dx), T, P(df), T, P(de), T, C, T, 1, np.pi/2, 1, 2, 0))
    return fwd, bwd


def timed(b, f, n):
    name, B, ok, cb, pf, pe, e0, e1 = b
    f(); ok(B.hipdsp_ctx_synchronize(cb))
    ok(B.hipdsp_event_record(cb, e0))
    for _ in range(n):
        f()
    ok(B.hipdsp_event_record(cb, e1)); ok(B.hipdsp_ctx_synchronize(cb))
    ms = ctypes.c_float()
    ok(B.hipdsp_event_elapsed_ms(cb, e0, e1, ctypes.byref(ms)))
    return ms.value/n


res = {b[0]: {'fwd': [], 'bwd': []} for b in builds}
for b in builds:                       # each context's scratch holds its own tile states: forward first
    fwd, bwd = launches(b)
    timed(b, fwd, 1); timed(b, bwd, 1)
for _ in range(rounds):
    for b in builds:
        fwd, bwd = launches(b)
        res[b[0]]['fwd'].append(timed(b, fwd, reps))
        res[b[0]]['bwd'].append(timed(b, bwd, reps))
med = lambda v: float(np.median(v))
spread = lambda v: 100*(max(v) - min(v))/med(v)
base = res[builds[0][0]]
bf, bb = med(base['fwd']), med(base['bwd'])
print(f'{C} ch x {secs:g} s x {rate/1000:g} kHz, {nfft}/{hop}, {rounds} rounds of {reps} launches; ms, ratio to the first build, spread of the rounds')
for name, r in res.items():
    f, w = med(r['fwd']), med(r['bwd'])
    print(f'{name:28s} fwd {f:7.3f} ({100*(f/bf - 1):+5.2f} %, spread {spread(r["fwd"]):4.2f} %)   '
          f'bwd {w:7.3f} ({100*(w/bb - 1):+5.2f} %, spread {spread(r["bwd"]):4.2f} %)   '
          f'sum {f + w:7.3f} ({100*((f + w)/(bf + bb) - 1):+5.2f} %)', flush=True)
