"""Per-bin spectrogram accuracy on every path hipdsp_spectrogram and hipdsp_chain_forward take
(spectrogram.hip's dispatch, the fused sweep's six windows): each frame against the float64 oracle under the
bound of tests/spectral_bound.py (calibrated on the CPU by tests/test_spectral_bound.py), on signal families that
span 60-120 dB inside a frame, with the dB image held to the same bound.  A failure names the path, nfft, hop,
family and the worst frame; test_zz_worst_per_path prints the worst rho and beta of every path measured.
"""

import numpy as np
import pytest

import gpu_helpers as gh
import spectral_bound as sb

pytestmark = pytest.mark.gpu

RATE = 48000.0
WORST = {}


def note(path, nfft, rb):
    old = WORST.get((path, nfft), (0.0, 0.0))
    WORST[(path, nfft)] = (max(old[0], rb[0]), max(old[1], rb[1]))


def frames_for(nfft):
    return 3 if nfft <= 16384 else 2


def reference(oracle, x, nfft, hop, frames_out):
    """float64 PSD of the float32 input laid out (C, frames_out, F) like the kernel's output."""
    want = np.zeros((frames_out, x.shape[1], nfft//2 + 1))
    oracle.spectrogram_process(x.astype(np.float64), want, RATE, nfft, hop)
    return want.transpose(1, 0, 2)


def run_spec(x, nfft, hop, frames_out, options=(), want_db=False):
    """hipdsp_spectrogram with context options set for the call; (C, frames_out, F) PSD and dB image (or None)."""
    from audian_amd import hipdsp
    c = gh.ctx()
    T, C = x.shape
    F = nfft//2 + 1
    for k, v in options:
        c.set_option(k, v)
    try:
        dx = gh.to_planar(c, x)
        out = hipdsp.DeviceArray(c, (C, frames_out, F), np.float32)
        db = hipdsp.DeviceArray(c, (C, frames_out, F), np.float32) if want_db else None
        for arr in (out, db) if want_db else (out,):
            hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(arr), 0x7f, 4*C*frames_out*F)   # every bin must be written
        hipdsp.spectrogram(c, dx, T, C, T, nfft, hop, RATE, out, frames_out, db_out=db)
        return out.to_host(), (db.to_host() if want_db else None)
    finally:
        for k, _ in options:
            c.set_option(k, 0)


def check_case(oracle, path, name, nfft, hop, options=(), want_db=False, frames=None, direct=False, seed=0):
    frames = frames or frames_for(nfft)
    x = sb.family(name, (frames - 1)*hop + nfft, nfft, RATE, seed=seed + nfft + hop)
    got, db = run_spec(x, nfft, hop, frames + 1, options, want_db)          # one frame past the input: zero
    want = reference(oracle, x, nfft, hop, frames + 1)
    assert np.all(got[:, frames] == 0), (path, nfft, hop, name, 'zero tail')
    if want_db:
        assert np.all(db[:, frames] == -np.inf), (path, nfft, hop, name, 'zero tail dB')
    what = '%s nfft %d hop %d family %s%s' % (path, nfft, hop, name, ' +dB' if want_db else '')
    rb = sb.assert_within(got, want, nfft, what, direct=direct, db=db)
    note(path, nfft, rb)


POW2 = [2**k for k in range(3, 20)]


@pytest.mark.parametrize('nfft', POW2)
def test_default_dispatch(oracle, nfft):
    """Every power of two with the default kernel choice, every family, the dB image on every other one."""
    names = sb.FAMILIES if nfft <= 65536 else ('tones', 'edges', 'offset')
    for i, name in enumerate(names):
        check_case(oracle, 'default', name, nfft, nfft//2, want_db=i % 2 == 1)


@pytest.mark.parametrize('nfft', POW2)
def test_spec_kernel_2(oracle, nfft):
    """"spec_kernel" 2: the two-stage kernel / run_wg up to 32768, the four-step path through HBM from 65536."""
    for i, name in enumerate(('tones', 'edges', 'chirp')):
        check_case(oracle, 'spec_kernel=2', name, nfft, nfft//2, options=[('spec_kernel', 2)], want_db=i == 1)


@pytest.mark.parametrize('nfft', [256, 512, 1024, 4096])
def test_spec_kernel_3(oracle, nfft):
    for i, name in enumerate(('tones', 'bandpass', 'edges')):
        for hop in (nfft//2, nfft//4):
            check_case(oracle, 'spec_kernel=3', name, nfft, hop, options=[('spec_kernel', 3)], want_db=i == 2)


@pytest.mark.parametrize('fpw', [1, 3])
@pytest.mark.parametrize('nfft', [8, 32, 128, 256, 1024])
def test_spec_fpw(oracle, nfft, fpw):
    """Frames per wave forced on the short-window kernels, over a run of frames long enough to use it."""
    for name in ('tones', 'edges'):
        check_case(oracle, 'spec_fpw=%d' % fpw, name, nfft, nfft//2, options=[('spec_fpw', fpw)], frames=40)


@pytest.mark.parametrize('nfft', [256, 512, 1024, 2048])
def test_spec_no_half(oracle, nfft):
    for name in ('tones', 'edges', 'offset'):
        check_case(oracle, 'spec_no_half', name, nfft, nfft//2, options=[('spec_no_half', 1)], frames=8)


@pytest.mark.parametrize('nfft', [256, 4096, 16384])
def test_force_generic_fft(oracle, nfft):
    for i, name in enumerate(('tones', 'edges', 'offset')):
        check_case(oracle, 'force_generic_fft', name, nfft, nfft//2, options=[('force_generic_fft', 1)],
                   want_db=i == 1)


def hops(nfft):
    return [nfft, nfft//2, nfft//4, (nfft//3) | 1]


@pytest.mark.parametrize('nfft', [8, 64, 512, 1024, 2048, 4096, 8192, 65536])
def test_hops_with_and_without_db(oracle, nfft):
    """hop nfft, nfft/2, nfft/4 and an odd hop, with and without the dB image (at 512 and 1024 the kernel choice
    depends on both)."""
    for j, hop in enumerate(hops(nfft)):
        for want_db in (False, True):
            name = sb.FAMILIES[(j + 2*want_db) % len(sb.FAMILIES)] if nfft <= 8192 else ('tones', 'edges')[want_db]
            check_case(oracle, 'default', name, nfft, hop, want_db=want_db, frames=6 if nfft <= 8192 else 2)


@pytest.mark.parametrize('nfft', [24, 1000, 3000, 12000])
def test_direct_dft(oracle, nfft):
    """Sizes that are not powers of two: the direct DFT, under its own bound (sqrt(nfft) growth)."""
    names = sb.FAMILIES if nfft <= 3000 else ('tones', 'edges')
    for i, name in enumerate(names):
        check_case(oracle, 'direct', name, nfft, nfft//2 + (i % 2), want_db=i % 2 == 0, direct=True,
                   frames=2 if nfft <= 3000 else 1)


SHAPES = [(2048, 1024), (2048, 512), (1024, 512), (1024, 256), (512, 256), (256, 128)]


@pytest.mark.parametrize('nfft,hop', SHAPES)
def test_fused_sweep(oracle, nfft, hop):
    """hipdsp_chain_forward's spectrogram for all six windows, 2- and 4-section band-passes, with and without the
    envelope plan, with the dB image, spec_first > 0, one segment and many.  The oracle reads the filtered trace
    the same launch wrote, so the bound measures the transform alone."""
    from audian_amd import hipdsp
    from audian_amd.design import butter_sos
    c = gh.ctx()
    C, T = 2, 60001
    F = nfft//2 + 1
    cases = [(1, 'tones', True, True, 0, 0), (2, 'edges', False, True, 300, 1), (1, 'chirp', True, False, 5, 37),
             (2, 'bandpass', False, False, 0, 1)]
    for order, name, with_env, with_db, spec_first, max_segments in cases:
        x = sb.family(name, T, nfft, RATE, seed=nfft + hop + order)
        sos = butter_sos(order, (300.0, 9000.0), 'bandpass', RATE)           # order 1 / 2: one / two sections
        sos = np.concatenate([sos, butter_sos(order, (200.0, 12000.0), 'bandpass', RATE)])
        esos = butter_sos(2, 20.0, 'lowpass', RATE)
        fplan = hipdsp.SosPlan(c, sos)
        eplan = hipdsp.SosPlan(c, esos) if with_env else None
        nsrc = T - spec_first
        nd = (nsrc + hop - 1)//hop + 1
        c.set_max_segments(max_segments)
        try:
            dx = gh.to_planar(c, x)
            yf = hipdsp.DeviceArray(c, (C, T), np.float32)
            ps = hipdsp.DeviceArray(c, (C, nd, F), np.float32)
            db = hipdsp.DeviceArray(c, (C, nd, F), np.float32) if with_db else None
            for arr in (ps, db) if with_db else (ps,):
                hipdsp.lib.hipdsp_memset(c.handle, hipdsp._p(arr), 0x7f, 4*C*nd*F)
            hipdsp.chain_forward(c, fplan, eplan, dx, T, yf, T, C, T, nfft, hop, RATE, ps, nd, db_out=db,
                                 spec_first=spec_first)
            gf, gs = yf.to_host(), ps.to_host()
            gdb = db.to_host() if with_db else None
        finally:
            c.set_max_segments(0)
        want = np.zeros((nd, C, F))
        oracle.spectrogram_process(gf.T[spec_first:].astype(np.float64), want, RATE, nfft, hop)
        want = want.transpose(1, 0, 2)
        zero = np.max(want, axis=-1) == 0
        assert zero.any() and not zero.all()
        what = 'fused %d/%d family %s, %d sections%s%s, spec_first %d, max_segments %d' % (
            nfft, hop, name, len(sos), ', envelope' if with_env else '', ' +dB' if with_db else '', spec_first,
            max_segments)
        rb = sb.assert_within(gs, want, nfft, what, db=gdb)
        note('fused %d/%d' % (nfft, hop), nfft, rb)


def test_zz_worst_per_path():
    """The worst rho and beta of every path measured above (run with -s to see the table)."""
    if not WORST:
        print('\n(no path measured in this session)')
        return
    lines = ['%-22s %7s %8s %8s %8s' % ('path', 'nfft', 'rho', 'beta', 'beta max')]
    for (path, nfft), (rho, beta) in sorted(WORST.items()):
        lines.append('%-22s %7d %8.3f %8.2f %8.0f' % (path, nfft, rho, beta, sb.beta_max(nfft)))
    print('\n' + '\n'.join(lines))
