"""The equalised spectrogram in a small graph on the GPU, walked under the ledger of tests/facade_ledger.py:

    data -> filtered -> spectrogram (256 / 128) -> equalized -> bandpower, peakfreq, match

facade_ledger.Ledger is imported as it is; it knows twelve classes and would take the thirteenth for a spectrogram of
its source, so a subclass here adds the one definition (tests/noise_profile_definition.py on the device's own source
slab, bit for bit) and the step of 1.  The three consumers hang below `equalized` and are held to the rules the ledger
already has for them -- their source slab is now the equalised mirror."""

import numpy as np
import pytest

import facade_ledger as fl
import gpu_helpers as gh
import noise_profile_definition as nd

pytestmark = pytest.mark.gpu


def rule_bits(got, want):
    """NaN exactly where `want` has it, the same float32 bits everywhere else."""
    got32 = np.ascontiguousarray(got, dtype=np.float32)
    bad = np.isnan(got32) != np.isnan(want)
    ok = ~np.isnan(want) & ~np.isnan(got32)
    bad |= ok & (got32.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    return bad


class Ledger(fl.Ledger):

    @staticmethod
    def _step_of(t):
        from audian_amd.bufferedequalizedspectrogram import BufferedEqualizedSpectrogram
        return 1 if isinstance(t, BufferedEqualizedSpectrogram) else fl.Ledger._step_of(t)

    def _define(self, t, slab, nbefore, n, first, soffset):
        from audian_amd.bufferedequalizedspectrogram import BufferedEqualizedSpectrogram
        if not isinstance(t, BufferedEqualizedSpectrogram):
            return fl.Ledger._define(self, t, slab, nbefore, n, first, soffset)
        src = np.ascontiguousarray(slab[nbefore:nbefore + n], dtype=np.float32)
        if t.stale:
            want = np.full(src.shape, np.nan, dtype=np.float32)
        elif t.profile is None:
            want = src
        else:
            want = nd.equalize(src.transpose(1, 0, 2), t.profile.values, t.mode).transpose(1, 0, 2)
        return fl.Segment(first, rule_bits, want=np.ascontiguousarray(want, dtype=np.float32))


def device_db(power, floor):
    """v of the template match's definition: hipdsp_decibel on the same powers, clamped on the host."""
    from audian_amd import hipdsp
    c = gh.ctx()
    power = np.ascontiguousarray(power, dtype=np.float32)
    d = hipdsp.DeviceArray.from_host(c, power)
    o = hipdsp.DeviceArray(c, power.shape, np.float32)
    hipdsp.decibel(c, d, o, power.size, 1.0, 0.0)
    v = o.to_host()
    d.free()
    o.free()
    return np.where(v < np.float32(floor), np.float32(floor), v)


def build(x):
    from audian_amd.bufferedbandpower import BufferedBandPower
    from audian_amd.bufferedequalizedspectrogram import BufferedEqualizedSpectrogram
    from audian_amd.bufferedfilter import BufferedFilter
    from audian_amd.bufferedspectralfeature import BufferedSpectralFeature
    from audian_amd.bufferedspectrogram import BufferedSpectrogram
    from audian_amd.bufferedtemplatematch import BufferedTemplateMatch
    from audian_amd.tracegraph import TraceGraph
    g = TraceGraph(2.5, 0.5)
    for t in (BufferedFilter(name='filtered', source='data'),
              BufferedSpectrogram(name='spectrogram', source='filtered', nfft=256, overlap_frac=0.5),
              BufferedEqualizedSpectrogram(name='equalized', source='spectrogram'),
              BufferedBandPower(name='bandpower', source='equalized', fmin=1000.0, fmax=3000.0),
              BufferedSpectralFeature(name='peakfreq', source='equalized', fmin=500.0, fmax=3500.0),
              BufferedTemplateMatch(name='match', source='equalized')):
        g.add_trace(t)
    g.setup_traces()
    g.open(x, fl.RATE)
    for t in g.traces:
        t.plot_items = [fl.Item() for _ in range(t.channels)]
    g.set_need_update()
    return g


def host_route_profile(s, i0, i1, percentile, frame_step):
    """noise_profile of the same buffer with the mirror declared invalid: the numpy route on trace.buffer."""
    vars(s)['_mirror_valid'] = lambda a, b: False
    try:
        return s.noise_profile(i0, i1, percentile, frame_step)
    finally:
        vars(s).pop('_mirror_valid')


def test_walk_of_the_equalized_graph(oracle):
    from audian_amd import hipdsp
    from audian_amd.noiseprofile import NoiseProfile
    x = fl.recording(40.0, 77)
    g = build(x)
    f, s, e, bp, pf, m = (g[n] for n in ('filtered', 'spectrogram', 'equalized', 'bandpower', 'peakfreq', 'match'))
    ledger = Ledger(g, oracle, db=device_db)
    before = dict(hipdsp.launches)
    log = []

    def done(what):
        log.append(what)
        for t in (e, bp, pf, m):
            assert (t.rate, t.offset, len(t._hostbuf)) == (s.rate, s.offset, len(s._hostbuf)), (what, t.name)
        assert e.shape == s.shape and (e.nfft, e.hop, e.fresolution) == (s.nfft, s.hop, s.fresolution)
        try:
            ledger.check()
        except AssertionError as err:
            raise AssertionError('%s\n  after: %s' % (err, ' | '.join(log[-5:])))

    def launched(name):
        return hipdsp.launches.get(name, 0) - before.get(name, 0)

    g.update_times(0.0, 1.5)
    done('window 0')
    f.highpass_cutoff, f.lowpass_cutoff = 300.0, 3500.0
    f.update()
    done('filter')
    assert e.profile is None and launched('spec_equalize') == 0          # no profile: a copy of the source
    g.update_times(0.6, 2.0)
    done('scroll')
    # the profile: the device route and the host route on the same buffer, bit for bit
    i0, i1 = s.offset + 3, s.offset + len(s._hostbuf) - 2
    for percentile, step in ((50.0, 1), (95.0, 3), (0.0, 2), (100.0, 1), (12.5, 1)):
        n0 = launched('bin_quantiles')
        dev = s.noise_profile(i0, i1, percentile, step)
        assert launched('bin_quantiles') == n0 + 1
        host = host_route_profile(s, i0, i1, percentile, step)
        assert launched('bin_quantiles') == n0 + 1
        assert nd.exact_bits(dev.values, host.values) and (dev.t0, dev.t1, dev.percentile) == (host.t0, host.t1, host.percentile)
        slab = fl.mirror_read(s, 0, len(s._hostbuf)).transpose(1, 0, 2)
        lo_hi, count = nd.bin_quantiles(slab, 3, -(-(i1 - i0)//step), step, 0, 129, percentile/100.0)
        assert nd.exact_bits(dev.values, NoiseProfile(nd.finish_percentile(lo_hi, count, percentile/100.0), 1.0, 1.0).values)
    prof = g.estimate_noise_profile(percentile=50.0)
    assert prof.fits(e) and np.all(prof.values > 0)
    e.set_profile(prof)
    done('set_profile')
    assert launched('spec_equalize') >= 1 and e._mirror_valid(0, len(e._hostbuf)) and not e.stale
    white = fl.peek(e)[:s.complete_frames() - s.offset]                      # (the profile leaves the zero tail out)
    assert np.all(np.abs(np.median(white, axis=0) - 1.0) < 1e-6)           # the profile was taken over this very buffer
    tm = g.cut_template(1.3, 1.3 + 12/s.rate, 1500.0, 3000.0, 0, spec_name='equalized', floor_db=-40.0)
    done('cut_template')
    m.set_template(tm)
    done('set_template')
    assert np.nanmax(fl.peek(m)[:, 0]) > 0.9
    keep = {e.offset + i: (fl.peek(s, i, 1)[0].copy(), fl.peek(e, i, 1)[0].copy()) for i in range(5, len(e._hostbuf), 97)}
    same = 0
    spec_calls = ledger.stats['spectrogram']['calls']
    for t0, t1 in ((0.9, 2.3), (14.0, 15.5), (15.2, 16.7), (27.0, 28.5), (28.1, 29.6), (3.0, 4.5), (38.6, 40.0)):
        g.update_times(t0, t1)
        done('window %.1f' % t0)
        for frame, (src_row, row) in keep.items():                         # a scroll changes no value whose source stays
            if e.offset <= frame < e.offset + len(e._hostbuf) and nd.exact_bits(fl.peek(s, frame - s.offset, 1)[0], src_row):
                assert nd.exact_bits(fl.peek(e, frame - e.offset, 1)[0], row)
                same += 1
    assert same >= 1
    assert ledger.stats['equalized']['partial'] >= 1 and ledger.stats['spectrogram']['calls'] > spec_calls
    spec_calls = ledger.stats['spectrogram']['calls']
    whole = ledger.stats['equalized']['whole']
    e.update(mode='subtract')
    done('subtract')
    assert fl.peek(e).min() == 0 and e.unit == s.unit
    e.update(mode='divide')
    done('divide')
    e.set_profile(g.estimate_noise_profile(percentile=25.0, frame_step=2))
    done('set_profile 25')
    assert ledger.stats['equalized']['whole'] == whole + 3 and ledger.stats['spectrogram']['calls'] == spec_calls
    bad = NoiseProfile(np.ones((3, 65)), s.fresolution, s.tresolution)
    n_eq = launched('spec_equalize')
    with pytest.raises(ValueError):
        e.set_profile(bad)
    assert launched('spec_equalize') == n_eq
    # the spectrogram's window changes: the profile and the template are stale, NaN down the graph, nothing raises
    s.update(nfft=512, overlap_frac=0.75)
    done('spectrogram 512')
    assert e.stale and m.stale and e.shape[2] == 257 and np.all(np.isnan(fl.peek(e))) and np.all(np.isnan(fl.peek(bp)))
    e.set_profile(g.estimate_noise_profile())
    done('set_profile 512')
    assert not e.stale and m.stale and e._mirror_valid(0, len(e._hostbuf))
    m.set_template(g.cut_template(39.3, 39.3 + 24/s.rate, 1500.0, 3000.0, 0, spec_name='equalized', floor_db=-40.0))
    done('set_template 512')
    g.update_times(37.5, 39.0)
    done('window 37.5')
    e.set_profile(None)
    done('no profile')
    # clear, then take a new one: the profile before is gone (its address is free for the next object of the same shape),
    # and what the device divides by must be the new one's values -- also after they were edited in place
    e.set_profile(g.estimate_noise_profile(percentile=75.0))
    done('a new profile after none')
    e.profile.values[:, ::2] *= np.float32(4.0)
    e.update()
    done('the profile edited in place')
    e.set_profile(None)
    assert e._dev_profile is None                                          # the device copy goes with the profile
    e.set_profile(g.estimate_noise_profile(percentile=75.0))
    done('the same kind of profile again')
    for t in (e, bp, pf, m):
        assert t._mirror_valid(0, len(t._hostbuf)), t.name
    for name in ('bin_quantiles', 'spec_equalize', 'band_power', 'spectral_features', 'template_match'):
        assert launched(name) > 0, name
    ledger.close()
