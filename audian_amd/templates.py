"""Spectrogram templates: one example call cut out of a spectrogram, and its correlation with every window of a
spectrogram -- the second standard detector of bioacoustics beside the threshold on an envelope, and the reference's open
item "Provide interface for event detectors" (README.md:66-69).  The contract is the definition in ``include/hip_dsp.h``
(hipdsp_template_match); ``host_template_scores`` is that definition in numpy float64 (what a host-only graph computes),
``template_scores`` runs all templates over a spectrogram's buffer, on its device mirror when it has one."""

import numpy as np

from .bufferedspectrogram import decibel

MAX_TEMPLATES = 16          # per launch (hipdsp_tmplplan_set)
MAX_FRAMES, MAX_VALUES = 256, 65536
RESOLUTION_RTOL = 1e-9


class Template(object):
    """A patch of a spectrogram: `values` (Tt frames, Fb bins) float64 -- dB (re 1, floored at `floor_db`) with `log`,
    else the power itself -- whose lowest bin sits at `fmin` Hz, on a grid of `fresolution` Hz and `tresolution`
    seconds.  It fits every spectrogram of the same two resolutions whose band holds it."""

    def __init__(self, values, fmin, fresolution, tresolution, log=True, floor_db=-120.0, name='template'):
        values = np.array(values, dtype=np.float64)
        if values.ndim != 2 or values.size == 0:
            raise ValueError('template values must be shape (frames, bins), at least one of each')
        if not np.all(np.isfinite(values)):
            raise ValueError('template values must be finite (cut with a floor_db, not through silence at -inf dB)')
        if values.shape[0] > MAX_FRAMES or values.size > MAX_VALUES:
            raise ValueError(f'a template holds at most {MAX_FRAMES} frames and {MAX_VALUES} values, '
                             f'got {values.shape[0]} x {values.shape[1]}')
        self.values = values
        self.fmin, self.fresolution, self.tresolution = float(fmin), float(fresolution), float(tresolution)
        self.log, self.floor_db, self.name = bool(log), float(floor_db), str(name)

    @property
    def duration(self):
        return self.values.shape[0]*self.tresolution

    @property
    def bandwidth(self):
        return self.values.shape[1]*self.fresolution

    @property
    def floor(self):
        """The floor of the values the template is compared with: floor_db in dB, none for powers."""
        return self.floor_db if self.log else -np.inf

    def first_bin(self, spec):
        """The bin of `spec` (a BufferedSpectrogram) the template's lowest bin lies on.  ValueError when the
        resolutions differ (relative 1e-9) or the band does not fit into the spectrogram's bins."""
        for what, mine, its in (('fresolution', self.fresolution, float(spec.fresolution)),
                                ('tresolution', self.tresolution, float(spec.tresolution))):
            if not abs(mine - its) <= RESOLUTION_RTOL*abs(its):
                raise ValueError(f'template {self.name}: {what} {mine!r} is not the spectrogram\'s {its!r}')
        nfreq = int(spec.shape[2])
        k0 = int(round(self.fmin/self.fresolution))
        if k0 < 0 or k0 + self.values.shape[1] > nfreq:
            raise ValueError(f'template {self.name}: bins [{k0}, {k0 + self.values.shape[1]}) do not fit into the '
                             f'spectrogram\'s {nfreq}')
        return k0

    def save(self, path):
        np.savez(path, values=self.values, fmin=self.fmin, fresolution=self.fresolution, tresolution=self.tresolution,
                 log=self.log, floor_db=self.floor_db, name=self.name)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z['values'], float(z['fmin']), float(z['fresolution']), float(z['tresolution']), bool(z['log']),
                       float(z['floor_db']), str(z['name']))


def default_pivot(values):
    """The pivot a launch takes by default: the mean of the templates' own values, as float32."""
    return float(np.float32(np.mean(np.asarray(values, dtype=np.float64))))


def host_values(power, log, floor):
    """v of the definition for a float64 array of powers: decibel (re 1, -inf at 0) with `log`, then the floor."""
    with np.errstate(invalid='ignore'):
        v = decibel(power, 1.0, 0.0) if log else np.array(power, dtype=np.float64)
        return np.where(v < floor, floor, v)


def host_template_scores(slab, values, k0, first, n_out, normalize=True, log=True, floor=-np.inf, min_std=0.0,
                         block=1 << 22):
    """hipdsp_template_match in numpy float64 on a host slab (frames, channels, nfreq) of powers: the scores of the
    templates `values` (K, Tt, Fb) over the windows that start at frame first + i, i < n_out, as float32
    (K, channels, n_out).  The taps are hipdsp_template_prepare_host's (float32); only the order of the sums is
    numpy's."""
    from . import hipdsp
    taps, _, q = hipdsp.template_prepare(values, normalize)
    K, Tt, Fb = taps.shape
    n = Tt*Fb
    g = taps.reshape(K, n).astype(np.float64)
    slab = np.asarray(slab)
    frames, channels = slab.shape[:2]
    out = np.full((K, channels, max(0, int(n_out))), np.nan)
    lo, hi = max(0, -int(first)), min(int(n_out), frames - Tt + 1 - int(first))
    if hi <= lo or channels == 0:
        return out.astype(np.float32)
    v = host_values(np.asarray(slab[first + lo:first + hi - 1 + Tt, :, k0:k0 + Fb], dtype=np.float64), log, floor)
    win = np.lib.stride_tricks.sliding_window_view(v, Tt, axis=0)        # (windows, channels, Fb, Tt)
    rows = max(1, block//n)
    with np.errstate(all='ignore'):
        for a in range(0, hi - lo, rows):
            w = win[a:a + rows].transpose(0, 1, 3, 2).reshape(-1, channels, n)
            if normalize:
                finite = np.all(np.isfinite(w), axis=2)
                d = w - np.mean(w, axis=2, keepdims=True)
                D = np.sum(d*d, axis=2)
                r = np.einsum('kn,wcn->kwc', g, d)/np.sqrt(q[:, None, None]*D[None])
                r = np.where((finite & (D > n*float(min_std)**2))[None], np.clip(r, -1.0, 1.0), np.nan)
            else:
                r = np.einsum('kn,wcn->kwc', g, w)
            out[:, :, lo + a:lo + a + len(w)] = r.transpose(0, 2, 1)
    with np.errstate(over='ignore'):
        return out.astype(np.float32)


def _groups(templates, spec):
    """The templates in groups that one launch serves: equal shape, first bin, log and floor, at most 16 each, in
    the order of their first member: [(k0, log, floor, [indices])]."""
    keyed = {}
    for j, t in enumerate(templates):
        key = (t.values.shape, t.first_bin(spec), t.log, t.floor)
        keyed.setdefault(key, []).append(j)
    out = []
    for (shape, k0, log, floor), idx in keyed.items():
        for a in range(0, len(idx), MAX_TEMPLATES):
            out.append((k0, log, floor, idx[a:a + MAX_TEMPLATES]))
    return out


def template_scores(spec, templates, i0=None, i1=None, normalize=True, min_std=0.1, pivot=None):
    """All `templates` (Template objects) over frames [i0, i1) of the spectrogram trace `spec` (absolute frame indices
    inside its current buffer; by default the whole buffer): row k holds at frame t the score of template k against
    the window that starts at frame t - Tt_k//2 -- a peak of the row is the middle of a call -- and NaN where that
    window leaves the buffer.  The templates are grouped by shape, band and value transform, 16 per launch.  With a
    valid device mirror the result is ONE (K, channels, i1 - i0) float32 device array and nothing crosses PCIe;
    without one (a host-only graph) it is that array in numpy, from host_template_scores.  `pivot` None: the mean of
    each group's templates.  ValueError, before anything is launched, for a template that does not fit the
    spectrogram."""
    from . import hipdsp
    templates = list(templates)
    n_buf = len(spec._hostbuf)
    a = 0 if i0 is None else int(i0) - spec.offset
    b = n_buf if i1 is None else int(i1) - spec.offset
    if a < 0 or b > n_buf or b < a:
        raise IndexError('range outside the loaded buffer')
    groups = _groups(templates, spec)
    for k0, log, floor, idx in groups:                                   # refusals before any launch
        hipdsp.template_prepare(np.stack([templates[j].values for j in idx]), normalize)
    if not float(min_std) >= 0:
        raise ValueError(f'min_std must be >= 0, got {min_std}')
    K, C, m, F = len(templates), spec.channels, b - a, int(spec.shape[2])
    on_device = m > 0 and C > 0 and K > 0 and spec._mirror_valid(0, n_buf)
    if not on_device:
        out = np.full((K, C, m), np.nan, dtype=np.float32)
        if m > 0 and C > 0:
            for k0, log, floor, idx in groups:
                values = np.stack([templates[j].values for j in idx])
                out[idx] = host_template_scores(spec.buffer[:], values, k0, a - values.shape[1]//2, m, normalize, log,
                                                floor, min_std)
        return out
    out = hipdsp.DeviceArray(spec.ctx, (K, C, m), np.float32)
    plan = hipdsp.TmplPlan(spec.ctx)
    for k0, log, floor, idx in groups:
        values = np.stack([templates[j].values for j in idx])
        plan.set(values, normalize)
        in_place = idx == list(range(idx[0], idx[0] + len(idx)))         # the group's rows lie together in `out`
        rows = out.view(idx[0]*C*m, (1,)) if in_place else hipdsp.DeviceArray(spec.ctx, (len(idx), C, m), np.float32)
        hipdsp.template_match(spec.ctx, plan, spec._dev, spec._pitch(), C, n_buf, F, k0, a - values.shape[1]//2, m, rows,
                              db=log, ref_power=1.0, min_power=0.0, floor=floor,
                              pivot=default_pivot(values) if pivot is None else pivot, min_std=min_std)
        if not in_place:
            for i, j in enumerate(idx):                                  # a group scattered among the others
                hipdsp.memcpy2d(spec.ctx, out.view(j*C*m, (1,)), 4*C*m, rows.view(i*C*m, (1,)), 4*C*m, 4*C*m, 1)
            spec.ctx.synchronize()
            rows.free()
    plan.close()           # waits for the stream
    return out
