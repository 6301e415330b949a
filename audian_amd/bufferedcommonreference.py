"""Common-reference subtraction on the fly: the reference's "Subtract common mean" plug-in (README.md:61) as a derived
trace, and the median across channels that arrays use instead -- one loud channel does not leak into the others with
opposite sign.  Placed between ``data`` and ``filtered`` it takes hum, handling noise and crosstalk that sit on every
channel off everything below it.  ``process()`` is one ``hipdsp_common_reference`` call from the source's device mirror
(the loader's slab on the device when the source is the recording itself) into this trace's."""

import numpy as np

from .buffereddata import BufferedData

METHODS = ('mean', 'median')


def common_reference_host(x, group, use, method):
    """The definition of hipdsp_common_reference on a (frames, channels) array, in numpy: the samples as float32, all
    arithmetic in float64, one rounding to float32 at the end.  The mean's sum runs over the reference channels one by
    one in ascending order; a NaN among them makes the reference NaN."""
    x = np.asarray(x)
    x32 = x.reshape(len(x), -1).astype(np.float32)
    x64 = x32.astype(np.float64)
    y = x32.copy()
    group = np.asarray(group)
    use = np.ones(len(group), dtype=bool) if use is None else np.asarray(use, dtype=bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in np.unique(group[group >= 0]):
            members = np.flatnonzero(group == g)
            refs = members[use[members]]
            if method == 'mean':
                s = np.zeros(len(x64))
                for c in refs:
                    s = s + x64[:, c]
                ref = s/float(len(refs))
            else:
                v = np.sort(x64[:, refs], axis=1)                 # NaNs go last
                n = len(refs)
                ref = v[:, n//2] if n % 2 else (v[:, n//2 - 1] + v[:, n//2])*0.5
                ref = np.where(np.isnan(v[:, -1]), np.nan, ref)
            y[:, members] = (x64[:, members] - ref[:, None]).astype(np.float32)
    return y


class BufferedCommonReference(BufferedData):
    """``source - reference`` per group of channels, the reference the mean or the median over the group's channels that
    are not in `exclude`.  `groups`: None for all channels in one group, or a list of channel lists, one group each
    (channels in no list pass through unchanged).  `exclude`: channels (dead, clipping) that get the reference taken off
    but do not contribute to it.  Same rate, shape, unit and amplitude range as the source, no pre- or post-roll."""

    def __init__(self, name='rereferenced', source='data', panel='trace', method='mean', groups=None, exclude=(),
                 color='#008888', lw_thin=1.1, lw_thick=2):
        BufferedData.__init__(self, name, source, tbefore=0, panel=panel, panel_type='trace', color=color,
                              lw_thin=lw_thin, lw_thick=lw_thick)
        self.method, self.groups, self.exclude = method, groups, tuple(exclude)
        self.group, self.use = None, None              # per channel: group id or -1; contributes to the reference

    def open(self, source):
        if len(getattr(source, 'shape', (0, 0))) != 2:
            raise ValueError(f'{self.name}: the source {source.name!r} is not a trace of (frames, channels)')
        BufferedData.open(self, source)
        self.update()

    def update(self, method=None, groups=None, exclude=None):
        """A new method, grouping or list of excluded channels (None: as it is; one group of all channels is
        ``groups=[range(channels)]``).  Raises ValueError for a bad one and then changes nothing.  Recomputes this
        trace and what hangs below it, never the source."""
        method = self.method if method is None else method
        groups = self.groups if groups is None else [list(g) for g in groups]
        exclude = self.exclude if exclude is None else tuple(exclude)
        if self.source is None:                        # not open yet: open() checks them against the channels
            self.method, self.groups, self.exclude = method, groups, exclude
            return
        group, use = self._table(method, groups, exclude)
        self.method, self.groups, self.exclude, self.group, self.use = method, groups, exclude, group, use
        self.recompute_all()

    def _table(self, method, groups, exclude):
        """(group id or -1, use flag) per channel of the source; ValueError when the arguments do not describe one."""
        C = self.channels
        if method not in METHODS:
            raise ValueError(f'method {method!r}: one of {METHODS}')

        def channel(c, what):
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 0 <= c < C:
                raise ValueError(f'{what}: channel {c!r} is not one of 0 ... {C - 1}')
            return int(c)

        group = np.full(C, -1, dtype=np.int32)
        if groups is None:
            group[:] = 0
        else:
            for g, chans in enumerate(groups):
                if g >= C:
                    raise ValueError(f'groups: more groups than the {C} channels')
                chans = [channel(c, 'groups') for c in chans]
                if not chans:
                    raise ValueError(f'groups: group {g} is empty')
                for c in chans:
                    if group[c] >= 0:
                        raise ValueError(f'groups: channel {c} is listed twice')
                    group[c] = g
        use = np.ones(C, dtype=bool)
        for c in exclude:
            use[channel(c, 'exclude')] = False
        for g in np.unique(group[group >= 0]):
            if not np.any(use[group == g]):
                raise ValueError(f'exclude: no channel of group {g} is left for the reference')
        return group, use

    def process(self, source, dest, nbefore):
        """dest = source[nbefore:] minus its groups' references (common_reference_host is the definition)."""
        from . import hipdsp
        self._check_lengths(source, dest, nbefore)
        call = self._take_call(source, dest)
        if len(dest) == 0:
            return
        if self._source_mirror(call) is not None or (call is not None and not isinstance(self.source, BufferedData)):
            # the source's mirror, or the loader's slab uploaded as the filter does it (kept between recomputes)
            dsrc, spitch, keep = self._device_source(source, call)
            ddst, dpitch, is_mirror = self._device_dest(dest, call)
            hipdsp.common_reference(self.ctx, dsrc.view(nbefore, (1,)), spitch, ddst, dpitch, self.channels, len(dest),
                                    self.group, self.use, self.method)
            self._finish_dest(dest, ddst, dpitch, is_mirror, call)
            if keep is not None or not is_mirror:
                self.ctx.synchronize()
            return
        # a derived source without a mirror (a host-only graph), or plain arrays: the same definition in numpy
        slab = np.asarray(source[nbefore:]).reshape(len(dest), -1)
        dest[...] = common_reference_host(slab, self.group, self.use, self.method).reshape(dest.shape)
        self._host_wrote(call)
