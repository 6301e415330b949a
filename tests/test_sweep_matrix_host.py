"""The sweep matrix (tests/test_gpu_sweep_matrix.py) must equal the launch tables, both ways: every instantiation of
chain_fwd_kernel and sos_ckpt_kernel that the sources can launch has a row, and every row is an instantiation.  Read from
the source text (no GPU, no build): the HD_CASE and HD_BARRIER lists of csrc/chain_shape.inc, the chain_w<nfft>_<hop>.hip
units of csrc/Makefile, the HD_CKPT list of csrc/sos.hip.  An instantiation added later without a row fails here."""

import os
import re

import test_gpu_sweep_matrix as matrix

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'audian_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def listed(text, macro):
    """The (a, b) of every `macro(a, b);` with literal arguments, in order (the #define itself has letters)."""
    return [(int(a), int(b)) for a, b in re.findall(r'\b%s\((\d+), *(\d+)\);' % macro, text)]


def shape_units():
    """(nfft, hop) of every chain_w<nfft>_<hop>.hip that the Makefile builds; each must be there and define its shape."""
    srcs = re.search(r'^SRCS *=(.*)$', source('Makefile'), re.M).group(1).split()
    shapes = []
    for unit in srcs:
        m = re.fullmatch(r'chain_w(\d+)_(\d+)\.hip', unit)
        if m:
            nfft, hop = int(m.group(1)), int(m.group(2))
            text = source(unit)
            assert re.search(r'#define CHAIN_SHAPE_NFFT %d\b' % nfft, text) and re.search(r'#define CHAIN_SHAPE_HOP %d\b' % hop, text), unit
            assert '#include "chain_shape.inc"' in text, unit
            shapes.append((nfft, hop))
    on_disk = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r'chain_w\d+_\d+\.hip', f))
    assert on_disk == sorted('chain_w%d_%d.hip' % s for s in shapes), 'a chain_w*.hip that the Makefile does not build'
    return shapes


def test_the_fused_rows_are_the_launch_table():
    inc = source('chain_shape.inc')
    cases, barriers = listed(inc, 'HD_CASE'), listed(inc, 'HD_BARRIER')
    assert len(set(cases)) == len(cases) == 12 and len(set(barriers)) == len(barriers) == 4
    # what the two macros stand for: each case launches with and without the dB image; the barrier list is compiled at
    # one shape only
    assert inc.count('if (want_db) HD_GO(A, B, true, true, false);') == 1 and inc.count('else HD_GO(A, B, true, false, false);') == 1
    assert inc.count('if (want_db) HD_GO(A, B, false, true, false);') == 1 and inc.count('else HD_GO(A, B, false, false, false);') == 1
    assert '#if CHAIN_SHAPE_NFFT == %d && CHAIN_SHAPE_HOP == %d' % matrix.BARRIER_SHAPE in inc and inc.count('HD_BARRIER(A, B)') == 1
    shapes = shape_units()
    assert len(shapes) == 6 and matrix.BARRIER_SHAPE in shapes
    built = {(nfft, hop, sf, se, db, False) for nfft, hop in shapes for sf, se in cases for db in (False, True)}
    built |= {matrix.BARRIER_SHAPE + (sf, se, db, True) for sf, se in barriers for db in (False, True)}
    rows = matrix.fused_rows()
    assert len(rows) == len(set(rows)) == 6*12*2 + 8
    assert set(rows) - built == set(), 'rows without an instantiation'
    assert built - set(rows) == set(), 'instantiations without a row'
    # ... and the parametrized test walks exactly these rows
    params = {(nfft, hop, sf) for nfft, hop, sf, _, _, _ in rows}
    assert params == {(nfft, hop, sf) for nfft, hop in matrix.SHAPES for sf in (1, 2, 3, 4)} and matrix.FUSED_ROWS == rows


def test_the_ckpt_rows_are_the_launch_table():
    sos = source('sos.hip')
    pairs = listed(sos, 'HD_CKPT')
    assert len(set(pairs)) == len(pairs) == 20
    # the macro: a prefetching build for pairs of at most two sections each, taken when "sos_prefetch" is on
    assert sos.count('if (pf && (A) <= 2 && (B) <= 2)') == 1
    assert sos.count('sos_ckpt_kernel<A, B, ((A) <= 2 && (B) <= 2)>') == 1 and sos.count('sos_ckpt_kernel<A, B, false>') == 1
    built = {(a, b, False) for a, b in pairs} | {(a, b, True) for a, b in pairs if a <= 2 and b <= 2}
    rows = matrix.ckpt_rows()
    assert len(rows) == len(set(rows)) == 16 + 4 and matrix.CKPT_ROWS == rows
    assert sum(1 for r in rows if r[2] == 0) == 4
    mine = {matrix.ckpt_instantiation(*r) for r in rows}
    assert len(mine) == len(rows)
    envelope = {matrix.ckpt_instantiation(*r) for r in matrix.envelope_rows()}          # SF = 0: test_envelope's
    assert all(r[0] == 0 for r in envelope) and all(r[0] > 0 for r in mine)
    assert mine == {r for r in built if r[0] > 0}, (mine ^ {r for r in built if r[0] > 0})
    assert envelope == {r for r in built if r[0] == 0}, (envelope ^ {r for r in built if r[0] == 0})
