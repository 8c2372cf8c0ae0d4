"""CPU tests of the restricted Jacobian kernels' geometry: which spans of a
block an evaluation into a registered output writes again
(``codegen.program.kept_spans``), how many 128-byte lines that is, and what
the printer makes of it (``opty_jac_var`` / ``opty_conjac_var``)."""
import re

import pytest

from examples import problems
from opty_amd import ConstraintCollocator
from opty_amd.codegen.program import (SKIP_MIN_RUN, kept_lines_per_node,
                                      kept_spans, line_owner_ranges,
                                      varying_entries)

#: the fixtures of test_varying_entries_against_the_reference_values
FIXTURES = ['config3_10link_small', 'pend2_link_vardur_unkmass_small',
            'gaitlike_3link_be_small', 'chaplygin_be_small', 'msd_be_small']


def _program(name, **kw):
    col = ConstraintCollocator(**kw, **problems.build(name))
    return col, col._build_program()


def test_kept_spans_of_the_10link_pendulum():
    """One kept span.  Rows 0..10 (entries [0, 495)) hold no varying entry,
    the first one is 496, the last one 987: the span is [496, 988) -- inside
    [495, 989), the rows' extent, and its line-rounded equivalent (the owner
    range of the waves) is [480, 988).  The skipped run wraps from one node's
    block into the next (2 + 496 entries)."""
    _, prog = _program('config3_10link_small')
    var = varying_entries(prog)
    assert (prog.P, len(var), var[0], var[-1]) == (990, 330, 496, 987)
    assert not [e for e in var if e < 495]
    spans = kept_spans(prog)
    assert spans == [(496, 988)]
    assert 495 <= spans[0][0] and spans[0][1] <= 989
    assert line_owner_ranges(prog) == [(480, 988)]
    # static gaps inside the span are shorter than a line
    inside = sorted(set(range(496, 988)) - set(var))
    runs, n = [], 0
    for a, b in zip(inside, inside[1:] + [None]):
        n += 1
        if b != a + 1:
            runs.append(n)
            n = 0
    assert max(runs) <= 12


def test_line_count_of_the_10link_pendulum():
    """Lines per node that hold a varying entry, averaged over the 16 line
    phases of a node's row: 31.69 of 61.88 (the issue's 31.6 / 61.9) -- 4056
    of 7920 bytes.  The kernels round the first owner down to a line of the
    block (480 instead of 481): 31.75 lines."""
    _, prog = _program('config3_10link_small')
    kept, total = kept_lines_per_node(prog)
    assert total == 990/16.0 and abs(total - 61.9) < 0.05
    assert kept == 507/16.0 and abs(kept - 31.6) < 0.1
    (lo, hi), = line_owner_ranges(prog)
    assert (hi - lo)/16.0 == 31.75


@pytest.mark.parametrize('name', FIXTURES)
def test_every_varying_entry_is_kept(name):
    _, prog = _program(name)
    spans = kept_spans(prog)
    var = varying_entries(prog)
    assert spans == sorted(spans) and all(0 <= a < b <= prog.P
                                          for a, b in spans)
    for e in var:
        assert any(a <= e < b for a, b in spans)
    # what is skipped between two spans is a run worth skipping
    for (_, b), (c, _) in zip(spans, spans[1:]):
        assert c - b >= SKIP_MIN_RUN
    # the lines a wave owns (first entry in its range) cover every line that
    # holds a varying entry, in every phase, and never start before the block
    for lo, hi in line_owner_ranges(prog, spans):
        assert lo >= 0 and lo % 16 == 0
    owners = line_owner_ranges(prog, spans)
    if owners:
        for e in var:
            for first in range(e - 15, e + 1):      # the line's first entry
                assert any(lo <= first < hi for lo, hi in owners)


@pytest.mark.parametrize('name,kw', [
    ('msd_be_small', {}), ('pend2_link_vardur_unkmass_small', {}),
    ('gaitlike_3link_be_small', {}), ('biped_small', {}),
    ('config3_10link_small', dict(jacobian_layout='csr')),
    ('config3_10link_small', dict(prune_zeros=True))])
def test_nothing_to_skip_no_variant(name, kw):
    """Small blocks flushed as one span, blocks whose static entries read an
    unknown parameter / a free interval or come in short runs only, and the
    opt-in layouts get no restricted kernels."""
    col, _ = _program(name, **kw)
    source, meta = col.generate_source()
    assert 'jac_var' not in meta['kernels']
    assert 'conjac_var' not in meta['kernels']
    assert 'restricted' not in meta
    assert 'opty_jac_var' not in source and 'opty_conjac_var' not in source


@pytest.mark.parametrize('launch_nodes', [None, 99999, 12500])
def test_restricted_kernels_stage_only_the_kept_spans(launch_nodes):
    """The generated ``opty_jac_var`` / ``opty_conjac_var`` of the 10-link
    pendulum: strips cut inside the owner range, every ring write and every
    flush within [480, 988 + 15) (past 990: the next node's first entries),
    no head piece, and the per-entry code of the full kernel."""
    col, prog = _program('config3_10link_small', launch_nodes=launch_nodes)
    source, meta = col.generate_source()
    (lo, hi), = meta['restricted']['owner_ranges']
    assert (lo, hi) == (480, 988)
    for key, name in (('groups', 'opty_jac_var'),
                      ('fused_groups', 'opty_conjac_var')):
        strips = sorted(tuple(rg) for grp in meta['restricted'][key]
                        for rg in grp)
        assert strips[0][0] == lo and strips[-1][1] == hi
        assert all(a[1] == b[0] for a, b in zip(strips, strips[1:]))
        assert all(a % 16 == 0 for a, _ in strips)
        body = source[source.index('\n%s(' % name):]
        body = body[:body.index('\n}\n')]
        assert 'opty_head_piece' not in body
        printed = [tuple(int(x) for x in m) for m in
                   re.findall(r'// strip (\d+) (\d+)', body)]
        assert sorted(printed) == strips
        flushes = re.findall(
            r'opty_flush_lines<\d+, (\d+), \d+>\(ring, jrow, 990, b0, '
            r'(-?\d+), \d+, (\d+), (\d+), (\d+), nvalid, lane\);', body)
        assert flushes
        R = int(flushes[0][0])
        for _, c_lo, own_lo, own_hi, avail in flushes:
            assert (int(own_lo), int(own_hi)) in strips
            assert lo - 15 <= int(c_lo) and int(avail) <= hi + 15
        # ring rows written: those of the staged entries of the strips
        rows = {int(m)//65 for m in
                re.findall(r'ring\[(\d+) \+ lane\] = ', body)}
        want = {v % R for a, b in strips for v in range(a, b + 15)}
        assert rows == want
    names = re.findall(r'\n(opty_[a-z_]+)\(', source)
    assert names.count('opty_jac_var') == names.count('opty_conjac_var') == 1
    assert meta['kernels']['jac_var']['persist'] == 0


def test_restricted_option_and_block_size_rule():
    """``EmitOptions(restricted=0)`` prints no restricted kernels; the
    automatic rule leaves them out of blocks beyond ``RESTRICTED_MAX_P``
    entries (their two extra kernels would make the builds of 24-link
    systems half as long again) unless ``restricted=1`` asks for them."""
    from opty_amd.codegen import emit_hip
    from opty_amd.codegen.emit_hip import EmitOptions, emit_module
    _, prog = _program('config3_10link_small')
    assert prog.P <= emit_hip.RESTRICTED_MAX_P < 5100
    _, meta = emit_module(prog, EmitOptions(restricted=0))
    assert 'jac_var' not in meta['kernels']
    _, meta = emit_module(prog, EmitOptions())
    assert 'jac_var' in meta['kernels']
    cap = emit_hip.RESTRICTED_MAX_P
    try:
        emit_hip.RESTRICTED_MAX_P = prog.P - 1
        _, meta = emit_module(prog, EmitOptions())
        assert 'jac_var' not in meta['kernels']
        _, meta = emit_module(prog, EmitOptions(restricted=1))
        assert 'jac_var' in meta['kernels']
    finally:
        emit_hip.RESTRICTED_MAX_P = cap
    assert 'restricted' not in EmitOptions().key()
    assert 'restricted=1' in EmitOptions(restricted=1).key()
