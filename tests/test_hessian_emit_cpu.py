"""CPU tests of the source ``codegen/emit_hessian.py`` emits: the strip cut,
the tiling of a node's PH entries by the LDS tile flushes, the strip switch,
and which flush variants the problems of tests/test_hessian_kernel_gpu.py
instantiate (so that a change of the cut cannot silently take a variant out
of the GPU suite)."""
import pytest

import hessian_cases as hc

from examples import problems
from opty_amd.codegen.emit_hessian import (CHUNK, emit_hessian_module,
                                           strips)

LABELS = sorted(hc.KERNEL_PROBLEMS) + ['config3_10link_small']
BUDGETS = (1500, 200, 40)

_COLS = {}


def _col(label):
    """One collocator per problem, shared (the Hessian program is built
    once and never changed)."""
    if label not in _COLS:
        if label in hc.KERNEL_PROBLEMS:
            _COLS[label] = hc.collocator(label, 65)
        else:
            import opty_amd
            _COLS[label] = opty_amd.ConstraintCollocator(
                **problems.build(label))
    return _COLS[label]


@pytest.mark.parametrize('label', LABELS)
def test_strips_partition_the_entries(label):
    prog = _col(label)._build_hessian_program()
    assert prog.PH == len(prog.hess_out) > 0
    for budget in BUDGETS + (1, 10**9):
        cut = strips(prog, budget)
        assert cut[0][0] == 0 and cut[-1][1] == prog.PH, (budget, cut)
        for (a0, a1), (b0, b1) in zip(cut, cut[1:]):
            assert a1 == b0, (budget, cut)
        assert all(e0 < e1 for e0, e1 in cut), (budget, cut)
    assert len(strips(prog, 10**9)) == 1


@pytest.mark.parametrize('forget', [False, True])
@pytest.mark.parametrize('budget', BUDGETS)
@pytest.mark.parametrize('label', LABELS)
def test_flushes_tile_the_block_and_cases_match_the_cut(label, budget,
                                                        forget):
    col = _col(label)
    prog = col._build_hessian_program()
    PH = prog.PH
    source, cut = emit_hessian_module(prog, budget, forget)
    assert cut == strips(prog, budget)
    # the switch: case s for every strip of the cut, no others, and the
    # descriptor's strip count (the grid's y extent) is that number
    cases = hc.switch_cases(source)
    assert [s for s, _ in cases] == list(range(len(cut)))
    assert hc.descriptor(col, cut)['strips'] == len(cases)
    # the flushes of strip s tile [e0, e1) once, in order ...
    at = 0
    for (s, text), (e0, e1) in zip(cases, cut):
        assert at == e0, (s, at, e0)
        calls = hc.flush_calls(text)
        assert calls, ('no flush in case', s)
        for kind, w, c0, pitch in calls:
            assert c0 == at, ('gap or overlap', s, c0, at)
            assert 1 <= w <= CHUNK, (s, w)
            assert pitch == PH, (s, pitch)
            if kind == 16:
                assert PH % 2 == 0 and c0 % 2 == 0 and w % 2 == 0, \
                    ('misaligned 16-byte flush', s, PH, c0, w)
            at += w
        assert at == e1, (s, at, e1)
    # ... and all of them [0, PH); none hides outside the switch
    assert at == PH
    assert len(hc.flush_calls(source)) == \
        sum(len(hc.flush_calls(text)) for _, text in cases)
    # ``forget`` changes what a chunk recomputes, never what is flushed
    if forget:
        plain, _ = emit_hessian_module(prog, budget, False)
        assert hc.flush_calls(plain) == hc.flush_calls(source)


def test_uniform_trig_twin_has_the_same_flushes():
    prog = _col('A')._build_hessian_program()
    one, cut1 = emit_hessian_module(prog, *hc.DEFAULT_VARIANT)
    two, cut2 = emit_hessian_module(prog, 1500, False, 2)
    assert cut1 == cut2 and one != two
    assert hc.flush_calls(one) == hc.flush_calls(two)


def flush_variants():
    """``{variant name: [(label, (budget, forget, fast_trig)), ...]}`` over
    the modules the GPU file launches (``hessian_cases.GPU_MODULES``)."""
    table = {}
    for label, variant in hc.GPU_MODULES:
        prog = _col(label)._build_hessian_program()
        source, cut = emit_hessian_module(prog, *variant)
        for (s, text), (e0, e1) in zip(hc.switch_cases(source), cut):
            for kind, w, c0, _ in hc.flush_calls(text):
                names = ['flush%d<%d>' % (kind, w)]
                if kind == 16 and w < CHUNK and c0 > 0:
                    names.append('flush16<w<16> at c0>0')
                if kind == 8 and prog.PH % 2 == 0 and e0 % 2 == 1:
                    names.append('flush8 in a strip that starts odd, even PH')
                for n in names:
                    hit = (label, variant)
                    if hit not in table.setdefault(n, []):
                        table[n].append(hit)
    return table


def test_gpu_problems_cover_every_flush_variant(capsys):
    table = flush_variants()
    with capsys.disabled():
        print()
        for name in sorted(table):
            print('  %-44s %s' % (name, ', '.join(
                '%s%s' % (k, '' if v == hc.DEFAULT_VARIANT else list(v))
                for k, v in table[name])))
    for name in ('flush16<16>', 'flush16<w<16> at c0>0', 'flush8<16>',
                 'flush8 in a strip that starts odd, even PH'):
        assert name in table, 'no GPU problem instantiates ' + name
    # at the default budget, as the table of problems promises
    default = {n: {k for k, v in hits if v == hc.DEFAULT_VARIANT}
               for n, hits in table.items()}
    assert {'A', 'B', 'C', 'D'} <= default['flush16<16>']
    assert 'A' in default['flush16<4>'] and 'B' in default['flush16<8>']
    assert 'C' in default['flush16<14>']
    assert 'E' in default['flush8<16>'] and 'E' in default['flush8<5>']
    assert 'D' in default['flush8 in a strip that starts odd, even PH']
    assert 'D' in default['flush8<16>']
