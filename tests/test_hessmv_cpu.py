"""CPU tests of the host statement of the Hessian operator
(``codegen/program.py``: ``hessian_side_table`` / ``assemble_hessmv``, the
decomposition ``opty_hessmv`` implements) against ``scipy.sparse`` on the
triplets, with random values: no GPU is needed."""
import numpy as np
import pytest

import hessmv_cases as mc

from opty_amd.codegen.program import assemble_hessmv, hessian_side_table

NODE_CASES = [(k, m) for k in 'ABCDE' for m in mc.CPU_EDGES] + \
    [('vardur_pendulum_small', None)]
OBJECTIVE_CASES = [(name, m) for name in ('trig_be', 'all_mid')
                   for m in mc.CPU_EDGES]


def _draw(seed, nnz, num_free):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, nnz), rng.uniform(-1.0, 1.0, num_free)


@pytest.mark.parametrize('label,ncn', NODE_CASES)
def test_node_section_and_instance_entries(label, ncn):
    N, nrows, ntail, pattern, rows, cols = mc.node_tables(label, ncn)
    PH = len(pattern)
    num_free = nrows*N + ntail
    at = (N - 1)*PH
    if label == 'C':
        assert len(rows) > at       # it has an instance entry
    if label == 'vardur_pendulum_small':
        # the free interval h is the last tail entry and has node entries
        assert np.any(rows[:at] == num_free - 1)
    values, v = _draw(21, len(rows), num_free)
    y = assemble_hessmv(N, nrows, ntail, values, v, pattern,
                        inst_rows=rows[at:], inst_cols=cols[at:])
    mc.check('%s N-1=%s' % (label, N - 1), y, num_free, rows, cols, values,
             v)


@pytest.mark.parametrize('name,ncn', OBJECTIVE_CASES)
def test_objective_section_alone(name, ncn):
    N = ncn + 1
    nrows, r, pattern, pairs, base = mc.objective_program(name)
    rows, cols = mc.objective_tables(name, N)
    num_free = nrows*N + r
    tail = nrows*N
    values, v = _draw(22, len(rows), num_free)
    y = assemble_hessmv(N, nrows, r, values, v, (), obj_pattern=pattern,
                        obj_base=base, tail_rows=tail + pairs[:, 0],
                        tail_cols=tail + pairs[:, 1])
    mc.check('%s N=%d' % (name, N), y, num_free, rows, cols, values, v)


def test_both_sections_in_one_product():
    """Constraint triplets of problem C (instance entry, unknown parameter)
    and an objective section over the same free vector, as ``Problem.
    hessian`` lays them out."""
    N, nrows, ntail, pattern, crows, ccols = mc.node_tables('C', 65)
    at = (N - 1)*len(pattern)
    assert ntail and len(crows) > at
    # an objective pattern on C's own rows: both diagonals of row 0, a
    # coupling of row 0 and the last row, a row-tail and a tail-tail entry
    last = nrows - 1
    obj = np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1),
                    (last, 1, 0, 0), (-1, 0, 0, 1), (-1, 0, -1, 0)],
                   dtype=np.int32)
    from opty_amd.objective import objective_hessian_indices
    pairs = np.array([(0, 0)], dtype=np.int64)
    orows, ocols = objective_hessian_indices(obj, pairs, nrows, 0, N,
                                             'midpoint')
    assert np.all(orows >= ocols)
    num_free = nrows*N + ntail
    rows, cols = np.r_[crows, orows], np.r_[ccols, ocols]
    values, v = _draw(23, len(rows), num_free)
    tail = nrows*N
    y = assemble_hessmv(N, nrows, ntail, values, v, pattern,
                        inst_rows=crows[at:], inst_cols=ccols[at:],
                        obj_pattern=obj, obj_base=0,
                        tail_rows=tail + pairs[:, 0],
                        tail_cols=tail + pairs[:, 1])
    mc.check('C + objective', y, num_free, rows, cols, values, v)


@pytest.mark.parametrize('label', list('ABCDE'))
def test_side_table(label):
    """Every ``(row, slot)`` of both patterns has exactly one slot, tails
    come after trajectories, and the entries name the sides they had."""
    _, nrows, ntail, pattern, _, _ = mc.node_tables(label, 65)
    _, _, obj, _, base = mc.objective_program('all_mid')
    obj = obj[np.all(obj[:, (0, 2)] < nrows, axis=1)]
    sides, ntraj, entries, obj_entries = hessian_side_table(pattern, obj,
                                                            base)
    assert len(set(sides)) == len(sides)
    assert all(row >= 0 and slot in (0, 1) for row, slot in sides[:ntraj])
    assert all(row == -1 for row, _ in sides[ntraj:])
    assert sides[:ntraj] == sorted(sides[:ntraj])
    assert sides[ntraj:] == sorted(sides[ntraj:])
    want = set()
    for pat, b, table in ((pattern, 0, entries), (obj, base, obj_entries)):
        assert len(table) == len(pat)
        for (ra, oa, rb, ob), (sa, sb) in zip(pat.tolist(), table):
            a = (ra, oa + b) if ra >= 0 else (-1, oa)
            c = (rb, ob + b) if rb >= 0 else (-1, ob)
            assert sides[sa] == a and sides[sb] == c
            want |= {a, c}
    assert set(sides) == want


def test_side_table_refuses_what_the_kernel_cannot_index():
    with pytest.raises(ValueError, match='slot'):
        hessian_side_table([(0, 2, 0, 0)])
    with pytest.raises(ValueError, match='slot'):
        hessian_side_table([], [(0, 1, 0, 0)], 1)
    with pytest.raises(ValueError):
        hessian_side_table([(-2, 0, 0, 0)])
