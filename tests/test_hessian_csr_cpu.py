"""CPU tests of the host statement of the CSR Hessian (``codegen/program.py``:
``hessian_csr_structure`` / ``assemble_hessian_csr``, the decomposition
``opty_hesscsr`` implements) against ``scipy.sparse`` and ``np.add.at`` on the
triplets with random values, of the bindings and of the refusals: no GPU is
needed."""
import ctypes
import os

import numpy as np
import pytest

import hessian_csr_cases as cc

from examples import problems
from opty_amd.codegen.program import (assemble_hessian_csr,
                                      hessian_csr_structure)

NODE_CASES = [(k, m) for k in 'ABCDE' for m in cc.CPU_EDGES] + \
    [(name, None) for name in cc.ZOO]
OBJECTIVE_CASES = [(name, m) for name in ('trig_be', 'all_mid')
                   for m in cc.CPU_EDGES]


def _hold(what, N, nrows, ntail, desc, rows, cols, seed):
    """Structure, slots and values of one case; returns ``(reference,
    slot)``."""
    num_free = nrows*N + ntail
    values = np.random.default_rng(seed).uniform(-1.0, 1.0, len(rows))
    ref = cc.Reference(num_free, nrows*N, N - 1, rows, cols, values)
    indptr, indices, slot = hessian_csr_structure(N, nrows, ntail, **desc)
    cc.check_structure(what, ref, indptr, indices)
    # every triplet lands on its own pair
    assert slot.dtype == np.int64 and slot.shape == rows.shape
    row_of = np.repeat(np.arange(num_free), np.diff(indptr))
    assert np.array_equal(row_of[slot], rows), what
    assert np.array_equal(indices[slot], cols), what
    assert np.array_equal(slot, ref.group), what
    data = assemble_hessian_csr(N, nrows, ntail, values, **desc)
    cc.check_values(what, ref, data)
    return ref, slot


@pytest.mark.parametrize('label,ncn', NODE_CASES)
def test_node_section_and_instance_entries(label, ncn):
    N, nrows, ntail, desc, rows, cols = cc.node_descriptor(label, ncn)
    ref, _ = _hold('%s N-1=%s' % (label, N - 1), N, nrows, ntail, desc, rows,
                   cols, 61)
    distinct, triplets = len(ref.count), len(rows)
    # what keeps a case from hiding a failure
    if label in 'ABCD' and (N - 1 >= 2 or label == 'C'):
        assert distinct < triplets
    if label in ('E', 'config3_10link_small'):
        assert distinct == triplets         # a pure reordering
    if label == 'C':
        assert len(desc['inst_rows']) > 0
    if label == 'vardur_pendulum_small':
        assert N - 1 == 59 and int(ref.long.sum()) == 3
        assert np.all(ref.count[ref.long] == N - 1)
        assert (triplets, distinct) == (826, 362)
    if label == 'pend2_link_vardur_unkmass_small':
        assert ref.long.any()


def test_counts_of_the_midpoint_problems():
    for label, want in (('B', (2600, 1896)), ('D', (12350, 9150))):
        N, nrows, ntail, desc, rows, cols = cc.node_descriptor(label, 65)
        indptr = hessian_csr_structure(N, nrows, ntail, **desc)[0]
        assert (len(rows), int(indptr[-1])) == want


@pytest.mark.parametrize('name,ncn', OBJECTIVE_CASES)
def test_objective_section_alone(name, ncn):
    N, nrows, r, desc, rows, cols = cc.objective_descriptor(name, ncn + 1)
    assert len(desc['tail_rows']) > 0 or name == 'trig_be'
    _hold('%s N=%d' % (name, N), N, nrows, r, desc, rows, cols, 62)


def test_both_sections_and_explicit_entries_off_the_pattern():
    """Problem C with an objective section on top (a long group: the tail x
    tail objective entry plus a parameter-parameter entry on the same pair),
    then with instance entries that fall OUTSIDE the regular pattern: in an
    interior trajectory row (its later rows shift), in a first row, in a
    tail row between two segments and on an element of a segment."""
    N, nrows, ntail, desc, rows, cols = cc.both_sections()
    ref, _ = _hold('C + objective', N, nrows, ntail, desc, rows, cols, 63)
    assert ref.long.sum() == 1
    tail = nrows*N
    indptr, indices, _ = hessian_csr_structure(N, nrows, ntail, **desc)
    have = set(zip(np.repeat(np.arange(tail + ntail), np.diff(indptr)),
                   indices))
    last = nrows - 1
    extra = [(last*N + 7, 3), (last*N + 7, 5), (last*N, 0), (tail, 1),
             (tail, N + 9), (last*N + 30, last*N + 30)]
    assert sum(pair in have for pair in extra) in range(1, len(extra))
    at = (N - 1)*len(desc['pattern']) + len(desc['inst_rows'])
    more = dict(desc,
                inst_rows=np.r_[desc['inst_rows'], [r for r, _ in extra]],
                inst_cols=np.r_[desc['inst_cols'], [c for _, c in extra]])
    rows2 = np.r_[rows[:at], [r for r, _ in extra], rows[at:]]
    cols2 = np.r_[cols[:at], [c for _, c in extra], cols[at:]]
    _hold('C + objective + explicit', N, nrows, ntail, more, rows2, cols2, 64)


def test_what_the_structure_refuses():
    with pytest.raises(ValueError, match='above the diagonal'):
        hessian_csr_structure(5, 2, 0, [(0, 0, 1, 0)])
    with pytest.raises(ValueError, match='above the diagonal'):
        hessian_csr_structure(5, 2, 0, [(0, 0, 0, 1)])
    with pytest.raises(ValueError, match='outside the problem'):
        hessian_csr_structure(5, 2, 0, [(2, 0, 0, 0)])
    with pytest.raises(ValueError, match='lower triangle'):
        hessian_csr_structure(5, 2, 0, [(0, 0, 0, 0)], inst_rows=[1],
                              inst_cols=[2])
    with pytest.raises(ValueError, match='slot'):
        hessian_csr_structure(5, 2, 0, [(0, 2, 0, 0)])


def test_bindings_and_abi_version():
    from opty_amd import hip_backend as hb
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = {
        'opty_hip_hesscsr_create': (ctypes.c_int, [
            P, ctypes.POINTER(hb._HessmvDesc), ctypes.POINTER(P)]),
        'opty_hip_hesscsr_destroy': (ctypes.c_int, [P]),
        'opty_hip_hesscsr_nnz': (i64, [P]),
        'opty_hip_hesscsr_nnz_unique': (i64, [P]),
        'opty_hip_hesscsr_structure': (ctypes.c_int, [P, P, P, i32]),
        'opty_hip_hesscsr_compress': (ctypes.c_int, [P, P, P, i32]),
    }
    for name, signature in want.items():
        assert hb._SIGNATURES[name] == signature, name
    assert hb.ABI_VERSION == 12
    assert 'hesscsr.cpp' in hb.RUNTIME_SOURCES
    header = open(os.path.join(os.path.dirname(hb.__file__), '..', 'include',
                               'opty_hip.h')).read()
    assert '#define OPTY_HIP_ABI_VERSION 12' in header
    comment = header[header.index('Version of this header'):
                     header.index('#define OPTY_HIP_ABI_VERSION')]
    assert 'opty_hip_hesscsr_*' in comment
    for name in want:
        assert name + '(' in header, name


def test_sharded_problem_has_none_of_it():
    import opty_amd
    prob = object.__new__(opty_amd.ShardedProblem)
    with pytest.raises(NotImplementedError, match='hessian_csr_structure'):
        prob.hessian_csr_structure()
    with pytest.raises(NotImplementedError, match=r'no hessian_csr\.'):
        prob.hessian_csr(None, None)


def test_host_only_objective_hessian_is_refused(monkeypatch):
    """A hand-written ``values`` callable has no index pattern: the
    ``TypeError`` of ``hessian_operator`` under the method's own name."""
    import opty_amd
    from opty_amd import direct_collocation as dc
    none = np.zeros(0, dtype=np.int64)
    # (what a Problem asks the device for at construction is not what this
    # test is about)
    for name, stub in (('jacobian_indices', lambda self: (none, none)),
                       ('hessian_indices', lambda self: (none, none)),
                       ('generate_constraint_function',
                        lambda self, recycle=False: None),
                       ('generate_jacobian_function', lambda self: None),
                       ('generate_hessian_function', lambda self: None)):
        monkeypatch.setattr(dc.ConstraintCollocator, name, stub)
    kw = problems.pendulum_swing_up(num_nodes=11)
    hand = ([0], [0], lambda free: np.ones(1))
    prob = opty_amd.Problem(lambda f: 0.0, lambda f: 0.0*f, obj_hessian=hand,
                            **kw)
    free, lam = np.zeros(prob.num_free), np.zeros(prob.num_constraints)
    with pytest.raises(TypeError, match=r'Problem\.hessian_csr needs.*'
                       r'values\.handle'):
        prob.hessian_csr(free, lam)
    with pytest.raises(TypeError, match=r'Problem\.hessian_csr_structure '
                       r'needs'):
        prob.hessian_csr_structure()
    with pytest.raises(TypeError, match=r'Problem\.hessian_operator needs'):
        prob.hessian_operator(free, lam)
    plain = opty_amd.Problem(lambda f: 0.0, lambda f: 0.0*f, **kw)
    assert not hasattr(plain, 'hessian_csr')
    assert not hasattr(plain, 'hessian_csr_structure')


def test_problems_without_a_hessian_are_refused():
    """Implicit known trajectories and known trajectories given as functions
    of ``free``: the exceptions of ``generate_hessian_function``, before a
    device is asked for."""
    import opty_amd
    col = opty_amd.ConstraintCollocator(
        **problems.build('implicit_traj_be_small'))
    with pytest.raises(NotImplementedError):
        col.hessian_csr_structure()
    with pytest.raises(NotImplementedError):
        col.generate_hessian_csr_function()
    kw = problems.build('msd_be_small')
    (f, vals), = kw['known_trajectory_map'].items()
    kw['known_trajectory_map'] = {f: lambda free: vals}
    col = opty_amd.ConstraintCollocator(**kw)
    with pytest.raises(NotImplementedError):
        col.generate_hessian_csr_function()
