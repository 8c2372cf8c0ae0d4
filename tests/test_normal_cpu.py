"""CPU tests of the normal-matrix solver's host statement
(``codegen/program.py``: ``normal_blocks`` / ``normal_factor`` /
``normal_solve``, the statement of ``csrc/normal.cpp``'s kernels) against an
independent ``S`` by ``scipy.sparse`` and ``longdouble`` sums
(``normal_cases.Reference``): the block-tridiagonal pattern, every element of
the blocks within the bound of a sum of products, the backward error of the
block cyclic reduction against LAPACK's, a pivot failure; and of what needs
no device: the bindings against the header, the refusals, the ABI version."""
import ctypes
import os
import re

import numpy as np
import pytest

import kkt_csr_cases as kc
import normal_cases as nc

from opty_amd.codegen.program import (normal_blocks, normal_columns,
                                      normal_factor, normal_solve)


@pytest.mark.parametrize('label', nc.LABELS)
def test_blocks_against_scipy(label):
    """Both layouts, pruned and not, at every edge: nothing outside the block
    tridiagonal, every element of ``normal_blocks`` within ``2 (t + 2) u
    sum|terms|`` of its ``longdouble`` sum."""
    worst = 0.0
    for ncn in nc.EDGES:
        for layout in ('coo', 'csr'):
            for prune in (False, True):
                what = '%s N-1=%d %s prune=%s' % (label, ncn, layout, prune)
                delta_c = nc.DELTAS[ncn % 2]
                col, ref, jac, d, _ = nc.case(label, ncn, prune, layout,
                                              delta_c)
                ref.nothing_outside_the_tridiagonal()
                prog = col._build_program()
                A, B = normal_blocks(prog, ncn + 1, jac, d, delta_c)
                assert A.shape == (ncn, prog.M, prog.M), what
                assert B.shape == (ncn - 1, prog.M, prog.M), what
                worst = max(worst, ref.check_blocks(what, A, B))
                assert np.array_equal(A, np.transpose(A, (0, 2, 1))), what
    print('%s: largest share of the bound in use %.3f' % (label, worst))


def test_cases_cannot_hide_a_failure():
    """``A`` has an unknown input -- backward Euler: it has no offset-0
    column, so a coupling gets fewer terms than a diagonal block --, ``C`` has
    instance rows and ``vardur`` a tail column, and neither is in ``S``."""
    col, ref, jac, d, _ = nc.case('A', 5, False, 'coo', 1.0)
    prog = col._build_program()
    assert prog.q >= 1 and prog.method == 'backward euler'
    sides, ent, coupled = normal_columns(prog)
    assert len(coupled) == prog.n and len(sides) == 2*prog.n + prog.q
    _, _, (tA, tB) = ref.block_views()
    assert tB.max() < tA.max() - 1          # (the - 1: delta_c on a diagonal)
    assert prog.r + prog.s > 0              # its unknown masses: tail columns

    col, ref, jac, d, _ = nc.case('C', 5, False, 'coo', 1.0)
    assert len(col._inst_rows) > 0
    assert ref.m == col._build_program().M*5 < col.num_constraints
    A, B = normal_blocks(col._build_program(), 6, jac, d, 1.0)
    assert A.shape[0]*A.shape[1] == ref.m

    col, ref, jac, d, _ = nc.case('vardur', 5, False, 'coo', 1.0)
    prog = col._build_program()
    assert prog.s == 1
    cols = kc.jacobian_coo(col)[1]
    assert np.any(cols >= ref.T)            # stored entries in the tail ...
    assert ref.Jc.shape[1] == ref.T         # ... that S does not see
    # ... and the statement does not read: other values there, the same S
    other = np.array(jac)
    tail = np.flatnonzero(cols >= ref.T)
    other[tail] = 1e30
    A0, B0 = normal_blocks(prog, 6, jac, d, 1.0)
    A1, B1 = normal_blocks(prog, 6, other, d, 1.0)
    assert np.array_equal(A0, A1) and np.array_equal(B0, B1)


def _lapack_eta():
    """The largest ``eta`` ``numpy.linalg.solve`` reaches over the cases of
    the factor / solve test."""
    worst = 0.0
    for label in nc.LABELS:
        for ncn in nc.EDGES:
            for layout, prune in nc.SOLVE_LAYOUTS:
                for delta_c in nc.DELTAS:
                    _, ref, _, _, r = nc.case(label, ncn, prune, layout,
                                              delta_c)
                    worst = max(worst, ref.eta(np.linalg.solve(ref.S, r), r))
    return worst


def test_factor_and_solve_against_lapack():
    """``eta`` of the block cyclic reduction within 8 times the largest
    ``eta`` of ``numpy.linalg.solve`` over the same cases (the 8 allows for
    the different elimination order; it is a margin over the reference)."""
    limit = nc.MARGIN*_lapack_eta()
    worst = 0.0
    for label in nc.LABELS:
        for ncn in nc.EDGES:
            for layout, prune in nc.SOLVE_LAYOUTS:
                for delta_c in nc.DELTAS:
                    eta = nc.host_eta(label, ncn, prune, layout, delta_c)
                    worst = max(worst, eta)
                    assert eta <= limit, (label, ncn, layout, prune, delta_c,
                                          eta, limit)
    print('largest eta %.3g, LAPACK %.3g' % (worst, limit/nc.MARGIN))


def test_one_and_three_columns_agree():
    col, ref, jac, d, r = nc.case('E', 65, False, 'coo', 1e-8)
    A, B = normal_blocks(col._build_program(), 66, jac, d, 1e-8)
    factors = normal_factor(A, B)
    Y = normal_solve(factors, r)
    assert Y.shape == r.shape
    for c in range(3):
        y = normal_solve(factors, r[:, c])
        assert y.shape == (ref.m,)
        assert ref.eta(y, r[:, c]) <= 1e-15
        assert np.allclose(y, Y[:, c], rtol=0, atol=1e-9*np.abs(y).max())


@pytest.mark.parametrize('ncn', (1, 2, 65))
def test_pivot_failure_names_level_zero(ncn):
    col, ref, jac, d, r = nc.case('A', ncn, False, 'coo', 1e-8)
    prog = col._build_program()
    A, B = normal_blocks(prog, ncn + 1, jac, -np.ones(col.num_free), 0.0)
    with pytest.raises(np.linalg.LinAlgError,
                       match='level 0, row %d' % (0 if ncn == 1 else 1)):
        normal_factor(A, B)
    # a non-finite block too
    A, B = normal_blocks(prog, ncn + 1, jac, d, 1.0)
    A[-1 if ncn % 2 == 0 or ncn == 1 else -2] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match='level 0'):
        normal_factor(A, B)


def test_arguments_are_refused():
    col, ref, jac, d, r = nc.case('A', 5, False, 'coo', 1.0)
    prog = col._build_program()
    with pytest.raises(ValueError, match='delta_c'):
        normal_blocks(prog, 6, jac, d, -1.0)
    with pytest.raises(ValueError, match='delta_c'):
        normal_blocks(prog, 6, jac, d, np.nan)
    with pytest.raises(ValueError, match='block values'):
        normal_blocks(prog, 6, jac[:10], d, 0.0)
    with pytest.raises(ValueError, match='d must'):
        normal_blocks(prog, 6, jac, d[:10], 0.0)
    A, B = normal_blocks(prog, 6, jac, d, 1.0)
    with pytest.raises(ValueError, match='shape'):
        normal_factor(A, B[:-1])
    with pytest.raises(ValueError, match='shape'):
        normal_solve(normal_factor(A, B), r[:-1])
    # d is optional: ones
    A1, B1 = normal_blocks(prog, 6, jac)
    A2, B2 = normal_blocks(prog, 6, jac, np.ones(col.num_free), 0.0)
    assert np.array_equal(A1, A2) and np.array_equal(B1, B2)


def test_varying_first_is_refused_without_a_device(monkeypatch):
    from opty_amd import direct_collocation as dc

    def no_device(self):
        raise AssertionError('a device was asked for')
    monkeypatch.setattr(dc.ConstraintCollocator, '_ensure_hip', no_device)
    col = kc.collocator('A', 5, layout='varying_first')
    with pytest.raises(ValueError, match='varying_first'):
        col.generate_normal_solver()
    with pytest.raises(ValueError, match='varying_first'):
        col.normal_operator(np.zeros(col.num_free))


def test_bindings_and_abi_version():
    from opty_amd import hip_backend as hb
    P, i32, i64, f64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                        ctypes.c_double)
    want = {
        'opty_hip_normal_create': (ctypes.c_int,
                                   [P, ctypes.POINTER(hb._NormalDesc),
                                    ctypes.POINTER(P)]),
        'opty_hip_normal_destroy': (ctypes.c_int, [P]),
        'opty_hip_normal_workspace_bytes': (i64, [P]),
        'opty_hip_normal_max_equations': (i32, [P]),
        'opty_hip_normal_blocks': (ctypes.c_int, [P, P, P, f64, P, P, i32]),
        'opty_hip_normal_factor': (ctypes.c_int, [P, P, P, f64, i32]),
        'opty_hip_normal_factor_status': (ctypes.c_int, [P, P, P]),
        'opty_hip_normal_solve': (ctypes.c_int, [P, P, P, i32, i64, i32]),
    }
    for name, signature in want.items():
        assert hb._SIGNATURES[name] == signature, name
    header = open(os.path.join(os.path.dirname(hb.__file__), '..', 'include',
                               'opty_hip.h')).read()
    # every opty_hip_normal_* symbol of the header is bound
    declared = set(re.findall(r'\b(opty_hip_normal_\w+)\(', header))
    assert declared == set(want)
    # the descriptor as the header lays it out
    struct = header[header.index('typedef struct opty_hip_normal_desc {'):
                    header.index('} opty_hip_normal_desc;')]
    fields = re.findall(r'^\s+(?:const )?(\w+) \*?(\w+);', struct, re.M)
    assert [name for _, name in fields] == \
        [name for name, _ in hb._NormalDesc._fields_]
    assert [kind for kind, _ in fields] == ['int32_t']*4
    assert hb._NormalDesc._fields_[3][1] is ctypes.c_void_p
    assert ctypes.sizeof(hb._NormalDesc) == 24
    assert hb.HipNormalSolver._create == 'opty_hip_normal_create'
    assert hb.HipNormalSolver._destroy == 'opty_hip_normal_destroy'
    assert hb.ABI_VERSION == 12
    assert 'normal.cpp' in hb.RUNTIME_SOURCES
    assert '#define OPTY_HIP_ABI_VERSION 12' in header
    comment = header[header.index('Version of this header'):
                     header.index('#define OPTY_HIP_ABI_VERSION')]
    assert 'opty_hip_normal_*' in comment
    assert 'Normal matrix' in header


def test_refusals_of_the_library_that_need_no_device():
    """Null handles are refused by every entry point before anything else is
    looked at, with a message."""
    from opty_amd import hip_backend as hb
    lib = hb.load_library()
    out = ctypes.c_void_p()
    desc = hb._NormalDesc(M=1, P=0, layout=0, pattern=None)
    assert lib.opty_hip_normal_create(None, ctypes.byref(desc),
                                      ctypes.byref(out)) != 0
    assert b'null argument' in lib.opty_hip_last_error()
    assert lib.opty_hip_normal_blocks(None, None, None, 0.0, None, None,
                                      hb.HOST) != 0
    assert lib.opty_hip_normal_factor(None, None, None, 0.0, hb.HOST) != 0
    assert lib.opty_hip_normal_factor_status(None, None, None) != 0
    assert lib.opty_hip_normal_solve(None, None, None, 1, 1, hb.HOST) != 0
    assert b'null argument' in lib.opty_hip_last_error()
    assert lib.opty_hip_normal_workspace_bytes(None) == -1
    assert lib.opty_hip_normal_max_equations(None) == -1
    assert lib.opty_hip_normal_destroy(None) == 0


def test_sharded_problem_has_none_of_it():
    import opty_amd
    prob = object.__new__(opty_amd.ShardedProblem)
    with pytest.raises(NotImplementedError, match='normal_operator'):
        prob.normal_operator(None)
