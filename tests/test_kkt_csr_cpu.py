"""CPU tests of the host statement of the augmented system as CSR
(``codegen/program.py``: ``kkt_csr_structure`` / ``assemble_kkt_csr``, the
``with_diagonal`` mode of the CSR Hessian) against ``scipy.sparse`` alone, of
the refusals and of the bindings: no GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import hessian_csr_cases as cc
import kkt_csr_cases as kc

from opty_amd.codegen.program import (assemble_hessian_csr, assemble_kkt_csr,
                                      hessian_csr_structure,
                                      kkt_csr_structure)

CASES = [(label, m, prune) for label in kc.CPU_LABELS for m in kc.CPU_EDGES
         for prune in (False, True)]


def _tables(col):
    """Arguments of the host statement for ``col``."""
    desc = col._hessmv_descriptor()
    return col._build_program(), col.num_collocation_nodes, dict(
        desc, jac_inst_rows=col._inst_rows, jac_inst_cols=col._inst_cols)


@pytest.mark.parametrize('label,ncn,prune', CASES)
def test_host_statement_against_scipy(label, ncn, prune):
    import scipy.sparse as sp
    what = '%s N-1=%d prune=%s' % (label, ncn, prune)
    col = kc.collocator(label, ncn, prune)
    prog, N, desc = _tables(col)
    hprog = col._build_hessian_program()
    ref = kc.Reference(col)
    n, m = ref.n, ref.m
    indptr, indices = kkt_csr_structure(prog, N, **desc)
    ref.check_structure(what, indptr, indices)

    rng = np.random.default_rng(81)
    hvals = rng.uniform(-1.0, 1.0, len(ref.hrows))
    jvals = rng.uniform(-1.0, 1.0, ref.J.nnz)
    sigma = rng.uniform(0.0, 1.0, n)
    hdesc = {k: v for k, v in desc.items() if not k.startswith('jac_')}
    nrows, ntail = hprog.n + hprog.q, hprog.r + hprog.s
    hptr, hidx, _ = hessian_csr_structure(N, nrows, ntail, **hdesc)
    hdata = assemble_hessian_csr(N, nrows, ntail, hvals, **hdesc)
    H = sp.csr_matrix((hdata, hidx, hptr), shape=(n, n)).toarray()
    J = sp.csr_matrix((jvals, ref.J.indices, ref.J.indptr),
                      shape=(m, n)).toarray()
    for sig, dw, dc in ((sigma, 1e-4, 1e-8), (None, 0.0, 0.0)):
        dense = np.zeros((n + m, n + m))
        dense[:n, :n] = H
        dense[np.arange(n), np.arange(n)] = \
            (np.diag(H) + (0.0 if sig is None else sig)) + dw
        dense[n:, :n] = J
        dense[n + np.arange(m), n + np.arange(m)] = 0.0 - dc
        data = assemble_kkt_csr(prog, N, hvals, jvals, sigma=sig, delta_w=dw,
                                delta_c=dc, **desc)
        got = sp.csr_matrix((data, indices, indptr),
                            shape=(n + m, n + m)).toarray()
        assert np.array_equal(got, dense), what

    # what keeps a case from hiding a failure
    lens = np.diff(prog.row_start)
    if label == 'A':
        # backward Euler with an unknown input: never read at the first node
        assert len(ref.absent) > 0
    if label == 'C':
        assert len(col._inst_rows) > 0 and prog.inst_jac_out
    if label == 'vardur':
        assert col._variable_duration
        if ncn >= 3:
            keys = ref.hrows*n + ref.hcols
            assert np.bincount(np.unique(keys, return_inverse=True)[1]
                               ).max() >= ncn
    if label == 'A' and prune:
        assert len(set(lens.tolist())) > 1
    if not prune:
        assert np.all(lens == prog.C)


def test_with_diagonal_off_is_what_it_was():
    for label, ncn in (('A', 65), ('C', 64), ('vardur_pendulum_small', None)):
        N, nrows, ntail, desc, rows, cols = cc.node_descriptor(label, ncn)
        values = np.random.default_rng(82).uniform(-1.0, 1.0, len(rows))
        ref = cc.Reference(nrows*N + ntail, nrows*N, N - 1, rows, cols,
                           values)
        for kw in ({}, dict(with_diagonal=False)):
            indptr, indices, slot = hessian_csr_structure(
                N, nrows, ntail, **dict(desc, **kw))
            cc.check_structure(label, ref, indptr, indices)
            assert np.array_equal(slot, ref.group)
            data = assemble_hessian_csr(N, nrows, ntail, values,
                                        **dict(desc, **kw))
            cc.check_values(label, ref, data)


def test_with_diagonal_adds_exactly_the_missing_diagonals():
    N, nrows, ntail, desc, rows, cols = cc.node_descriptor('A', 65)
    num_free = nrows*N + ntail
    values = np.random.default_rng(83).uniform(-1.0, 1.0, len(rows))
    ptr0, idx0, slot0 = hessian_csr_structure(N, nrows, ntail, **desc)
    ptr1, idx1, slot1 = hessian_csr_structure(N, nrows, ntail,
                                              with_diagonal=True, **desc)
    row0 = np.repeat(np.arange(num_free), np.diff(ptr0))
    row1 = np.repeat(np.arange(num_free), np.diff(ptr1))
    absent = np.setdiff1d(np.arange(num_free), row0[row0 == idx0])
    assert len(absent) > 0
    assert len(idx1) == len(idx0) + len(absent)
    assert np.array_equal(idx1[ptr1[1:] - 1], np.arange(num_free))
    old = np.ones(len(idx1), dtype=bool)
    old[ptr1[1:][absent] - 1] = False
    assert np.array_equal(row1[old], row0)
    assert np.array_equal(idx1[old], idx0)
    assert np.array_equal(np.flatnonzero(old)[slot0], slot1)
    data0 = assemble_hessian_csr(N, nrows, ntail, values, **desc)
    data1 = assemble_hessian_csr(N, nrows, ntail, values,
                                 with_diagonal=True, **desc)
    assert np.array_equal(cc.bits(data1[old]), cc.bits(data0))
    assert np.array_equal(cc.bits(data1[~old]),
                          cc.bits(np.zeros(len(absent))))     # +0.0


def test_jacobian_enumeration_of_the_helper_against_the_oracle():
    """``kkt_csr_cases.jacobian_coo`` (unpruned) is the oracle's set of
    pairs."""
    from oracle.collocation_oracle import OracleCollocator
    import hessian_cases as hc
    for label in ('A', 'C'):
        col = kc.collocator(label, 5)
        orc = OracleCollocator(name='kkt_' + label,
                               **hc.KERNEL_PROBLEMS[label](6))
        rows, cols = orc.jacobian_indices()
        mine = kc.jacobian_coo(col)
        size = col.num_free
        assert np.array_equal(np.sort(rows*size + cols),
                              np.sort(mine[0]*size + mine[1]))


def test_other_layouts_are_refused_without_a_device(monkeypatch):
    from opty_amd import direct_collocation as dc

    def no_device(self):
        raise AssertionError('a device was asked for')
    monkeypatch.setattr(dc.ConstraintCollocator, '_ensure_hip', no_device)
    for layout in ('coo', 'varying_first'):
        col = kc.collocator('A', 5, layout=layout)
        with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
            col.kkt_csr_structure()
        with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
            col.generate_kkt_csr_function()
    col = kc.collocator('A', 5, layout='coo')
    prog, N, desc = _tables(col)
    with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
        kkt_csr_structure(prog, N, **desc)
    with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
        assemble_kkt_csr(prog, N, np.zeros(1), np.zeros(1), **desc)


def test_unsorted_instance_entries_are_refused():
    col = kc.collocator('C', 5)
    prog, N, desc = _tables(col)
    assert len(desc['jac_inst_rows']) >= 2
    with pytest.raises(ValueError, match='instance rows'):
        kkt_csr_structure(prog, N, **dict(
            desc, jac_inst_rows=desc['jac_inst_rows'][:1],
            jac_inst_cols=desc['jac_inst_cols'][:1]))
    with pytest.raises(ValueError, match='sorted by row'):
        kkt_csr_structure(prog, N, **dict(
            desc, jac_inst_rows=desc['jac_inst_rows'][::-1].copy(),
            jac_inst_cols=desc['jac_inst_cols'][::-1].copy()))


def test_bindings_and_abi_version():
    from opty_amd import hip_backend as hb
    P, i32, i64, f64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                        ctypes.c_double)
    create = (ctypes.c_int, [P, ctypes.POINTER(hb._HessmvDesc),
                             ctypes.POINTER(P)])
    want = {
        'opty_hip_hesscsr_create_with_diagonal': create,
        'opty_hip_kktcsr_create': create,
        'opty_hip_kktcsr_destroy': (ctypes.c_int, [P]),
        'opty_hip_kktcsr_nnz': (i64, [P]),
        'opty_hip_kktcsr_nnz_hessian': (i64, [P]),
        'opty_hip_kktcsr_nnz_triplets': (i64, [P]),
        'opty_hip_kktcsr_structure': (ctypes.c_int, [P, P, P, i32]),
        'opty_hip_kktcsr_assemble': (ctypes.c_int,
                                     [P, P, P, P, f64, f64, P, i32]),
        'opty_hip_kktcsr_assemble_timed': (ctypes.c_int,
                                           [P, P, P, P, f64, f64, P, P]),
    }
    for name, signature in want.items():
        assert hb._SIGNATURES[name] == signature, name
    header = open(os.path.join(os.path.dirname(hb.__file__), '..', 'include',
                               'opty_hip.h')).read()
    # every opty_hip_kktcsr_* symbol of the header is bound
    declared = set(re.findall(r'\b(opty_hip_kktcsr_\w+)\(', header))
    assert declared == {k for k in want if 'kktcsr' in k}
    for name in declared:
        assert name in hb._SIGNATURES, name
    assert hb.HipKktCsr._create == 'opty_hip_kktcsr_create'
    assert hb.HipKktCsr._destroy == 'opty_hip_kktcsr_destroy'
    assert hb.ABI_VERSION == 12
    assert 'kktcsr.cpp' in hb.RUNTIME_SOURCES
    assert '#define OPTY_HIP_ABI_VERSION 12' in header
    comment = header[header.index('Version of this header'):
                     header.index('#define OPTY_HIP_ABI_VERSION')]
    assert 'opty_hip_kktcsr_*' in comment
    assert 'Augmented system as CSR' in header


def test_sharded_problem_has_none_of_it():
    import opty_amd
    prob = object.__new__(opty_amd.ShardedProblem)
    with pytest.raises(NotImplementedError, match='kkt_csr_structure'):
        prob.kkt_csr_structure()
    with pytest.raises(NotImplementedError, match=r'no kkt_csr\.'):
        prob.kkt_csr(None, None)
