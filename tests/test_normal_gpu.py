"""GPU tests of the normal-matrix solver (``csrc/normal.cpp``:
``opty_normal_blocks`` / ``opty_normal_elim`` / ``opty_normal_update`` and the
kernels of one right-hand side; C ABI ``opty_hip_normal_*``;
``ConstraintCollocator.generate_normal_solver`` / ``normal_operator``): the
blocks against the host statement and the ``longdouble`` sums of
``normal_cases.Reference`` inside guard bands, the backward error of the
solve against the host statement's on the same case, every parity of every
level, both layouts, pruned and not, both memory kinds, determinism, the
largest ``M`` and one more, a pivot failure, the operator and the example."""
import ctypes
import types

import numpy as np
import pytest

import kkt_csr_cases as kc
import normal_cases as nc

pytestmark = pytest.mark.gpu


def _device(values):
    import torch
    # (a copy: the cases' arrays are read-only)
    return torch.from_numpy(
        np.array(values, dtype=np.float64, order='C')).cuda()


def _run_case(label, ncn, prune, layout, delta_c):
    """One case through every check of the shapes; returns what the other
    tests go on with."""
    import torch
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import normal_blocks
    what = '%s N-1=%d %s prune=%s delta_c=%g' % (label, ncn, layout, prune,
                                                 delta_c)
    col, ref, jac, d, r = nc.case(label, ncn, prune, layout, delta_c)
    ns = col.generate_normal_solver()
    handle, hip = ns.handle, col.hip
    M, m = ref.M, ref.m
    assert (ns.M, ns.num_nodes, ns.size) == (M, ncn, m)
    assert len(jac) == hip.nnz

    # the blocks: inside guard bands, every element written, within the
    # bound of their longdouble sums and of the host statement
    djac, dd, dr = _device(jac), _device(d), _device(r.T)    # (3, m)
    bufA, bufB = kc.Guarded(ncn*M*M), kc.Guarded((ncn - 1)*M*M)
    torch.cuda.synchronize()
    handle.blocks(djac, dd, delta_c, bufA.doubles, bufB.doubles, hb.DEVICE)
    hip.synchronize()
    A = bufA.check(what + ' A').reshape(ncn, M, M)
    B = bufB.check(what + ' B').reshape(ncn - 1, M, M)
    share = ref.check_blocks(what, A, B)
    hA, hB = normal_blocks(col._build_program(), ncn + 1, jac, d, delta_c)
    (_, _), (mA, mB), (tA, tB) = ref.block_views()
    for got, host, mag, t in ((A, hA, mA, tA), (B, hB, mB, tB)):
        err = np.abs(got.astype(np.longdouble) - host)
        assert np.all(err <= 2*(t + 2)*np.longdouble(nc.U)*mag), what
    assert np.array_equal(A, np.transpose(A, (0, 2, 1))), what
    # ... the same bits from host memory, through the solver's own method,
    # and again
    A2, B2 = ns.blocks(jac, d, delta_c)
    assert np.array_equal(kc.bits(A2), kc.bits(A)), what
    assert np.array_equal(kc.bits(B2), kc.bits(B)), what
    A3, B3 = ns.blocks(djac, dd, delta_c)
    assert np.array_equal(kc.bits(A3.cpu().numpy()), kc.bits(A)), what
    assert np.array_equal(kc.bits(B3.cpu().numpy()), kc.bits(B)), what

    # factor and solve: device memory, the solution inside guard bands
    ns.factor_values(djac, dd, delta_c)
    bufY = kc.Guarded(3*m)
    torch.cuda.synchronize()
    handle.solve(dr, bufY.doubles, 3, m, hb.DEVICE)
    hip.synchronize()
    Y = bufY.check(what + ' y').reshape(3, m).T
    assert np.array_equal(dr.cpu().numpy(), r.T), what      # inputs intact
    assert np.array_equal(djac.cpu().numpy(), jac), what
    eta, host = ref.eta(Y, r), nc.host_eta(label, ncn, prune, layout, delta_c)
    print('%s: eta %.3g, host statement %.3g, blocks use %.3f of their '
          'bound' % (what, eta, host, share))
    assert eta <= nc.MARGIN*host, (what, eta, host)
    # a (., 3) right-hand side is its three columns, bit for bit
    for c in range(3):
        y = ns.solve(dr[c])
        assert np.array_equal(kc.bits(y.cpu().numpy()), kc.bits(Y[:, c])), what
    Y2 = ns.solve(dr.t())
    assert Y2.shape == (m, 3)
    assert np.array_equal(kc.bits(Y2.cpu().numpy()), kc.bits(Y)), what
    # host memory: the same bits, factorisation and solve
    ns.factor_values(jac, d, delta_c)
    Y3 = ns.solve(r)
    assert isinstance(Y3, np.ndarray) and Y3.shape == (m, 3)
    assert np.array_equal(kc.bits(Y3), kc.bits(Y)), what
    y3 = ns.solve(r[:, 1])
    assert y3.shape == (m,)
    assert np.array_equal(kc.bits(y3), kc.bits(Y[:, 1])), what
    return dict(col=col, ns=ns, ref=ref, jac=jac, d=d, r=r, Y=Y, A=A, B=B,
                eta=eta, host=host)


@pytest.mark.parametrize('label,ncn,prune,layout', nc.GPU_CASES)
def test_shapes(label, ncn, prune, layout):
    """M in 2, 4, 7, 8 (and 6); N - 1 over every parity of every level, a
    last odd row without V and the single-row level; both layouts, pruned
    and not; both memory kinds; determinism."""
    got = _run_case(label, ncn, prune, layout, nc.DELTAS[ncn % 2])
    M = got['ref'].M
    assert M == {'vardur': 2, 'C': 4, 'B': 6, 'E': 7, 'A': 8}[label]
    want = sum(8*(k*M*M + (k - 1)*M*M + 3*k*M) for k in _level_rows(ncn))
    assert got['ns'].workspace_bytes >= want
    assert got['ns'].workspace_bytes < want + 64*1024
    if prune:
        prog = got['col']._build_program()
        assert len(prog.pattern) < prog.M*prog.C


def _level_rows(n):
    rows = [n]
    while rows[-1] > 1:
        rows.append((rows[-1] + 1)//2)
    return rows


@pytest.mark.parametrize('delta_c', nc.DELTAS)
def test_ten_link_pendulum(delta_c):
    """``config3_10link_small``: M = 22."""
    got = _run_case(nc.CONFIG3, 40, False, 'coo', delta_c)
    assert got['ref'].M == 22


def _fake_program(col, desc):
    """What ``normal_blocks`` reads of a program, for a descriptor."""
    prog = col._build_program()
    M, C = desc['M'], prog.C
    return types.SimpleNamespace(
        n=prog.n, q=prog.q, method=prog.method, M=M, layout='coo',
        pattern=[(int(j), int(k)) for j, k in desc['pattern']],
        row_start=[j*C for j in range(M + 1)])


def test_largest_m_and_one_more():
    """A dense pattern at the largest ``M`` creation accepts -- more than 64
    KiB of LDS per block, at least the config-5 class --, then one more,
    which is refused with the limit named, then a working handle."""
    import torch
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import (normal_blocks, normal_factor,
                                          normal_solve)
    some = nc.collocator(*nc.ONE_CASE[:2]).generate_normal_solver()
    M = some.handle.max_equations
    assert M >= 50
    assert 3*M*(M | 1)*8 > 65536
    col, desc, jac, d, S = nc.synthetic(M)
    ncn, delta_c = nc.SYNTH_EDGE, 1.0
    m = M*ncn
    handle = hb.HipNormalSolver(col.hip, desc)
    djac, dd = _device(jac), _device(d)
    bufA, bufB = kc.Guarded(ncn*M*M), kc.Guarded((ncn - 1)*M*M)
    torch.cuda.synchronize()
    handle.blocks(djac, dd, delta_c, bufA.doubles, bufB.doubles, hb.DEVICE)
    col.hip.synchronize()
    A = bufA.check('A').reshape(ncn, M, M)
    B = bufB.check('B').reshape(ncn - 1, M, M)
    # the definition, term by term in longdouble
    prog = col._build_program()
    n, N = prog.n, ncn + 1
    G = jac.reshape(ncn, M, prog.C).astype(np.longdouble)
    dl = d.astype(np.longdouble)
    for a in range(ncn):
        dn = np.concatenate((dl[np.arange(n)*N + a + 1],
                             dl[np.arange(n)*N + a]))
        Gt = G[a, :, :2*n]
        exact = (Gt/dn) @ Gt.T + delta_c*np.eye(M)
        mag = (np.abs(Gt)/dn) @ np.abs(Gt).T + delta_c*np.eye(M)
        t = 2*n + np.eye(M)
        assert np.all(np.abs(A[a] - exact) <= 2*(t + 2)*nc.U*mag), a
        if a + 1 < ncn:
            # x_{a+1}: offset 0 of node a + 1 (columns n ..), offset 1 of a
            dn = dl[np.arange(n)*N + a + 1]
            exact = (G[a + 1, :, n:2*n]/dn) @ G[a, :, :n].T
            mag = (np.abs(G[a + 1, :, n:2*n])/dn) @ np.abs(G[a, :, :n]).T
            assert np.all(np.abs(B[a] - exact) <= 2*(n + 2)*nc.U*mag), a
    # ... and the solve against the host statement's
    full = S + delta_c*np.eye(m)
    r = np.random.default_rng(3).standard_normal((m, 2))

    def eta(y):
        Sl, yl, rl = (x.astype(np.longdouble) for x in (full, y, r))
        return float((np.abs(Sl @ yl - rl).max(axis=0)/(
            np.abs(Sl).sum(axis=1).max()*np.abs(yl).max(axis=0) +
            np.abs(rl).max(axis=0))).max())
    hA, hB = normal_blocks(_fake_program(col, desc), N, jac, d, delta_c)
    host = eta(normal_solve(normal_factor(hA, hB), r))
    handle.factor(jac, d, delta_c, hb.HOST)
    assert handle.status() is None
    Y = np.full((m, 2), np.nan, order='F')
    handle.solve(np.asfortranarray(r), Y, 2, m, hb.HOST)
    print('M = %d: eta %.3g, host statement %.3g' % (M, eta(Y), host))
    assert eta(Y) <= nc.MARGIN*host
    handle.release()

    # one more
    with pytest.raises(hb.HipBackendError) as refused:
        hb.HipNormalSolver(col.hip, nc.synthetic(M + 1)[1])
    text = str(refused.value)
    assert '%d equations need' % (M + 1) in text
    assert 'the limit is' in text and '(%d equations)' % M in text
    # ... and a working handle after the refusal
    again = hb.HipNormalSolver(col.hip, desc)
    again.factor(jac, d, delta_c, hb.HOST)
    assert again.status() is None
    Y2 = np.full((m, 2), np.nan, order='F')
    again.solve(np.asfortranarray(r), Y2, 2, m, hb.HOST)
    assert np.array_equal(kc.bits(Y2), kc.bits(Y))
    again.release()


def test_factor_at_free_has_the_bits_of_factor_values():
    import torch
    label, ncn, prune, layout = nc.ONE_CASE
    col = nc.collocator(label, ncn, prune, layout)
    ns = col.generate_normal_solver()
    assert col.generate_normal_solver() is ns
    rng = np.random.default_rng(8)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    d = rng.uniform(0.5, 2.0, col.num_free)
    r = rng.standard_normal(ns.size)
    jac = col.generate_jacobian_function()(free).copy()
    ns.factor_values(jac, d, 1e-8)
    want = ns.solve(r)
    ns.factor(free, d, 1e-8)
    assert np.array_equal(kc.bits(ns.solve(r)), kc.bits(want))
    # ... and on the device
    ns.factor(_device(free), _device(d), 1e-8)
    got = ns.solve(_device(r))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert np.array_equal(kc.bits(got.cpu().numpy()), kc.bits(want))
    # without d: ones
    ns.factor(free, delta_c=1e-8)
    ones = ns.solve(r)
    ns.factor_values(jac, np.ones(col.num_free), 1e-8)
    assert np.array_equal(kc.bits(ns.solve(r)), kc.bits(ones))
    # the shapes are checked before anything is converted
    with pytest.raises(ValueError, match='free must have shape'):
        ns.factor(free[:-1])
    with pytest.raises(ValueError, match='r must have shape'):
        ns.solve(r[:-1])
    with pytest.raises(ValueError, match='jac_values must have shape'):
        ns.blocks(jac[:-1])


def test_pivot_failure_is_a_status():
    """``d = -1`` with ``delta_c = 0``: ``LinAlgError`` naming level 0, solve
    is refused, and the next factorisation on the same handle works."""
    from opty_amd import hip_backend as hb
    label, ncn, prune, layout = nc.ONE_CASE
    col, ref, jac, d, r = nc.case(label, ncn, prune, layout, 1e-8)
    ns = col.generate_normal_solver()
    ns.factor_values(jac, d, 1e-8)
    want = ns.solve(r)
    with pytest.raises(np.linalg.LinAlgError, match='level 0, row 1'):
        ns.factor_values(jac, -np.ones(col.num_free), 0.0)
    assert ns.handle.status() == (0, 1)
    with pytest.raises(hb.HipBackendError, match='level 0, row 1'):
        ns.solve(r)
    with pytest.raises(np.linalg.LinAlgError, match='level 0, row 1'):
        ns.factor_values(_device(jac), _device(-np.ones(col.num_free)), 0.0)
    # a NaN block: node 3 is eliminated at level 0; node 4 survives twice and
    # is row 1 of level 2 (the host statement says the same)
    from opty_amd.codegen.program import normal_blocks, normal_factor
    prog = col._build_program()
    P = len(prog.pattern)
    for node, where in ((3, 'level 0, row 3'), (4, 'level 2, row 1')):
        bad = np.array(jac)
        bad[node*P:(node + 1)*P] = np.nan
        with pytest.raises(np.linalg.LinAlgError, match=where):
            ns.factor_values(bad, d, 1e-8)
        with pytest.raises(np.linalg.LinAlgError, match=where):
            normal_factor(*normal_blocks(prog, ncn + 1, bad, d, 1e-8))
    ns.factor_values(jac, d, 1e-8)
    assert ns.handle.status() is None
    assert np.array_equal(kc.bits(ns.solve(r)), kc.bits(want))


def test_operator_against_scipy():
    """``normal_operator(free, d, 1.0)`` applied to ``S x`` from the
    independent SciPy matrix returns ``x`` within ``cond(S) 8 eta_host``."""
    import scipy.sparse as sp
    import torch
    from opty_amd.codegen.program import (normal_blocks, normal_factor,
                                          normal_solve)
    col = nc.collocator('A', 5)
    rng = np.random.default_rng(21)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    d = rng.uniform(0.5, 2.0, col.num_free)
    delta_c = 1.0
    op = col.normal_operator(free, d, delta_c)
    prog = col._build_program()
    M, N = prog.M, col.num_collocation_nodes
    m, T = M*(N - 1), (prog.n + prog.q)*N
    assert op.shape == (m, m)
    jac = col.generate_jacobian_function()(free).copy()
    rows, cols = col.jacobian_indices()
    J = sp.coo_matrix((jac, (rows, cols)),
                      shape=(col.num_constraints, col.num_free)).tocsr()
    Jc = J[:m, :T]
    S = (Jc @ sp.diags(1.0/d[:T]) @ Jc.T + delta_c*sp.identity(m)).toarray()
    x = rng.standard_normal((m, 3))
    rhs = S @ x

    def eta(y):
        Sl, yl, rl = (a.astype(np.longdouble) for a in (S, y, rhs))
        return float((np.abs(Sl @ yl - rl).max(axis=0)/(
            np.abs(Sl).sum(axis=1).max()*np.abs(yl).max(axis=0) +
            np.abs(rl).max(axis=0))).max())
    A, B = normal_blocks(prog, N, jac, d, delta_c)
    host = eta(normal_solve(normal_factor(A, B), rhs))
    cond = np.linalg.cond(S, np.inf)
    bound = cond*nc.MARGIN*host
    got = np.column_stack([op.matvec(rhs[:, c]) for c in range(3)])
    err = np.abs(got - x).max()/np.abs(x).max()
    print('cond %.3g, eta_host %.3g, error %.3g, bound %.3g'
          % (cond, host, err, bound))
    assert err <= bound
    block = op.matmat(rhs)
    assert np.array_equal(kc.bits(block), kc.bits(got))
    assert np.array_equal(kc.bits(op.rmatvec(rhs[:, 0])), kc.bits(got[:, 0]))
    tensor = op.matvec(_device(rhs[:, 0]))
    assert isinstance(tensor, torch.Tensor) and tensor.is_cuda
    assert np.array_equal(kc.bits(tensor.cpu().numpy()), kc.bits(got[:, 0]))
    # Problem forwards it; a later factorisation makes the operator stale
    col.generate_normal_solver().factor(free, d, 2.0)
    with pytest.raises(RuntimeError, match='stale'):
        op.matvec(rhs[:, 0])


def test_refusals_of_the_c_abi():
    """Refused before anything is enqueued, with a message: null pointers, a
    bad memory kind, ``delta_c < 0`` or not finite, ``y`` overlapping ``r``,
    ``solve`` before a successful ``factor``, ``ld < M(N-1)``, a bad
    descriptor."""
    from opty_amd import hip_backend as hb
    lib = hb.load_library()
    label, ncn, prune, layout = nc.ONE_CASE
    col, ref, jac, d, r = nc.case(label, ncn, prune, layout, 1e-8)
    prog = col._build_program()
    handle = hb.HipNormalSolver(col.hip, dict(
        M=prog.M, layout=layout, pattern=prog.pattern))
    h = handle._handle()
    m, M = ref.m, ref.M
    A, B = np.zeros((ncn, M, M)), np.zeros((ncn - 1, M, M))
    y = np.zeros(m)
    r0 = np.ascontiguousarray(r[:, 0])
    ptr = hb._ptr

    def message():
        return lib.opty_hip_last_error().decode()
    # solve before any factorisation
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(y), 1, m, hb.HOST) != 0
    assert 'before a successful factorisation' in message()
    level, row = ctypes.c_int32(), ctypes.c_int64()
    assert lib.opty_hip_normal_factor_status(
        h, ctypes.addressof(level), ctypes.addressof(row)) != 0
    assert 'no factorisation' in message()
    for bad in (-1e-300, -1.0, float('nan'), float('inf')):
        assert lib.opty_hip_normal_factor(h, ptr(jac), ptr(d), bad,
                                          hb.HOST) != 0
        assert 'delta_c' in message()
        assert lib.opty_hip_normal_blocks(h, ptr(jac), ptr(d), bad, ptr(A),
                                          ptr(B), hb.HOST) != 0
        assert 'delta_c' in message()
    assert lib.opty_hip_normal_factor(h, None, ptr(d), 0.0, hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_normal_factor(h, ptr(jac), ptr(d), 0.0, 7) != 0
    assert 'bad memory kind 7' in message()
    assert lib.opty_hip_normal_blocks(h, ptr(jac), ptr(d), 0.0, None, ptr(B),
                                      hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_normal_blocks(h, ptr(jac), ptr(d), 0.0, ptr(A), None,
                                      hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_normal_blocks(h, ptr(jac), ptr(d), 0.0, ptr(A),
                                      ptr(B), 7) != 0
    assert 'bad memory kind 7' in message()
    both = np.zeros(2*ncn*M*M)
    assert lib.opty_hip_normal_blocks(h, ptr(jac), ptr(d), 0.0, ptr(both),
                                      ptr(both[8:]), hb.HOST) != 0
    assert 'overlaps' in message()
    # (nothing above was enqueued: still no factorisation)
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(y), 1, m, hb.HOST) != 0
    assert 'before a successful factorisation' in message()
    handle.factor(jac, d, 1e-8, hb.HOST)
    assert handle.status() is None
    assert lib.opty_hip_normal_solve(h, None, ptr(y), 1, m, hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_normal_solve(h, ptr(r0), None, 1, m, hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(y), 1, m, 7) != 0
    assert 'bad memory kind 7' in message()
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(y), 1, m - 1,
                                     hb.HOST) != 0
    assert 'ld %d is less than' % (m - 1) in message()
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(r0[1:]), 1, m,
                                     hb.HOST) != 0
    assert 'y overlaps r' in message()
    two = np.zeros(3*m)
    assert lib.opty_hip_normal_solve(h, ptr(two), ptr(two[m + 5:]), 2, m,
                                     hb.HOST) != 0
    assert 'y overlaps r' in message()
    assert lib.opty_hip_normal_solve(h, ptr(r0), ptr(y), -1, m, hb.HOST) != 0
    # ... and the handle still solves
    handle.solve(r0, y, 1, m, hb.HOST)
    assert ref.eta(y, r0) <= 1e-15
    # no column, no launch
    handle.solve(r0, y, 0, m, hb.HOST)
    handle.release()

    # descriptors
    def create(**kw):
        desc = dict(dict(M=prog.M, layout=layout, pattern=prog.pattern), **kw)
        with pytest.raises(hb.HipBackendError) as err:
            hb.HipNormalSolver(col.hip, desc)
        return str(err.value)
    assert 'layout 2' in create(layout=2)
    assert 'bad normal-matrix descriptor' in create(M=0)
    assert 'outside' in create(pattern=[(prog.M, 0)])
    assert 'outside' in create(pattern=[(0, prog.C)])
    assert 'repeats' in create(pattern=[(0, 0), (1, 0), (0, 0)])
    assert 'not grouped' in create(layout='csr', pattern=[(1, 0), (0, 0)])
    assert 'null block pattern' in create(pattern=[], P=3)


def test_the_handle_follows_its_problem():
    """Released with the problem's C handle, created again on the next call
    -- without a factorisation --, and the same bits after the next one."""
    from opty_amd import hip_backend as hb
    label, ncn, prune, layout = nc.ONE_CASE
    col, ref, jac, d, r = nc.case(label, ncn, prune, layout, 1e-8)
    ns = col.generate_normal_solver()
    ns.factor_values(jac, d, 1e-8)
    want = ns.solve(r)
    col._respecialize(col._hip)
    assert ns.handle._h is None
    with pytest.raises(hb.HipBackendError, match='before a successful'):
        ns.solve(r)
    assert ns.handle._h is not None
    ns.factor_values(jac, d, 1e-8)
    assert np.array_equal(kc.bits(ns.solve(r)), kc.bits(want))


def test_example_preconditioned_minres():
    """``examples/kkt_minres_normal.py`` at 20 nodes: both MINRES runs report
    ``info == 0``; the iteration counts are printed, not gated."""
    from examples import kkt_minres_normal
    out = kkt_minres_normal.main(nc.EXAMPLE_NODES, verbose=False)
    print('MINRES iterations: %d plain, %d preconditioned'
          % (out['plain'][1], out['preconditioned'][1]))
    assert out['plain'][0] == 0
    assert out['preconditioned'][0] == 0
