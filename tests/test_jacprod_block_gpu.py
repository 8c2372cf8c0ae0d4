"""GPU tests of the block products of the Jacobian operator
(``ConstraintCollocator.generate_jvp_block_function`` /
``generate_vjp_block_function``, ``matmat`` / ``rmatmat`` of
``jacobian_operator``, C ABI ``opty_hip_jacprod_block_*``, kernels
``opty_jvp_block`` / ``opty_jvp_block_inst`` / ``opty_vjp_block`` /
``opty_vjp_block_fin``) against the CPU interpreter of the same roots and
against the GPU Jacobian of the same collocator.  Small shapes only."""
import numpy as np
import pytest

import jacprod_block_cases as cases
from golden_util import assert_close
from test_jacprod_cpu import draw, product_tolerances, worst_ratio
from test_jacprod_gpu import _matrices

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _inputs(seed, col, k):
    """``free`` and ``k`` distinct columns each of ``V`` and ``W``."""
    rng = np.random.default_rng(seed)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.02
    V = np.stack([draw(rng, col.num_free) for _ in range(k)], axis=1) \
        if k else np.zeros((col.num_free, 0))
    W = np.stack([draw(rng, col.num_constraints) for _ in range(k)],
                 axis=1) if k else np.zeros((col.num_constraints, 0))
    return free, V, W


def _functions(col):
    return col.generate_jvp_block_function(), \
        col.generate_vjp_block_function()


def _check_against_interpreter(col, free, V, W, JV, JTW, width, what):
    wv, ww, bv, bw = cases.interpreted_block(col, free, V, W, width)
    for c in range(V.shape[1]):
        assert_close(JV[:, c], wv[:, c], rtol=1e-12, bound=bv[:, c],
                     what='%s jvp column %d' % (what, c))
        assert_close(JTW[:, c], ww[:, c], rtol=1e-12, bound=bw[:, c],
                     what='%s vjp column %d' % (what, c))


@pytest.mark.parametrize('name', cases.PARITY + ['nonlinear_instance'])
def test_block_products_on_the_device(name):
    from opty_amd import hip_backend as hb
    col = cases.collocator(name)
    jmm, jtmm = _functions(col)
    k = 5
    free, V, W = _inputs(1, col, k)
    JV, JTW = jmm(free, V), jtmm(free, W)
    assert JV.shape == (col.num_constraints, k)
    assert JTW.shape == (col.num_free, k)
    _check_against_interpreter(col, free, V, W, JV, JTW, jmm.width, name)
    # against the GPU Jacobian of the same collocator
    J, A, F, K = _matrices(col, free)
    for c in range(k):
        tv, tw = product_tolerances(A, F, K, V[:, c], W[:, c])
        ev = np.abs(JV[:, c] - J @ V[:, c])
        ew = np.abs(JTW[:, c] - J.T @ W[:, c])
        print('%s column %d: worst error/tolerance against coo(jacobian): '
              'jvp %.3g, vjp %.3g' % (name, c, worst_ratio(ev, tv),
                                      worst_ratio(ew, tw)))
        assert np.all(ev <= tv), (name, c, 'jvp', worst_ratio(ev, tv))
        assert np.all(ew <= tw), (name, c, 'vjp', worst_ratio(ew, tw))
    # bit-identical over three calls
    for _ in range(2):
        assert np.array_equal(_bits(jmm(free, V)), _bits(JV))
        assert np.array_equal(_bits(jtmm(free, W)), _bits(JTW))
    meta = col._jacprod_block_meta
    print('%s: width %d, builds tried %s' % (name, meta['width'],
                                             meta['tried']))
    assert meta['verdict']['ok'] is True
    assert meta['width'] == jmm.width == jtmm.width
    if meta['width'] == 1:
        # every block build spills: the columns went through the single
        # kernels
        names, hsaco = col._JACPROD_KERNELS, col._jacprod_meta['hsaco']
    else:
        names, hsaco = col._JACPROD_BLOCK_KERNELS, meta['hsaco']
    res = hb.cached_kernel_resources(hsaco)
    for kernel in names:
        assert res[kernel]['.vgpr_spill_count'] == 0, (name, kernel)


@pytest.mark.parametrize('name', cases.TAILED)
def test_column_counts(name):
    col = cases.collocator(name)
    jmm, jtmm = _functions(col)
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    assert jmm.width in (2, 4)
    free, V8, W8 = _inputs(2, col, max(cases.COLUMN_COUNTS))
    for k in cases.COLUMN_COUNTS:
        V, W = V8[:, :k], W8[:, :k]
        JV, JTW = jmm(free, V), jtmm(free, W)
        assert JV.shape == (col.num_constraints, k)
        assert JTW.shape == (col.num_free, k)
        assert JV.dtype == JTW.dtype == np.float64
        if k == 1:
            assert np.array_equal(_bits(JV[:, 0]), _bits(jvp(free, V[:, 0])))
            assert np.array_equal(_bits(JTW[:, 0]),
                                  _bits(vjp(free, W[:, 0])))
        _check_against_interpreter(col, free, V, W, JV, JTW, jmm.width,
                                   '%s k=%d' % (name, k))
    # either memory order, the same bits
    a = jmm(free, np.ascontiguousarray(V8[:, :3]))
    b = jmm(free, np.asfortranarray(V8[:, :3]))
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize('num_nodes', cases.EDGE_NODES)
@pytest.mark.parametrize('method', cases.EDGE_METHODS)
def test_both_ends_and_block_edges(num_nodes, method):
    """``N - 1`` below, at and off the multiples of 63 and 64, and ``N = 2``,
    three columns (a partial pass): right values in every column at both
    ends of every row and in the tail."""
    col = cases.edge_collocator(num_nodes, method)
    jmm, jtmm = _functions(col)
    free, V, W = _inputs(6, col, 3)
    JV, JTW = jmm(free, V), jtmm(free, W)
    assert np.all(np.isfinite(JV)) and np.all(np.isfinite(JTW))
    _check_against_interpreter(col, free, V, W, JV, JTW, jmm.width,
                               'N=%d %s' % (num_nodes, method))


def test_columns_do_not_leak_into_each_other():
    col = cases.collocator('config3_10link_small')
    jmm, jtmm = _functions(col)
    free, V, W = _inputs(7, col, 4)
    J, A, F, K = _matrices(col, free)
    for f, X, pattern in ((jmm, V, A), (jtmm, W, A.T.tocsr())):
        clean = f(free, X)
        bad = X.copy()
        bad[:, 1] = np.nan
        dirty = f(free, bad)
        for c in (0, 2, 3):
            assert np.array_equal(_bits(clean[:, c]), _bits(dirty[:, c])), c
        touched = np.asarray(pattern.sum(axis=1)).ravel() > 0
        assert touched.any()
        assert np.all(np.isnan(dirty[touched, 1]))
        assert np.all(np.isfinite(clean))


def _abi(col):
    from opty_amd import hip_backend as hb
    jmm, _ = _functions(col)
    assert jmm.handle is not None
    return hb, hb.load_library(), jmm.handle


def test_leading_dimensions_through_the_c_abi():
    col = cases.collocator('pend2_link_vardur_unkmass_small')
    hb, lib, handle = _abi(col)
    k, pad, sentinel = 5, 3, -777.0
    free, V, W = _inputs(8, col, k)
    nfree, ncon = col.num_free, col.num_constraints
    for call, X, nin, nout in ((handle.jvp_block, V, nfree, ncon),
                               (handle.vjp_block, W, ncon, nfree)):
        # tightly packed, host
        tight = np.empty((k, nout))
        call(free, np.ascontiguousarray(X.T), nin, tight, nout, k, hb.HOST)
        ldi, ldo = nin + pad, nout + pad
        padded_in = np.full((k, ldi), sentinel)
        padded_in[:, :nin] = X.T
        # host, padded on both sides
        out = np.full((k, ldo), sentinel)
        call(free, padded_in, ldi, out, ldo, k, hb.HOST)
        assert np.all(out[:, nout:] == sentinel)
        assert np.array_equal(_bits(out[:, :nout]), _bits(tight))
        # device, padded on both sides, interior pointers of larger buffers
        lead = 7
        d_free = hb.DeviceVector(free)
        d_in = hb.DeviceVector(np.r_[np.full(lead, sentinel),
                                     padded_in.ravel()])
        d_out = hb.DeviceVector(np.full(lead + k*ldo + lead, sentinel))
        try:
            call(d_free, d_in.ptr + 8*lead, ldi, d_out.ptr + 8*lead, ldo, k,
                 hb.DEVICE)
            col.hip.synchronize()
            got = d_out.numpy()
        finally:
            for x in (d_free, d_in, d_out):
                x.close()
        assert np.all(got[:lead] == sentinel)
        assert np.all(got[lead + k*ldo:] == sentinel)
        body = got[lead:lead + k*ldo].reshape(k, ldo)
        assert np.all(body[:, nout:] == sentinel)
        assert np.array_equal(_bits(body[:, :nout]), _bits(tight))


def test_torch_tensors_give_the_host_path_bits():
    import torch
    col = cases.collocator('pend2_link_vardur_unkmass_small')
    jmm, jtmm = _functions(col)
    free, V, W = _inputs(9, col, 5)
    host_jv, host_jtw = jmm(free, V), jtmm(free, W)
    dfree = torch.from_numpy(free).cuda()
    dev_jv = jmm(dfree, torch.from_numpy(V).cuda())
    dev_jtw = jtmm(dfree, torch.from_numpy(W).cuda())
    assert dev_jv.is_cuda and dev_jtw.is_cuda
    assert tuple(dev_jv.shape) == host_jv.shape
    assert tuple(dev_jtw.shape) == host_jtw.shape
    assert np.array_equal(_bits(host_jv), _bits(dev_jv.cpu().numpy()))
    assert np.array_equal(_bits(host_jtw), _bits(dev_jtw.cpu().numpy()))
    empty = jmm(dfree, torch.from_numpy(V[:, :0]).cuda())
    assert empty.is_cuda and tuple(empty.shape) == (col.num_constraints, 0)
    one = jtmm(dfree, torch.from_numpy(W[:, :1]).cuda())
    assert np.array_equal(_bits(one.cpu().numpy()[:, 0]),
                          _bits(jtmm(free, W[:, :1])[:, 0]))
    with pytest.raises(ValueError):
        jmm(free, V[:-1])
    with pytest.raises(ValueError):
        jmm(free, V[:, 0])
    with pytest.raises(ValueError):
        jtmm(free[:-1], W)
    with pytest.raises(ValueError):
        jtmm(free, V)
    with pytest.raises(ValueError):
        jmm(dfree, torch.from_numpy(W).cuda())
    with pytest.raises(ValueError):
        jtmm(dfree, torch.from_numpy(W[:, 0]).cuda())


def test_known_parameter_change_is_seen():
    from examples import problems
    import opty_amd
    kw = problems.build('config3_10link_small')
    col = opty_amd.ConstraintCollocator(**kw)
    jmm, jtmm = _functions(col)
    free, V, W = _inputs(10, col, 3)
    first = jmm(free, V), jtmm(free, W)
    g = [p for p in col.known_parameters if str(p) == 'g'][0]
    col.known_parameter_map[g] = 3.5
    second = jmm(free, V), jtmm(free, W)
    kw2 = dict(kw, known_parameter_map=dict(kw['known_parameter_map']))
    kw2['known_parameter_map'][g] = 3.5
    fresh = opty_amd.ConstraintCollocator(**kw2)
    want = _functions(fresh)
    want = want[0](free, V), want[1](free, W)
    for a, b, c in zip(first, second, want):
        assert not np.array_equal(a, b)
        np.testing.assert_allclose(b, c, rtol=1e-13, atol=1e-300)


def test_operator_matmat_and_rmatmat():
    import opty_amd
    from examples import problems
    import torch
    from test_jacprod_cpu import interpreted_products
    kw = problems.build('config2_pendulum_small')
    col = opty_amd.ConstraintCollocator(**kw)
    k = 5
    free, V, W = _inputs(11, col, k)
    op = col.jacobian_operator(free)
    JV, JTW = op.matmat(V), op.rmatmat(W)
    assert JV.shape == (col.num_constraints, k)
    assert JTW.shape == (col.num_free, k)
    width = col._jacprod_block_meta['width']
    _, _, bv, bw = cases.interpreted_block(col, free, V, W, width)
    U = 2.0**-53
    for c in range(k):
        # matvec on the column: the single program; both within their bounds
        # of the exact product, so within the sum of the two of each other
        mv, rmv = op.matvec(V[:, c]), op.rmatvec(W[:, c])
        _, _, sv, sw = interpreted_products(col, free, V[:, c], W[:, c],
                                            with_bounds=True)
        assert np.all(np.abs(JV[:, c] - mv) <= 64*U*(bv[:, c] + sv))
        assert np.all(np.abs(JTW[:, c] - rmv) <= 64*U*(bw[:, c] + sw))
    # one column is matvec, bit for bit
    assert np.array_equal(_bits(op.matmat(V[:, :1])[:, 0]),
                          _bits(op.matvec(V[:, 0])))
    assert np.array_equal(_bits(op.rmatmat(W[:, :1])[:, 0]),
                          _bits(op.rmatvec(W[:, 0])))
    # a CUDA free: a CUDA block is answered with a CUDA tensor
    dop = col.jacobian_operator(torch.from_numpy(free).cuda())
    dJV = dop.matmat(torch.from_numpy(V).cuda())
    assert dJV.is_cuda
    assert np.array_equal(_bits(dJV.cpu().numpy()), _bits(JV))
    assert np.array_equal(_bits(dop.rmatmat(W)), _bits(JTW))
    # the Problem facade forwards
    args = {key: v for key, v in kw.items()
            if key not in ('equations_of_motion', 'state_symbols',
                           'num_collocation_nodes', 'node_time_interval')}
    prob = opty_amd.Problem(
        lambda f: 0.0, lambda f: np.zeros_like(f), kw['equations_of_motion'],
        kw['state_symbols'], kw['num_collocation_nodes'],
        kw['node_time_interval'], **args)
    pop = prob.jacobian_operator(free)
    assert pop.shape == op.shape
    assert np.array_equal(_bits(pop.matmat(V)), _bits(JV))
    assert np.array_equal(_bits(pop.rmatmat(W)), _bits(JTW))


def test_sketch_example(capsys):
    from examples import jacobian_sketch
    B, B_ref = jacobian_sketch.main()
    out = capsys.readouterr().out
    assert 'singular value estimates' in out
    print(out)
    assert B.shape == (jacobian_sketch.COLUMNS,)*2
    assert np.all(np.abs(B - B_ref) <= 1e-10*np.abs(B_ref).max())


# ---- C ABI errors, each on its own ------------------------------------------

@pytest.fixture(scope='module')
def abi():
    col = cases.collocator('vardur_pendulum_small')
    hb, lib, handle = _abi(col)
    free, V, W = _inputs(12, col, 3)
    state = dict(col=col, hb=hb, lib=lib, handle=handle, free=free,
                 V=np.ascontiguousarray(V.T), W=np.ascontiguousarray(W.T),
                 Y=np.full((3, col.num_constraints), -5.0),
                 G=np.full((3, col.num_free), -5.0))
    yield state
    # the handle still works afterwards
    jmm, jtmm = _functions(col)
    assert np.all(np.isfinite(jmm(free, V)))
    assert np.all(np.isfinite(jtmm(free, W)))
    assert np.all(state['Y'] == -5.0) and np.all(state['G'] == -5.0)


def _jvp(s, h='handle', free='free', V='V', ldv=None, Y='Y', ldy=None,
         ncols=3, mem=None):
    hb, col = s['hb'], s['col']
    get = lambda x: None if x is None else hb._ptr(s[x])  # noqa: E731
    rc = s['lib'].opty_hip_jacprod_block_jvp(
        None if h is None else s['handle']._handle(), get(free), get(V),
        col.num_free if ldv is None else ldv, get(Y),
        col.num_constraints if ldy is None else ldy, ncols,
        hb.HOST if mem is None else mem)
    return rc, s['lib'].opty_hip_last_error()


def test_abi_null_handle(abi):
    rc, msg = _jvp(abi, h=None)
    assert rc != 0 and b'null' in msg
    assert abi['lib'].opty_hip_jacprod_block_width(None) == -1


@pytest.mark.parametrize('which', ['free', 'V', 'Y'])
def test_abi_null_arrays(abi, which):
    rc, msg = _jvp(abi, **{which: None})
    assert rc != 0 and b'null' in msg


def test_abi_negative_ncols(abi):
    rc, msg = _jvp(abi, ncols=-1)
    assert rc != 0 and b'ncols -1' in msg


def test_abi_ldv_too_small(abi):
    n = abi['col'].num_free
    rc, msg = _jvp(abi, ldv=n - 1)
    assert rc != 0 and b'ldv %d' % (n - 1) in msg and b'%d' % n in msg


def test_abi_ldy_too_small(abi):
    n = abi['col'].num_constraints
    rc, msg = _jvp(abi, ldy=n - 1)
    assert rc != 0 and b'ldy %d' % (n - 1) in msg and b'%d' % n in msg


def test_abi_result_overlaps_the_input(abi):
    # Y starts inside V: num_constraints < num_free, so Y's three columns
    # with ldy = num_free lie within V's
    col = abi['col']
    assert col.num_constraints <= col.num_free
    rc, msg = _jvp(abi, Y='V', ldy=col.num_free)
    assert rc != 0 and b'overlaps' in msg and b'3 columns' in msg
    assert np.array_equal(abi['V'], np.ascontiguousarray(
        _inputs(12, col, 3)[1].T))


def test_abi_bad_memory_kind(abi):
    rc, msg = _jvp(abi, mem=7)
    assert rc != 0 and b'memory kind 7' in msg


def test_abi_zero_columns_launch_nothing(abi):
    rc, _ = _jvp(abi, ncols=0)
    assert rc == 0
    assert np.all(abi['Y'] == -5.0)


def _create(s, hsaco=None, **changes):
    hb, col = s['hb'], s['col']
    meta = col._jacprod_block_meta
    prog = col._build_jacprod_program()
    good = dict(width=meta['width'], jvp_strips=meta['jvp_strips'],
                vjp_strips=meta['vjp_strips'], num_tail=prog.r + prog.s,
                nnz_inst=len(prog.inst_jac_out))
    return hb.HipJacobianBlockProduct(col.hip, dict(good, **changes),
                                      meta['hsaco'] if hsaco is None
                                      else hsaco)


def test_abi_width_3_is_refused(abi):
    with pytest.raises(abi['hb'].HipBackendError, match='width 3'):
        _create(abi, width=3)


def test_abi_wrong_num_tail_is_refused(abi):
    with pytest.raises(abi['hb'].HipBackendError, match='num_tail 3'):
        _create(abi, num_tail=3)


def test_abi_code_object_without_the_block_kernels(abi):
    # the single product module: none of the four block kernels
    abi['col'].generate_jvp_function()
    with pytest.raises(abi['hb'].HipBackendError,
                       match='opty_jvp_block missing'):
        _create(abi, hsaco=abi['col']._jacprod_meta['hsaco'])


def test_abi_destroy_null(abi):
    assert abi['lib'].opty_hip_jacprod_block_destroy(None) == 0
    # a second handle on the same module comes and goes
    extra = _create(abi)
    assert extra.width == abi['col']._jacprod_block_meta['width']
    extra.release()


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_block_functions_take_their_arguments(label):
    """Host blocks: a new column-major array per call.  A tensor block that
    is neither float64 nor contiguous: its columns are gathered on the device
    and the result, the bits of the host path, is the transposed view of a
    ``(k, n)`` buffer; no column, no launch; one column is the single
    product."""
    import torch
    import hessian_cases as hc
    col, free, lam = hc.surface_case(label)
    jmm, jtmm = _functions(col)
    singles = (col.generate_jvp_function(), col.generate_vjp_function())
    dfree, free32 = hc.odd(free)
    rng = np.random.default_rng(23)
    for f, single, nin, nout in (
            (jmm, singles[0], col.num_free, col.num_constraints),
            (jtmm, singles[1], col.num_constraints, col.num_free)):
        k = 2*f.width + 1
        X = rng.uniform(-1.0, 1.0, (nin, k))
        dX, X32 = hc.odd(X)
        assert dX.dtype == torch.float32 and not dX.is_contiguous()
        want = f(free32, X32.tolist())
        assert want.flags.f_contiguous and f(free32, X32) is not want
        out = f(dfree, dX)
        assert out.is_cuda and out.dtype == torch.float64
        assert tuple(out.shape) == (nout, k) and out.t().is_contiguous()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        empty = f(dfree, dX[:, :0])
        assert empty.is_cuda and tuple(empty.shape) == (nout, 0)
        assert f(free32, X32[:, :0]).shape == (nout, 0)
        one = f(dfree, dX[:, 1:2])
        assert tuple(one.shape) == (nout, 1)
        assert np.array_equal(_bits(one.cpu().numpy()[:, 0]),
                              _bits(single(free32, X32[:, 1])))
        with pytest.raises(ValueError, match=r'must have shape \(%d, k\), '
                           r'got \(%d, %d\)' % (nin, nin - 1, k)):
            f(free32, X32[1:])
        with pytest.raises(ValueError, match=r'must have shape \(%d, k\)'
                           % nin):
            f(dfree, dX[1:])
        with pytest.raises(ValueError, match='free must have shape'):
            f(dfree[1:], dX)
