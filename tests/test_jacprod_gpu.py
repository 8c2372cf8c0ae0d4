"""GPU tests of the matrix-free Jacobian products
(``ConstraintCollocator.generate_jvp_function`` / ``generate_vjp_function`` /
``jacobian_operator``, C ABI ``opty_hip_jacprod_*``, kernels ``opty_jvp`` /
``opty_jvp_inst`` / ``opty_vjp`` / ``opty_vjp_fin``) against the CPU
interpreter of the same roots and against the GPU Jacobian of the same
collocator."""
import numpy as np
import pytest

from golden_util import assert_close
from test_hessian_cpu import _nonlinear_instance_pendulum
from test_jacprod_cpu import (U, draw, interpreted_products,
                              product_tolerances, worst_ratio)

from examples import problems

pytestmark = pytest.mark.gpu

#: the problem list of tests/test_hessian_gpu.py plus the two implicit ones
PROBLEMS = ['msd_be_small', 'msd_mid_small', 'vardur_pendulum_small',
            'pend2_link_vardur_unkmass_small', 'config2_pendulum_small',
            'config3_10link_small', 'piecewise_be_small', 'c99_be_small',
            'biped_small', 'biped_mid_small', 'one_legged_small',
            'implicit_traj_be_small', 'implicit_traj_mid_small']


def _collocator(kw, **extra):
    import opty_amd
    return opty_amd.ConstraintCollocator(**dict(kw, **extra))


def _inputs(seed, col):
    rng = np.random.default_rng(seed)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.02
    return free, draw(rng, col.num_free), draw(rng, col.num_constraints)


def _matrices(col, free):
    """``(J, |J|, zero floor, entry counts)`` of the GPU Jacobian of ``col``
    as CSR matrices."""
    import scipy.sparse as sp
    jac = np.array(col.generate_jacobian_function()(free))
    rows, cols = col.jacobian_indices()
    shape = (col.num_constraints, col.num_free)
    J = sp.coo_matrix((jac, (rows, cols)), shape=shape).tocsr()
    A = sp.coo_matrix((np.abs(jac), (rows, cols)), shape=shape).tocsr()
    K = sp.coo_matrix((np.ones(len(jac)), (rows, cols)), shape=shape).tocsr()
    return J, A, sp.csr_matrix(shape), K


def _check_against_interpreter(col, free, v, w, jv, jtw, what):
    """``assert_close(rtol=1e-12)`` with every entry's bound assembled from
    its roots' bounds (a ``vjp`` node entry: the sum of its two roots'; the
    tail: the sum over the nodes)."""
    wjv, wjtw, bv, bw = interpreted_products(col, free, v, w,
                                             with_bounds=True)
    assert_close(jv, wjv, rtol=1e-12, bound=bv, what=what + ' jvp')
    assert_close(jtw, wjtw, rtol=1e-12, bound=bw, what=what + ' vjp')


@pytest.mark.parametrize('name', PROBLEMS)
def test_products_on_the_device(name):
    from opty_amd import hip_backend as hb
    col = _collocator(problems.build(name))
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    free, v, w = _inputs(1, col)
    jv, jtw = jvp(free, v).copy(), vjp(free, w).copy()
    assert jv.shape == (col.num_constraints,)
    assert jtw.shape == (col.num_free,)
    _check_against_interpreter(col, free, v, w, jv, jtw, name)
    # against the GPU Jacobian of the same collocator
    J, A, F, K = _matrices(col, free)
    tv, tw = product_tolerances(A, F, K, v, w)
    ev, ew = np.abs(jv - J @ v), np.abs(jtw - J.T @ w)
    print('%s: worst error/tolerance against coo(jacobian): jvp %.3g, vjp '
          '%.3g' % (name, worst_ratio(ev, tv), worst_ratio(ew, tw)))
    assert np.all(ev <= tv), (name, 'jvp', worst_ratio(ev, tv))
    assert np.all(ew <= tw), (name, 'vjp', worst_ratio(ew, tw))
    # bit-identical over three calls
    for _ in range(2):
        assert np.array_equal(jvp(free, v).view(np.int64), jv.view(np.int64))
        assert np.array_equal(vjp(free, w).view(np.int64),
                              jtw.view(np.int64))
    meta = col._jacprod_meta
    assert meta['verdict']['ok'] is True
    res = hb.cached_kernel_resources(meta['hsaco'])
    kernels = [k for k in res if k.startswith(('opty_jvp', 'opty_vjp'))]
    assert sorted(kernels) == ['opty_jvp', 'opty_jvp_inst', 'opty_vjp',
                               'opty_vjp_fin']
    for k in kernels:
        assert res[k]['.vgpr_spill_count'] == 0, (name, k, res[k])


def test_nonlinear_instance_constraints():
    col = _collocator(_nonlinear_instance_pendulum(num_nodes=11))
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    free, v, w = _inputs(2, col)
    jv, jtw = jvp(free, v).copy(), vjp(free, w).copy()
    _check_against_interpreter(col, free, v, w, jv, jtw, 'nonlinear instance')
    J, A, F, K = _matrices(col, free)
    tv, tw = product_tolerances(A, F, K, v, w)
    assert np.all(np.abs(jv - J @ v) <= tv)
    assert np.all(np.abs(jtw - J.T @ w) <= tw)


@pytest.mark.parametrize('extra', [dict(prune_zeros=True),
                                   dict(jacobian_layout='csr')])
def test_products_do_not_depend_on_the_jacobian_layout(extra):
    kw = problems.build('config3_10link_small')
    plain, other = _collocator(kw), _collocator(kw, **extra)
    free, v, w = _inputs(3, plain)
    a = plain.generate_jvp_function()(free, v).copy()
    b = other.generate_jvp_function()(free, v).copy()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    a = plain.generate_vjp_function()(free, w).copy()
    b = other.generate_vjp_function()(free, w).copy()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_torch_tensors_give_the_host_path_bits():
    import torch
    col = _collocator(problems.build('pend2_link_vardur_unkmass_small'))
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    free, v, w = _inputs(4, col)
    host_jv, host_jtw = jvp(free, v).copy(), vjp(free, w).copy()
    dfree = torch.from_numpy(free).cuda()
    dev_jv = jvp(dfree, torch.from_numpy(v).cuda())
    dev_jtw = vjp(dfree, torch.from_numpy(w).cuda())
    assert dev_jv.is_cuda and dev_jtw.is_cuda
    assert np.array_equal(host_jv.view(np.int64),
                          dev_jv.cpu().numpy().view(np.int64))
    assert np.array_equal(host_jtw.view(np.int64),
                          dev_jtw.cpu().numpy().view(np.int64))
    with pytest.raises(ValueError):
        jvp(free, v[:-1])
    with pytest.raises(ValueError):
        vjp(free[:-1], w)
    with pytest.raises(ValueError):
        vjp(dfree, torch.from_numpy(v).cuda()[:3])


def test_known_parameter_change_is_seen():
    kw = problems.build('config3_10link_small')
    col = _collocator(kw)
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    free, v, w = _inputs(5, col)
    first = jvp(free, v).copy(), vjp(free, w).copy()
    g = [p for p in col.known_parameters if str(p) == 'g'][0]
    col.known_parameter_map[g] = 3.5
    second = jvp(free, v).copy(), vjp(free, w).copy()
    kw2 = dict(kw, known_parameter_map=dict(kw['known_parameter_map']))
    kw2['known_parameter_map'][g] = 3.5
    fresh = _collocator(kw2)
    want = (fresh.generate_jvp_function()(free, v),
            fresh.generate_vjp_function()(free, w))
    for a, b, c in zip(first, second, want):
        assert not np.array_equal(a, b)
        np.testing.assert_allclose(b, c, rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize('num_nodes', [2, 3, 64, 65, 127, 128, 130, 200])
@pytest.mark.parametrize('method', ['backward euler', 'midpoint'])
def test_both_ends_and_block_edges(num_nodes, method):
    """``N - 1`` below, at and off the multiples of 63 and 64, and ``N = 2``:
    right values at both ends of every row and in the tail."""
    kw = problems.variable_duration_pendulum(num_nodes=num_nodes,
                                             method=method)
    col = _collocator(kw)
    free, v, w = _inputs(6, col)
    jv = col.generate_jvp_function()(free, v).copy()
    jtw = col.generate_vjp_function()(free, w).copy()
    assert np.all(np.isfinite(jv)) and np.all(np.isfinite(jtw))
    _check_against_interpreter(col, free, v, w, jv, jtw,
                               'N=%d %s' % (num_nodes, method))


def test_large_window_and_operator():
    """The 10-link pendulum at N = 100 000: both products against the GPU
    Jacobian of the same collocator."""
    col = _collocator(problems.build('config3_10link'))
    free, v, w = _inputs(7, col)
    op = col.jacobian_operator(free)
    assert op.shape == (col.num_constraints, col.num_free)
    jv, jtw = op.matvec(v), op.rmatvec(w)
    J, A, F, K = _matrices(col, free)
    tv, tw = product_tolerances(A, F, K, v, w)
    ev, ew = np.abs(jv - J @ v), np.abs(jtw - J.T @ w)
    print('config3 N=100000: worst error/tolerance jvp %.3g, vjp %.3g'
          % (worst_ratio(ev, tv), worst_ratio(ew, tw)))
    assert np.all(ev <= tv) and np.all(ew <= tw)


def test_operator_through_lsmr():
    """``lsmr`` drives ``matvec`` / ``rmatvec``: the minimum-norm solution of
    ``J x = b`` equals the one from the assembled sparse matrix."""
    import opty_amd
    from scipy.sparse.linalg import lsmr
    kw = problems.build('config2_pendulum_small')
    col = _collocator(kw)
    free, _, w = _inputs(8, col)
    op = col.jacobian_operator(free)
    J, _, _, _ = _matrices(col, free)
    x_op = lsmr(op, w, atol=1e-13, btol=1e-13, maxiter=5000)[0]
    x_mat = lsmr(J, w, atol=1e-13, btol=1e-13, maxiter=5000)[0]
    assert np.linalg.norm(J @ x_op - w) <= 1e-8*np.linalg.norm(w)
    np.testing.assert_allclose(x_op, x_mat, rtol=1e-6,
                               atol=1e-8*np.abs(x_mat).max())
    # the Problem facade forwards
    args = {k: v for k, v in kw.items()
            if k not in ('equations_of_motion', 'state_symbols',
                         'num_collocation_nodes', 'node_time_interval')}
    prob = opty_amd.Problem(
        lambda f: 0.0, lambda f: np.zeros_like(f), kw['equations_of_motion'],
        kw['state_symbols'], kw['num_collocation_nodes'],
        kw['node_time_interval'], **args)
    pop = prob.jacobian_operator(free)
    assert pop.shape == op.shape
    assert np.array_equal(pop.matvec(x_op), op.matvec(x_op))


def test_feasible_guess_example(capsys):
    from examples import feasible_guess_lsmr
    _, norms = feasible_guess_lsmr.main()
    out = capsys.readouterr().out
    assert '||c||' in out
    print(out)
    assert norms[-1] < norms[0]
    assert norms[-1] < 1e-6*norms[0]


def test_c_abi_errors():
    """Null handle, null arrays, a wrong memory kind and a bad descriptor
    return non-zero with a message; nothing aborts."""
    from opty_amd import hip_backend as hb
    col = _collocator(problems.build('msd_be_small'))
    jvp = col.generate_jvp_function()
    lib = hb.load_library()
    free, v, w = _inputs(9, col)
    out = np.empty(col.num_constraints)
    rc = lib.opty_hip_jacprod_jvp(None, hb._ptr(free), hb._ptr(v),
                                  hb._ptr(out), hb.HOST)
    assert rc != 0 and b'null' in lib.opty_hip_last_error()
    rc = lib.opty_hip_jacprod_vjp(None, hb._ptr(free), hb._ptr(w),
                                  hb._ptr(free.copy()), hb.HOST)
    assert rc != 0 and b'null' in lib.opty_hip_last_error()
    with pytest.raises(hb.HipBackendError, match='memory kind'):
        jvp.handle.jvp(free, v, out, 7)
    with pytest.raises(hb.HipBackendError, match='memory kind'):
        jvp.handle.vjp(free, w, free.copy(), -1)
    with pytest.raises(hb.HipBackendError, match='null'):
        jvp.handle.jvp(free, None, out, hb.HOST)
    hsaco = col._jacprod_meta['hsaco']
    good = dict(jvp_strips=1, vjp_strips=1, num_tail=1, nnz_inst=0)
    with pytest.raises(hb.HipBackendError, match='descriptor'):
        hb.HipJacobianProduct(col.hip, dict(good, vjp_strips=0), hsaco)
    with pytest.raises(hb.HipBackendError, match='num_tail'):
        hb.HipJacobianProduct(col.hip, dict(good, num_tail=3), hsaco)
    with pytest.raises(hb.HipBackendError, match='hipModuleLoad'):
        hb.HipJacobianProduct(col.hip, good, '/nonexistent/module.hsaco')
    # a code object without the product kernels
    with pytest.raises(hb.HipBackendError, match='missing'):
        hb.HipJacobianProduct(col.hip, good, col._kernel_meta['hsaco']
                              if 'hsaco' in col._kernel_meta
                              else hb.compile_module(col.generate_source()[0]))
    assert lib.opty_hip_jacprod_destroy(None) == 0
    # the handle still works
    assert np.all(np.isfinite(jvp(free, v)))


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_functions_take_their_arguments(label):
    """Host arrays: one persistent buffer per function.  Tensors that are
    neither float64 nor contiguous: converted on the device, a new tensor per
    call with the bits of the host path."""
    import torch
    import hessian_cases as hc
    col, free, lam = hc.surface_case(label)
    dfree, free32 = hc.odd(free)
    for f, name, x in ((col.generate_jvp_function(), 'v', free[::-1]),
                       (col.generate_vjp_function(), 'w', lam)):
        first = f(free, x)
        assert f(free.tolist(), x.astype(np.float32)) is first
        dx, x32 = hc.odd(x)
        assert dx.dtype == torch.float32 and not dx.is_contiguous()
        want = f(free32, x32).copy()
        out, again = f(dfree, dx), f(dfree, dx)
        assert out.is_cuda and out.dtype == torch.float64
        assert out.data_ptr() != again.data_ptr()
        assert np.array_equal(hc.bits(out), hc.bits(want))
        assert np.array_equal(hc.bits(again), hc.bits(want))
        with pytest.raises(ValueError, match=r'%s must have shape \(%d,\), '
                           r'got \(%d,\)' % (name, len(x), len(x) - 1)):
            f(free, x[1:])
        with pytest.raises(ValueError, match='%s must have shape' % name):
            f(dfree, dx[1:])
        with pytest.raises(ValueError, match='free must have shape'):
            f(dfree[1:], dx)
