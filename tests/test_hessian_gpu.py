"""GPU tests of the exact Hessian of the constraint Lagrangian
(``ConstraintCollocator.generate_hessian_function`` / ``hessian_indices``,
C ABI ``opty_hip_hessian_*``, kernels ``opty_hess`` / ``opty_hess_inst``)
against the CPU interpreter of the same DAG, the closed-form indices, a
finite difference of the GPU Jacobian and the ``Problem`` callbacks."""
import numpy as np
import pytest

from golden_util import assert_close
from hessian_cases import interpreted as _interpreted
from test_hessian_cpu import _nonlinear_instance_pendulum

from examples import problems

pytestmark = pytest.mark.gpu

PROBLEMS = ['msd_be_small', 'msd_mid_small', 'vardur_pendulum_small',
            'pend2_link_vardur_unkmass_small', 'config2_pendulum_small',
            'config3_10link_small', 'piecewise_be_small', 'c99_be_small',
            'biped_small', 'biped_mid_small', 'one_legged_small']


def _inputs(seed, col):
    rng = np.random.default_rng(seed)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.02
    return free, rng.uniform(-1.0, 1.0, col.num_constraints)


def _collocator(kw):
    import opty_amd
    return opty_amd.ConstraintCollocator(**kw)


@pytest.mark.parametrize('name', PROBLEMS)
def test_device_values_and_indices(name):
    from opty_amd import hip_backend as hb
    col = _collocator(problems.build(name))
    hess = col.generate_hessian_function()
    rows, cols = col.hessian_indices()
    r0, c0 = col.hessian_indices_closed_form()
    assert rows.dtype == np.int64 and cols.dtype == np.int64
    assert np.array_equal(rows, r0) and np.array_equal(cols, c0)
    assert np.all(rows >= cols)
    free, lam = _inputs(1, col)
    got = hess(free, lam).copy()
    prog = col._build_hessian_program()
    ncn, PH = col.num_collocation_nodes - 1, prog.PH
    block, inst, bnd = _interpreted(col, free, lam)
    assert len(got) == ncn*PH + len(inst)
    assert_close(got[:ncn*PH], block.ravel(), rtol=1e-12, bound=bnd.ravel(),
                 what=name)
    np.testing.assert_allclose(got[ncn*PH:], inst, rtol=1e-12, atol=1e-300)
    meta = col._hessian_meta
    assert meta['verdict']['ok'] is True
    res = hb.cached_kernel_resources(meta['hsaco'])
    kernels = [k for k in res if k.startswith('opty_hess')]
    assert kernels
    for k in kernels:
        assert res[k]['.vgpr_spill_count'] == 0, (name, k, res[k])


def test_finite_difference_of_the_gpu_jacobian():
    """Nonlinear instance constraints: the summed triplets equal a central
    finite difference of ``J(free)^T lagrange`` from the GPU Jacobian."""
    kw = _nonlinear_instance_pendulum(num_nodes=11)
    col = _collocator(kw)
    hess = col.generate_hessian_function()
    rows, cols = col.hessian_indices()
    jac = col.generate_jacobian_function()
    jr, jc = col.jacobian_indices()
    free, lam = _inputs(2, col)

    def grad(x):
        g = np.zeros(col.num_free)
        np.add.at(g, jc, jac(x)*lam[jr])
        return g
    step = 1e-6
    fd = np.empty((col.num_free, col.num_free))
    for k in range(col.num_free):
        d = np.zeros(col.num_free)
        d[k] = step
        fd[:, k] = (grad(free + d) - grad(free - d))/(2*step)
    fd = np.tril(0.5*(fd + fd.T))
    dense = np.zeros_like(fd)
    np.add.at(dense, (rows, cols), hess(free, lam))
    assert col._build_hessian_program().inst_hess_out
    np.testing.assert_allclose(dense, fd, rtol=1e-6,
                               atol=1e-6*max(1.0, np.abs(fd).max()))


def test_host_and_device_pointers_agree_and_large_window():
    """Host arrays and torch CUDA tensors give the same bytes; a node window
    of the 10-link pendulum at N = 100 000 equals the interpreter."""
    import torch
    kw = problems.build('config3_10link')
    col = _collocator(kw)
    hess = col.generate_hessian_function()
    free, lam = _inputs(3, col)
    host = hess(free, lam).copy()
    dev = hess(torch.from_numpy(free).cuda(), torch.from_numpy(lam).cuda())
    assert np.array_equal(host.view(np.int64),
                          dev.cpu().numpy().view(np.int64))
    PH = col._build_hessian_program().PH
    ncn = col.num_collocation_nodes - 1
    nodes = np.r_[np.arange(70), np.arange(50000, 50070),
                  np.arange(ncn - 70, ncn)]
    block, _, bnd = _interpreted(col, free, lam, nodes)
    got = host[:ncn*PH].reshape(ncn, PH)[nodes]
    assert_close(got.ravel(), block.ravel(), rtol=1e-12, bound=bnd.ravel(),
                 what='config3 window')


def test_known_parameter_change_is_seen():
    """Change a known parameter between two calls: the second call equals a
    fresh collocator's (no stale tables)."""
    kw = problems.build('config3_10link_small')
    col = _collocator(kw)
    hess = col.generate_hessian_function()
    free, lam = _inputs(4, col)
    first = hess(free, lam).copy()
    g = [p for p in col.known_parameters if str(p) == 'g'][0]
    col.known_parameter_map[g] = 3.5
    second = hess(free, lam).copy()
    kw2 = dict(kw, known_parameter_map=dict(kw['known_parameter_map']))
    kw2['known_parameter_map'][g] = 3.5
    fresh = _collocator(kw2).generate_hessian_function()(free, lam)
    assert not np.array_equal(first, second)
    np.testing.assert_allclose(second, fresh, rtol=1e-13, atol=1e-300)


def test_problem_with_objective_hessian():
    import opty_amd
    kw = problems.build('config2_pendulum_small')
    N = kw['num_collocation_nodes']
    T = kw['state_symbols'][0].func   # placeholder, not used
    del T
    col0 = _collocator(kw)
    num_free = col0.num_free
    # objective: sum of squares of the input trajectory (rows 2N..3N)
    h = kw['node_time_interval']
    idx = np.arange(2*N, 3*N, dtype=np.int64)

    def obj(free):
        return h*np.sum(free[idx]**2)

    def obj_grad(free):
        g = np.zeros(num_free)
        g[idx] = 2*h*free[idx]
        return g

    def obj_hess(free):
        return np.full(N, 2*h)
    args = {k: v for k, v in kw.items()
            if k not in ('equations_of_motion', 'state_symbols',
                         'num_collocation_nodes', 'node_time_interval')}
    prob = opty_amd.Problem(obj, obj_grad, kw['equations_of_motion'],
                            kw['state_symbols'], N, h,
                            obj_hessian=(idx, idx, obj_hess), **args)
    free, lam = _inputs(5, prob.collocator)
    rows, cols = prob.hessianstructure()
    vals = prob.hessian(free, lam, 0.7)
    assert len(rows) == len(cols) == len(vals)
    con = prob.collocator.generate_hessian_function()(free, lam)
    np.testing.assert_array_equal(vals[:len(con)], con)
    np.testing.assert_allclose(vals[len(con):], 0.7*2*h, rtol=1e-15)
    plain = opty_amd.Problem(obj, obj_grad, kw['equations_of_motion'],
                             kw['state_symbols'], N, h, **args)
    assert not hasattr(plain, 'hessian')
    assert not hasattr(plain, 'hessianstructure')


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_function_takes_its_arguments(label):
    """Host arrays: one persistent buffer, whatever the arrays were made of.
    Tensors that are neither float64 nor contiguous: converted on the device,
    a new tensor per call with the bits of the host path."""
    import torch
    import hessian_cases as hc
    col, free, lam = hc.surface_case(label)
    hess = col.generate_hessian_function()
    first = hess(free, lam)
    assert hess(free.tolist(), lam.astype(np.float32)) is first
    dfree, free32 = hc.odd(free)
    dlam, lam32 = hc.odd(lam)
    assert dfree.dtype == torch.float32 and not dfree.is_contiguous()
    want = hess(free32, lam32).copy()
    out, again = hess(dfree, dlam), hess(dfree, dlam)
    assert out.is_cuda and out.dtype == torch.float64
    assert tuple(out.shape) == want.shape
    assert out.data_ptr() != again.data_ptr()
    assert np.array_equal(hc.bits(out), hc.bits(want))
    assert np.array_equal(hc.bits(again), hc.bits(want))
    with pytest.raises(ValueError, match=r'lagrange must have shape \(%d,\), '
                       r'got \(%d,\)' % (len(lam), len(lam) - 1)):
        hess(free, lam[1:])
    with pytest.raises(ValueError, match='free must have shape'):
        hess(dfree[1:], dlam)
    with pytest.raises(ValueError, match='lagrange must have shape'):
        hess(dfree, dlam[1:])


def test_exact_hessian_example_converges(capsys):
    from examples import vyasarayani_exact_hessian, vyasarayani_scipy
    p_hat, res = vyasarayani_exact_hessian.main()
    p_qn, _ = vyasarayani_scipy.main(verbose=False)
    assert abs(p_hat - p_qn) <= 1e-4, (p_hat, p_qn)
    out = capsys.readouterr().out
    assert 'iterations' in out
    print(out)
