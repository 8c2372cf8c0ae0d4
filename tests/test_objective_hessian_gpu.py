"""GPU tests of the objective's exact Hessian
(``opty_amd.create_objective_hessian_function``, C ABI
``opty_hip_objhess_*``, ``Problem.hessian`` on the device) against the
independent SymPy answer of ``tests/objective_hessian_cases.py``."""
import ctypes

import numpy as np
import pytest

import objective_hessian_cases as ohc

pytestmark = pytest.mark.gpu

METHODS = [('trig_be'), ('trig_mid')]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_all_cases_against_the_independent_answer():
    """Every objective at N = 20 through the host path; the device's
    closed-form indices equal the host's."""
    N = 20
    for case in ohc.CASES:
        rows, cols, values = ohc.function(case['name'], N)
        hrows, hcols = values.indices_closed_form()
        assert rows.dtype == cols.dtype == np.int64
        assert np.array_equal(rows, hrows) and np.array_equal(cols, hcols)
        free = ohc.make_free(case, N)
        got = values(free)
        assert isinstance(got, np.ndarray) and got.shape == rows.shape
        ohc.check(case, N, free, rows, cols, got)


@pytest.mark.parametrize('name', METHODS)
@pytest.mark.parametrize('N', [2, 64, 65, 66, 130])
def test_block_edges(name, N):
    """1, 63, 64 and 65 points, then 129 in three blocks with a ragged last
    wave: in the 66 and 130 runs a midpoint ``adj`` load crosses a block edge,
    in the 130 run the tail entries sum the partials of several blocks."""
    case = ohc.BY_NAME[name]
    rows, cols, values = ohc.function(name, N)
    hrows, hcols = values.indices_closed_form()
    assert np.array_equal(rows, hrows) and np.array_equal(cols, hcols)
    free = ohc.make_free(case, N, seed=N)
    ohc.check(case, N, free, rows, cols, values(free))


def test_tail_sums_over_several_blocks():
    """``all``: parameter-parameter entries that ARE quadrature sums
    (``c**2*f2**2``), over three blocks."""
    for name in ('all_be', 'all_mid'):
        case, N = ohc.BY_NAME[name], 130
        rows, cols, values = ohc.function(name, N)
        free = ohc.make_free(case, N, seed=5)
        ohc.check(case, N, free, rows, cols, values(free))


@pytest.mark.parametrize('name', METHODS)
@pytest.mark.parametrize('N', [65, 130])
def test_every_value_written_once_and_nothing_else(name, N):
    """Device output: the interior view [64 : 64 + nnz] of a NaN buffer.  No
    NaN is left inside, both 64-double guards are bitwise untouched."""
    import torch
    case = ohc.BY_NAME[name]
    rows, cols, values = ohc.function(name, N)
    nnz = values.handle.nnz
    buf = torch.full((nnz + 128,), float('nan'), dtype=torch.float64,
                     device='cuda')
    before = buf.view(torch.int64).clone()
    free = ohc.make_free(case, N, seed=N)
    out = values(_cuda(free), 1.0, buf[64:64 + nnz])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + 64*8
    assert not torch.isnan(buf[64:64 + nnz]).any()
    after = buf.view(torch.int64)
    assert torch.equal(after[:64], before[:64])
    assert torch.equal(after[64 + nnz:], before[64 + nnz:])
    ohc.check(case, N, free, rows, cols, out.cpu().numpy())


@pytest.mark.parametrize('name', METHODS + ['all_mid'])
def test_two_calls_give_the_same_bits(name):
    import torch
    case, N = ohc.BY_NAME[name], 130
    rows, cols, values = ohc.function(name, N)
    free = _cuda(ohc.make_free(case, N, seed=7))
    first = values(free).clone()
    second = values(free)
    torch.cuda.synchronize()
    assert torch.equal(first, second)


@pytest.mark.parametrize('name', METHODS)
def test_obj_factor(name):
    case, N = ohc.BY_NAME[name], 65
    rows, cols, values = ohc.function(name, N)
    free = ohc.make_free(case, N, seed=9)
    one = values(free)
    for factor in (0.0, 1.0, -2.5):
        got = values(free, factor)
        ohc.check(case, N, free, rows, cols, got, factor=factor)
        # the factor is applied last: obj_factor*values(free), bit for bit
        assert np.array_equal(got, factor*one)
    zero = values(free, 0.0)
    assert not np.isnan(zero).any() and np.all(zero == 0.0)


def test_empty_hessians_launch_nothing_that_writes():
    """``nnz == 0`` (a linear objective): empty arrays of the right types, a
    NaN buffer stays as it is.  ``E == 0`` (``m**2`` alone): one entry."""
    import torch
    N = 20
    for name in ('linear_be', 'linear_mid'):
        case = ohc.BY_NAME[name]
        rows, cols, values = ohc.function(name, N)
        assert values.handle.nnz == 0
        assert rows.shape == cols.shape == (0,) and rows.dtype == np.int64
        free = ohc.make_free(case, N)
        got = values(free)
        assert isinstance(got, np.ndarray) and got.shape == (0,)
        buf = torch.full((128,), float('nan'), dtype=torch.float64,
                         device='cuda')
        before = buf.view(torch.int64).clone()
        out = values(_cuda(free), 1.0, buf[64:64])
        torch.cuda.synchronize()
        assert out.is_cuda and tuple(out.shape) == (0,)
        assert torch.equal(buf.view(torch.int64), before)
    for name in ('param_only_be', 'param_only_mid'):
        case = ohc.BY_NAME[name]
        rows, cols, values = ohc.function(name, N)
        assert values.handle.desc['E'] == 0 and values.handle.nnz == 1
        tail = ohc.num_free(case, N) - 1            # m: the last parameter
        assert rows.tolist() == [tail] and cols.tolist() == [tail]
        free = ohc.make_free(case, N)
        assert values(free).tolist() == [2.0]
        assert values(_cuda(free), -2.5).cpu().tolist() == [-5.0]


@pytest.mark.parametrize('name', METHODS + ['all_be'])
def test_torch_path_equals_the_host_path(name):
    import torch
    case, N = ohc.BY_NAME[name], 130
    rows, cols, values = ohc.function(name, N)
    free = ohc.make_free(case, N, seed=11)
    host = values(free, 0.7)
    dev = values(_cuda(free), 0.7)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert dev.dtype == torch.float64
    assert np.array_equal(dev.cpu().numpy(), host)
    # on a stream of the caller's
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        side = values(_cuda(free), 0.7)
    stream.synchronize()
    assert np.array_equal(side.cpu().numpy(), host)


@pytest.fixture(scope='module')
def pendulum():
    prob, hess = ohc.pendulum_problem(41)
    rng = np.random.default_rng(3)
    free = rng.uniform(-1.0, 1.0, prob.num_free)
    lam = rng.uniform(-1.0, 1.0, prob.num_constraints)
    return prob, hess, free, lam


def test_problem_with_host_inputs(pendulum):
    """``Problem(obj_hessian=create_objective_hessian_function(...))`` with
    no further argument: the structure is the two index sets, the values
    ``[con_hess(free, lam), 0.7*values(free)]``."""
    prob, (rows, cols, values), free, lam = pendulum
    crows, ccols = prob.collocator.hessian_indices()
    srows, scols = prob.hessianstructure()
    assert np.array_equal(srows, np.concatenate((crows, rows)))
    assert np.array_equal(scols, np.concatenate((ccols, cols)))
    con_hess = prob.collocator.generate_hessian_function()
    want = np.concatenate((np.array(con_hess(free, lam)),
                           0.7*values(free)))
    got = prob.hessian(free, lam, 0.7)
    assert isinstance(got, np.ndarray)
    assert np.array_equal(got, want)
    # the objective's part: 2 h on the diagonal of the torque's nodes 1 .. N-1
    N, h = 41, prob.collocator.node_time_interval
    assert np.array_equal(rows, 2*N + 1 + np.arange(N - 1))
    assert np.array_equal(cols, rows)
    np.testing.assert_allclose(values(free), 2.0*h, rtol=1e-15)


def test_problem_with_cuda_inputs(pendulum):
    """One CUDA tensor ``[constraint triplets | objective triplets]``, equal
    to the host result bit for bit; a hand-written ``values`` is refused."""
    import torch
    prob, hess, free, lam = pendulum
    want = prob.hessian(free, lam, 0.7)
    got = prob.hessian(_cuda(free), _cuda(lam), 0.7)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    hand, _ = ohc.pendulum_problem(41, obj_hessian='hand')
    assert np.array_equal(hand.hessian(free, lam, 0.7), want)
    with pytest.raises(TypeError, match='values.handle'):
        hand.hessian(_cuda(free), _cuda(lam), 0.7)


def test_c_abi_errors():
    """Every misuse of ``opty_hip_objhess_*`` returns non-zero with a
    message; the handle still works afterwards."""
    from opty_amd import hip_backend as hb
    from opty_amd.objective import compile_objective
    case, N = ohc.BY_NAME['trig_mid'], 20
    rows, cols, values = ohc.function('trig_mid', N)
    handle = values.handle
    lib = hb.load_library()
    hsaco = ohc.compile_case(case)[0]
    good = dict(handle.desc)
    program = ohc.compile_case(case)[1]
    pattern, pairs = program[1][1], program[1][4]
    table = np.concatenate((np.array(pattern, dtype=np.int32).ravel(),
                            np.array(pairs, dtype=np.int32).ravel()))
    out = ctypes.c_void_p()

    def message():
        return lib.opty_hip_last_error().decode()

    def create(desc, tab, path, outp):
        d = hb._ObjHessDesc(**desc) if desc is not None else None
        return lib.opty_hip_objhess_create(
            ctypes.byref(d) if d is not None else None,
            tab.ctypes.data if tab is not None else None, path, outp)
    assert create(None, table, hsaco.encode(), ctypes.byref(out)) != 0
    assert 'null' in message()
    assert create(good, table, None, ctypes.byref(out)) != 0
    assert 'null' in message()
    assert create(good, table, hsaco.encode(), None) != 0
    assert 'null' in message()
    assert create(good, None, hsaco.encode(), ctypes.byref(out)) != 0
    assert 'pattern' in message()
    assert create(dict(good, N=1), table, hsaco.encode(),
                  ctypes.byref(out)) != 0
    assert 'at least 2' in message()
    assert create(dict(good, device=99), table, hsaco.encode(),
                  ctypes.byref(out)) != 0
    assert 'device' in message()
    assert create(good, table, b'/nonexistent/module.hsaco',
                  ctypes.byref(out)) != 0
    assert 'hipModuleLoad' in message()
    # a pattern that leaves the free vector
    bad = table.copy()
    bad[1] = 2
    assert create(good, bad, hsaco.encode(), ctypes.byref(out)) != 0
    assert 'outside' in message()
    # the objective's own module has neither kernel
    states, inputs, unknowns = case['args']
    other = compile_objective(case['expr'], states, inputs, unknowns, N,
                              case['method'], ohc.t)[0]
    with pytest.raises(hb.HipBackendError, match='missing'):
        hb.HipObjectiveHessian(good, pattern, pairs, other)
    assert not out.value
    free = ohc.make_free(case, N)
    res = np.empty(handle.nnz)
    with pytest.raises(hb.HipBackendError, match='memory kind'):
        handle.evaluate(free, 1.0, res, 7)
    with pytest.raises(hb.HipBackendError, match='memory kind'):
        handle.indices(rows.copy(), cols.copy(), 7)
    with pytest.raises(hb.HipBackendError, match='null'):
        handle.evaluate(None, 1.0, res, hb.HOST)
    with pytest.raises(hb.HipBackendError, match='null'):
        handle.evaluate(free, 1.0, None, hb.HOST)
    with pytest.raises(hb.HipBackendError, match='null'):
        handle.indices(None, cols.copy(), hb.HOST)
    assert lib.opty_hip_objhess_eval(None, None, 1.0, None, 0) != 0
    assert lib.opty_hip_objhess_set_stream(None, None) != 0
    assert lib.opty_hip_objhess_nnz(None) == -1
    assert lib.opty_hip_objhess_destroy(None) == 0
    ohc.check(case, N, free, rows, cols, values(free))
