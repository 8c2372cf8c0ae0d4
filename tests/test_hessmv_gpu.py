"""GPU tests of the Hessian operator (``opty_hessmv`` / ``opty_hessmv_fin``,
C ABI ``opty_hip_hessmv_*``, ``ConstraintCollocator.
generate_hessian_product_function`` / ``hessian_operator``, ``Problem.
hessian_operator``): ``y = H v`` from the stored triplets against
``scipy.sparse`` on the same triplets (``hessmv_cases.reference``, tolerance
``4 (k_r + 2) 2**-53 (|H| |v|)_r``) at block edges, inside guard bands, bit
for bit between calls and memory kinds, with an objective section, as an
operator, and the error paths of the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

import hessian_cases as hc
import hessmv_cases as mc
import objective_hessian_cases as ohc

from examples import problems

pytestmark = pytest.mark.gpu

#: a quiet NaN with a payload that no arithmetic produces
SENTINEL = 0x7FF8DEADBEEF1234
GUARD = 256


class Guarded(object):
    """A CUDA buffer of ``n`` doubles between two guard bands, all of it
    filled with ``SENTINEL`` (the idea of tests/test_hessian_kernel_gpu.py);
    ``shift`` moves the view by that many doubles."""

    def __init__(self, n, shift=0):
        import torch
        self.n, self.lo = n, GUARD + shift
        self.raw = torch.full((n + 2*GUARD + 2,), SENTINEL,
                              dtype=torch.int64, device='cuda')
        self.doubles = self.raw.view(torch.float64)[self.lo:self.lo + n]
        torch.cuda.synchronize()

    def check(self, what):
        """The ``n`` doubles after both bands were found untouched and every
        inner item written."""
        got = self.raw.cpu().numpy()
        lo, n = self.lo, self.n
        for name, band in (('below', got[:lo]), ('above', got[lo + n:])):
            hit = np.flatnonzero(band != SENTINEL)
            assert hit.size == 0, (what, name, hit[:8])
        left = np.flatnonzero(got[lo:lo + n] == SENTINEL)
        assert left.size == 0, (what, 'never written', left[:8])
        return got[lo:lo + n].copy().view(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _device_product(col, handle, values, v, what):
    """``handle``'s product for device pointers: ``y`` inside guard bands,
    the values one double off the allocation's alignment."""
    import torch
    from opty_amd import hip_backend as hb
    raw = torch.empty(len(values) + 1, dtype=torch.float64, device='cuda')
    dval = raw[1:]
    dval.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    assert len(values) == 0 or dval.data_ptr() % 16 == 8
    dv = torch.from_numpy(v).cuda()
    buf = Guarded(col.num_free)
    torch.cuda.synchronize()
    handle.apply(dval, dv, buf.doubles, hb.DEVICE)
    col.hip.synchronize()
    return buf.check(what)


def _constraint_case(col, what, seed=31):
    """Values of ``generate_hessian_function``; the product from device and
    from host memory and twice: right, all written, the same bits."""
    hess = col.generate_hessian_function()
    hmv = col.generate_hessian_product_function()
    rows, cols = col.hessian_indices_closed_form()
    free, lam = hc.inputs(seed, col)
    values = hess(free, lam).copy()
    assert hmv.handle.nnz == len(values) == len(rows)
    v = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, col.num_free)
    dev = _device_product(col, hmv.handle, values, v, what)
    mc.check(what, dev, col.num_free, rows, cols, values, v)
    host = hmv(values, v).copy()
    assert np.array_equal(_bits(host), _bits(dev)), what
    again = _device_product(col, hmv.handle, values, v, what + ' again')
    assert np.array_equal(_bits(again), _bits(dev)), what
    return hmv, values, v, dev


@pytest.mark.parametrize('label,ncn', mc.GPU_EDGES)
def test_block_edges(label, ncn):
    col = hc.collocator(label, ncn)
    prog = col._build_hessian_program()
    if label == 'C':
        assert prog.inst_hess_out and prog.r
    if label == 'A':
        assert prog.r
    hmv = _constraint_case(col, '%s N-1=%d' % (label, ncn))[0]
    # the handle's side table is the host statement's
    from opty_amd.codegen.program import hessian_side_table
    sides, ntraj = hessian_side_table(prog.index_pattern())[:2]
    assert hmv.handle.sides() == (sides, ntraj)


def test_variable_duration_free_interval_in_the_tail():
    import opty_amd
    col = opty_amd.ConstraintCollocator(
        **problems.build('vardur_pendulum_small'))
    assert col._variable_duration
    _constraint_case(col, 'vardur_pendulum_small')


def test_torch_tensors_in_and_out():
    import torch
    col = hc.collocator('E', 65)
    hmv, values, v, dev = _constraint_case(col, 'E torch')
    out = hmv(torch.from_numpy(values).cuda(), torch.from_numpy(v).cuda())
    assert out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(dev))
    with pytest.raises(ValueError, match='shape'):
        hmv(torch.from_numpy(values[1:]).cuda(), torch.from_numpy(v).cuda())
    with pytest.raises(ValueError, match='shape'):
        hmv(values, v[1:])
    with pytest.raises(ValueError, match='shape'):
        hmv(values[1:], v)


# -- objective section --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pendulum():
    return ohc.pendulum_problem(41)


def _problem_reference(prob, free, lam, factor, v):
    rows, cols = prob.hessianstructure()
    values = np.array(prob.hessian(free, lam, factor))
    return rows, cols, values


def test_problem_operator_with_objective_section():
    prob, _ = _pendulum()
    free, lam = hc.inputs(41, prob.collocator)
    v = np.random.default_rng(42).uniform(-1.0, 1.0, prob.num_free)
    op = prob.hessian_operator(free, lam, 0.7)
    assert op.shape == (prob.num_free, prob.num_free)
    rows, cols, values = _problem_reference(prob, free, lam, 0.7, v)
    assert np.array_equal(_bits(op.values.numpy()), _bits(values))
    y = op @ v
    mc.check('pendulum, obj_factor 0.7', y, prob.num_free, rows, cols,
             values, v)
    # the objective's entries are there: without them the product differs
    con = prob.collocator.hessian_operator(free, lam) @ v
    assert not np.array_equal(con, y)


def test_operator_owns_its_values_and_is_symmetric():
    """NumPy and torch CUDA vectors give equal bits, ``rmatvec`` is
    ``matvec``, and a later Hessian evaluation does not reach an existing
    operator."""
    import torch
    prob, _ = _pendulum()
    free, lam = hc.inputs(43, prob.collocator)
    free2, lam2 = hc.inputs(44, prob.collocator)
    v = np.random.default_rng(45).uniform(-1.0, 1.0, prob.num_free)
    op = prob.hessian_operator(free, lam)
    first = op.matvec(v)
    assert np.array_equal(_bits(op.rmatvec(v)), _bits(first))
    on_device = op.matvec(torch.from_numpy(v).cuda())
    assert on_device.is_cuda
    assert np.array_equal(_bits(on_device.cpu().numpy()), _bits(first))
    dev = prob.hessian_operator(torch.from_numpy(free).cuda(),
                                torch.from_numpy(lam).cuda())
    assert dev.values.is_cuda
    assert np.array_equal(_bits(dev.matvec(v)), _bits(first))
    assert np.array_equal(
        _bits(dev.rmatvec(torch.from_numpy(v).cuda()).cpu().numpy()),
        _bits(first))
    other = np.array(prob.hessian(free2, lam2, 1.0))
    prob.collocator.generate_hessian_function()(free2, lam2)
    assert not np.array_equal(other, op.values.numpy())
    assert np.array_equal(_bits(op.matvec(v)), _bits(first))
    # the constraint operator of the collocator alone
    cop = prob.collocator.hessian_operator(free, lam)
    crows, ccols = prob.collocator.hessian_indices_closed_form()
    cvals = prob.collocator.generate_hessian_function()(free, lam).copy()
    prob.collocator.generate_hessian_function()(free2, lam2)
    mc.check('constraint operator', cop.matvec(v), prob.num_free, crows,
             ccols, cvals, v)


def _objective_only_handle(name, N):
    """A product handle made directly from an objective pattern, PH = 0, on
    the carrier problem's handle."""
    import opty_amd
    from opty_amd import hip_backend as hb
    nrows, r, pattern, pairs, base = mc.objective_program(name)
    col = opty_amd.ConstraintCollocator(**mc.carrier_problem(N))
    prog = col._build_hessian_program()
    assert (prog.n + prog.q, prog.r, prog.s) == (nrows, r, 0)
    tail = nrows*N
    handle = hb.HipHessianProduct(col.hip, dict(
        obj_pattern=pattern, obj_base=base, tail_rows=tail + pairs[:, 0],
        tail_cols=tail + pairs[:, 1]))
    return col, handle


def test_objective_only_midpoint_tail_sums_over_three_blocks():
    N = mc.OBJECTIVE_ONLY_NODES
    assert (N - 1 + 62)//63 >= 3
    col, handle = _objective_only_handle('all_mid', N)
    rows, cols, values_of = ohc.function('all_mid', N)
    assert values_of.handle.desc['T'] > 0 and handle.nnz == len(rows)
    tail = col.num_free - 3
    # parameters meet trajectories: tail sums over every block
    assert np.any((rows >= tail) & (cols < tail))
    free = ohc.make_free(ohc.BY_NAME['all_mid'], N)
    v = np.random.default_rng(46).uniform(-1.0, 1.0, col.num_free)
    values = values_of(free, 0.7)
    dev = _device_product(col, handle, values, v, 'all_mid')
    mc.check('all_mid N=%d' % N, dev, col.num_free, rows, cols, values, v)
    from opty_amd import hip_backend as hb
    host = np.full(col.num_free, np.nan)
    handle.apply(values, v, host, hb.HOST)
    assert np.array_equal(_bits(host), _bits(dev))
    # obj_factor = 0: every value is zero and so is every element of y
    zero = values_of(free, 0.0)
    assert not zero.any()
    out = _device_product(col, handle, zero, v, 'all_mid, obj_factor 0')
    assert np.array_equal(_bits(out), _bits(np.zeros(col.num_free)))
    handle.release()


# -- lifecycle ----------------------------------------------------------------
def test_handle_is_released_and_made_again_with_the_problem_handle():
    from opty_amd import hip_backend as hb
    col = hc.collocator('A', 65)
    hmv, values, v, dev = _constraint_case(col, 'A lifecycle')
    handle = hmv.handle
    col._respecialize(col._hip)
    assert handle._h is None
    assert np.array_equal(_bits(hmv(values, v)), _bits(dev))
    assert handle._h is not None
    col._hip.close()
    assert handle._h is None
    with pytest.raises(hb.HipBackendError, match='closed'):
        hmv(values, v)


# -- errors ---------------------------------------------------------------------
def test_problem_operator_errors():
    import opty_amd
    hand, _ = ohc.pendulum_problem(41, obj_hessian='hand')
    free, lam = hc.inputs(47, hand.collocator)
    with pytest.raises(TypeError, match='values.handle'):
        hand.hessian_operator(free, lam)
    # an objective Hessian of another size (N = 41 against 31)
    _, hess = _pendulum()
    kw = problems.pendulum_swing_up(num_nodes=41, method=ohc.BE)
    rows, cols, values = hess
    small = ohc.function('effort_be', 31)[2]
    assert small.handle.desc['N'] == 31

    def values31(free, obj_factor=1.0, out=None):
        return values(free, obj_factor, out)
    values31.handle = small.handle
    prob = opty_amd.Problem(lambda f: 0.0, lambda f: 0*f,
                            obj_hessian=(rows, cols, values31), **kw)
    with pytest.raises(ValueError, match='built for'):
        prob.hessian_operator(free, lam)
    plain = opty_amd.Problem(lambda f: 0.0, lambda f: 0*f, **kw)
    assert not hasattr(plain, 'hessian_operator')


def test_c_abi_rejections():
    """Every misuse returns non-zero with a message, before any launch."""
    from opty_amd import hip_backend as hb
    col = hc.collocator('C', 65)
    hmv = col.generate_hessian_product_function()
    good = col._hessmv_descriptor()
    prog = col._build_hessian_program()
    nrows, ntail = prog.n + prog.q, prog.r + prog.s
    assert len(good['inst_rows']) == 1
    lib = hb.load_library()

    def refused(match, **change):
        with pytest.raises(hb.HipBackendError, match=match):
            hb.HipHessianProduct(col.hip, dict(good, **change))

    def pattern(e, k, value):
        pat = np.array(good['pattern'], dtype=np.int32).copy()
        pat[e, k] = value
        return pat
    refused('bad Hessian-product descriptor', PH=-1)
    refused('bad Hessian-product descriptor', nnz_inst=-1)
    refused('bad Hessian-product descriptor', E=-1)
    refused('bad Hessian-product descriptor', T=-1)
    refused('null index pattern', pattern=(), PH=3)
    refused('null objective index pattern', E=2)
    refused('null instance indices', inst_rows=(), inst_cols=(), nnz_inst=1)
    refused('null parameter-parameter indices', T=1)
    tails = [e for e, row in enumerate(good['pattern']) if row[0] == -1]
    trajs = [e for e, row in enumerate(good['pattern']) if row[0] >= 0]
    refused(r'row %d outside \[-1, %d\)' % (nrows, nrows),
            pattern=pattern(trajs[0], 0, nrows))
    refused(r'row -2 outside', pattern=pattern(trajs[0], 2, -2))
    refused(r'slot 2 outside \{0, 1\}', pattern=pattern(trajs[0], 1, 2))
    refused(r'slot -1 outside \{0, 1\}', pattern=pattern(trajs[0], 1, -1))
    refused(r'tail offset %d outside \[0, %d\)' % (ntail, ntail),
            pattern=pattern(tails[0], 1, ntail))
    one = np.array([(0, 0, 0, 0)], dtype=np.int32)
    refused(r'objective pattern entry 0: slot 2',
            obj_pattern=np.array([(0, 1, 0, 1)], dtype=np.int32), obj_base=1)
    refused(r'obj_base 2 outside', obj_pattern=one, obj_base=2)
    nf = col.num_free
    refused(r'instance entry 0: \(%d, 0\) outside \[0, %d\)' % (nf, nf),
            inst_rows=[nf], inst_cols=[0])
    refused(r'instance entry 0: \(0, -1\) outside', inst_rows=[0],
            inst_cols=[-1])
    refused(r'instance entry 0: \(3, 5\) is above the diagonal',
            inst_rows=[3], inst_cols=[5])
    refused(r'parameter-parameter entry 0: \(%d, 0\) outside' % nf,
            tail_rows=[nf], tail_cols=[0])
    refused(r'parameter-parameter entry 0: \(1, 2\) is above the diagonal',
            tail_rows=[1], tail_cols=[2])
    def message():
        return lib.opty_hip_last_error().decode()
    out = ctypes.c_void_p()
    desc = hmv.handle._descriptor()
    assert lib.opty_hip_hessmv_create(None, ctypes.byref(desc),
                                      ctypes.byref(out)) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_hessmv_create(col.hip._h, None,
                                      ctypes.byref(out)) != 0
    assert lib.opty_hip_hessmv_create(col.hip._h, ctypes.byref(desc),
                                      None) != 0
    assert 'null argument' in message()
    h = hmv.handle._handle()
    y = np.zeros(nf)
    assert lib.opty_hip_hessmv_apply(h, None, y.ctypes.data, y.ctypes.data,
                                     hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_hessmv_apply(None, None, None, None, hb.HOST) != 0
    vals = np.zeros(hmv.handle.nnz)
    assert lib.opty_hip_hessmv_apply(h, vals.ctypes.data, y.ctypes.data,
                                     y.copy().ctypes.data, 7) != 0
    assert 'bad memory kind 7' in message()
    assert lib.opty_hip_hessmv_nnz(None) == -1
    assert lib.opty_hip_hessmv_sides(None, None, 0, None) == -1
    assert lib.opty_hip_hessmv_destroy(None) == 0
    # ... and the handle is as good as before
    _constraint_case(col, 'C after the refusals')


def test_more_than_64_kib_of_lds():
    """48 sides need 64.5 KiB of LDS per block, more than a kernel gets
    without asking: every side of the planar biped's 24 trajectory rows, on
    the diagonal and coupled to the row before it, with random values."""
    import opty_amd
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import hessian_side_table
    col = opty_amd.ConstraintCollocator(**problems.build('biped_small'))
    N = col.num_collocation_nodes
    nrows = col.num_states + col.num_unknown_input_trajectories
    pattern = np.array(
        [(R, s, R, s) for R in range(nrows) for s in (0, 1)] +
        [(R, 0, R - 1, 1) for R in range(1, nrows)], dtype=np.int32)
    sides = hessian_side_table(pattern)[0]
    assert 64*33*8 + len(sides)*2*64*8 > 65536
    handle = hb.HipHessianProduct(col.hip, dict(pattern=pattern))
    assert handle.sides()[0] == sides
    i = np.arange(N - 1)[:, None]
    rows = (pattern[:, 0]*N + i + pattern[:, 1]).ravel()
    cols = (pattern[:, 2]*N + i + pattern[:, 3]).ravel()
    assert np.all(rows >= cols) and handle.nnz == len(rows)
    rng = np.random.default_rng(50)
    values = rng.uniform(-1.0, 1.0, len(rows))
    v = rng.uniform(-1.0, 1.0, col.num_free)
    dev = _device_product(col, handle, values, v, 'biped, 48 sides')
    mc.check('biped, 48 sides', dev, col.num_free, rows, cols, values, v)
    handle.release()


# -- example --------------------------------------------------------------------
def test_kkt_operator_of_the_example():
    """``[[H, J^T], [J, 0]] z`` of examples/kkt_minres.py at N = 20 against
    the dense assembly from the triplets and ``jacobian(free)``: the lower
    triangle of K is the Hessian's triplets and the Jacobian's, moved down
    by ``num_free`` rows."""
    from examples import kkt_minres
    prob = kkt_minres.problem(20)
    n, m = prob.num_free, prob.num_constraints
    free, lam = hc.inputs(48, prob.collocator)
    K, H, J = kkt_minres.kkt_operator(prob, free, lam, 0.7)
    assert K.shape == (n + m, n + m)
    z = np.random.default_rng(49).uniform(-1.0, 1.0, n + m)
    hrows, hcols = prob.hessianstructure()
    hvals = np.array(prob.hessian(free, lam, 0.7))
    jrows, jcols = prob.jacobianstructure()
    jvals = np.array(prob.jacobian(free))
    mc.check('KKT N=20', K.matvec(z), n + m, np.r_[hrows, n + jrows],
             np.r_[hcols, jcols], np.r_[hvals, jvals], z)
    step, history = kkt_minres.main(20, maxiter=5, verbose=False)
    assert step.shape == (n + m,) and len(history) >= 1


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_product_takes_its_arguments(label):
    """Host arrays: one persistent buffer.  Tensors that are neither float64
    nor contiguous: converted on the device, a new tensor per call with the
    bits of the host path."""
    import torch
    col, free, lam = hc.surface_case(label)
    hmv = col.generate_hessian_product_function()
    values = np.array(col.generate_hessian_function()(free, lam))
    v = free[::-1]
    first = hmv(values, v)
    assert hmv(values.tolist(), v.astype(np.float32)) is first
    dvalues, values32 = hc.odd(values)
    dv, v32 = hc.odd(v)
    assert dv.dtype == torch.float32 and not dv.is_contiguous()
    want = hmv(values32, v32).copy()
    out, again = hmv(dvalues, dv), hmv(dvalues, dv)
    assert out.is_cuda and out.dtype == torch.float64
    assert out.data_ptr() != again.data_ptr()
    assert np.array_equal(hc.bits(out), hc.bits(want))
    assert np.array_equal(hc.bits(again), hc.bits(want))
    with pytest.raises(ValueError, match=r'v must have shape \(%d,\), got '
                       r'\(%d,\)' % (len(v), len(v) - 1)):
        hmv(values, v[1:])
    with pytest.raises(ValueError, match='values must have shape'):
        hmv(dvalues[1:], dv)
    with pytest.raises(ValueError, match='v must have shape'):
        hmv(dvalues, dv[1:])
