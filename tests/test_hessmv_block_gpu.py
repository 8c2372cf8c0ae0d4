"""GPU tests of the block products of the Hessian operator
(``opty_hessmv_block<K>`` / ``opty_hessmv_block_fin``, C ABI
``opty_hip_hessmv_apply_block`` / ``opty_hip_hessmv_block_width``,
``ConstraintCollocator.generate_hessian_block_product_function``, ``matmat``
of the Hessian operators): every column of ``Y = H V`` against
``scipy.sparse`` on the triplets (``hessmv_cases.check``, its tolerance) AND
bit for bit against the single product of that column, at block edges and for
every pass structure, with padded leading dimensions inside guard bands, with
tail sums, between calls and memory kinds, at the width the LDS rule gives a
many-sided pattern, through the Python surface, and the refusals of the C
ABI."""
import ctypes

import numpy as np
import pytest

import hessian_cases as hc
import hessmv_block_cases as bc
import hessmv_cases as mc
import objective_hessian_cases as ohc
import test_hessmv_gpu as single

from examples import problems

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = single.SENTINEL, single.GUARD
_bits = single._bits


def _lds_limit():
    """The LDS a block may ask for on the device of the tests."""
    import torch
    return torch.cuda.get_device_properties(0).shared_memory_per_block


def _block(handle, values, V, mem, pad_v=0, pad_y=0):
    """``handle.apply_block`` on the columns of ``V`` with leading dimensions
    ``num_free + pad``: the padding of ``V`` is NaN, ``Y`` lies between two
    guard bands and all of it starts as ``SENTINEL`` (a NaN).  Returns ``Y``
    of shape ``(num_free, k)`` after both bands and the padding of every
    column were found untouched and every element of a column finite."""
    import torch
    from opty_amd import hip_backend as hb
    nfree, k = V.shape
    ldv, ldy = nfree + pad_v, nfree + pad_y
    vin = np.full(max(1, k*ldv), np.nan)
    for c in range(k):
        vin[c*ldv:c*ldv + nfree] = V[:, c]
    total = 2*GUARD + k*ldy
    if mem == hb.HOST:
        raw = np.full(total, SENTINEL, dtype=np.int64)
        handle.apply_block(values, vin, ldv, raw[GUARD:].view(np.float64),
                           ldy, k, mem)
        got = raw
    else:
        dval = torch.from_numpy(np.ascontiguousarray(values)).cuda()
        dvin = torch.from_numpy(vin).cuda()
        raw = torch.full((total,), SENTINEL, dtype=torch.int64,
                         device='cuda')
        torch.cuda.synchronize()
        handle.apply_block(dval, dvin, ldv, raw[GUARD:].view(torch.float64),
                           ldy, k, mem)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL), 'guard band below Y'
    assert np.all(got[GUARD + k*ldy:] == SENTINEL), 'guard band behind Y'
    body = got[GUARD:GUARD + k*ldy].reshape(k, ldy)
    assert np.all(body[:, nfree:] == SENTINEL), 'padding of Y'
    Y = body[:, :nfree].copy().view(np.float64).T
    assert np.all(np.isfinite(Y))
    return Y


def _singles(handle, values, V):
    """``handle.apply`` column by column, device memory."""
    import torch
    from opty_amd import hip_backend as hb
    dval = torch.from_numpy(np.ascontiguousarray(values)).cuda()
    out = []
    for c in range(V.shape[1]):
        dv = torch.from_numpy(np.ascontiguousarray(V[:, c])).cuda()
        dy = torch.full((V.shape[0],), np.nan, dtype=torch.float64,
                        device='cuda')
        torch.cuda.synchronize()
        handle.apply(dval, dv, dy, hb.DEVICE)
        torch.cuda.synchronize()
        out.append(dy.cpu().numpy())
    return out


def _draw(seed, nnz, nfree, k):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, nnz), rng.uniform(-1.0, 1.0, (nfree, k))


def _held(what, Y, ones, nfree, rows, cols, values, V):
    """Every column of ``Y``: right by ``hessmv_cases.check`` and the bits of
    the single product ``ones[c]``."""
    for c in range(Y.shape[1]):
        mc.check('%s, column %d of %d' % (what, c, Y.shape[1]), Y[:, c],
                 nfree, rows, cols, values, V[:, c])
        assert np.array_equal(_bits(Y[:, c]), _bits(ones[c])), (what, c)


def _width(handle):
    """The handle's pass width, held to the LDS rule."""
    from opty_amd.codegen.program import hessian_block_width
    width = handle.block_width
    assert width == hessian_block_width(len(handle.sides()[0]), _lds_limit())
    return width


@pytest.mark.parametrize('label,ncn', bc.EDGES)
def test_block_edges_and_pass_structure(label, ncn):
    from opty_amd import hip_backend as hb
    col = hc.collocator(label, ncn)
    handle = col._ensure_hessmv()
    rows, cols = col.hessian_indices_closed_form()
    assert handle.nnz == len(rows)
    width = _width(handle)
    counts = bc.ncols_of(width)
    values, V = _draw(61, len(rows), col.num_free, max(counts))
    ones = _singles(handle, values, V)
    for ncols in counts:
        Y = _block(handle, values, V[:, :ncols], hb.DEVICE)
        _held('%s N-1=%d' % (label, ncn), Y, ones, col.num_free, rows, cols,
              values, V)


@pytest.mark.parametrize('mem', ['HOST', 'DEVICE'])
def test_guard_bands_with_padded_leading_dimensions(mem):
    """``ldv = num_free + 3``, ``ldy = num_free + 5``: the padding of ``V``
    is NaN and is never read into a result, the padding of ``Y`` and the
    guard region behind the last column keep their NaN."""
    from opty_amd import hip_backend as hb
    col = hc.collocator(*bc.GUARD_CASE)
    handle = col._ensure_hessmv()
    rows, cols = col.hessian_indices_closed_form()
    ncols = 2*_width(handle) + 1
    values, V = _draw(62, len(rows), col.num_free, ncols)
    Y = _block(handle, values, V, getattr(hb, mem), pad_v=3, pad_y=5)
    _held('guard bands, %s' % mem, Y, _singles(handle, values, V),
          col.num_free, rows, cols, values, V)


def test_variable_duration_free_interval_in_the_tail():
    import opty_amd
    from opty_amd import hip_backend as hb
    col = opty_amd.ConstraintCollocator(
        **problems.build('vardur_pendulum_small'))
    assert col._variable_duration
    handle = col._ensure_hessmv()
    rows, cols = col.hessian_indices_closed_form()
    # the free interval is the last tail entry and has node entries
    assert np.any(rows == col.num_free - 1) and handle.sides()[0][-1][0] == -1
    values, V = _draw(63, len(rows), col.num_free, 3)
    Y = _block(handle, values, V, hb.DEVICE)
    _held('vardur_pendulum_small', Y, _singles(handle, values, V),
          col.num_free, rows, cols, values, V)


def test_objective_only_midpoint_tail_partials_of_three_blocks():
    from opty_amd import hip_backend as hb
    N = mc.OBJECTIVE_ONLY_NODES
    assert (N - 1 + 62)//63 >= 3
    col, handle = single._objective_only_handle('all_mid', N)
    rows, cols = mc.objective_tables('all_mid', N)
    assert handle.nnz == len(rows)
    tail = col.num_free - 3
    assert np.any((rows >= tail) & (cols < tail))
    values, V = _draw(64, len(rows), col.num_free, 3)
    Y = _block(handle, values, V, hb.DEVICE)
    _held('all_mid N=%d' % N, Y, _singles(handle, values, V), col.num_free,
          rows, cols, values, V)
    handle.release()


def test_same_bits_between_calls_and_memory_kinds():
    from opty_amd import hip_backend as hb
    col = hc.collocator(*bc.INSTANCE_CASE)
    handle = col._ensure_hessmv()
    rows, cols = col.hessian_indices_closed_form()
    PH = len(col._build_hessian_program().index_pattern())
    assert len(rows) > PH*bc.INSTANCE_CASE[1]       # an instance entry
    ncols = 2*_width(handle) + 1
    values, V = _draw(65, len(rows), col.num_free, ncols)
    first = _block(handle, values, V, hb.DEVICE)
    _held('C', first, _singles(handle, values, V), col.num_free, rows, cols,
          values, V)
    again = _block(handle, values, V, hb.DEVICE)
    assert np.array_equal(_bits(again), _bits(first))
    host = _block(handle, values, V, hb.HOST)
    assert np.array_equal(_bits(host), _bits(first))
    # ... and a single product from host memory after the staging grew
    y = np.full(col.num_free, np.nan)
    handle.apply(values, np.ascontiguousarray(V[:, 1]), y, hb.HOST)
    assert np.array_equal(_bits(y), _bits(first[:, 1]))


def test_many_sides_take_narrow_passes():
    """The 48 sides of ``test_more_than_64_kib_of_lds``: three columns would
    need 16 896 + 3*48*1 024 = 164 352 bytes of LDS, so a pass takes two
    columns where a block gets 160 KiB and one where it gets less than
    115 200 bytes."""
    import opty_amd
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import hessian_block_width
    col = opty_amd.ConstraintCollocator(**problems.build('biped_small'))
    N = col.num_collocation_nodes
    nrows = col.num_states + col.num_unknown_input_trajectories
    pattern = np.array(
        [(R, s, R, s) for R in range(nrows) for s in (0, 1)] +
        [(R, 0, R - 1, 1) for R in range(1, nrows)], dtype=np.int32)
    handle = hb.HipHessianProduct(col.hip, dict(pattern=pattern))
    assert len(handle.sides()[0]) == 48
    want = hessian_block_width(48, _lds_limit())
    assert want in (1, 2) and handle.block_width == want
    i = np.arange(N - 1)[:, None]
    rows = (pattern[:, 0]*N + i + pattern[:, 1]).ravel()
    cols = (pattern[:, 2]*N + i + pattern[:, 3]).ravel()
    values, V = _draw(66, len(rows), col.num_free, 3)
    Y = _block(handle, values, V, hb.DEVICE)
    _held('biped, 48 sides', Y, _singles(handle, values, V), col.num_free,
          rows, cols, values, V)
    handle.release()


# -- Python surface -----------------------------------------------------------
def test_block_product_function():
    import torch
    col = hc.collocator(*bc.SURFACE_CASE)
    hmm = col.generate_hessian_block_product_function()
    hmv = col.generate_hessian_product_function()
    assert hmm.handle is hmv.handle
    nfree, k = col.num_free, 2*hmm.handle.block_width + 1
    rows, cols = col.hessian_indices_closed_form()
    values, V = _draw(67, hmm.handle.nnz, nfree, k)
    ones = [hmv(values, np.ascontiguousarray(V[:, c])).copy()
            for c in range(k)]
    for given in (np.ascontiguousarray(V), np.asfortranarray(V)):
        Y = hmm(values, given)
        assert Y.shape == (nfree, k) and Y.dtype == np.float64
        _held('hmm', Y, ones, nfree, rows, cols, values, V)
    out = hmm(torch.from_numpy(values).cuda(), torch.from_numpy(V).cuda())
    assert isinstance(out, torch.Tensor) and out.is_cuda
    assert tuple(out.shape) == (nfree, k) and out.dtype == torch.float64
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(np.stack(ones, 1)))
    assert hmm(values, V[:, :0]).shape == (nfree, 0)
    with pytest.raises(ValueError, match='shape'):
        hmm(values, V[1:])
    with pytest.raises(ValueError, match='shape'):
        hmm(values[1:], V)
    with pytest.raises(ValueError, match='shape'):
        hmm(values, V[:, 0])
    with pytest.raises(ValueError, match='shape'):
        hmm(torch.from_numpy(values).cuda(), torch.from_numpy(V[1:]).cuda())
    # the single product keeps its contract
    with pytest.raises(ValueError, match='shape'):
        hmv(values, V)


def _matmat_is_the_column_stack(op, X):
    import torch
    stack = np.stack([op.matvec(np.ascontiguousarray(X[:, c]))
                      for c in range(X.shape[1])], axis=1)
    Y = op.matmat(X)
    assert Y.shape == X.shape
    assert np.array_equal(_bits(Y), _bits(stack))
    assert np.array_equal(_bits(op @ X), _bits(stack))
    assert np.array_equal(_bits(op.rmatmat(X)), _bits(stack))
    on_device = op.matmat(torch.from_numpy(X).cuda())
    assert on_device.is_cuda and tuple(on_device.shape) == X.shape
    assert np.array_equal(_bits(on_device.cpu().numpy()), _bits(stack))
    return stack


def test_matmat_of_the_collocator_operator():
    import torch
    col = hc.collocator(*bc.SURFACE_CASE)
    free, lam = hc.inputs(68, col)
    op = col.hessian_operator(free, lam)
    k = 2*op.handle.block_width + 1
    X = np.random.default_rng(69).uniform(-1.0, 1.0, (col.num_free, k))
    stack = _matmat_is_the_column_stack(op, X)
    rows, cols = col.hessian_indices_closed_form()
    values = col.generate_hessian_function()(free, lam).copy()
    for c in range(k):
        mc.check('matmat, column %d' % c, stack[:, c], col.num_free, rows,
                 cols, values, X[:, c])
    # the operator over CUDA values
    dev = col.hessian_operator(torch.from_numpy(free).cuda(),
                               torch.from_numpy(lam).cuda())
    assert dev.values.is_cuda
    assert np.array_equal(_bits(_matmat_is_the_column_stack(dev, X)),
                          _bits(stack))
    with pytest.raises(ValueError):
        op.matmat(X[1:])


def test_matmat_of_the_problem_operator_with_objective_section():
    prob, _ = ohc.pendulum_problem(41)
    free, lam = hc.inputs(70, prob.collocator)
    op = prob.hessian_operator(free, lam, 0.7)
    k = op.handle.block_width + 1
    X = np.random.default_rng(71).uniform(-1.0, 1.0, (prob.num_free, k))
    stack = _matmat_is_the_column_stack(op, X)
    rows, cols = prob.hessianstructure()
    values = np.array(prob.hessian(free, lam, 0.7))
    for c in range(k):
        mc.check('pendulum matmat, column %d' % c, stack[:, c],
                 prob.num_free, rows, cols, values, X[:, c])
    # the objective's entries are there
    con = prob.collocator.hessian_operator(free, lam).matmat(X)
    assert not np.array_equal(con, stack)


# -- errors -------------------------------------------------------------------
def test_c_abi_rejections():
    """Every misuse returns non-zero with a message that names the offending
    number, before anything is enqueued: ``Y`` keeps its NaN."""
    from opty_amd import hip_backend as hb
    col = hc.collocator(*bc.INSTANCE_CASE)
    handle = col._ensure_hessmv()
    lib, h = hb.load_library(), handle._handle()
    nf = col.num_free
    values, V = _draw(72, handle.nnz, nf, 2)
    vals = np.ascontiguousarray(values)
    vin = np.asfortranarray(V)
    Y = np.full(2*nf, np.nan)

    def call(values, V, ldv, Y, ldy, ncols, mem=hb.HOST):
        def ptr(a):
            return None if a is None else a.ctypes.data
        return lib.opty_hip_hessmv_apply_block(h, ptr(values), ptr(V), ldv,
                                               ptr(Y), ldy, ncols, mem)

    def refused(match, *args):
        assert call(*args) != 0
        message = lib.opty_hip_last_error().decode()
        assert match in message, message
        assert np.all(np.isnan(Y))
    refused('ncols -1 < 0', vals, vin, nf, Y, nf, -1)
    refused('ldv %d < num_free %d' % (nf - 1, nf), vals, vin, nf - 1, Y, nf,
            2)
    refused('ldy %d < num_free %d' % (nf - 1, nf), vals, vin, nf, Y, nf - 1,
            2)
    refused('ldy 0 < num_free', vals, vin, nf, Y, 0, 1)
    refused('null argument', vals, None, nf, Y, nf, 2)
    refused('null argument', vals, vin, nf, None, nf, 2)
    refused('null argument', None, vin, nf, Y, nf, 2)
    refused('bad memory kind 7', vals, vin, nf, Y, nf, 2, 7)
    # Y starts inside the second column of V / inside the values
    both = np.full(3*nf, np.nan)
    assert call(vals, both, nf, both[2*nf - 1:], nf, 2) != 0
    message = lib.opty_hip_last_error().decode()
    assert 'Y (2 columns, ldy %d) overlaps V (ldv %d)' % (nf, nf) in message
    both[nf:2*nf] = V[:, 0]
    assert call(vals, both[nf:], nf, both, nf, 1) == 0      # side by side
    assert np.all(np.isfinite(both[:nf]))
    over = np.full(handle.nnz + nf, np.nan)
    assert call(over, vin, nf, over[handle.nnz - 1:], nf, 1) != 0
    message = lib.opty_hip_last_error().decode()
    assert 'overlaps the %d values' % handle.nnz in message, message
    assert lib.opty_hip_hessmv_apply_block(None, None, None, 0, None, 0, 0,
                                           hb.HOST) != 0
    assert lib.opty_hip_hessmv_block_width(None) == -1
    # no column: success, nothing written
    assert call(vals, vin, nf, Y, nf, 0) == 0
    assert np.all(np.isnan(Y))
    assert call(vals, vin, nf, Y, nf, 0, hb.DEVICE) == 0
    # ... and the handle is as good as before
    rows, cols = col.hessian_indices_closed_form()
    out = _block(handle, values, V, hb.HOST)
    _held('C after the refusals', out, _singles(handle, values, V), nf, rows,
          cols, values, V)


# -- example ------------------------------------------------------------------
def test_extreme_eigenvalues_of_the_example():
    """examples/hessian_lobpcg.py at 20 nodes against ``eigvalsh`` of the
    dense matrix assembled from the triplets; LOBPCG's residual tolerance
    times the spectral radius bounds the error of a converged eigenvalue (by
    the residual itself for a symmetric matrix, and the residual tolerance is
    relative to nothing smaller than the radius here: it is above 1)."""
    from examples import hessian_lobpcg as ex
    smallest, largest, radius, products = ex.main(bc.EXAMPLE_NODES,
                                                  verbose=False)
    prob, free, lam, H = ex.operator(bc.EXAMPLE_NODES)
    n = prob.num_free
    rows, cols = prob.hessianstructure()
    L = np.zeros((n, n))
    np.add.at(L, (rows, cols), np.array(prob.hessian(free, lam, 1.0)))
    w = np.linalg.eigvalsh(L + L.T - np.diag(np.diag(L)))
    tol = ex.TOL*radius
    print('eigenvalues', smallest, largest, 'dense', w[:ex.BLOCK],
          w[-ex.BLOCK:], 'radius', radius, 'products', products)
    assert radius >= 1.0
    assert abs(radius - max(abs(w[0]), abs(w[-1]))) <= tol
    assert np.all(np.abs(smallest - w[:ex.BLOCK]) <= tol)
    assert np.all(np.abs(largest - w[-ex.BLOCK:]) <= tol)
    assert products > 2


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_block_product_takes_its_arguments(label):
    """Host blocks: a new column-major array per call.  A tensor block that
    is neither float64 nor contiguous: its columns are gathered on the device
    and the result, the bits of the host path, is the transposed view of a
    ``(k, n)`` buffer; no column, no launch."""
    import torch
    col, free, lam = hc.surface_case(label)
    hmm = col.generate_hessian_block_product_function()
    nfree, k = col.num_free, 2*hmm.handle.block_width + 1
    values = np.array(col.generate_hessian_function()(free, lam))
    V = np.random.default_rng(29).uniform(-1.0, 1.0, (nfree, k))
    dvalues, values32 = hc.odd(values)
    dV, V32 = hc.odd(V)
    assert dV.dtype == torch.float32 and not dV.is_contiguous()
    want = hmm(values32, V32.tolist())
    assert want.flags.f_contiguous and hmm(values32, V32) is not want
    out = hmm(dvalues, dV)
    assert out.is_cuda and out.dtype == torch.float64
    assert tuple(out.shape) == (nfree, k) and out.t().is_contiguous()
    assert np.array_equal(hc.bits(out), hc.bits(want))
    empty = hmm(dvalues, dV[:, :0])
    assert empty.is_cuda and tuple(empty.shape) == (nfree, 0)
    one = hmm(dvalues, dV[:, 1:2])
    assert np.array_equal(hc.bits(one)[:, 0], hc.bits(want[:, 1]))
    with pytest.raises(ValueError, match=r'V must have shape \(%d, k\), got '
                       r'\(%d, %d\)' % (nfree, nfree - 1, k)):
        hmm(values, V[1:])
    with pytest.raises(ValueError, match='V must have shape'):
        hmm(dvalues, dV[1:])
    with pytest.raises(ValueError, match='values must have shape'):
        hmm(dvalues[1:], dV)
