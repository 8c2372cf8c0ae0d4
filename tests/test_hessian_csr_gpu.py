"""GPU tests of the CSR Hessian (``opty_hesscsr`` / ``opty_hesscsr_fin``, C ABI
``opty_hip_hesscsr_*``, ``ConstraintCollocator.hessian_csr_structure`` /
``generate_hessian_csr_function``, ``Problem.hessian_csr``): the triplets
compressed on the device against ``scipy.sparse`` and ``np.add.at`` on the same
triplets (``hessian_csr_cases.Reference``: a group of ``k`` addends within
``(k - 1) 2**-53 sum|a|``, short groups bit for bit) at block edges, inside
guard bands, bit for bit between calls and memory kinds, with long groups
across block edges, with an objective section, and the error paths of the C
ABI."""
import ctypes

import numpy as np
import pytest

import hessian_cases as hc
import hessian_csr_cases as cc
import hessmv_cases as mc
import objective_hessian_cases as ohc

from examples import problems

pytestmark = pytest.mark.gpu

#: a quiet NaN with a payload that no arithmetic produces
SENTINEL = 0x7FF8DEADBEEF1234
GUARD = 256


class Guarded(object):
    """A CUDA buffer of ``n`` doubles between two guard bands, all of it
    filled with ``SENTINEL`` (the class of tests/test_hessmv_gpu.py)."""

    def __init__(self, n):
        import torch
        self.n, self.lo = n, GUARD
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


def _device_compress(hip, handle, values, what):
    """``handle``'s compression for device pointers: ``data`` inside guard
    bands, the values one double off the allocation's alignment."""
    import torch
    from opty_amd import hip_backend as hb
    raw = torch.empty(len(values) + 1, dtype=torch.float64, device='cuda')
    dval = raw[1:]
    dval.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    assert dval.data_ptr() % 16 == 8
    buf = Guarded(handle.nnz_unique)
    torch.cuda.synchronize()
    handle.compress(dval, buf.doubles, hb.DEVICE)
    hip.synchronize()
    return buf.check(what)


def _hold(what, hip, handle, N, nrows, ntail, desc, rows, cols, values,
          ref=None):
    """The handle's structure (both memory kinds) against the host
    statement's and SciPy's; its data from device memory, from host memory
    and a second time: right, all written, the same bits.  Returns ``(data,
    reference)``.  ``ref``: the reference where it is not that of the
    triplets alone (a handle with every diagonal: ``desc`` then says
    ``with_diagonal`` to the host statement)."""
    import torch
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import hessian_csr_structure
    num_free = nrows*N + ntail
    assert handle.nnz == len(values) == len(rows)
    if ref is None:
        ref = cc.Reference(num_free, nrows*N, N - 1, rows, cols, values)
    assert handle.nnz_unique == len(ref.count)
    indptr = np.empty(num_free + 1, dtype=np.int64)
    indices = np.empty(handle.nnz_unique, dtype=np.int64)
    handle.structure(indptr, indices, hb.HOST)
    cc.check_structure(what, ref, indptr, indices)
    want = hessian_csr_structure(N, nrows, ntail, **desc)
    assert np.array_equal(indptr, want[0]), what
    assert np.array_equal(indices, want[1]), what
    dptr = torch.full((num_free + 1,), -1, dtype=torch.int64, device='cuda')
    didx = torch.full((len(indices),), -1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    handle.structure(dptr, didx, hb.DEVICE)
    assert np.array_equal(dptr.cpu().numpy(), indptr), what
    assert np.array_equal(didx.cpu().numpy(), indices), what

    dev = _device_compress(hip, handle, values, what)
    cc.check_values(what, ref, dev)
    host = np.full(handle.nnz_unique, np.nan)
    handle.compress(np.ascontiguousarray(values), host, hb.HOST)
    assert np.array_equal(cc.bits(host), cc.bits(dev)), what
    again = _device_compress(hip, handle, values, what + ' again')
    assert np.array_equal(cc.bits(again), cc.bits(dev)), what
    return dev, ref


def _constraint_case(col, what, seed=71):
    """Values of ``generate_hessian_function`` through the handle of
    ``generate_hessian_csr_function``; the function and its ``compress``
    give the handle's bits."""
    hess = col.generate_hessian_function()
    hcsr = col.generate_hessian_csr_function()
    rows, cols = col.hessian_indices_closed_form()
    free, lam = hc.inputs(seed, col)
    values = hess(free, lam).copy()
    prog = col._build_hessian_program()
    dev, ref = _hold(what, col.hip, hcsr.handle, col.num_collocation_nodes,
                     prog.n + prog.q, prog.r + prog.s,
                     col._hessmv_descriptor(), rows, cols, values)
    indptr, indices = col.hessian_csr_structure()
    assert indptr.dtype == indices.dtype == np.int64
    assert np.array_equal(indptr, ref.csr.indptr)
    assert np.array_equal(indices, ref.csr.indices)
    assert np.array_equal(cc.bits(hcsr.compress(values)), cc.bits(dev)), what
    assert np.array_equal(cc.bits(hcsr(free, lam)), cc.bits(dev)), what
    return hcsr, free, lam, values, dev, ref


@pytest.mark.parametrize('label,ncn', hc.BLOCK_EDGE_CASES)
def test_block_edges(label, ncn):
    col = hc.collocator(label, ncn)
    prog = col._build_hessian_program()
    if label == 'C':
        assert prog.inst_hess_out and prog.r
    ref = _constraint_case(col, '%s N-1=%d' % (label, ncn))[-1]
    # no long group: every element has the bits of np.add.at
    assert not ref.long.any()
    if label in 'ABCD' and (ncn >= 2 or label == 'C'):
        assert len(ref.count) < len(ref.group)
    if label == 'E':
        assert len(ref.count) == len(ref.group)


@pytest.mark.parametrize('ncn', cc.VARDUR_EDGES)
def test_long_groups_across_block_edges(ncn):
    col = cc.vardur_collocator(ncn)
    assert col._variable_duration
    ref = _constraint_case(col, 'vardur N-1=%d' % ncn)[-1]
    assert int(ref.long.sum()) == 3
    assert np.all(ref.count[ref.long] == ncn)


def test_long_groups_with_unknown_masses():
    import opty_amd
    col = opty_amd.ConstraintCollocator(
        **problems.build('pend2_link_vardur_unkmass_small'))
    ref = _constraint_case(col, 'pend2_link_vardur_unkmass_small')[-1]
    assert ref.long.any()


def test_torch_tensors_in_and_out():
    import torch
    col = hc.collocator('B', 65)
    hcsr, free, lam, values, dev, _ = _constraint_case(col, 'B torch')
    out = hcsr(torch.from_numpy(free).cuda(), torch.from_numpy(lam).cuda())
    assert out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(cc.bits(out.cpu().numpy()), cc.bits(dev))
    again = hcsr(torch.from_numpy(free).cuda(), torch.from_numpy(lam).cuda())
    assert again.data_ptr() != out.data_ptr()
    out = hcsr.compress(torch.from_numpy(values).cuda())
    assert out.is_cuda
    assert np.array_equal(cc.bits(out.cpu().numpy()), cc.bits(dev))
    with pytest.raises(ValueError, match='shape'):
        hcsr.compress(torch.from_numpy(values[1:]).cuda())
    with pytest.raises(ValueError, match='shape'):
        hcsr.compress(values[1:])
    with pytest.raises(ValueError, match='shape'):
        hcsr(free, lam[1:])
    with pytest.raises(ValueError, match='shape'):
        hcsr(free[1:], lam)


# -- objective section --------------------------------------------------------
def test_problem_csr_with_objective_section():
    prob = mc.kkt_problem(20)
    col = prob.collocator
    free, lam = hc.inputs(72, col)
    rows, cols = prob.hessianstructure()
    prog = col._build_hessian_program()
    tail = (prog.n + prog.q)*col.num_collocation_nodes
    indptr, indices = prob.hessian_csr_structure()
    for factor in (1.0, 0.7):
        values = np.array(prob.hessian(free, lam, factor))
        ref = cc.Reference(prob.num_free, tail, col.num_collocation_nodes - 1,
                           rows, cols, values)
        cc.check_structure('kkt_problem', ref, indptr, indices)
        data = np.array(prob.hessian_csr(free, lam, factor))
        cc.check_values('kkt_problem, obj_factor %g' % factor, ref, data)
    import torch
    out = prob.hessian_csr(torch.from_numpy(free).cuda(),
                           torch.from_numpy(lam).cuda(), 0.7)
    assert out.is_cuda
    assert np.array_equal(cc.bits(out.cpu().numpy()), cc.bits(data))
    # the handle's own checks, objective section included
    objective = col._hesscsr_objective_of
    handle = col._ensure_hesscsr(objective)
    # (the objective's triplets are there)
    assert handle.nnz > col.generate_hessian_csr_function().handle.nnz
    _hold('kkt_problem handle', col.hip, handle, col.num_collocation_nodes,
          prog.n + prog.q, prog.r + prog.s,
          col._hessmv_descriptor(objective), rows, cols, values)


def test_objective_only_midpoint_long_groups_over_three_blocks():
    import opty_amd
    from opty_amd import hip_backend as hb
    N = mc.OBJECTIVE_ONLY_NODES
    assert (N - 1 + 62)//63 >= 3
    _, nrows, r, desc, rows, cols = cc.objective_descriptor('all_mid', N)
    col = opty_amd.ConstraintCollocator(**mc.carrier_problem(N))
    prog = col._build_hessian_program()
    assert (prog.n + prog.q, prog.r, prog.s) == (nrows, r, 0) and r == 3
    handle = hb.HipHessianCsr(col.hip, desc)
    orows, ocols, values_of = ohc.function('all_mid', N)
    assert np.array_equal(orows, rows) and np.array_equal(ocols, cols)
    assert values_of.handle.desc['T'] > 0
    free = ohc.make_free(ohc.BY_NAME['all_mid'], N)
    values = np.array(values_of(free, 0.7))
    _hold('all_mid N=%d' % N, col.hip, handle, N, nrows, r, desc, rows, cols,
          values)
    handle.release()


# -- errors -------------------------------------------------------------------
def test_problem_csr_errors():
    hand, _ = ohc.pendulum_problem(41, obj_hessian='hand')
    free, lam = hc.inputs(73, hand.collocator)
    with pytest.raises(TypeError, match=r'Problem\.hessian_csr needs.*'
                       r'values\.handle'):
        hand.hessian_csr(free, lam)
    with pytest.raises(TypeError, match=r'Problem\.hessian_csr_structure'):
        hand.hessian_csr_structure()


def test_c_abi_rejections():
    """Every misuse returns non-zero with a message, before any launch, and
    a following good call still works."""
    import torch
    from opty_amd import hip_backend as hb
    col = hc.collocator('C', 65)
    hcsr = col.generate_hessian_csr_function()
    good = col._hessmv_descriptor()
    lib = hb.load_library()

    def refused(match, **change):
        with pytest.raises(hb.HipBackendError, match=match):
            hb.HipHessianCsr(col.hip, dict(good, **change))

    def pattern(e, k, value):
        pat = np.array(good['pattern'], dtype=np.int32).copy()
        pat[e, k] = value
        return pat
    prog = col._build_hessian_program()
    nrows = prog.n + prog.q
    refused('bad Hessian-product descriptor', PH=-1)
    refused('null index pattern', pattern=(), PH=3)
    refused('null instance indices', inst_rows=(), inst_cols=(), nnz_inst=1)
    trajs = [e for e, row in enumerate(good['pattern']) if row[0] >= 0]
    refused(r'row %d outside \[-1, %d\)' % (nrows, nrows),
            pattern=pattern(trajs[0], 0, nrows))
    refused(r'slot 2 outside \{0, 1\}', pattern=pattern(trajs[0], 1, 2))
    refused(r'instance entry 0: \(3, 5\) is above the diagonal',
            inst_rows=[3], inst_cols=[5])
    # both sides exchanged: a pair above the diagonal
    off = [e for e, row in enumerate(good['pattern'])
           if tuple(row[:2]) != tuple(row[2:])]
    swapped = np.array(good['pattern'], dtype=np.int32).copy()
    swapped[off[0]] = swapped[off[0], [2, 3, 0, 1]]
    refused(r'pattern entry %d: .* is above the diagonal' % off[0],
            pattern=swapped)

    def message():
        return lib.opty_hip_last_error().decode()
    out = ctypes.c_void_p()
    desc = hcsr.handle._descriptor()
    assert lib.opty_hip_hesscsr_create(None, ctypes.byref(desc),
                                       ctypes.byref(out)) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_hesscsr_create(col.hip._h, None,
                                       ctypes.byref(out)) != 0
    assert lib.opty_hip_hesscsr_create(col.hip._h, ctypes.byref(desc),
                                       None) != 0
    assert 'null argument' in message()
    h = hcsr.handle._handle()
    nnz, nu = hcsr.handle.nnz, hcsr.handle.nnz_unique
    vals, data = np.zeros(nnz), np.zeros(nu)
    assert lib.opty_hip_hesscsr_compress(h, None, data.ctypes.data,
                                         hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_hesscsr_compress(h, vals.ctypes.data, None,
                                         hb.HOST) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_hesscsr_compress(None, None, None, hb.HOST) != 0
    assert lib.opty_hip_hesscsr_compress(h, vals.ctypes.data,
                                         data.ctypes.data, 7) != 0
    assert 'bad memory kind 7' in message()
    assert lib.opty_hip_hesscsr_structure(h, None, None, hb.HOST) != 0
    assert 'null argument' in message()
    # data inside values, from either end, in both memory kinds
    both = np.zeros(nnz + nu)
    dboth = torch.zeros(nnz + nu, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    for base, mem in ((both.ctypes.data, hb.HOST),
                      (dboth.data_ptr(), hb.DEVICE)):
        for data_at in (base + 8*(nnz - 1), base):
            values_at = base if data_at != base else base + 8*(nu - 1)
            assert lib.opty_hip_hesscsr_compress(h, values_at, data_at,
                                                 mem) != 0
            assert 'overlaps' in message()
        # (side by side is fine)
        assert lib.opty_hip_hesscsr_compress(h, base, base + 8*nnz,
                                             mem) == 0
    col.hip.synchronize()
    assert not both.any() and not dboth.cpu().numpy().any()
    assert lib.opty_hip_hesscsr_nnz(None) == -1
    assert lib.opty_hip_hesscsr_nnz_unique(None) == -1
    assert lib.opty_hip_hesscsr_destroy(None) == 0
    # ... and the handle is as good as before
    _constraint_case(col, 'C after the refusals')


def test_handle_is_released_and_made_again_with_the_problem_handle():
    from opty_amd import hip_backend as hb
    col = hc.collocator('A', 65)
    hcsr, free, lam, values, dev, _ = _constraint_case(col, 'A lifecycle')
    handle = hcsr.handle
    col._respecialize(col._hip)
    assert handle._h is None
    assert np.array_equal(cc.bits(hcsr.compress(values)), cc.bits(dev))
    assert handle._h is not None
    col._hip.close()
    assert handle._h is None
    with pytest.raises(hb.HipBackendError, match='closed'):
        hcsr.compress(values)


# -- example --------------------------------------------------------------------
def test_direct_kkt_step_of_the_example():
    """``examples/kkt_direct.py`` at N = 20: the direct step's residual
    through the operators, and the step against ``minres``'s: with ``K z_d -
    rhs = r_d`` and ``K z_m - rhs = r_m``, ``|K (z_d - z_m)| <= |r_d| +
    |r_m|``, ``|r_m|`` the residual that ``minres`` reports last."""
    from examples import kkt_direct, kkt_minres
    step, residual, rhs_norm = kkt_direct.main(20, verbose=False)
    print('direct step: residual %.3e, |rhs| %.3e' % (residual, rhs_norm))
    assert residual < 1e-8*rhs_norm
    mstep, history = kkt_minres.main(20, verbose=False)
    prob = kkt_minres.problem(20)
    free = 0.1*np.random.default_rng(0).standard_normal(prob.num_free)
    K = kkt_minres.kkt_operator(prob, free,
                                np.zeros(prob.num_constraints))[0]
    apart = float(np.linalg.norm(K.matvec(step - mstep)))
    print('|K (z_direct - z_minres)| = %.3e, minres residual %.3e'
          % (apart, history[-1]))
    assert apart <= residual + history[-1]*(1 + 1e-12)


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_functions_take_their_arguments(label):
    """Host arrays: ``hcsr`` and ``hcsr.compress`` answer from one persistent
    buffer, ``compress.result``.  Tensors that are neither float64 nor
    contiguous: converted on the device, a new tensor per call with the bits
    of the host path."""
    import torch
    col, free, lam = hc.surface_case(label)
    hcsr = col.generate_hessian_csr_function()
    first = hcsr(free, lam)
    assert first is hcsr.compress.result
    assert hcsr(free.tolist(), lam.astype(np.float32)) is first
    values = np.array(col.generate_hessian_function()(free, lam))
    assert hcsr.compress(values.tolist()) is first
    dfree, free32 = hc.odd(free)
    dlam, lam32 = hc.odd(lam)
    assert dlam.dtype == torch.float32 and not dlam.is_contiguous()
    want = hcsr(free32, lam32).copy()
    out, again = hcsr(dfree, dlam), hcsr(dfree, dlam)
    assert out.is_cuda and out.dtype == torch.float64
    assert out.data_ptr() != again.data_ptr()
    assert np.array_equal(cc.bits(out.cpu().numpy()), cc.bits(want))
    assert np.array_equal(cc.bits(again.cpu().numpy()), cc.bits(want))
    dvalues, values32 = hc.odd(values)
    want = hcsr.compress(values32).copy()
    out = hcsr.compress(dvalues)
    assert out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(cc.bits(out.cpu().numpy()), cc.bits(want))
    with pytest.raises(ValueError, match=r'values must have shape \(%d,\), '
                       r'got \(%d,\)' % (len(values), len(values) - 1)):
        hcsr.compress(values[1:])
    with pytest.raises(ValueError, match='values must have shape'):
        hcsr.compress(dvalues[1:])
    with pytest.raises(ValueError, match='lagrange must have shape'):
        hcsr(dfree, dlam[1:])
