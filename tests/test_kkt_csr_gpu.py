"""GPU tests of the augmented system as CSR (``opty_kkt_diag`` /
``opty_kkt_jrows`` / ``opty_kkt_inst`` behind ``opty_hesscsr``, C ABI
``opty_hip_kktcsr_*``, ``ConstraintCollocator.kkt_csr_structure`` /
``generate_kkt_csr_function``, ``Problem.kkt_csr``): the structure against the
host statement's and SciPy's, ``data`` bit for bit against NumPy scatters of
``hcsr(free, lagrange)`` and ``jacobian(free)`` at block and tile edges,
inside guard bands, between calls and memory kinds, the regularisation, the
``Problem`` level against ``examples/kkt_direct.py``, torch tensors, the error
paths of the C ABI and the handle's lifetime."""
import ctypes

import numpy as np
import pytest

import hessian_cases as hc
import kkt_csr_cases as kc

pytestmark = pytest.mark.gpu


def _off_by_eight(values):
    """``values`` on the device, 8 bytes off a 16-byte boundary."""
    import torch
    raw = torch.empty(len(values) + 1, dtype=torch.float64, device='cuda')
    out = raw[1:]
    out.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    assert out.data_ptr() % 16 == 8
    return out


def _device_assemble(hip, handle, hvals, jvals, sigma, dw, dc, what):
    """``handle``'s assembly for device pointers: ``data`` inside guard
    bands, the inputs one double off the allocation's alignment."""
    import torch
    from opty_amd import hip_backend as hb
    dh, dj = _off_by_eight(hvals), _off_by_eight(jvals)
    ds = None if sigma is None else _off_by_eight(sigma)
    buf = kc.Guarded(handle.nnz_kkt)
    torch.cuda.synchronize()
    handle.assemble(dh, dj, ds, dw, dc, buf.doubles, hb.DEVICE)
    hip.synchronize()
    return buf.check(what)


def _case(label, ncn, prune, seed=91, col=None):
    """One collocator (``col``: a problem that is not on the list) through
    every check of the block-edge cases; returns what the other tests go on
    with."""
    import torch
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import kkt_csr_structure
    what = '%s N-1=%d prune=%s' % (label, ncn, prune)
    if col is None:
        col = kc.collocator(label, ncn, prune)
    kkt = col.generate_kkt_csr_function()
    handle = kkt.handle
    ref = kc.Reference(col)
    n, m = ref.n, ref.m

    # the structure: the handle's in both memory kinds, the host statement's,
    # SciPy's
    indptr, indices = col.kkt_csr_structure()
    ref.check_structure(what, indptr, indices)
    assert handle.nnz_kkt == len(indices)
    want = kkt_csr_structure(
        col._build_program(), col.num_collocation_nodes,
        jac_inst_rows=col._inst_rows, jac_inst_cols=col._inst_cols,
        **col._hessmv_descriptor())
    assert np.array_equal(indptr, want[0]), what
    assert np.array_equal(indices, want[1]), what
    dptr = torch.full((n + m + 1,), -1, dtype=torch.int64, device='cuda')
    didx = torch.full((len(indices),), -1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    handle.structure(dptr, didx, hb.DEVICE)
    assert np.array_equal(dptr.cpu().numpy(), indptr), what
    assert np.array_equal(didx.cpu().numpy(), indices), what

    # the values the existing functions give
    free, lam = hc.inputs(seed, col)
    hvals = col.generate_hessian_function()(free, lam).copy()
    hptr, hidx = col.hessian_csr_structure()
    hdata = col.generate_hessian_csr_function()(free, lam).copy()
    jvals = col.generate_jacobian_function()(free).copy()
    jrows, jcols = col.jacobian_indices()
    sigma = np.random.default_rng(seed + 1).uniform(0.0, 1.0, n)
    assert handle.nnz == len(hvals) and col.hip.nnz == len(jvals)
    assert handle.nnz_hessian == len(hidx) + len(ref.absent)

    out = {}
    for tag, sig, dw, dc in (('reg', sigma, 1e-4, 1e-8),
                             ('plain', None, 0.0, 0.0)):
        expect = ref.expected(hptr, hidx, hdata, jrows, jcols, jvals, sig,
                              dw, dc)
        dev = _device_assemble(col.hip, handle, hvals, jvals, sig, dw, dc,
                               what)
        assert np.array_equal(kc.bits(dev), kc.bits(expect)), (what, tag)
        host = np.full(handle.nnz_kkt, np.nan)
        handle.assemble(hvals, jvals, sig, dw, dc, host, hb.HOST)
        assert np.array_equal(kc.bits(host), kc.bits(dev)), (what, tag)
        again = _device_assemble(col.hip, handle, hvals, jvals, sig, dw, dc,
                                 what + ' again')
        assert np.array_equal(kc.bits(again), kc.bits(dev)), (what, tag)
        # the function itself and its assemble
        kw = dict(sigma=sig, delta_w=dw, delta_c=dc)
        assert np.array_equal(kc.bits(kkt(free, lam, **kw)), kc.bits(dev)), \
            (what, tag)
        assert np.array_equal(kc.bits(kkt.assemble(hvals, jvals, **kw)),
                              kc.bits(dev)), (what, tag)
        out[tag] = dev
    return dict(col=col, kkt=kkt, ref=ref, free=free, lam=lam, hvals=hvals,
                jvals=jvals, sigma=sigma, indptr=indptr, indices=indices,
                hdata=hdata, hptr=hptr, hidx=hidx, **out)


@pytest.mark.parametrize('label,ncn,prune', kc.GPU_CASES)
def test_block_edges(label, ncn, prune):
    got = _case(label, ncn, prune)
    col = got['col']
    if label == 'C':
        assert len(col._inst_rows) > 0
    if prune:
        lens = np.diff(col._build_program().row_start)
        assert len(set(lens.tolist())) > 1


def test_equation_span_of_more_than_two_tiles():
    label, ncn, prune = kc.LONG_SPAN_CASE
    col = kc.collocator(label, ncn, prune)
    lens = np.diff(col._build_program().row_start)
    span = ncn*(int(lens.max()) + 1)
    assert span > 2*kc.JROWS_TILE and span % kc.JROWS_TILE not in (0, 1)
    _case(label, ncn, prune)


def test_regularisation_touches_the_diagonals_alone():
    got = _case('A', 65, False, seed=93)
    ref, n = got['ref'], got['ref'].n
    indptr = got['indptr']
    assert len(ref.absent) > 0      # structurally absent Hessian diagonals
    wdiag, cdiag = indptr[1:n + 1] - 1, indptr[n + 1:] - 1
    off = np.ones(len(got['indices']), dtype=bool)
    off[wdiag] = off[cdiag] = False
    assert np.array_equal(kc.bits(got['reg'][off]),
                          kc.bits(got['plain'][off]))
    # h of every free row from the compressed Hessian, +0.0 where absent
    h = np.zeros(n)
    hrow = np.repeat(np.arange(n), np.diff(got['hptr']))
    on = hrow == got['hidx']
    h[hrow[on]] = got['hdata'][on]
    assert np.array_equal(kc.bits(got['reg'][wdiag]),
                          kc.bits((h + got['sigma']) + 1e-4))
    assert np.array_equal(kc.bits(got['plain'][wdiag]),
                          kc.bits((h + 0.0) + 0.0))
    assert np.array_equal(kc.bits(got['plain'][wdiag][ref.absent]),
                          kc.bits(np.zeros(len(ref.absent))))
    assert np.array_equal(kc.bits(got['reg'][cdiag]),
                          kc.bits(np.full(ref.m, 0.0 - 1e-8)))
    assert np.array_equal(kc.bits(got['plain'][cdiag]),
                          kc.bits(np.zeros(ref.m)))


def test_torch_tensors_in_and_out():
    import torch
    got = _case('B', 65, False, seed=94)
    kkt, free, lam = got['kkt'], got['free'], got['lam']

    def cuda(a):
        return torch.from_numpy(a).cuda()
    out = kkt(cuda(free), cuda(lam), sigma=cuda(got['sigma']), delta_w=1e-4,
              delta_c=1e-8)
    assert out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(kc.bits(out.cpu().numpy()), kc.bits(got['reg']))
    again = kkt(cuda(free), cuda(lam))
    assert again.data_ptr() != out.data_ptr()
    assert np.array_equal(kc.bits(again.cpu().numpy()), kc.bits(got['plain']))
    out = kkt.assemble(cuda(got['hvals']), cuda(got['jvals']))
    assert out.is_cuda
    assert np.array_equal(kc.bits(out.cpu().numpy()), kc.bits(got['plain']))
    with pytest.raises(ValueError, match='shape'):
        kkt.assemble(cuda(got['hvals'][1:]), cuda(got['jvals']))
    with pytest.raises(ValueError, match='shape'):
        kkt.assemble(got['hvals'], got['jvals'][1:])
    with pytest.raises(ValueError, match='shape'):
        kkt.assemble(got['hvals'], got['jvals'], sigma=got['sigma'][1:])
    with pytest.raises(ValueError, match='shape'):
        kkt(free, lam[1:])
    with pytest.raises(ValueError, match='shape'):
        kkt(free[1:], lam)
    with pytest.raises(ValueError, match='shape'):
        kkt(cuda(free), cuda(lam), sigma=cuda(got['sigma'][1:]))


def test_problem_level_against_the_direct_example():
    import scipy.sparse as sp
    import torch
    from examples import kkt_augmented, kkt_direct
    prob = kkt_augmented.problem(20)
    col = prob.collocator
    n, m = prob.num_free, prob.num_constraints
    free, lam = hc.inputs(95, col)
    indptr, indices = prob.kkt_csr_structure()
    assert np.array_equal(indices[indptr[1:] - 1], np.arange(n + m))
    for factor in (1.0, 0.7):
        data = np.array(prob.kkt_csr(free, lam, factor))
        got = sp.csr_matrix((data, indices, indptr), shape=(n + m, n + m))
        assert got.has_canonical_format
        # the triangle of the example with explicit diagonals (zeros)
        L = kkt_direct.kkt_lower_triangle(prob, col, free, lam, factor)
        assert np.array_equal(got.toarray(), L.toarray())
        want = L.copy()
        want.data[:] = 1.0
        want = (want + sp.identity(n + m)).tocsr()
        want.sort_indices()
        assert np.array_equal(want.indptr, indptr)
        assert np.array_equal(want.indices, indices)
        # the W part off the diagonal: the bits of Problem.hessian_csr
        hptr, hidx = prob.hessian_csr_structure()
        hdata = np.array(prob.hessian_csr(free, lam, factor))
        hrow = np.repeat(np.arange(n), np.diff(hptr))
        size = n + m
        key = np.repeat(np.arange(size), np.diff(indptr))*size + indices
        at = np.searchsorted(key, hrow*size + hidx)
        assert np.array_equal(key[at], hrow*size + hidx)
        offd = hrow != hidx
        assert np.array_equal(kc.bits(data[at[offd]]), kc.bits(hdata[offd]))
        assert np.array_equal(kc.bits(data[at[~offd]]),
                              kc.bits((hdata[~offd] + 0.0) + 0.0))
    assert prob.hessian_csr_structure()[1].size < \
        int(indptr[n])                    # diagonals were added
    sigma = np.random.default_rng(96).uniform(0.0, 1.0, n)
    reg = np.array(prob.kkt_csr(free, lam, 0.7, sigma=sigma, delta_w=1e-4,
                                delta_c=1e-8))
    wdiag, cdiag = indptr[1:n + 1] - 1, indptr[n + 1:] - 1
    assert np.array_equal(kc.bits(reg[wdiag]),
                          kc.bits((data[wdiag] + sigma) + 1e-4))
    assert np.array_equal(kc.bits(reg[cdiag]),
                          kc.bits(np.full(m, 0.0 - 1e-8)))
    out = prob.kkt_csr(torch.from_numpy(free).cuda(),
                       torch.from_numpy(lam).cuda(), 0.7,
                       sigma=torch.from_numpy(sigma).cuda(), delta_w=1e-4,
                       delta_c=1e-8)
    assert out.is_cuda
    assert np.array_equal(kc.bits(out.cpu().numpy()), kc.bits(reg))


def test_problem_level_refusals():
    from examples import kkt_minres
    prob = kkt_minres.problem(20)       # the Jacobian in the COO layout
    free, lam = hc.inputs(97, prob.collocator)
    with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
        prob.kkt_csr_structure()
    with pytest.raises(ValueError, match=r"jacobian_layout='csr'"):
        prob.kkt_csr(free, lam)


def test_augmented_step_of_the_example():
    """``examples/kkt_augmented.py`` at N = 20: the regularised step solves
    the unregularised system up to the regularisation -- ``K z - rhs =
    -diag(delta_w, -delta_c) z`` exactly, so the residual through the
    operators is at most ``delta |z|`` plus the solver's own residual, held
    to the ``1e-8 |rhs|`` of the direct example -- and approaches the direct
    step as ``delta -> 0``."""
    from examples import kkt_augmented
    steps, residuals, distances, rhs_norm = kkt_augmented.main(
        20, verbose=False)
    for delta, step, res, dist in zip(kkt_augmented.DELTAS, steps, residuals,
                                      distances):
        print('delta %.0e: residual %.3e, distance %.3e, |z| %.3e, |rhs| '
              '%.3e' % (delta, res, dist, np.linalg.norm(step), rhs_norm))
        assert res <= delta*np.linalg.norm(step) + 1e-8*rhs_norm
    assert distances[-1] < distances[0]


def test_c_abi_rejections():
    """Every misuse returns non-zero with a message, before any launch, and
    a following good call still works."""
    import torch
    from opty_amd import hip_backend as hb
    got = _case('C', 65, False, seed=98)
    col, handle = got['col'], got['kkt'].handle
    lib = hb.load_library()

    def message():
        return lib.opty_hip_last_error().decode()
    out = ctypes.c_void_p()
    desc = handle._descriptor()
    assert lib.opty_hip_kktcsr_create(None, ctypes.byref(desc),
                                      ctypes.byref(out)) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_kktcsr_create(col.hip._h, None,
                                      ctypes.byref(out)) != 0
    assert 'null argument' in message()
    assert lib.opty_hip_kktcsr_create(col.hip._h, ctypes.byref(desc),
                                      None) != 0
    assert 'null argument' in message()
    # a problem handle in the COO layout
    coo = kc.collocator('C', 65, layout='coo')
    assert lib.opty_hip_kktcsr_create(coo.hip._h, ctypes.byref(desc),
                                      ctypes.byref(out)) != 0
    assert 'OPTY_HIP_LAYOUT_CSR' in message() and \
        "jacobian_layout='csr'" in message()
    with pytest.raises(hb.HipBackendError, match='OPTY_HIP_LAYOUT_CSR'):
        hb.HipKktCsr(coo.hip, col._hessmv_descriptor())

    h = handle._handle()
    nh, nj, nk = handle.nnz, col.hip.nnz, handle.nnz_kkt
    hv, jv, data = np.zeros(nh), np.zeros(nj), np.zeros(nk)

    def assemble(hess, jac, sigma, dat, mem):
        return lib.opty_hip_kktcsr_assemble(h, hess, jac, sigma, 0.0, 0.0,
                                            dat, mem)
    for args in ((None, jv.ctypes.data, None, data.ctypes.data),
                 (hv.ctypes.data, None, None, data.ctypes.data),
                 (hv.ctypes.data, jv.ctypes.data, None, None)):
        assert assemble(*args, hb.HOST) != 0
        assert 'null argument' in message()
    assert lib.opty_hip_kktcsr_assemble(None, None, None, None, 0.0, 0.0,
                                        None, hb.HOST) != 0
    assert assemble(hv.ctypes.data, jv.ctypes.data, None, data.ctypes.data,
                    7) != 0
    assert 'bad memory kind 7' in message()
    assert lib.opty_hip_kktcsr_structure(h, None, None, hb.HOST) != 0
    assert 'null argument' in message()
    # data overlapping an input, from either end, in both memory kinds
    both = np.zeros(nh + nj + nk)
    dboth = torch.zeros(nh + nj + nk, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    for base, mem in ((both.ctypes.data, hb.HOST),
                      (dboth.data_ptr(), hb.DEVICE)):
        hess_at, jac_at, data_at = base, base + 8*nh, base + 8*(nh + nj)
        assert assemble(hess_at, jac_at, None, hess_at + 8*(nh - 1),
                        mem) != 0
        assert 'overlaps' in message() and 'Hessian' in message()
        assert assemble(hess_at, jac_at, None, data_at - 8, mem) != 0
        assert 'overlaps' in message() and 'Jacobian' in message()
        assert assemble(hess_at, jac_at, data_at + 8*(nk - 1), data_at,
                        mem) != 0
        assert 'overlaps' in message() and 'sigma' in message()
        # (side by side is fine)
        assert assemble(hess_at, jac_at, None, data_at, mem) == 0
    col.hip.synchronize()
    assert lib.opty_hip_kktcsr_nnz(None) == -1
    assert lib.opty_hip_kktcsr_nnz_hessian(None) == -1
    assert lib.opty_hip_kktcsr_nnz_triplets(None) == -1
    assert lib.opty_hip_kktcsr_destroy(None) == 0
    # ... and the handle is as good as before
    again = got['kkt'](got['free'], got['lam'])
    assert np.array_equal(kc.bits(again), kc.bits(got['plain']))


def test_handle_lifetime():
    from opty_amd import hip_backend as hb
    got = _case('A', 64, False, seed=99)
    col, kkt = got['col'], got['kkt']
    handle = kkt.handle
    # a second function reuses the handle
    assert col.generate_kkt_csr_function().handle is handle
    col._respecialize(col._hip)
    assert handle._h is None
    assert np.array_equal(
        kc.bits(kkt.assemble(got['hvals'], got['jvals'])),
        kc.bits(got['plain']))
    assert handle._h is not None
    # releasing the collocator's problem handle releases the handle
    col._hip.close()
    assert handle._h is None
    with pytest.raises(hb.HipBackendError, match='closed'):
        kkt.assemble(got['hvals'], got['jvals'])


@pytest.mark.parametrize('label', ['A', 'C'])
def test_how_the_functions_take_their_arguments(label):
    """Host arrays: ``kkt`` and ``kkt.assemble`` answer from one persistent
    buffer, ``assemble.result``.  Tensors that are neither float64 nor
    contiguous, ``sigma`` among them: converted on the device, a new tensor
    per call with the bits of the host path."""
    import torch
    col, free, lam = hc.surface_case(label)
    kkt = col.generate_kkt_csr_function()
    sigma = np.random.default_rng(31).uniform(0.0, 1.0, col.num_free)
    first = kkt(free, lam)
    assert first is kkt.assemble.result
    assert kkt(free.tolist(), lam.astype(np.float32),
               sigma=sigma.tolist()) is first
    hvals = np.array(col.generate_hessian_function()(free, lam))
    jvals = np.array(col.generate_jacobian_function()(free))
    assert kkt.assemble(hvals.tolist(), jvals.tolist()) is first
    dfree, free32 = hc.odd(free)
    dlam, lam32 = hc.odd(lam)
    dsigma, sigma32 = hc.odd(sigma)
    assert dsigma.dtype == torch.float32 and not dsigma.is_contiguous()
    for given, host in ((dict(), dict()),
                        (dict(sigma=dsigma, delta_w=1e-4, delta_c=1e-8),
                         dict(sigma=sigma32, delta_w=1e-4, delta_c=1e-8))):
        want = kkt(free32, lam32, **host).copy()
        out, again = kkt(dfree, dlam, **given), kkt(dfree, dlam, **given)
        assert out.is_cuda and out.dtype == torch.float64
        assert out.data_ptr() != again.data_ptr()
        assert np.array_equal(kc.bits(out.cpu().numpy()), kc.bits(want))
        assert np.array_equal(kc.bits(again.cpu().numpy()), kc.bits(want))
    dh, h32 = hc.odd(hvals)
    dj, j32 = hc.odd(jvals)
    want = kkt.assemble(h32, j32, sigma32, 1e-4).copy()
    out = kkt.assemble(dh, dj, dsigma, 1e-4)
    assert out.is_cuda and out.dtype == torch.float64
    assert np.array_equal(kc.bits(out.cpu().numpy()), kc.bits(want))
    with pytest.raises(ValueError, match=r'sigma must have shape \(%d,\), '
                       r'got \(%d,\)' % (len(sigma), len(sigma) - 1)):
        kkt(free, lam, sigma=sigma[1:])
    with pytest.raises(ValueError, match='sigma must have shape'):
        kkt(dfree, dlam, sigma=dsigma[1:])
    with pytest.raises(ValueError, match='jac_values must have shape'):
        kkt.assemble(dh, dj[1:])
    with pytest.raises(ValueError, match='lagrange must have shape'):
        kkt(dfree, dlam[1:])
