"""GPU tests of the Hessian kernels at the edges the generator can reach
(``opty_hess`` / ``opty_hess_inst`` / ``opty_hess_indices_kernel``, the
16-byte and 8-byte LDS tile flushes of ``csrc/opty_device.h``, C ABI
``opty_hip_hessian_*`` / ``opty_hip_eval_hess``): full and partial 64-node
blocks, every flush variant of tests/test_hessian_emit_cpu.py's table, the
emission paths a small problem never takes by itself, outputs inside guard
bands (the kernels write their ``nnz`` values, all of them and nothing else),
an independent finite-difference check of the largest DAGs, and the error
paths of the C ABI."""
import ctypes

import numpy as np
import pytest

import hessian_cases as hc
from golden_util import assert_close
from test_jacprod_cpu import draw

from examples import problems

pytestmark = pytest.mark.gpu

#: a quiet NaN with a payload that no arithmetic produces (operations on
#: finite inputs give the default NaN, 0x7ff8000000000000 or its negative)
SENTINEL = 0x7FF8DEADBEEF1234


def _band(PH):
    """Guard doubles on either side: more than a whole 64-node block of rows
    (what a flush that goes one row, or one block, too far would touch);
    even, so that the guarded view keeps the allocation's 16-byte
    alignment."""
    return 64*PH + 64


class Guarded(object):
    """A CUDA buffer of ``n`` 8-byte items between two guard bands, all of it
    filled with ``SENTINEL``; ``shift`` moves the view by that many items."""

    def __init__(self, n, PH, shift=0):
        import torch
        self.n, self.G, self.shift = n, _band(PH), shift
        assert self.G % 2 == 0
        self.raw = torch.full((n + 2*self.G + 2,), SENTINEL,
                              dtype=torch.int64, device='cuda')
        assert self.raw.data_ptr() % 16 == 0
        lo = self.G + shift
        self.ints = self.raw[lo:lo + n]
        self.doubles = self.raw.view(torch.float64)[lo:lo + n]
        torch.cuda.synchronize()

    def check(self, what, written=True):
        """The inner items after the guards were found untouched and (with
        ``written``) no inner item still holds the sentinel."""
        got = self.raw.cpu().numpy()
        lo = self.G + self.shift
        below, inner, above = got[:lo], got[lo:lo + self.n], \
            got[lo + self.n:]
        for name, band in (('below', below), ('above', above)):
            hit = np.flatnonzero(band != SENTINEL)
            assert hit.size == 0, (
                '%s: %d items written %s the output, first at band offset '
                '%d' % (what, hit.size, name, hit[0]))
        left = np.flatnonzero(inner == SENTINEL)
        if written:
            assert left.size == 0, (
                '%s: %d of %d items never written, first %s'
                % (what, left.size, self.n, left[:8]))
        else:
            assert left.size == self.n, (what, 'written', self.n - left.size)
        return inner.copy()


def _device_inputs(free, lam):
    import torch
    return torch.from_numpy(free).cuda(), torch.from_numpy(lam).cuda()


def _guarded_eval(col, handle, free, lam, what, shift=0):
    """``handle``'s values for device pointers into a guarded buffer."""
    from opty_amd import hip_backend as hb
    PH = col._build_hessian_program().PH
    dfree, dlam = _device_inputs(free, lam)
    buf = Guarded(handle.nnz, PH, shift)
    col.sync_known()
    handle.evaluate(dfree, dlam, buf.doubles, hb.DEVICE)
    col.hip.synchronize()
    return buf.check(what).view(np.float64)


def _compare(col, free, lam, got, what):
    """All of ``got`` against the CPU interpreter of the Hessian DAG."""
    prog = col._build_hessian_program()
    ncn, PH = col.num_collocation_nodes - 1, prog.PH
    block, inst, bnd = hc.interpreted(col, free, lam)
    assert len(got) == ncn*PH + len(inst)
    assert_close(got[:ncn*PH], block.ravel(), rtol=1e-12, bound=bnd.ravel(),
                 what=what)
    np.testing.assert_allclose(got[ncn*PH:], inst, rtol=1e-12, atol=1e-300)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize('label,ncn', hc.BLOCK_EDGE_CASES)
def test_block_edges(label, ncn):
    """One node, partial, full and nearly empty last blocks: right values at
    every node, nothing outside the ``nnz`` doubles, every one of them
    written, the same bits from host and device memory and from call to
    call."""
    col = hc.collocator(label, ncn)
    what = '%s N-1=%d' % (label, ncn)
    hess = col.generate_hessian_function()
    prog = col._build_hessian_program()
    assert hess.handle.nnz == ncn*prog.PH + len(prog.inst_hess_out)
    if label == 'C':
        assert prog.inst_hess_out
    free, lam = hc.inputs(11, col)
    dev = _guarded_eval(col, hess.handle, free, lam, what)
    _compare(col, free, lam, dev, what)
    host = hess(free, lam).copy()
    assert np.array_equal(_bits(host), _bits(dev)), what
    again = _guarded_eval(col, hess.handle, free, lam, what + ' again')
    assert np.array_equal(_bits(again), _bits(dev)), what


@pytest.mark.parametrize('label,ncn', [c for c in hc.BLOCK_EDGE_CASES
                                       if c[0] in 'CE'])
def test_device_indices_inside_guard_bands(label, ncn):
    from opty_amd import hip_backend as hb
    col = hc.collocator(label, ncn)
    handle = col.generate_hessian_function().handle
    PH = col._build_hessian_program().PH
    rows, cols = Guarded(handle.nnz, PH), Guarded(handle.nnz, PH)
    handle.indices(rows.ints, cols.ints, hb.DEVICE)
    col.hip.synchronize()
    what = '%s N-1=%d' % (label, ncn)
    r0, c0 = col.hessian_indices_closed_form()
    assert np.array_equal(rows.check(what + ' rows'), r0)
    assert np.array_equal(cols.check(what + ' cols'), c0)
    hr, hcols = col.hessian_indices()
    assert np.array_equal(hr, r0) and np.array_equal(hcols, c0)


@pytest.mark.parametrize(
    'label,variant', hc.FORCED_VARIANTS,
    ids=['%s-%d-%s-%d' % ((k,) + v) for k, v in hc.FORCED_VARIANTS])
def test_forced_emission_variants(label, variant):
    """Many strips, chunks that recompute what they share, and the
    uniform-sincos twin: built as ``_ensure_hessian`` builds a handle, held
    to the interpreter (not to ``_verify_hessian``, which is under test)."""
    from opty_amd import hip_backend as hb
    col = hc.collocator(label, 65)
    hsaco, cut, source = hc.forced_module(col, variant)
    default_source = hc.forced_module(col, hc.DEFAULT_VARIANT)[2]
    assert source != default_source
    budget, forget, fast_trig = variant
    if budget < 1500:
        assert len(cut) > len(hc.forced_module(col, hc.DEFAULT_VARIANT)[1])
    handle = hb.HipHessian(col.hip, hc.descriptor(col, cut), hsaco)
    try:
        what = '%s %s' % (label, list(variant))
        free, lam = hc.inputs(12, col)
        got = _guarded_eval(col, handle, free, lam, what)
        _compare(col, free, lam, got, what)
        again = _guarded_eval(col, handle, free, lam, what + ' again')
        assert np.array_equal(_bits(again), _bits(got))
    finally:
        handle.release()


def test_misaligned_device_output_is_refused_for_wide_stores():
    """An even PH is flushed with 16-byte stores: a device pointer at 8 mod
    16 is refused before anything is enqueued.  An odd PH takes 8-byte stores
    and the same offset gives the aligned call's bits."""
    from opty_amd import hip_backend as hb
    col = hc.collocator('B', 65)
    handle = col.generate_hessian_function().handle
    PH = col._build_hessian_program().PH
    assert PH % 2 == 0
    free, lam = hc.inputs(13, col)
    dfree, dlam = _device_inputs(free, lam)
    buf = Guarded(handle.nnz, PH, shift=1)
    assert buf.doubles.data_ptr() % 16 == 8
    col.sync_known()
    with pytest.raises(hb.HipBackendError, match='aligned'):
        handle.evaluate(dfree, dlam, buf.doubles, hb.DEVICE)
    col.hip.synchronize()
    buf.check('refused call', written=False)
    # ... and the handle is as good as before
    _compare(col, free, lam,
             _guarded_eval(col, handle, free, lam, 'B aligned'), 'B aligned')
    odd = hc.collocator('E', 65)
    handle = odd.generate_hessian_function().handle
    assert odd._build_hessian_program().PH % 2 == 1
    free, lam = hc.inputs(13, odd)
    aligned = _guarded_eval(odd, handle, free, lam, 'E aligned')
    shifted = _guarded_eval(odd, handle, free, lam, 'E shifted', shift=1)
    assert np.array_equal(_bits(aligned), _bits(shifted))
    _compare(odd, free, lam, shifted, 'E shifted')


def _with_known_trajectory(kw, scale):
    traj = {f: scale*np.asarray(v) for f, v in
            kw['known_trajectory_map'].items()}
    return dict(kw, known_trajectory_map=traj)


@pytest.mark.parametrize('name', ['msd_be_small', 'C'])
def test_known_trajectory_change_is_seen(name):
    """Change the known trajectory between two calls: the second call equals
    a fresh collocator's (the Hessian borrows the problem handle's tables).
    In ``msd_be_small`` the trajectory enters linearly and the values stay;
    in problem C (``-k(t)/(1 + y**2)``) they have to move."""
    import opty_amd
    kw = problems.build(name) if name != 'C' else hc.KERNEL_PROBLEMS['C'](66)
    col = opty_amd.ConstraintCollocator(**kw)
    hess = col.generate_hessian_function()
    free, lam = hc.inputs(14, col)
    first = hess(free, lam).copy()
    kw2 = _with_known_trajectory(kw, -1.75)
    for f, v in kw2['known_trajectory_map'].items():
        col.known_trajectory_map[f] = v
    second = hess(free, lam).copy()
    dev = _guarded_eval(col, hess.handle, free, lam, name + ' new trajectory')
    fresh_col = opty_amd.ConstraintCollocator(**kw2)
    fresh = fresh_col.generate_hessian_function()(free, lam)
    assert np.array_equal(_bits(second), _bits(fresh))
    assert np.array_equal(_bits(dev), _bits(fresh))
    _compare(fresh_col, free, lam, second, name + ' new trajectory')
    if name == 'C':
        assert not np.array_equal(first, second)
    else:
        assert np.array_equal(first, second)


#: ``free`` is drawn from [-1, 1] and multiplied by this before the
#: finite-difference check (the duration stays): 1.0 where the differences
#: at eps and 2 eps agree within a quarter of the tolerance as drawn (both
#: bipeds: 0.007 of it at the worst).  The one-legged model's muscle terms
#: GROW as its states shrink, so scaling down makes the two differences
#: part: 0.28 of the tolerance at 1.0, 0.44 at 0.8, 0.94 at 0.55, 7.2 at
#: 0.2, 116 at 0.05 (and single nodes cross a pole at 0.97, 0.75, 0.7, 0.5).
#: It is scaled UP instead: 0.23 at 1.1, 0.18 at 1.25, 0.125 at 1.5.
FD_FREE_SCALE = {'biped_small': 1.0, 'biped_mid_small': 1.0,
                 'one_legged_small': 1.5}


@pytest.mark.parametrize('name', hc.FD_PROBLEMS)
def test_hessian_times_vector_is_the_difference_of_the_gpu_vjp(name):
    """The three largest Hessian DAGs against something that is not their
    own interpreter: ``H v`` from the summed triplets equals the central
    difference of ``J(free)^T lagrange`` (the GPU ``vjp``) along ``v``."""
    import opty_amd
    import scipy.sparse as sp
    col = opty_amd.ConstraintCollocator(**problems.build(name))
    hess = col.generate_hessian_function()
    rows, cols = col.hessian_indices()
    vjp = col.generate_vjp_function()
    free, lam = hc.inputs(15, col)
    tail = free[-1]
    free = free*FD_FREE_SCALE[name]
    if col._variable_duration:
        free[-1] = tail
    n = col.num_free
    L = sp.coo_matrix((np.array(hess(free, lam)), (rows, cols)),
                      shape=(n, n)).tocsr()
    H = L + sp.tril(L, -1).T
    rng = np.random.default_rng(16)
    eps = 1e-6
    worst, worst_pair = 0.0, 0.0
    for _ in range(3):
        v = draw(rng, n)
        fd, fd2 = [(np.array(vjp(free + e*v, lam)) -
                    np.array(vjp(free - e*v, lam)))/(2*e)
                   for e in (eps, 2*eps)]
        atol = 1e-6*max(1.0, np.abs(fd).max())
        tol = atol + 1e-6*np.abs(fd)
        pair = np.max(np.abs(fd - fd2)/tol)
        worst_pair = max(worst_pair, pair)
        assert pair <= 0.25, (
            '%s: the differences at eps and 2 eps disagree (%.3g of the '
            'tolerance): the input, not the kernel' % (name, pair))
        hv = H @ v
        worst = max(worst, np.max(np.abs(hv - fd)/tol))
        np.testing.assert_allclose(hv, fd, rtol=1e-6, atol=atol)
    print('%s: worst |H v - fd| / tolerance %.3g; eps against 2 eps %.3g'
          % (name, worst, worst_pair))


def test_c_abi_errors():
    """``opty_hip_hessian_*`` / ``opty_hip_eval_hess``: every misuse returns
    non-zero with its message, nothing is launched, and the good handle
    still evaluates correctly afterwards."""
    import opty_amd
    from opty_amd import hip_backend as hb
    col = opty_amd.ConstraintCollocator(**problems.build('msd_be_small'))
    hess = col.generate_hessian_function()
    handle = hess.handle
    lib = hb.load_library()
    free, lam = hc.inputs(17, col)
    out = np.empty(handle.nnz)
    P = hb._ptr

    def refused(rc, word):
        msg = lib.opty_hip_last_error().decode()
        assert rc != 0 and word in msg, (rc, word, msg)

    refused(lib.opty_hip_eval_hess(None, P(free), P(lam), P(out), hb.HOST),
            'null')
    refused(lib.opty_hip_hessian_indices(None, P(out), P(out), hb.HOST),
            'null')
    for args in ((None, lam, out), (free, None, out), (free, lam, None)):
        with pytest.raises(hb.HipBackendError, match='null'):
            handle.evaluate(*args, hb.HOST)
    for kind in (7, -1):
        with pytest.raises(hb.HipBackendError, match='memory kind'):
            handle.evaluate(free, lam, out, kind)
        with pytest.raises(hb.HipBackendError, match='memory kind'):
            handle.indices(np.empty(handle.nnz, np.int64),
                           np.empty(handle.nnz, np.int64), kind)
    hsaco = col._hessian_meta['hsaco']
    good = hc.descriptor(col, [None]*col._hessian_meta['strips'])
    assert good['nnz_inst'] == 0 and good['PH'] > 0
    with pytest.raises(hb.HipBackendError, match='descriptor'):
        hb.HipHessian(col.hip, dict(good, strips=0), hsaco)
    with pytest.raises(hb.HipBackendError, match='descriptor'):
        hb.HipHessian(col.hip, dict(good, PH=-1), hsaco)
    # PH > 0 and a null pattern (the Python class always passes an array)
    desc = hb._HessDesc(PH=good['PH'], nnz_inst=0, strips=good['strips'],
                        pattern=None, inst_rows=None, inst_cols=None)
    made = ctypes.c_void_p()
    refused(lib.opty_hip_hessian_create(col.hip._h, ctypes.byref(desc),
                                        hsaco.encode(), ctypes.byref(made)),
            'null index pattern')
    assert not made.value
    one = np.zeros(1, dtype=np.int64)
    with pytest.raises(hb.HipBackendError, match='no instance'):
        hb.HipHessian(col.hip, dict(good, nnz_inst=1, inst_rows=one,
                                    inst_cols=one), hsaco)
    with pytest.raises(hb.HipBackendError, match='hipModuleLoad'):
        hb.HipHessian(col.hip, good, '/nonexistent/module.hsaco')
    # a code object without the Hessian kernels: the Jacobian module
    with pytest.raises(hb.HipBackendError, match='missing'):
        hb.HipHessian(col.hip, good,
                      hb.compile_module(col.generate_source()[0]))
    assert lib.opty_hip_hessian_destroy(None) == 0
    assert lib.opty_hip_hessian_nnz(None) == -1
    # the good handle still works: host and guarded device memory
    got = hess(free, lam).copy()
    _compare(col, free, lam, got, 'msd_be_small after the refusals')
    dev = _guarded_eval(col, handle, free, lam, 'msd_be_small device')
    assert np.array_equal(_bits(dev), _bits(got))
