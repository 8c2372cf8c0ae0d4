"""GPU tests of the CSR Hessian and the Hessian operator on SYNTHETIC patterns
(``hessian_synth_cases``; tests/test_hessian_synth_cpu.py holds the same
descriptors to the host statement): the paths of ``opty_hesscsr`` /
``opty_hesscsr_fin``, of the table builders of ``csrc/hesscsr.cpp`` and
``csrc/hessmv.cpp`` and of ``csrc/kktcsr.cpp`` that no problem of the zoo
reaches -- second and third column chunks, windows above 64 entries, dynamic
LDS above 64 KiB and its refusal, unsorted patterns, interior trajectory rows
and tail-row elements owned by items, long source lists, every diagonal, the
operator above 64 KiB of LDS and with ``block_width`` 1 -- through the checks
of tests/test_hessian_csr_gpu.py (``_hold``), tests/test_hessmv_gpu.py and
tests/test_hessmv_block_gpu.py, and one real problem with nonlinear instance
constraints at interior nodes."""
import functools
import re

import numpy as np
import pytest

import hessian_cases as hc
import hessian_csr_cases as cc
import hessian_synth_cases as sc
import hessmv_cases as mc
import kkt_csr_cases as kc
import test_hessian_csr_gpu as csr
import test_hessmv_block_gpu as blk
import test_hessmv_gpu as single

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _with_diagonal():
    from opty_amd import hip_backend as hb

    class HipHessianCsrWithDiagonal(hb.HipHessianCsr):
        _create = 'opty_hip_hesscsr_create_with_diagonal'
    return HipHessianCsrWithDiagonal


def _values(seed, count):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, count)


def _plain(name, ncn, seed=85):
    """One case through every check of ``_hold``."""
    from opty_amd import hip_backend as hb
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    col = sc.carrier(cname, N)
    handle = hb.HipHessianCsr(col.hip, desc)
    try:
        return csr._hold('%s N-1=%d' % (name, ncn), col.hip, handle, N, nrows,
                         ntail, desc, rows, cols, _values(seed, len(rows)))
    finally:
        handle.release()


def _every_diagonal(col, what, N, nrows, ntail, desc, rows, cols, values):
    """The handle with every diagonal through ``_hold`` against the triplets
    plus one zero triplet per diagonal; a diagonal that no triplet hits is
    ``+0.0`` by bits.  Returns ``(data, reference, untouched diagonals)``."""
    num_free = nrows*N + ntail
    r2, c2, v2 = sc.with_every_diagonal(rows, cols, values, num_free)
    ref = cc.Reference(num_free, nrows*N, N - 1, r2, c2, v2)
    handle = _with_diagonal()(col.hip, desc)
    try:
        data, _ = csr._hold(what, col.hip, handle, N, nrows, ntail,
                            dict(desc, with_diagonal=True), rows, cols,
                            values, ref=ref)
    finally:
        handle.release()
    untouched = ref.count == 1
    untouched[ref.group[:len(rows)]] = False
    assert np.all(cc.bits(data[untouched]) == 0), what
    # the diagonal is the last entry of every row
    indptr = ref.csr.indptr
    assert np.array_equal(ref.csr.indices[indptr[1:] - 1],
                          np.arange(num_free)), what
    return data, ref, int(untouched.sum())


# -- 1. column chunks ---------------------------------------------------------
@pytest.mark.parametrize('name,ncn', sc.params(sc.CHUNK_CASES))
def test_second_and_third_column_chunk(name, ncn):
    _plain(name, ncn)


# -- 2. windows ---------------------------------------------------------------
@pytest.mark.parametrize('name,ncn', sc.params(sc.WINDOW_CASES))
def test_wide_and_overlapping_windows(name, ncn):
    """An unsorted pattern (every window spans most of a node, several tile
    groups, more than 64 KiB of LDS) and a class whose own window is wider
    than 64 entries (no whole node per 64 elements of the load loop)."""
    _plain(name, ncn)


# -- 3. the LDS limit ---------------------------------------------------------
_REFUSAL = re.compile(r'span (\d+) consecutive entries needs (\d+) bytes of '
                      r'LDS per block, the limit is (\d+) bytes '
                      r'\((\d+) entries\)')


def test_lds_limit_refusal_and_the_widest_window_it_admits():
    import torch
    from opty_amd import hip_backend as hb
    cname, ncn = sc.LDS_CARRIER, sc.LDS_EDGE
    nrows, ntail = sc.CARRIERS[cname]
    N = ncn + 1
    col = sc.carrier(cname, N)

    def held(handle, width, what, seed):
        desc = sc.window_descriptor(width)
        rows, cols = sc.triplets(desc, nrows, ntail, N)
        return csr._hold(what, col.hip, handle, N, nrows, ntail, desc, rows,
                         cols, _values(seed, len(rows)))

    def refused(width):
        with pytest.raises(hb.HipBackendError) as err:
            hb.HipHessianCsr(col.hip, sc.window_descriptor(width))
        found = _REFUSAL.search(str(err.value))
        assert found, str(err.value)
        got, need, limit, cap = (int(x) for x in found.groups())
        assert (got, need) == (width, sc.lds_bytes(width))
        assert need > limit
        return limit, cap

    good = hb.HipHessianCsr(col.hip, sc.window_descriptor(65))
    first = held(good, 65, 'window 65', 86)[0]
    limit, cap = refused(sc.LDS_REFUSED)
    print('LDS limit %d bytes per block, widest window %d entries (%d bytes)'
          % (limit, cap, sc.lds_bytes(cap)))
    assert limit == torch.cuda.get_device_properties(0).shared_memory_per_block
    # by the formula of create_impl a window of cap entries fits, cap + 2 not
    assert sc.lds_bytes(cap) <= limit < sc.lds_bytes(cap + 2)
    widest = hb.HipHessianCsr(col.hip, sc.window_descriptor(cap))
    if cap >= 95:
        assert sc.lds_bytes(cap) > 65536    # the launch asks for the attribute
    held(widest, cap, 'window %d (the cap)' % cap, 87)
    assert refused(cap + 2) == (limit, cap)
    # after the refusals both handles are as good as before
    held(widest, cap, 'window %d after the refusals' % cap, 87)
    again = held(good, 65, 'window 65 after the refusals', 86)[0]
    assert np.array_equal(cc.bits(again), cc.bits(first))
    widest.release()
    good.release()


# -- 4. explicit triplets -----------------------------------------------------
@pytest.mark.parametrize('name,ncn', sc.params(sc.EXPLICIT_CASES))
def test_explicit_triplets_in_interior_and_tail_rows(name, ncn):
    """Instance triplets on and off the pattern in interior rows of blocks 0
    and 1 and at node 63, in a first and a last row, on elements of segments,
    between two segments, on a long group and on a tail pair that is none;
    both sections and parameter-parameter entries."""
    data, ref = _plain(name, ncn)
    assert ref.long.any()
    assert len(ref.count) < len(ref.group)


# -- 5. every diagonal --------------------------------------------------------
@pytest.mark.parametrize('name,ncn', sc.params(sc.DIAGONAL_CASES))
def test_every_diagonal(name, ncn):
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    col = sc.carrier(cname, N)
    untouched = _every_diagonal(col, '%s N-1=%d, every diagonal' % (name, ncn),
                                N, nrows, ntail, desc, rows, cols,
                                _values(88, len(rows)))[2]
    if 'diagonal' in sc.CASES[name][3]:
        assert untouched >= 2


def test_augmented_system_over_a_synthetic_descriptor():
    """``HipKktCsr`` over the explicit descriptor on the carrier in the CSR
    layout: the W block is the data of the handle with every diagonal with
    ``(x + sigma) + delta_w`` on the diagonals, everything by
    ``kkt_csr_cases.Reference`` over the synthetic Hessian indices."""
    import test_kkt_csr_gpu as kkt
    from opty_amd import hip_backend as hb
    name, ncn = sc.KKT_CASE, sc.KKT_EDGE
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    what = 'augmented system over %s N-1=%d' % (name, ncn)
    col = sc.carrier(cname, N, 'csr')
    n = col.num_free
    assert n == nrows*N + ntail
    hvals = _values(89, len(rows))
    hdata, dref, _ = _every_diagonal(col, what, N, nrows, ntail, desc, rows,
                                     cols, hvals)
    hptr, hidx = dref.csr.indptr, dref.csr.indices
    handle = hb.HipKktCsr(col.hip, desc)
    ref = kc.Reference(col, rows, cols)
    assert handle.nnz == len(rows)
    assert handle.nnz_hessian == len(hidx)
    indptr = np.empty(n + col.num_constraints + 1, dtype=np.int64)
    indices = np.empty(handle.nnz_kkt, dtype=np.int64)
    handle.structure(indptr, indices, hb.HOST)
    ref.check_structure(what, indptr, indices)
    jrows, jcols = col.jacobian_indices()
    rng = np.random.default_rng(90)
    jvals = rng.uniform(-1.0, 1.0, col.hip.nnz)
    assert len(jvals) == len(jrows)
    sigma = rng.uniform(0.0, 1.0, n)
    for sig, dw, dc in ((sigma, 1e-4, 1e-8), (None, 0.0, 0.0)):
        expect = ref.expected(hptr, hidx, hdata, jrows, jcols, jvals, sig, dw,
                              dc)
        dev = kkt._device_assemble(col.hip, handle, hvals, jvals, sig, dw, dc,
                                   what)
        assert np.array_equal(kc.bits(dev), kc.bits(expect)), what
        host = np.full(handle.nnz_kkt, np.nan)
        handle.assemble(hvals, jvals, sig, dw, dc, host, hb.HOST)
        assert np.array_equal(kc.bits(host), kc.bits(dev)), what
        # the W block: the rows of the free vector, columns of W alone
        assert indptr[n] == len(hidx)
        want = hdata.copy()
        diag = hptr[1:] - 1
        want[diag] = (want[diag] + (0.0 if sig is None else sig)) + dw
        assert np.array_equal(kc.bits(dev[:indptr[n]]), kc.bits(want)), what
    handle.release()


# -- 6. H v on the same descriptors -------------------------------------------
def _product(col, handle, what, nfree, rows, cols, seed, widths):
    """``apply`` from device and host memory and twice, ``apply_block`` over
    ``widths`` columns against the single products."""
    from opty_amd import hip_backend as hb
    assert handle.nnz == len(rows) and col.num_free == nfree
    values, V = blk._draw(seed, len(rows), nfree, max(widths))
    v = np.ascontiguousarray(V[:, 0])
    dev = single._device_product(col, handle, values, v, what)
    mc.check(what, dev, nfree, rows, cols, values, v)
    host = np.full(nfree, np.nan)
    handle.apply(values, v, host, hb.HOST)
    assert np.array_equal(cc.bits(host), cc.bits(dev)), what
    again = single._device_product(col, handle, values, v, what + ' again')
    assert np.array_equal(cc.bits(again), cc.bits(dev)), what
    ones = blk._singles(handle, values, V)
    assert np.array_equal(cc.bits(ones[0]), cc.bits(dev)), what
    for k in widths:
        Y = blk._block(handle, values, V[:, :k], hb.DEVICE)
        blk._held(what, Y, ones, nfree, rows, cols, values, V)


@pytest.mark.parametrize('name,ncn', sc.params(sc.PRODUCT_CASES))
def test_operator_on_the_same_descriptors(name, ncn):
    from opty_amd import hip_backend as hb
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    col = sc.carrier(cname, N)
    handle = hb.HipHessianProduct(col.hip, desc)
    blk._width(handle)
    _product(col, handle, '%s N-1=%d' % (name, ncn), nrows*N + ntail, rows,
             cols, 91, (1, 3, 4))
    handle.release()


def test_operator_over_102_sides_above_64_kib_with_block_width_1():
    from opty_amd import hip_backend as hb
    cname, ncn = sc.SIDES_CARRIER, sc.SIDES_EDGE
    nrows, ntail = sc.CARRIERS[cname]
    N = ncn + 1
    desc = sc.all_sides_descriptor(nrows)
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    col = sc.carrier(cname, N)
    handle = hb.HipHessianProduct(col.hip, desc)
    sides, ntraj = handle.sides()
    assert len(sides) == ntraj == 102
    lds = 16896 + 1024*len(sides)
    print('opty_hessmv: %d sides, %d bytes of LDS, limit %d'
          % (len(sides), lds, blk._lds_limit()))
    assert 65536 < lds <= blk._lds_limit()
    assert blk._width(handle) == 1 == handle.block_width
    _product(col, handle, 'all 102 sides', nrows*N, rows, cols, 92, (1, 3, 4))
    handle.release()


def test_operator_refuses_more_sides_than_the_lds_of_a_block_holds():
    """144 sides: refused before any launch with the limit as the device
    reports it; a pattern over fewer sides of the same problem then works."""
    from opty_amd import hip_backend as hb
    cname, ncn = sc.REFUSED_SIDES_CARRIER, sc.REFUSED_SIDES_EDGE
    nrows, ntail = sc.CARRIERS[cname]
    N = ncn + 1
    col = sc.carrier(cname, N)
    with pytest.raises(hb.HipBackendError) as err:
        hb.HipHessianProduct(col.hip, sc.all_sides_descriptor(nrows))
    found = re.search(r'144 sides \(144 trajectory, 0 tail\) need (\d+) bytes '
                      r'of LDS per block, the limit is (\d+) bytes '
                      r'\((\d+) sides\)', str(err.value))
    assert found, str(err.value)
    need, limit, cap = (int(x) for x in found.groups())
    print('opty_hessmv: limit %d bytes per block, %d sides' % (limit, cap))
    assert need == 16896 + 1024*144 > limit == blk._lds_limit()
    assert 16896 + 1024*cap <= limit < 16896 + 1024*(cap + 1)
    desc = sc.all_sides_descriptor(51)
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    handle = hb.HipHessianProduct(col.hip, desc)
    assert len(handle.sides()[0]) == 102
    _product(col, handle, '102 of 144 sides after the refusal', nrows*N, rows,
             cols, 93, (1, 2))
    handle.release()


# -- 7. a real problem --------------------------------------------------------
def test_problem_with_interior_nonlinear_instance_constraints():
    import test_hessian_kernel_gpu as kernel
    import test_kkt_csr_gpu as kkt
    col = sc.interior_collocator()
    prog = col._build_hessian_program()
    N = col.num_collocation_nodes
    got = sc.reaches(col._hessmv_descriptor(), prog.n + prog.q, N,
                     prog.r + prog.s)
    nodes = [(p, x) for rows in got['interior_item_rows'].values()
             for p, x in rows]
    assert len(set((p - 1)//sc.STRIDE for p, _ in nodes)) == 2, got
    assert any(x > 0 for _, x in nodes) and any(x == 0 for _, x in nodes)
    assert got['L'] > 0
    what = 'interior instance constraints'
    free, lam = hc.inputs(71, col)
    values = col.generate_hessian_function()(free, lam).copy()
    kernel._compare(col, free, lam, values, what)
    hcsr, free2, lam2, values2 = csr._constraint_case(col, what, seed=71)[:4]
    assert np.array_equal(cc.bits(values2), cc.bits(values))
    kkt._case('interior', N - 1, False, col=col)
