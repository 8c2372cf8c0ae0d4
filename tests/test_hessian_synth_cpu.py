"""CPU tests of the synthetic Hessian patterns (``hessian_synth_cases``): every
case of tests/test_hessian_synth_gpu.py through the host statement
(``hessian_csr_structure`` / ``assemble_hessian_csr``, ``assemble_hessmv``),
plain and with every diagonal, against ``scipy.sparse`` and ``np.add.at`` on
the independently expanded triplets -- so the inputs of the GPU file are valid
and its reference holds --, and what each case reaches: a case that does not
reach the path it is there for fails here.  No GPU is needed."""
import numpy as np
import pytest

import hessian_csr_cases as cc
import hessian_synth_cases as sc
import hessmv_cases as mc

from opty_amd.codegen.program import (assemble_hessian_csr, assemble_hessmv,
                                      hessian_csr_structure)

ALL = sc.params(sc.CASES)


def _hold(what, N, nrows, ntail, desc, rows, cols, seed):
    """Structure, slots and values of one descriptor, plain and with every
    diagonal."""
    num_free = nrows*N + ntail
    values = np.random.default_rng(seed).uniform(-1.0, 1.0, len(rows))
    ref = cc.Reference(num_free, nrows*N, N - 1, rows, cols, values)
    indptr, indices, slot = hessian_csr_structure(N, nrows, ntail, **desc)
    cc.check_structure(what, ref, indptr, indices)
    assert np.array_equal(slot, ref.group), what
    data = assemble_hessian_csr(N, nrows, ntail, values, **desc)
    cc.check_values(what, ref, data)
    # the reference of the diagonal variant: one zero triplet per diagonal
    r2, c2, v2 = sc.with_every_diagonal(rows, cols, values, num_free)
    dref = cc.Reference(num_free, nrows*N, N - 1, r2, c2, v2)
    indptr, indices, slot = hessian_csr_structure(
        N, nrows, ntail, with_diagonal=True, **desc)
    what += ', every diagonal'
    cc.check_structure(what, dref, indptr, indices)
    assert np.array_equal(indices[indptr[1:] - 1], np.arange(num_free)), what
    assert np.array_equal(slot, dref.group[:len(rows)]), what
    data = assemble_hessian_csr(N, nrows, ntail, values, with_diagonal=True,
                                **desc)
    cc.check_values(what, dref, data)
    untouched = dref.count == 1
    untouched[dref.group[:len(rows)]] = False
    assert np.all(cc.bits(data[untouched]) == 0), what      # +0.0
    return ref, dref, int(untouched.sum())


@pytest.mark.parametrize('name,ncn', ALL)
def test_case_against_scipy_and_what_it_reaches(name, ncn):
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    got = sc.check_reaches(name, ncn)
    print(name, 'carrier', cname, 'N-1', ncn,
          {k: v for k, v in got.items() if k != 'interior_item_rows'})
    ref, dref, untouched = _hold('%s N-1=%d' % (name, ncn), N, nrows, ntail,
                                 desc, rows, cols, 81)
    tags = sc.CASES[name][3]
    if 'diagonal' in tags:
        assert untouched >= 2
    if 'explicit' in tags:
        assert ref.long.any()
    if 'sources' in tags:
        assert ref.count.max() >= 3


@pytest.mark.parametrize('name,ncn', sc.params(sc.PRODUCT_CASES))
def test_product_statement_on_the_same_descriptors(name, ncn):
    cname, N, nrows, ntail, desc, rows, cols = sc.case(name, ncn)
    rng = np.random.default_rng(82)
    values = rng.uniform(-1.0, 1.0, len(rows))
    v = rng.uniform(-1.0, 1.0, nrows*N + ntail)
    y = assemble_hessmv(N, nrows, ntail, values, v, **desc)
    mc.check('%s N-1=%d' % (name, ncn), y, nrows*N + ntail, rows, cols,
             values, v)


def test_patterns_do_not_depend_on_the_node_count():
    for name in sc.CASES:
        edges = sc.CASES[name][1]
        first = sc.case(name, edges[0])[4]
        for m in edges[1:]:
            desc = sc.case(name, m)[4]
            for key in ('pattern', 'obj_pattern'):
                assert np.array_equal(desc[key], first[key]), (name, key)


@pytest.mark.parametrize('width', [2, 65, 95, 285, 287, sc.LDS_REFUSED])
def test_window_descriptor_spans_exactly_its_width(width):
    """The descriptors of the LDS limit: one class, its window ``width``
    entries, nothing else in a window; valid at the N - 1 of the GPU file."""
    nrows, ntail = sc.CARRIERS[sc.LDS_CARRIER]
    N = sc.LDS_EDGE + 1
    desc = sc.window_descriptor(width)
    got = sc.reaches(desc, nrows, N, ntail)
    assert got['widest_window'] == got['tile_window'] == width
    assert (got['PH'], got['tile_groups'], got['L']) == (width, 1, 2)
    assert got['lds_bytes'] == 8*(64*(width | 1) + 64*33 + 64)
    if width >= 30:
        assert got['longest_source_list'] >= 3 and got['long_groups'] >= 2
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    _hold('window %d' % width, N, nrows, ntail, desc, rows, cols, 83)


def test_all_sides_descriptor_touches_every_side():
    from opty_amd.codegen.program import (hessian_block_width,
                                          hessian_side_table)
    nrows, ntail = sc.CARRIERS[sc.SIDES_CARRIER]
    N = sc.SIDES_EDGE + 1
    desc = sc.all_sides_descriptor(nrows)
    sides, ntraj = hessian_side_table(desc['pattern'])[:2]
    assert ntraj == len(sides) == 2*nrows == 102
    # above 64 KiB for one column, no room for two at 160 KiB
    assert 16896 + 1024*len(sides) > 65536
    assert hessian_block_width(len(sides), 160*1024) == 1
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    rng = np.random.default_rng(84)
    values = rng.uniform(-1.0, 1.0, len(rows))
    v = rng.uniform(-1.0, 1.0, nrows*N)
    y = assemble_hessmv(N, nrows, ntail, values, v, **desc)
    mc.check('all sides', y, nrows*N, rows, cols, values, v)


def test_more_sides_than_lds_holds_is_a_valid_pattern():
    """What the device must refuse for LDS is refused for nothing else."""
    from opty_amd.codegen.program import hessian_side_table
    nrows, ntail = sc.CARRIERS[sc.REFUSED_SIDES_CARRIER]
    N = sc.REFUSED_SIDES_EDGE + 1
    desc = sc.all_sides_descriptor(nrows)
    assert len(hessian_side_table(desc['pattern'])[0]) == 144
    assert 16896 + 1024*144 > 160*1024
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    rng = np.random.default_rng(85)
    values, v = rng.uniform(-1, 1, len(rows)), rng.uniform(-1, 1, nrows*N)
    y = assemble_hessmv(N, nrows, ntail, values, v, **desc)
    mc.check('144 sides', y, nrows*N, rows, cols, values, v)


def test_prebuild_jobs_cover_every_carrier_and_node_count():
    jobs = sc.prebuild_jobs()
    assert len(jobs) == len(sc.CARRIERS) + 1
    assert callable(jobs[0])
