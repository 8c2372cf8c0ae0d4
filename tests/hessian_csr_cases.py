"""What the CSR-Hessian test files share: the INDEPENDENT answer --
``scipy.sparse`` and ``np.add.at`` on the triplets and the project's existing
index functions, nothing of the kernel or of its host statement --, the
tolerance, the descriptors of the cases and the code objects that
``__graft_entry__.build`` prebuilds for them."""
import numpy as np

import hessian_cases as hc
import hessmv_cases as mc

from examples import problems

#: N - 1 of the CPU comparison
CPU_EDGES = (1, 2, 63, 64, 65, 127)
#: N - 1 of the variable-duration pendulum on the GPU: its three tail x tail
#: groups of N - 1 triplets each end inside, on and behind a block edge
VARDUR_EDGES = (59, 64, 65, 127, 129)
ZOO = ('vardur_pendulum_small', 'pend2_link_vardur_unkmass_small',
       'config3_10link_small')


class Reference(object):
    """The triplets ``(rows, cols, values)`` over ``num_free`` rows, of which
    the first ``tail`` are trajectory rows (``ncn`` constraint nodes),
    compressed without the project's
    code: SciPy's canonical CSR, the group of every triplet (``np.unique`` on
    ``row*num_free + col``: the order of a canonical CSR), ``np.add.at``'s sum
    and the bound ``(k - 1) 2**-53 sum|a|`` of a group of ``k`` addends, which
    holds for any order of summation."""

    def __init__(self, num_free, tail, ncn, rows, cols, values):
        import scipy.sparse as sp
        rows, cols = np.asarray(rows), np.asarray(cols)
        values = np.asarray(values, dtype=float)
        self.num_free = num_free
        self.csr = sp.coo_matrix((values, (rows, cols)),
                                 shape=(num_free, num_free)).tocsr()
        self.csr.sum_duplicates()
        self.csr.sort_indices()
        key, self.group = np.unique(rows*num_free + cols,
                                    return_inverse=True)
        self.group = self.group.ravel()
        self.count = np.bincount(self.group, minlength=len(key))
        self.added = np.zeros(len(key))
        np.add.at(self.added, self.group, values)
        self.tol = (self.count - 1)*2.0**-53*np.bincount(
            self.group, weights=np.abs(values), minlength=len(key))
        #: the long groups: tail x tail pairs with a triplet per constraint
        #: node (up to two addends have one sum whatever the order)
        self.long = (key // num_free >= tail) & (key % num_free >= tail) & \
            (self.count >= max(ncn, 3))
        # (SciPy keeps a pair whose triplets sum to zero)
        assert self.csr.nnz == len(key)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_structure(what, ref, indptr, indices):
    import scipy.sparse as sp
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    assert indptr.dtype == np.int64 and indices.dtype == np.int64, what
    assert indptr.shape == (ref.num_free + 1,), what
    assert len(indices) == len(ref.count) == indptr[-1], what
    rows = np.repeat(np.arange(ref.num_free), np.diff(indptr))
    key = rows*ref.num_free + indices
    assert np.all(np.diff(key) > 0), what          # ascending, every pair once
    assert np.all(indices <= rows) and np.all(indices >= 0), what
    assert np.array_equal(indptr, ref.csr.indptr), what
    assert np.array_equal(indices, ref.csr.indices), what
    m = sp.csr_matrix((np.ones(len(indices)), indices, indptr),
                      shape=(ref.num_free, ref.num_free))
    assert m.has_canonical_format, what


def check_values(what, ref, data):
    """``data`` within the tolerance of SciPy's sums, groups of one exact,
    short groups the bits of ``np.add.at``; no entry is excused.  Returns the
    worst error over its tolerance."""
    data = np.asarray(data)
    assert data.shape == ref.added.shape, what
    err = np.abs(data - ref.csr.data)
    live = ref.tol > 0
    worst = float((err[live]/ref.tol[live]).max(initial=0.0))
    print('%s: %d pairs, %d long groups, max error %.3g, max error/tolerance '
          '%.3g' % (what, len(data), int(ref.long.sum()),
                    err.max(initial=0.0), worst))
    assert np.all(np.isfinite(data)), what
    assert np.all(err <= ref.tol), (what, float(err.max()), worst)
    short = ~ref.long
    assert np.array_equal(bits(data[short]), bits(ref.added[short])), what
    return worst


def node_descriptor(label, ncn):
    """``(N, n + q, r + s, descriptor, rows, cols)`` of the constraint Hessian
    of a kernel problem or of a named problem of the zoo (``ncn`` None)."""
    N, nrows, ntail, pattern, rows, cols = mc.node_tables(label, ncn)
    at = (N - 1)*len(pattern)
    return N, nrows, ntail, dict(pattern=pattern, inst_rows=rows[at:],
                                 inst_cols=cols[at:]), rows, cols


def objective_descriptor(name, N):
    """The same of an objective case alone (PH = 0)."""
    nrows, r, pattern, pairs, base = mc.objective_program(name)
    rows, cols = mc.objective_tables(name, N)
    tail = nrows*N
    return N, nrows, r, dict(pattern=(), obj_pattern=pattern, obj_base=base,
                             tail_rows=tail + pairs[:, 0],
                             tail_cols=tail + pairs[:, 1]), rows, cols


def both_sections():
    """Constraint triplets of problem C (instance entry, unknown parameter)
    and an objective section over the same free vector, as ``Problem.
    hessian`` lays them out (the case of tests/test_hessmv_cpu.py)."""
    from opty_amd.objective import objective_hessian_indices
    N, nrows, ntail, pattern, crows, ccols = mc.node_tables('C', 65)
    at = (N - 1)*len(pattern)
    last = nrows - 1
    obj = np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1),
                    (last, 1, 0, 0), (-1, 0, 0, 1), (-1, 0, -1, 0)],
                   dtype=np.int32)
    pairs = np.array([(0, 0)], dtype=np.int64)
    orows, ocols = objective_hessian_indices(obj, pairs, nrows, 0, N,
                                             'midpoint')
    tail = nrows*N
    return N, nrows, ntail, dict(
        pattern=pattern, inst_rows=crows[at:], inst_cols=ccols[at:],
        obj_pattern=obj, obj_base=0, tail_rows=tail + pairs[:, 0],
        tail_cols=tail + pairs[:, 1]), np.r_[crows, orows], \
        np.r_[ccols, ocols]


def vardur_collocator(ncn):
    import opty_amd
    return opty_amd.ConstraintCollocator(
        **problems.variable_duration_pendulum(num_nodes=ncn + 1))


def prebuild_jobs():
    """Thunks that build the code objects of tests/test_hessian_csr_gpu.py
    which no other list builds (``__graft_entry__.build`` runs them side by
    side): the variable-duration sizes and the modules of the example."""
    def vardur(ncn):
        col = vardur_collocator(ncn)
        col.prebuild()
        col._build_hessian_code_object()

    def example():
        from examples import kkt_direct
        kkt_direct.prebuild(20)
    return [lambda m=m: vardur(m) for m in VARDUR_EDGES] + [example]
