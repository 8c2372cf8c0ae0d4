"""What the test files of the augmented system as CSR share: the cases, the
INDEPENDENT answer -- ``scipy.sparse`` on the Hessian's triplet indices and on
COO indices of the Jacobian enumerated here, NumPy scatters of the values of
the existing functions, nothing of the new kernels or of their host statement
--, the guarded device buffer and the code objects that
``__graft_entry__.build`` prebuilds for the GPU file."""
import numpy as np

import hessian_cases as hc

from examples import problems

#: N - 1 of the CPU comparison
CPU_EDGES = (1, 2, 63, 64, 65)
CPU_LABELS = ('A', 'B', 'C', 'E', 'vardur')
#: doubles of one tile of ``opty_kkt_jrows`` (kTile of csrc/kktcsr.cpp)
JROWS_TILE = 2048
#: (label, N - 1, prune_zeros) of the block-edge cases of the GPU file
GPU_CASES = ([(k, m, False) for k in 'AE' for m in (1, 2, 63, 64, 65, 129)] +
             [(k, m, False) for k in 'BC' for m in (1, 64, 65)] +
             [('A', m, True) for m in (1, 2, 63, 64, 65, 129)] +
             [('B', m, True) for m in (1, 64, 65)])
#: ... and the one whose longest equation span exceeds two full tiles plus a
#: partial one: an equation of A holds 19 + 1 values per node, 211 nodes of
#: them are 2*2048 + 124 doubles (the test checks this)
LONG_SPAN_CASE = ('A', 211, False)

#: a quiet NaN with a payload that no arithmetic produces
SENTINEL = 0x7FF8DEADBEEF1234
GUARD = 256


class Guarded(object):
    """A CUDA buffer of ``n`` doubles between two guard bands, all of it
    filled with ``SENTINEL`` (the class of tests/test_hessian_csr_gpu.py)."""

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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def collocator(label, ncn, prune=False, layout='csr'):
    import opty_amd
    if label == 'vardur':
        kw = problems.variable_duration_pendulum(num_nodes=ncn + 1)
    else:
        kw = hc.KERNEL_PROBLEMS[label](ncn + 1)
    return opty_amd.ConstraintCollocator(
        jacobian_layout=layout, prune_zeros=prune, **kw)


def jacobian_coo(col):
    """``(rows, cols)`` of the stored Jacobian entries of ``col`` as a SET of
    pairs, enumerated from the reference's column convention
    (``opty/direct_collocation.py:2719-2737``): backward Euler differentiates
    with respect to ``[x_{i+1}, x_i, u_{i+1}, tail]``, midpoint with respect
    to ``[x_i, x_{i+1}, u_i, u_{i+1}, tail]``; rows ``j*(N-1) + i``, then the
    instance entries."""
    prog = col._build_program()
    N = col.num_collocation_nodes
    n, q, tailn = prog.n, prog.q, prog.r + prog.s
    i = np.arange(N - 1, dtype=np.int64)[:, None]
    st = np.arange(n, dtype=np.int64)[None, :]*N
    uq = n*N + np.arange(q, dtype=np.int64)[None, :]*N
    tl = np.broadcast_to((n + q)*N + np.arange(tailn, dtype=np.int64),
                         (N - 1, tailn))
    if col.integration_method == 'backward euler':
        c = np.hstack((st + i + 1, st + i, uq + i + 1, tl))
    else:
        c = np.hstack((st + i, st + i + 1, uq + i, uq + i + 1, tl))
    jk = np.array(prog.pattern, dtype=np.int64).reshape(-1, 2)
    rows = (jk[:, 0][None, :]*(N - 1) + i).ravel()
    cols = c[:, jk[:, 1]].ravel()
    return (np.concatenate((rows, col._inst_rows)),
            np.concatenate((cols, col._inst_cols)))


class Reference(object):
    """The pattern of ``K`` from matrices of ones -- nothing cancels, every
    diagonal is there -- and what maps values to it, by SciPy alone."""

    def __init__(self, col, hrows=None, hcols=None):
        """``hrows, hcols``: the Hessian's triplet indices where they are not
        the problem's own (a handle made from a synthetic descriptor)."""
        import scipy.sparse as sp
        self.n, self.m = n, m = col.num_free, col.num_constraints
        if hrows is None:
            hrows, hcols = col.hessian_indices_closed_form()
        self.hrows, self.hcols = hrows, hcols
        Hpat = sp.coo_matrix((np.ones(len(hrows)), (hrows, hcols)),
                             shape=(n, n)).tocsr()
        jrows, jcols = jacobian_coo(col)
        Jpat = sp.coo_matrix((np.ones(len(jrows)), (jrows, jcols)),
                             shape=(m, n)).tocsr()
        assert Jpat.nnz == len(jrows)       # every pair once
        K = sp.tril(sp.bmat([[Hpat + sp.identity(n), None],
                             [Jpat, sp.identity(m)]]), format='csr')
        K.sum_duplicates()
        K.sort_indices()
        self.indptr = K.indptr.astype(np.int64)
        self.indices = K.indices.astype(np.int64)
        #: free rows whose Hessian diagonal is structurally absent
        self.absent = np.flatnonzero(Hpat.diagonal() == 0)
        #: canonical CSR of J: its data are the values of the CSR layout
        Jpat.sort_indices()
        self.J = Jpat

    def check_structure(self, what, indptr, indices):
        import scipy.sparse as sp
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        assert indptr.dtype == np.int64 and indices.dtype == np.int64, what
        assert np.array_equal(indptr, self.indptr), what
        assert np.array_equal(indices, self.indices), what
        size = self.n + self.m
        mat = sp.csr_matrix((np.ones(len(indices)), indices, indptr),
                            shape=(size, size))
        assert mat.has_canonical_format, what
        # every diagonal is stored and is the last entry of its row
        assert np.array_equal(indices[indptr[1:] - 1], np.arange(size)), what

    def positions(self, rows, cols):
        """Position in ``data`` of the pairs ``(rows, cols)`` of ``K``."""
        size = self.n + self.m
        key = np.repeat(np.arange(size), np.diff(self.indptr))*size + \
            self.indices
        at = np.searchsorted(key, rows*size + cols)
        assert np.array_equal(key[at], rows*size + cols)
        return at

    def expected(self, hptr, hidx, hdata, jrows, jcols, jdata, sigma,
                 delta_w, delta_c):
        """``data`` of ``K`` by NumPy: the compressed Hessian ``(hptr, hidx,
        hdata)`` scattered into the ``W`` slots with the diagonal formula,
        the Jacobian's values ``jdata`` at ``(jrows, jcols)`` scattered into
        theirs, ``0.0 - delta_c`` on the constraint diagonals.  Every slot is
        filled exactly once."""
        n, m = self.n, self.m
        filled = np.zeros(len(self.indices), dtype=np.int64)
        data = np.zeros(len(self.indices))      # +0.0: an absent diagonal
        wdiag = self.indptr[1:n + 1] - 1
        cdiag = self.indptr[n + 1:] - 1
        filled[wdiag] += 1
        hrow = np.repeat(np.arange(n), np.diff(hptr))
        at = self.positions(hrow, np.asarray(hidx))
        data[at] = hdata
        filled[at[hrow != hidx]] += 1
        at = self.positions(n + np.asarray(jrows), np.asarray(jcols))
        data[at] = jdata
        filled[at] += 1
        sigma = np.zeros(n) if sigma is None else sigma
        data[wdiag] = (data[wdiag] + sigma) + delta_w
        data[cdiag] = 0.0 - delta_c
        filled[cdiag] += 1
        assert np.all(filled == 1)
        return data


def prebuild_jobs():
    """Thunks that build the code objects of tests/test_kkt_csr_gpu.py
    (``__graft_entry__.build`` runs them side by side): the CSR-layout
    modules of every case (their geometry depends on the launch size), the
    Hessian modules, and the modules of the example."""
    def cases():
        seen = set()
        for label, ncn, prune in GPU_CASES + [LONG_SPAN_CASE]:
            col = collocator(label, ncn, prune)
            col.prebuild()
            if label not in seen:
                seen.add(label)
                col._build_hessian_code_object()

    def example():
        from examples import kkt_augmented
        kkt_augmented.prebuild(20)
    return [cases, example]
