"""The Newton step of ``examples/kkt_minres.py`` solved DIRECTLY: the lower
triangle of the KKT matrix

    [[H, J^T],     H = obj_factor d2 f + sum_k lagrange_k d2 c_k
     [J,  0 ]]     J = d c / d free

is assembled with ``scipy.sparse.bmat`` from two canonical CSR matrices that
the GPU hands over as they are -- ``Problem.hessian_csr`` (the Hessian's
triplets compressed to the unique lower triangle on the device) and the
Jacobian of a ``jacobian_layout='csr'`` collocator -- mirrored, and solved
with ``scipy.sparse.linalg.spsolve`` (without the variables that nothing
reads: their rows of K are zero).  Prints the residual ``|K z - rhs|``
computed with the two matrix-free operators of ``kkt_minres.kkt_operator``.

    python examples/kkt_direct.py [num_nodes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples import kkt_minres     # noqa: E402


def csr_collocator(num_nodes=20):
    """The problem's constraints with the Jacobian stored as CSR."""
    import opty_amd
    kw = kkt_minres._arguments(num_nodes)[0]
    return opty_amd.ConstraintCollocator(jacobian_layout='csr', **kw)


def prebuild(num_nodes=20):
    """Builds the code objects :func:`main` loads (no GPU needed)."""
    kkt_minres.prebuild(num_nodes)
    csr_collocator(num_nodes).prebuild()


def kkt_lower_triangle(prob, col, free, lagrange, obj_factor=1.0):
    """``scipy.sparse`` CSR matrix of the lower triangle ``[[H, 0], [J, 0]]``
    of the KKT matrix at ``(free, lagrange)``; ``col`` is the problem's
    ``jacobian_layout='csr'`` collocator."""
    import scipy.sparse as sp
    n, m = prob.num_free, prob.num_constraints
    indptr, indices = prob.hessian_csr_structure()
    H = sp.csr_matrix((np.array(prob.hessian_csr(free, lagrange, obj_factor)),
                       indices, indptr), shape=(n, n))
    assert H.has_canonical_format
    row_ptr, col_idx = col.jacobian_csr_structure()
    J = sp.csr_matrix((np.array(col.generate_jacobian_function()(free)),
                       col_idx, row_ptr), shape=(m, n))
    return sp.bmat([[H, None], [J, sp.csr_matrix((m, m))]], format='csr')


def main(num_nodes=20, verbose=True):
    """``(step, residual, |rhs|)`` of the direct Newton step."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    prob = kkt_minres.problem(num_nodes)
    col = csr_collocator(num_nodes)
    rng = np.random.default_rng(0)
    free = 0.1*rng.standard_normal(prob.num_free)
    lagrange = np.zeros(prob.num_constraints)
    K, H, J = kkt_minres.kkt_operator(prob, free, lagrange)
    rhs = -np.concatenate((prob.gradient(free) + J.rmatvec(lagrange),
                           prob.constraints(free)))
    L = kkt_lower_triangle(prob, col, free, lagrange)
    full = (L + sp.tril(L, -1).T).tocsr()
    # a free variable that neither the objective nor a constraint reads --
    # backward Euler never evaluates the input at the first node -- has a
    # zero row and column in K and a zero in rhs: the step leaves it alone
    live = np.asarray(abs(full).sum(axis=1)).ravel() > 0
    step = np.zeros(len(rhs))
    step[live] = spsolve(full[live][:, live].tocsc(), rhs[live])
    residual = float(np.linalg.norm(K.matvec(step) - rhs))
    if verbose:
        print('KKT matrix %d x %d (%d rows are zero), %d stored values in '
              'its lower triangle (Hessian: %d distinct pairs of %d '
              'triplets)'
              % (full.shape + (int((~live).sum()), L.nnz,
                               len(prob.hessian_csr_structure()[1]),
                               len(prob.hessianstructure()[0]))))
        print('spsolve: |K z - rhs| = %.3e through the operators, |rhs| = '
              '%.3e' % (residual, np.linalg.norm(rhs)))
    return step, residual, float(np.linalg.norm(rhs))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
