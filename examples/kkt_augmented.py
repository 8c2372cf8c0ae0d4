"""The Newton step of ``examples/kkt_direct.py`` from ONE matrix that the GPU
assembles: the lower triangle of the interior-point augmented system

    K = [[ W + diag(sigma) + delta_w I ,  J^T        ],
         [ J                           ,  -delta_c I ]]
    W = obj_factor d2 f + sum_k lagrange_k d2 c_k,   J = d c / d free

comes from ``Problem.kkt_csr`` as canonical CSR with every diagonal stored --
the Hessian's triplets and the Jacobian's values never leave the device, and
``delta_w`` / ``delta_c`` can change between two factorisations without a new
structure.  The triangle is mirrored once and handed to
``scipy.sparse.linalg.spsolve`` with NO mask of live rows: the stored diagonal
makes the rows that neither the objective nor a constraint reads regular.
Prints ``|K z - rhs|`` through the matrix-free operators of
``kkt_minres.kkt_operator`` (the unregularised system) and the distance to the
step of ``kkt_direct.main`` as ``delta -> 0``.

    python examples/kkt_augmented.py [num_nodes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples import kkt_direct, kkt_minres     # noqa: E402

DELTAS = (1e-4, 1e-6, 1e-8)


def problem(num_nodes=20):
    """The problem of ``kkt_minres`` with the Jacobian stored as CSR."""
    import opty_amd
    kw, args, okw = kkt_minres._arguments(num_nodes)
    obj, obj_grad = opty_amd.create_objective_function(*args, **okw)
    hess = opty_amd.create_objective_hessian_function(*args, **okw)
    return opty_amd.Problem(obj, obj_grad, obj_hessian=hess,
                            jacobian_layout='csr', **kw)


def prebuild(num_nodes=20):
    """Builds the code objects :func:`main` loads (no GPU needed)."""
    kkt_direct.prebuild(num_nodes)
    col = kkt_direct.csr_collocator(num_nodes)
    col._build_hessian_code_object()


def augmented_step(prob, structure, free, lagrange, rhs, delta_w, delta_c):
    """``(step, K)``: the solution of ``K z = rhs`` and the full symmetric
    matrix, mirrored from the triangle the GPU assembled."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    indptr, indices = structure
    size = prob.num_free + prob.num_constraints
    data = np.array(prob.kkt_csr(free, lagrange, delta_w=delta_w,
                                 delta_c=delta_c))
    L = sp.csr_matrix((data, indices, indptr), shape=(size, size))
    assert L.has_canonical_format
    full = (L + sp.tril(L, -1).T).tocsc()
    return spsolve(full, rhs), full


def main(num_nodes=20, verbose=True):
    """``(steps, residuals, distances, |rhs|)`` for ``delta_w = delta_c`` in
    ``DELTAS``: the steps, ``|K z - rhs|`` through the unregularised
    operators, and ``|z - z_direct|`` over the variables that something
    reads."""
    prob = problem(num_nodes)
    # (the operators and the right-hand side are those of kkt_direct.main)
    plain = kkt_minres.problem(num_nodes)
    rng = np.random.default_rng(0)
    free = 0.1*rng.standard_normal(prob.num_free)
    lagrange = np.zeros(prob.num_constraints)
    K, H, J = kkt_minres.kkt_operator(plain, free, lagrange)
    rhs = -np.concatenate((plain.gradient(free) + J.rmatvec(lagrange),
                           plain.constraints(free)))
    structure = prob.kkt_csr_structure()
    direct = kkt_direct.main(num_nodes, verbose=False)[0]
    steps, residuals, distances = [], [], []
    for delta in DELTAS:
        step, full = augmented_step(prob, structure, free, lagrange, rhs,
                                    delta, delta)
        steps.append(step)
        residuals.append(float(np.linalg.norm(K.matvec(step) - rhs)))
        distances.append(float(np.linalg.norm(step - direct)))
        if verbose:
            print('delta_w = delta_c = %.0e: K %d x %d, %d stored values in '
                  'its lower triangle; |K z - rhs| = %.3e through the '
                  'operators, |z - z_direct| = %.3e'
                  % (delta, full.shape[0], full.shape[1],
                     len(structure[1]), residuals[-1], distances[-1]))
    if verbose:
        print('|rhs| = %.3e' % np.linalg.norm(rhs))
    return steps, residuals, distances, float(np.linalg.norm(rhs))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
