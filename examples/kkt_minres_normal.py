"""The Newton step of ``examples/kkt_minres.py`` -- the pendulum swing-up with
the effort objective, ``K = [[H, J^T], [J, 0]]`` matrix-free on the GPU --
solved by MINRES WITH a preconditioner: the block diagonal

    M^-1 = diag( 1/d ,  S^-1 ,  1/s )

* ``1/d`` on the free block, ``d = |diag W| + delta_w`` from the Hessian's
  triplets;
* ``S^-1`` on the collocation rows: a direct solve with the block-tridiagonal
  normal matrix ``S = Jc[:, :T] diag(1/d[:T]) Jc[:, :T]^T``
  (``Problem.normal_operator``: formed, factorised by block cyclic reduction
  and solved with on the GPU);
* ``1/s_k``, ``s_k = sum_j J_kj^2 / d_j``, on the instance rows.

Prints the iteration counts with and without the preconditioner.

    python examples/kkt_minres_normal.py [num_nodes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def prebuild(num_nodes=20):
    """Builds the code objects :func:`main` loads (no GPU needed): those of
    ``examples/kkt_minres.py``; the solver's kernels are the runtime
    library's."""
    from examples import kkt_minres
    kkt_minres.prebuild(num_nodes)


def preconditioner(prob, free, lagrange, obj_factor=1.0, delta_w=1.0):
    """``(M, d)``: the block-diagonal preconditioner at ``(free, lagrange)``
    as a symmetric positive definite ``LinearOperator`` over ``num_free +
    num_constraints`` rows, and ``d``."""
    from scipy.sparse.linalg import LinearOperator
    n, m = prob.num_free, prob.num_constraints
    rows, cols = prob.hessianstructure()
    values = np.asarray(prob.hessian(free, lagrange, obj_factor))
    on = np.asarray(rows) == np.asarray(cols)
    diag = np.zeros(n)
    np.add.at(diag, np.asarray(rows)[on], values[on])
    d = np.abs(diag) + delta_w
    solve = prob.normal_operator(free, d=d, delta_c=0.0)
    mc = solve.shape[0]                 # collocation rows
    jrows, jcols = (np.asarray(x) for x in prob.jacobianstructure())
    jvals = np.asarray(prob.jacobian(free))
    inst = jrows >= mc
    s = np.zeros(m - mc)
    np.add.at(s, jrows[inst] - mc, jvals[inst]**2/d[jcols[inst]])

    def matvec(z):
        z = np.asarray(z, dtype=float).reshape(-1)
        w = z[n:]
        return np.concatenate((z[:n]/d, solve.matvec(w[:mc]), w[mc:]/s))
    return LinearOperator((n + m, n + m), dtype=np.float64, matvec=matvec,
                          rmatvec=matvec), d


def main(num_nodes=20, maxiter=None, delta_w=1.0, verbose=True):
    """``{'plain': (info, iterations, residual), 'preconditioned': ...}`` of
    the two MINRES runs on the same system."""
    from scipy.sparse.linalg import minres
    from examples import kkt_minres
    prob = kkt_minres.problem(num_nodes)
    rng = np.random.default_rng(0)
    free = 0.1*rng.standard_normal(prob.num_free)
    lagrange = np.zeros(prob.num_constraints)
    K, H, J = kkt_minres.kkt_operator(prob, free, lagrange)
    rhs = -np.concatenate((prob.gradient(free) + J.rmatvec(lagrange),
                           prob.constraints(free)))
    M, d = preconditioner(prob, free, lagrange, delta_w=delta_w)
    if maxiter is None:
        maxiter = 20*len(rhs)
    out = {}
    for name, kw in (('plain', {}), ('preconditioned', dict(M=M))):
        count = [0]

        def callback(z):
            count[0] += 1
        step, info = minres(K, rhs, maxiter=maxiter, callback=callback, **kw)
        residual = float(np.linalg.norm(K.matvec(step) - rhs))
        out[name] = (info, count[0], residual)
        if verbose:
            print('minres %-15s info %d after %4d iterations, |K z - rhs| = '
                  '%.3e (|rhs| = %.3e)' % (name + ':', info, count[0],
                                           residual, np.linalg.norm(rhs)))
    return out


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
