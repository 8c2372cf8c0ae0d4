"""A few extreme eigenvalues of the Hessian of the Lagrangian of the problem of
``examples/kkt_minres.py`` -- the pendulum swing-up with the effort objective
-- with ``scipy.sparse.linalg.lobpcg``: what a convexification or inertia
heuristic asks for before it trusts a Newton step.  LOBPCG works on a block of
vectors, so every product it asks for is ``H X`` for a few columns at once;
``Problem.hessian_operator`` answers ``matmat`` with one block product on the
GPU (``opty_hessmv_block``: every stored value is read once for the columns of
a pass), bit for bit the column stack of its ``matvec``.  Prints the
eigenvalues at both ends of the spectrum and the number of block products.

    python examples/hessian_lobpcg.py [num_nodes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#: eigenvalues per end of the spectrum
BLOCK = 3
#: residual tolerance handed to lobpcg
TOL = 1e-6


def prebuild(num_nodes=20):
    """Builds the code objects :func:`main` loads (no GPU needed)."""
    from examples import kkt_minres
    kkt_minres.prebuild(num_nodes)


def operator(num_nodes=20, obj_factor=1.0):
    """``(prob, free, lagrange, H)``: the Hessian operator at a seeded random
    point."""
    from examples import kkt_minres
    prob = kkt_minres.problem(num_nodes)
    rng = np.random.default_rng(0)
    free = rng.standard_normal(prob.num_free)
    lagrange = rng.uniform(-1.0, 1.0, prob.num_constraints)
    return prob, free, lagrange, prob.hessian_operator(free, lagrange,
                                                       obj_factor)


def extreme_eigenvalues(H, block=BLOCK, tol=TOL, maxiter=500):
    """``(smallest, largest, products)``: ``block`` eigenvalues at each end
    of the spectrum of the symmetric operator ``H``, ascending, and the
    number of block products ``H X`` that LOBPCG asked for."""
    from scipy.sparse.linalg import LinearOperator, lobpcg
    products = [0]

    def matmat(X):
        products[0] += 1
        return H.matmat(X)
    counted = LinearOperator(H.shape, dtype=np.float64, matmat=matmat,
                             matvec=lambda x: matmat(x.reshape(-1, 1)))
    ends = []
    for largest in (False, True):
        X = np.random.default_rng(1).standard_normal((H.shape[0], block))
        values, _ = lobpcg(counted, X, tol=tol, maxiter=maxiter,
                           largest=largest)
        ends.append(np.sort(values))
    return ends[0], ends[1], products[0]


def main(num_nodes=20, verbose=True):
    """``(smallest, largest, spectral radius, products)``."""
    prob, free, lagrange, H = operator(num_nodes)
    smallest, largest, products = extreme_eigenvalues(H)
    radius = float(max(abs(smallest[0]), abs(largest[-1])))
    if verbose:
        print('Hessian of the Lagrangian, %d x %d, %d columns per pass'
              % (H.shape[0], H.shape[1], H.handle.block_width))
        print('smallest eigenvalues:', ' '.join('%.9g' % x for x in smallest))
        print('largest eigenvalues: ', ' '.join('%.9g' % x for x in largest))
        print('spectral radius %.9g, %d block products of %d columns'
              % (radius, products, BLOCK))
    return smallest, largest, radius, products


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
