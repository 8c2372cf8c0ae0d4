"""One step of a randomised range finder on the constraint Jacobian ``J`` of
the 1-link pendulum swing-up (``config2_pendulum_small``) at a random point,
without ever forming ``J``: ``Y = J Omega`` for a Gaussian test block
``Omega``, ``Q = orth(J^T Y)`` -- an orthonormal basis that captures the
dominant row space -- and the projected Gram matrix ``B = (J Q)^T (J Q)``,
whose eigenvalues estimate the largest squared singular values of ``J``.
Every product is ONE ``matmat`` or ``rmatmat`` of
``ConstraintCollocator.jacobian_operator(free)``: a block product on the GPU
that evaluates what does not depend on the column once per pass.  Prints the
singular value estimates next to those from the assembled sparse Jacobian.

    python examples/jacobian_sketch.py [columns]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAME = 'config2_pendulum_small'
#: columns of the test block
COLUMNS = 6


def collocator():
    import opty_amd
    from examples import problems
    return opty_amd.ConstraintCollocator(**problems.build(NAME))


def prebuild():
    """Builds the code objects :func:`main` loads (no GPU needed)."""
    col = collocator()
    col.prebuild()
    col._build_jacprod_code_object()
    col._build_jacprod_block_code_object()


def sketch(J, omega):
    """``B = (J Q)^T (J Q)`` with ``Q = orth(J^T (J omega))``; ``J`` anything
    with ``matmat`` / ``rmatmat`` (three block products), or a matrix."""
    if hasattr(J, 'matmat'):
        matmat, rmatmat = J.matmat, J.rmatmat
    else:
        matmat, rmatmat = (lambda X: J @ X), (lambda X: J.T @ X)
    Y = matmat(omega)
    Q, _ = np.linalg.qr(rmatmat(Y))
    JQ = matmat(Q)
    return JQ.T @ JQ


def main(columns=COLUMNS, verbose=True):
    """``(B from the operator, B from the assembled sparse Jacobian)``."""
    import scipy.sparse as sp
    col = collocator()
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    omega = rng.standard_normal((col.num_free, columns))
    op = col.jacobian_operator(free)
    B = sketch(op, omega)
    jac = np.array(col.generate_jacobian_function()(free))
    rows, cols = col.jacobian_indices()
    J = sp.coo_matrix((jac, (rows, cols)), shape=op.shape).tocsr()
    B_ref = sketch(J, omega)
    if verbose:
        est = np.sqrt(np.maximum(np.linalg.eigvalsh(B)[::-1], 0.0))
        ref = np.sqrt(np.maximum(np.linalg.eigvalsh(B_ref)[::-1], 0.0))
        print('Jacobian %d x %d, %d columns per block product'
              % (op.shape + (columns,)))
        print('singular value estimates (operator): ',
              ' '.join('%.9g' % x for x in est))
        print('singular value estimates (assembled):',
              ' '.join('%.9g' % x for x in ref))
    return B, B_ref


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else COLUMNS)
