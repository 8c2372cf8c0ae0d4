#!/usr/bin/env python
"""Makes an initial guess dynamically consistent without ever forming the
constraint Jacobian: Gauss-Newton steps ``dx = lsmr(J, -c)`` on the 1-link
pendulum swing-up, where ``J`` is the matrix-free operator of
``ConstraintCollocator.jacobian_operator(free)`` (``matvec`` = ``J v`` and
``rmatvec`` = ``J^T w``, both evaluated on the GPU) and ``c`` is
``constraints(free)``.  LSMR returns the minimum-norm step, i.e. the guess
moves as little as the linearised dynamics allow.  Prints ``||c||`` per
iteration; exits non-zero if the norm did not fall."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                '..')))

import numpy as np
from scipy.sparse.linalg import lsmr

import opty_amd
from examples import problems


def main(num_nodes=101, iterations=6, verbose=True):
    kw = problems.pendulum_swing_up(num_nodes=num_nodes, duration=10.0)
    col = opty_amd.ConstraintCollocator(**kw)
    constraints = col.generate_constraint_function()
    N = num_nodes
    # a guess that knows the boundary values and nothing of the dynamics:
    # the angle goes linearly from 0 to pi, no speed, no torque
    free = np.zeros(col.num_free)
    free[:N] = np.linspace(0.0, np.pi, N)
    norms = []
    for it in range(iterations + 1):
        c = np.array(constraints(free))
        norms.append(float(np.linalg.norm(c)))
        if verbose:
            print('iteration %d: ||c|| = %.6e' % (it, norms[-1]))
        if it == iterations or norms[-1] < 1e-10:
            break
        J = col.jacobian_operator(free)
        dx = lsmr(J, -c, atol=1e-12, btol=1e-12, maxiter=4*col.num_free)[0]
        free = free + dx
    return free, norms


if __name__ == '__main__':
    _, norms = main()
    sys.exit(0 if norms[-1] < norms[0] else 1)
