"""One Newton step of an equality-constrained problem of the zoo -- the
pendulum swing-up with the effort objective ``Integral(T(t)**2, t)`` -- solved
matrix-free on the GPU: the KKT operator

    [[H, J^T],     H = obj_factor d2 f + sum_k lagrange_k d2 c_k
     [J,  0 ]]     J = d c / d free

is built from ``Problem.hessian_operator`` (H v from the stored triplets) and
``Problem.jacobian_operator`` (J v and J^T w without the matrix) and handed to
``scipy.sparse.linalg.minres``; nothing of the size of a matrix leaves the
device.  Prints the residual history.

    python examples/kkt_minres.py [num_nodes]
"""
import os
import sys

import numpy as np
import sympy as sm

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHOD = 'backward euler'


def _arguments(num_nodes):
    from examples import problems
    kw = problems.pendulum_swing_up(num_nodes=num_nodes, method=METHOD)
    t = kw['time_symbol']
    torque = sm.Function('T')(t)
    args = (sm.Integral(torque**2, t), kw['state_symbols'], [torque], [],
            num_nodes, kw['node_time_interval'])
    return kw, args, dict(integration_method=METHOD, time_symbol=t)


def problem(num_nodes=20):
    """The ``Problem`` with a device-backed exact Hessian of its objective."""
    import opty_amd
    kw, args, okw = _arguments(num_nodes)
    obj, obj_grad = opty_amd.create_objective_function(*args, **okw)
    hess = opty_amd.create_objective_hessian_function(*args, **okw)
    return opty_amd.Problem(obj, obj_grad, obj_hessian=hess, **kw)


def prebuild(num_nodes=20):
    """Builds the code objects :func:`problem` loads (no GPU needed)."""
    import opty_amd
    from opty_amd.objective import compile_objective, \
        compile_objective_hessian
    kw, args, okw = _arguments(num_nodes)
    compile_objective(*args[:-1], **okw)
    compile_objective_hessian(*args[:-1], **okw)
    col = opty_amd.ConstraintCollocator(**kw)
    col.prebuild()
    col._build_hessian_code_object()
    col._build_jacprod_code_object()


def kkt_operator(prob, free, lagrange, obj_factor=1.0):
    """``(K, H, J)``: the KKT operator at ``(free, lagrange)`` and the two
    operators it is made of.  ``K`` is symmetric: ``rmatvec`` is ``matvec``."""
    from scipy.sparse.linalg import LinearOperator
    H = prob.hessian_operator(free, lagrange, obj_factor)
    J = prob.jacobian_operator(free)
    n, m = prob.num_free, prob.num_constraints

    def matvec(z):
        z = np.asarray(z, dtype=float).reshape(-1)
        x, w = z[:n], z[n:]
        return np.concatenate((H.matvec(x) + J.rmatvec(w), J.matvec(x)))
    K = LinearOperator((n + m, n + m), dtype=np.float64, matvec=matvec,
                       rmatvec=matvec)
    return K, H, J


def main(num_nodes=20, maxiter=400, verbose=True):
    from scipy.sparse.linalg import minres
    prob = problem(num_nodes)
    rng = np.random.default_rng(0)
    free = 0.1*rng.standard_normal(prob.num_free)
    lagrange = np.zeros(prob.num_constraints)
    K, H, J = kkt_operator(prob, free, lagrange)
    rhs = -np.concatenate((prob.gradient(free) + J.rmatvec(lagrange),
                           prob.constraints(free)))
    history = []

    def callback(z):
        history.append(float(np.linalg.norm(K.matvec(z) - rhs)))
        if verbose and (len(history) % 20 == 1):
            print('iteration %4d   |K z - rhs| = %.3e'
                  % (len(history), history[-1]))
    step, info = minres(K, rhs, maxiter=maxiter, callback=callback)
    if verbose:
        print('minres: info %d after %d iterations, |rhs| = %.3e, final '
              'residual %.3e' % (info, len(history), np.linalg.norm(rhs),
                                 history[-1] if history else float('nan')))
    return step, history


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
