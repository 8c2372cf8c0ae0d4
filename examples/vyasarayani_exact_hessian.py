#!/usr/bin/env python
"""The parameter identification of ``vyasarayani_scipy.py`` with exact
second-order information: SciPy's ``trust-constr`` gets ``hess=`` for the
objective and ``NonlinearConstraint(..., hess=...)`` for the collocation
constraints.  The ``hess(x, v)`` of a ``NonlinearConstraint`` is exactly
``Problem.hessian``'s constraint part: ``sum_k v_k d2 con_k / d x^2``, here
the GPU Hessian of ``ConstraintCollocator.generate_hessian_function``
(lower-triangle triplets whose duplicates add up, which
``scipy.sparse.coo_matrix`` does).  Prints the iteration count next to the
quasi-Newton run of ``vyasarayani_scipy.py``."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                '..')))

import numpy as np
import scipy.optimize as so
import scipy.sparse as sp
import sympy as sym
from scipy.integrate import odeint

import opty_amd


def main(num_nodes=101, duration=5.0, seed=0, verbose=True):
    p, t = sym.symbols('p, t')
    y1, y2 = [f(t) for f in sym.symbols('y1, y2', cls=sym.Function)]
    y = sym.Matrix([y1, y2])
    eom = y.diff(t) - sym.Matrix([y2, -p*sym.sin(y1)])

    interval = duration/(num_nodes - 1)
    time = np.linspace(0.0, duration, num=num_nodes)
    p_true = 10.0
    y_meas = odeint(lambda y, t: [y[1], -p_true*np.sin(y[0])],
                    [np.pi/6.0, 0.0], time)
    rng = np.random.default_rng(seed)
    y1_meas = y_meas[:, 0] + rng.normal(scale=0.01, size=num_nodes)

    def obj(free):
        return interval*np.sum((y1_meas - free[:num_nodes])**2)

    def obj_grad(free):
        grad = np.zeros_like(free)
        grad[:num_nodes] = 2.0*interval*(free[:num_nodes] - y1_meas)
        return grad

    idx = np.arange(num_nodes, dtype=np.int64)
    prob = opty_amd.Problem(
        obj, obj_grad, eom, (y1, y2), num_nodes, interval, time_symbol=t,
        integration_method='midpoint',
        obj_hessian=(idx, idx, lambda free: np.full(num_nodes,
                                                    2.0*interval)))
    rows, cols = prob.jacobianstructure()
    n = prob.num_free
    shape = (prob.num_constraints, n)
    hrows, hcols = prob.hessianstructure()
    ncon = len(prob.collocator.hessian_indices()[0])

    def jac(free):
        return sp.coo_matrix((prob.jacobian(free), (rows, cols)),
                             shape=shape).tocsr()

    def full(values, r, c):
        low = sp.coo_matrix((values, (r, c)), shape=(n, n)).tocsr()
        return low + sp.triu(low.T, k=1)

    def con_hess(free, v):
        return full(prob.hessian(free, v, 0.0)[:ncon], hrows[:ncon],
                    hcols[:ncon])

    def obj_hess(free):
        zero = np.zeros(prob.num_constraints)
        return full(prob.hessian(free, zero, 1.0)[ncon:], hrows[ncon:],
                    hcols[ncon:])

    con = so.NonlinearConstraint(prob.constraints, 0.0, 0.0, jac=jac,
                                 hess=con_hess)
    x0 = np.hstack((y_meas[:, 0], y_meas[:, 1], 5.0))     # wrong parameter
    res = so.minimize(prob.objective, x0, jac=prob.gradient, hess=obj_hess,
                      constraints=[con], method='trust-constr',
                      options=dict(maxiter=300, gtol=1e-10, xtol=1e-12))
    p_hat = res.x[-1]
    if verbose:
        try:
            from examples.vyasarayani_scipy import main as quasi_newton
        except ImportError:
            from vyasarayani_scipy import main as quasi_newton
        p_qn, res_qn = quasi_newton(num_nodes, duration, seed,
                                    verbose=False)
        print('exact Hessian: p = %.4f in %d iterations; quasi-Newton: '
              'p = %.4f in %d iterations (true %.1f)'
              % (p_hat, res.nit, p_qn, res_qn.nit, p_true))
    return p_hat, res


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
