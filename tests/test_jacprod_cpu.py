"""CPU tests of the Jacobian-product program
(``opty_amd.codegen.program.build_jacobian_product_program``): its roots,
evaluated by the NumPy interpreter and assembled on the host into ``J v`` and
``J^T w``, against the sparse matrix of the reference's golden record (or, for
a problem without one, of the Jacobian program's own interpreted entries)."""
import numpy as np
import pytest

import dag_interp
import golden_util as gu
from test_hessian_cpu import _nonlinear_instance_pendulum

from examples import problems
from opty_amd.codegen import ir
from opty_amd.codegen.program import assemble_jvp, assemble_vjp

PROBLEMS = ['msd_be_small', 'msd_mid_small', 'vardur_pendulum_small',
            'pend2_link_vardur_unkmass_small', 'config3_10link_small',
            'piecewise_be_small', 'implicit_traj_be_small',
            'implicit_traj_mid_small', 'biped_small', 'nonlinear_instance']

U = 2.0**-53


def _collocator(name, **extra):
    import opty_amd
    kw = _nonlinear_instance_pendulum() if name == 'nonlinear_instance' \
        else problems.build(name)
    kw.update(extra)
    return opty_amd.ConstraintCollocator(**kw)


def draw(rng, size):
    """``|x|`` in [0.5, 1], random signs."""
    return rng.uniform(0.5, 1.0, size)*rng.choice([-1.0, 1.0], size)


def interpreted_products(col, free, v, w, with_bounds=False):
    """``(J v, J^T w)`` from the product program's roots through the NumPy
    interpreter and the host assembly; ``with_bounds``: also the assembled
    rounding-error bounds of both (units of round-off)."""
    prog = col._build_jacprod_program()
    N = col.num_collocation_nodes
    nodes = np.arange(N - 1)
    atoms = col._atom_free_index()
    fin = col._jacprod_inputs(free, v, nodes, 'jvp')
    rin = col._jacprod_inputs(free, w, nodes, 'vjp')
    tan, tb = dag_interp.evaluate_with_error_bound(prog.dag, prog.tan_out, fin)
    adj, ab = dag_interp.evaluate_with_error_bound(prog.dag, prog.adj_out, rin)
    inst, ib = dag_interp.evaluate_with_error_bound(prog.dag,
                                                    prog.inst_jac_out, fin)
    inst = [float(x) for x in inst]
    jv = assemble_jvp(prog, N, tan, inst, v, atoms)
    jtw = assemble_vjp(prog, N, adj, inst, w, atoms)
    if not with_bounds:
        return jv, jtw
    ib = [abs(float(x)) for x in ib]
    # the bound of a sum is the sum of the bounds (plus the additions' own
    # rounding, one unit of every partial sum: below)
    jvb = assemble_jvp(prog, N, [np.abs(x) for x in tb], ib, np.abs(v), atoms)
    jtwb = assemble_vjp(prog, N, [np.abs(x) for x in ab], ib, np.abs(w),
                        atoms)
    return jv, jtw, jvb, jtwb


def reference_matrix(name, col):
    """``(free, J, |J|, F)`` as scipy CSR matrices of shape (num_constraints,
    num_free): from the reference's golden record where the problem has one,
    otherwise from the Jacobian program's interpreted entries.  ``F``: the
    rounding-error floor the Jacobian parity tests grant the entries that meet
    the 1e-10 bar only through it (zero elsewhere)."""
    import scipy.sparse as sp
    shape = (col.num_constraints, col.num_free)
    if name in gu.MANIFEST:
        meta, z = gu.load(name)
        free, jac, rows, cols = z['free'], z['jac'], z['rows'], z['cols']
        _, ours = dag_interp.evaluate_collocator(col, free)
        _, jb = gu.error_bounds(col, free)
        N1, M, C = meta['N'] - 1, meta['M'], meta['C']
        _, cap = gu.caps_for(jac, meta['num_constraints'], N1, M, C)
        granted = np.minimum(gu.BOUND_UNITS*U*jb, 1e-10*cap)
        by_floor = np.abs(ours - jac) > 1e-10*np.abs(jac)
        floor = np.where(by_floor, granted, 0.0)
    else:
        rng = np.random.default_rng(23)
        free = rng.uniform(-1.0, 1.0, col.num_free)
        _, jac = dag_interp.evaluate_collocator(col, free)
        prog = col._build_program()
        N = col.num_collocation_nodes
        i = np.arange(N - 1)[:, None]
        from opty_amd.codegen.program import column_side
        side = np.array([column_side(prog.n, prog.q, prog.method, k)
                         for _, k in prog.pattern])
        eq = np.array([j for j, _ in prog.pattern])
        rows = (eq[None, :]*(N - 1) + i).ravel()
        cols = np.where(side[:, 0] >= 0, side[:, 0]*N + i + side[:, 1],
                        (prog.n + prog.q)*N + side[:, 1]).ravel()
        ir_, ic_ = col._instance_constraints_jacobian_indices()
        rows, cols = np.r_[rows, ir_], np.r_[cols, ic_]
        floor = np.zeros(len(jac))
    J = sp.coo_matrix((jac, (rows, cols)), shape=shape).tocsr()
    A = sp.coo_matrix((np.abs(jac), (rows, cols)), shape=shape).tocsr()
    F = sp.coo_matrix((floor, (rows, cols)), shape=shape).tocsr()
    K = sp.coo_matrix((np.ones(len(jac)), (rows, cols)), shape=shape).tocsr()
    return free, J, A, F, K


def product_tolerances(A, F, K, v, w):
    """The issue's tolerance per result entry for ``J v`` and ``J^T w``."""
    kv = np.asarray(K.sum(axis=1)).ravel()
    kw = np.asarray(K.sum(axis=0)).ravel()
    tv = (1e-10 + (kv + 2)*U)*(A @ np.abs(v)) + F @ np.abs(v)
    tw = (1e-10 + (kw + 2)*U)*(A.T @ np.abs(w)) + F.T @ np.abs(w)
    return tv, tw


def worst_ratio(err, tol):
    with np.errstate(all='ignore'):
        ratio = np.where(tol > 0, err/tol, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize('name', PROBLEMS)
def test_products_against_the_reference_matrix(name):
    col = _collocator(name)
    free, J, A, F, K = reference_matrix(name, col)
    rng = np.random.default_rng(31)
    v = draw(rng, col.num_free)
    w = draw(rng, col.num_constraints)
    jv, jtw = interpreted_products(col, free, v, w)
    tv, tw = product_tolerances(A, F, K, v, w)
    ev, ew = np.abs(jv - J @ v), np.abs(jtw - J.T @ w)
    print('%s: worst error/tolerance jvp %.3g, vjp %.3g'
          % (name, worst_ratio(ev, tv), worst_ratio(ew, tw)))
    assert np.all(ev <= tv), (name, 'jvp', worst_ratio(ev, tv))
    assert np.all(ew <= tw), (name, 'vjp', worst_ratio(ew, tw))


@pytest.mark.parametrize('name', PROBLEMS)
def test_adjoint_identity(name):
    """``w . (J v) == v . (J^T w)`` on the interpreter."""
    col = _collocator(name)
    free, J, A, F, K = reference_matrix(name, col)
    rng = np.random.default_rng(37)
    v = draw(rng, col.num_free)
    w = draw(rng, col.num_constraints)
    jv, jtw = interpreted_products(col, free, v, w)
    lhs, rhs = float(w @ jv), float(v @ jtw)
    tol = 64*U*float(np.abs(w) @ (A @ np.abs(v)))
    print('%s: |w.Jv - v.JTw| = %.3g, tolerance %.3g'
          % (name, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol


def test_emitted_source_has_the_four_kernels_and_no_atomics():
    from opty_amd.codegen.emit_jacprod import emit_jacprod_module
    for name in ('config3_10link_small', 'vardur_pendulum_small'):
        prog = _collocator(name)._build_jacprod_program()
        source, cuts = emit_jacprod_module(prog)
        for kernel in ('opty_jvp(', 'opty_jvp_inst(', 'opty_vjp(',
                       'opty_vjp_fin('):
            assert kernel in source, (name, kernel)
        assert 'atomic' not in source.lower()
        assert '__launch_bounds__(64)' in source
        assert 'asm' not in source


def _ops(dag, roots):
    return sum(dag.count_ops(roots).values())


def test_the_tangent_is_cheap():
    """One tangent pushed through the DAG: fewer operations than the
    Jacobian's entries (and a small multiple of the constraints')."""
    col = _collocator('config3_10link_small')
    prod = col._build_jacprod_program()
    jac = col._build_program()
    tangent = _ops(prod.dag, prod.tan_out)
    entries = _ops(jac.dag, jac.jac_out)
    con = _ops(jac.dag, jac.con_out)
    print('config3_10link_small: tangent %d ops, jac_out %d ops, con_out %d '
          'ops' % (tangent, entries, con))
    assert tangent < entries
    assert tangent <= 5*con


def test_implicit_trajectories_are_supported_and_inputs_are_named():
    col = _collocator('implicit_traj_mid_small')
    prog = col._build_jacprod_program()
    kinds = {prog.dag.args[i][0] for i in prog.dag.reachable(prog.tan_out)
             if prog.dag.op[i] == ir.INPUT}
    assert 'vcur' in kinds and 'vadj' in kinds and 'dir' not in kinds
    kinds = {prog.dag.args[i][0] for i in prog.dag.reachable(prog.adj_out)
             if prog.dag.op[i] == ir.INPUT}
    assert 'lam' in kinds and not kinds & {'vcur', 'vadj', 'vpar', 'vh'}
