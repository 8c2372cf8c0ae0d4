"""CPU tests of the Hessian program of the constraint Lagrangian
(``opty_amd.codegen.program.build_hessian_program``): its entries against
SymPy's own Hessian of ``sum_j lam_j eom_j``, the assembled matrix (triplets
summed, closed-form indices) against a central finite difference of
``J(free)^T lagrange`` from the oracle, and what is refused."""
import numpy as np
import pytest
import sympy as sm

import dag_interp
from golden_util import assert_close

from examples import problems

PROBLEMS = ['msd_be_small', 'msd_mid_small', 'vardur_pendulum_small',
            'pend2_link_vardur_unkmass_small', 'config2_pendulum_small',
            'config3_10link_small', 'piecewise_be_small', 'c99_be_small']


def _collocator(kw):
    import opty_amd
    return opty_amd.ConstraintCollocator(**kw)


def _nonlinear_instance_pendulum(num_nodes=101):
    """``config2_pendulum_small`` with a nonlinear instance constraint, so
    that the instance tail of the Hessian is not empty."""
    kw = problems.pendulum_swing_up(num_nodes=num_nodes)
    theta = kw['state_symbols'][0].func
    omega = kw['state_symbols'][1].func
    dur = kw['node_time_interval']*(num_nodes - 1)
    # (the collocator takes every applied function of an instance
    # constraint for a trajectory value, as the reference does: polynomials)
    kw['instance_constraints'] = (theta(0.0), theta(0.0)**2*theta(dur),
                                  omega(0.0)*omega(dur), omega(dur))
    return kw


def _symbol_inputs(col, prog, rng, count):
    """Random values for every discrete symbol and multiplier, and the
    matching ``inputs(kind, index)`` of the DAG interpreter (the interpreter
    is fed ``'lam'`` through that callback)."""
    be = col.integration_method == 'backward euler'
    state_adj = col.previous_discrete_state_symbols if be \
        else col.next_discrete_state_symbols
    cur = list(col.current_discrete_state_symbols) + \
        list(col.current_discrete_specified_symbols)
    adj = list(state_adj) + list(col.next_discrete_specified_symbols)
    lams = sm.symbols('lam0:%d' % prog.M, real=True)
    values = {}
    for s in cur + adj + list(col.parameters) + list(lams):
        values[s] = rng.uniform(-1.0, 1.0, count)
    values[col.time_interval_symbol] = rng.uniform(0.01, 0.1, count)

    def inputs(kind, idx):
        if kind == 'cur':
            return values[cur[idx]]
        if kind == 'adj':
            return values[adj[idx]]
        if kind == 'par':
            return values[col.parameters[idx]]
        if kind == 'h':
            return values[col.time_interval_symbol]
        if kind == 'lam':
            return values[lams[idx]]
        raise AssertionError(kind)
    return values, lams, inputs


@pytest.mark.parametrize('name', PROBLEMS)
def test_entries_equal_sympys_hessian(name):
    """Every stored entry equals SymPy's ``hessian(sum lam_j eom_j, wrt)``
    at random node values (1e-10 relative, rounding-error floors), and
    every lower-triangle entry that is not stored is zero there."""
    col = _collocator(problems.build(name))
    prog = col._build_hessian_program()
    rng = np.random.default_rng(3)
    count = 7
    values, lams, inputs = _symbol_inputs(col, prog, rng, count)
    wrt = list(col._wrt())
    L = sum(lam*e for lam, e in zip(lams, col.discrete_eom))
    # (derivatives of steps: zero away from the jump, as the DAG's rule)
    H = sm.hessian(L, wrt).replace(sm.DiracDelta, lambda *a: sm.S.Zero)
    args = list(values)
    f = sm.lambdify(args, list(H), modules=['numpy', 'scipy'])
    with np.errstate(all='ignore'):
        want = np.array([np.broadcast_to(np.asarray(v, dtype=float), (count,))
                         for v in f(*[values[s] for s in args])])
    want = want.reshape(len(wrt), len(wrt), count)
    got = dag_interp.evaluate(prog.dag, prog.hess_out, inputs)
    _, bound = dag_interp.evaluate_with_error_bound(prog.dag, prog.hess_out,
                                                    inputs)
    stored = set()
    for e, (a, b) in enumerate(prog.hess_pairs):
        stored.add((a, b))
        assert_close(np.broadcast_to(got[e], (count,)), want[a, b],
                     bound=np.broadcast_to(bound[e], (count,)),
                     what='%s entry %d (%d, %d)' % (name, e, a, b))
    from opty_amd.codegen.program import column_side, _side_order

    def order(k):
        return _side_order(column_side(prog.n, prog.q, prog.method, k))
    for a in range(len(wrt)):
        for b in range(len(wrt)):
            if order(a) >= order(b) and (a, b) not in stored:
                assert np.all(want[a, b] == 0.0), (name, a, b)
    assert len(set(prog.hess_pairs)) == prog.PH


def test_nonlinear_instance_constraint_entries():
    """The instance tail: second partials of each instance expression with
    respect to its atoms, lower triangle on the free indices."""
    col = _collocator(_nonlinear_instance_pendulum())
    prog = col._build_hessian_program()
    assert len(prog.inst_hess_out) == 3       # a**2*b: aa, ba; w0*wN: 1
    atoms = col._inst_atoms
    rng = np.random.default_rng(5)
    vals = rng.uniform(-1.0, 1.0, len(atoms))

    def inputs(kind, idx):
        if kind == 'free':
            return vals[idx]
        assert kind == 'par', kind
        return float(col.known_parameter_map[col.known_parameters[idx]])
    got = dag_interp.evaluate(prog.dag, prog.inst_hess_out, inputs)
    sym = {f: sm.Dummy() for f in atoms}
    place = {sym[f]: v for f, v in zip(atoms, vals)}
    idx = col.instance_constraints_free_index_map
    for t, (k, (a, b)) in enumerate(zip(prog.inst_hess_con,
                                        prog.inst_hess_atoms)):
        expr = sm.sympify(col.instance_constraints[k]).xreplace(sym)
        fa, fb = atoms[a], atoms[b]
        assert idx[fa] >= idx[fb]
        want = float(expr.diff(sym[fa]).diff(sym[fb]).xreplace(place))
        np.testing.assert_allclose(got[t], want, rtol=1e-12, atol=1e-15)


def _dense_hessian(col, free, lagrange):
    """Triplets (interpreter values, closed-form indices) summed into a
    dense lower triangle."""
    prog = col._build_hessian_program()
    N = col.num_collocation_nodes
    ncn = N - 1
    inputs0 = col._node_inputs(free, N, 0, ncn, col._known_trajectory_array(
        free) if col.num_known_input_trajectories else None)
    idx = col.instance_constraints_free_index_map \
        if col.num_instance_constraints else {}

    def inputs(kind, i):
        if kind == 'lam':
            return lagrange[i*ncn:(i + 1)*ncn]
        if kind == 'free':
            return free[idx[col._inst_atoms[i]]]
        return inputs0(kind, i)
    vals = dag_interp.evaluate(prog.dag, prog.hess_out, inputs)
    block = np.stack([np.broadcast_to(np.asarray(v, dtype=float), (ncn,))
                      for v in vals], axis=1) if vals else np.zeros((ncn, 0))
    ivals = dag_interp.evaluate(prog.dag, prog.inst_hess_out, inputs)
    ivals = np.array([float(v)*lagrange[prog.M*ncn + k]
                      for v, k in zip(ivals, prog.inst_hess_con)])
    values = np.concatenate((block.ravel(), ivals))
    rows, cols = col.hessian_indices_closed_form()
    assert rows.dtype == np.int64 and cols.dtype == np.int64
    assert len(rows) == len(values)
    assert np.all(rows >= cols)
    dense = np.zeros((col.num_free, col.num_free))
    np.add.at(dense, (rows, cols), values)
    return dense


@pytest.mark.parametrize('name', ['msd_be_small', 'vardur_pendulum_small',
                                  'pend2_link_vardur_unkmass_small',
                                  'nonlinear_instance'])
def test_assembled_matrix_against_finite_differences(name):
    """Sum of the triplets == central finite difference of
    ``J(free)^T lagrange`` (J from the oracle), symmetrised, lower
    triangle: pins the structure, the orientation of every entry and the
    sum-of-duplicates contract."""
    from oracle.collocation_oracle import OracleCollocator
    if name == 'nonlinear_instance':
        kw = _nonlinear_instance_pendulum(num_nodes=9)
    elif name == 'vardur_pendulum_small':
        kw = problems.variable_duration_pendulum(num_nodes=9)
    else:
        kw = problems.build(name)
    col = _collocator(kw)
    orc = OracleCollocator(name='hess_' + name + '_%d'
                           % col.num_collocation_nodes, **kw)
    jac = orc.generate_jacobian_function()
    jr, jc = orc.jacobian_indices()
    rng = np.random.default_rng(11)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.05
    lagrange = rng.uniform(-1.0, 1.0, col.num_constraints)

    def grad(x):
        g = np.zeros(col.num_free)
        np.add.at(g, jc, jac(x)*lagrange[jr])
        return g
    step = 1e-6
    fd = np.empty((col.num_free, col.num_free))
    for k in range(col.num_free):
        d = np.zeros(col.num_free)
        d[k] = step
        fd[:, k] = (grad(free + d) - grad(free - d))/(2*step)
    fd = np.tril(0.5*(fd + fd.T))
    got = _dense_hessian(col, free, lagrange)
    scale = max(1.0, np.abs(fd).max())
    np.testing.assert_allclose(got, fd, rtol=1e-6, atol=1e-6*scale)


def test_refused_problems():
    """Implicit known trajectories and known trajectories given as
    functions of ``free`` have no Hessian here."""
    col = _collocator(problems.build('implicit_traj_be_small'))
    with pytest.raises(NotImplementedError):
        col._build_hessian_program()
    kw = problems.build('msd_be_small')
    (f, vals), = kw['known_trajectory_map'].items()
    kw['known_trajectory_map'] = {f: lambda free: vals}
    col = _collocator(kw)
    with pytest.raises(NotImplementedError):
        col._build_hessian_program()


def test_instance_atoms_sharing_a_free_index():
    """Two distinct atoms at the same free index (both closest to node 0):
    both mixed partials land on that diagonal entry, so the summed triplets
    hold the whole second derivative."""
    kw = problems.pendulum_swing_up(num_nodes=11)
    theta = kw['state_symbols'][0].func
    kw['instance_constraints'] = (theta(0.0)*theta(0.001),)
    col = _collocator(kw)
    prog = col._build_hessian_program()
    # d2/dt0 dt1 twice (both orders); the squares vanish
    assert len(prog.inst_hess_out) == 2
    rows, cols = col.hessian_indices_closed_form()
    ncn = col.num_collocation_nodes - 1
    assert np.all(rows[ncn*prog.PH:] == 0) and np.all(cols[ncn*prog.PH:] == 0)


def test_problem_without_objective_hessian_has_no_hessian():
    """Without ``obj_hessian`` a Problem has no ``hessian`` (IPOPT keeps its
    limited-memory default); lower-triangle entries only are accepted."""
    import opty_amd
    assert not hasattr(opty_amd.Problem, 'hessian')
    assert not hasattr(opty_amd.Problem, 'hessianstructure')
    with pytest.raises(ValueError):
        opty_amd.Problem._check_obj_hessian(([0, 1], [1, 1], lambda f: f))
    rows, cols, _ = opty_amd.Problem._check_obj_hessian(
        ([1, 1], [0, 1], lambda f: f))
    assert rows.dtype == np.int64


def test_sharded_problem_refuses_an_objective_hessian():
    import opty_amd
    kw = problems.build('msd_be_small')
    with pytest.raises(NotImplementedError):
        opty_amd.ShardedProblem(
            lambda f: 0.0, lambda f: f, kw['equations_of_motion'],
            kw['state_symbols'], kw['num_collocation_nodes'],
            kw['node_time_interval'],
            obj_hessian=([0], [0], lambda f: np.ones(1)))
