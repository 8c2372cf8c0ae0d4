"""What the objective Hessian test files share: the objectives (the
expressions and argument orders of ``tests/objective_cases.py``), the
INDEPENDENT answer -- ``sympy.diff`` twice, ``lambdify``, a dense matrix
assembled by the two quadrature formulas; nothing of ``opty_amd.codegen`` --
and the code objects that ``__graft_entry__.build`` prebuilds.

``f = h sum_{i=1}^{N-1} G(z_i, p) + b(p)`` (backward Euler),
``f = h sum_{i=0}^{N-2} G((z_i + z_{i+1})/2, p) + b(p)`` (midpoint)."""
import functools

import numpy as np
import sympy as sym

import objective_cases

BE, MID = 'backward euler', 'midpoint'
t = sym.symbols('t')
x, v, u = [f(t) for f in sym.symbols('x, v, u', cls=sym.Function)]
f1, f2 = [f(t) for f in sym.symbols('f1:3', cls=sym.Function)]
m, c, k, p = sym.symbols('m, c, k, p')

_ALL = (sym.Integral(x**2 + m**2, t) + sym.Integral(c**2*f2**2, t) +
        sym.sin(k)**2)
_TRIG = sym.Integral(p*u**2 + sym.cos(x)*v**2, t) + 3*p**2
_STATES_ONLY = sym.Integral(sym.exp(-x)*v**2 + sym.sqrt(1 + x**2), t)
# unsorted inputs and parameters, as in objective_cases.cases()
_FULL = ([x, v], [f2, f1], [m, c, k])


def _case(name, expr, method, args, h):
    return dict(name=name, expr=expr, method=method, args=args, h=h)


def _both(name, expr, args, h):
    return [_case(name + '_be', expr, BE, args, h),
            _case(name + '_mid', expr, MID, args, h)]


#: every objective of the suite; ``args = (states, inputs, unknowns)``
CASES = (
    _both('all', _ALL, _FULL, 0.3) +
    _both('trig', _TRIG, ([x, v], [u], [p]), 0.01) +
    _both('effort', sym.Integral(u**2, t), ([x, v], [u], []), 0.0129) +
    [_case('states_only_mid', _STATES_ONLY, MID, ([x, v], [], []), 0.05)] +
    # no integral at all: E = 0, T = 1
    _both('param_only', m**2, _FULL, 0.3) +
    # linear: nnz == 0
    _both('linear', sym.Integral(x, t), _FULL, 0.5) +
    _both('no_states', sym.Integral(f1**2, t), ([], [f2, f1], [m, c, k]),
          1.0) +
    _both('no_inputs', sym.Integral(x**2, t), ([x, v], [], [m, c, k]), 1.0) +
    _both('no_unknowns', sym.Integral(x**2, t), ([x, v], [f2, f1], []), 1.0))
BY_NAME = {case['name']: case for case in CASES}
assert len(BY_NAME) == len(CASES)
# the expressions are those of tests/objective_cases.py
assert {str(cs['expr']) for cs in objective_cases.reference_cases()[1]} <= \
    {str(cs['expr']) for cs in CASES}


def dims(case):
    states, inputs, unknowns = case['args']
    return len(states), len(inputs), len(unknowns)


def num_free(case, N):
    n, q, r = dims(case)
    return (n + q)*N + r


def make_free(case, N, seed=0):
    return np.random.default_rng(1000 + seed).uniform(-1.0, 1.0,
                                                      num_free(case, N))


def _split(expr):
    """``G`` and ``b`` of ``sum_j a_j(p) Integral(g_j, t) + b(p)``, by SymPy
    alone."""
    expr = sym.sympify(expr)
    integrals = sorted(expr.atoms(sym.Integral), key=sym.default_sort_key)
    dummies = [sym.Dummy() for _ in integrals]
    flat = expr.xreplace(dict(zip(integrals, dummies)))
    G = sum((flat.diff(d)*i.function for d, i in zip(dummies, integrals)),
            sym.S.Zero)
    return G, flat.xreplace({d: 0 for d in dummies})


@functools.lru_cache(maxsize=None)
def _second_partials(name):
    """``[(a, b, lambdified d2G/da db or None, same of b)]`` over the variables
    ``z_0 .. z_{n+q-1}, p_0 .. p_{r-1}`` (name-sorted inputs / parameters),
    all pairs."""
    case = BY_NAME[name]
    states, inputs, unknowns = case['args']
    funcs = list(states) + sorted(inputs, key=lambda s: s.__class__.__name__)
    pars = sorted(unknowns, key=lambda s: s.name)
    G, b = _split(case['expr'])
    zs = [sym.Dummy('z%d' % i) for i in range(len(funcs))]
    G = G.xreplace(dict(zip(funcs, zs)))
    var = zs + pars
    out = []
    for ia, a in enumerate(var):
        for ib, bb in enumerate(var):
            dG, db = sym.diff(G, a, bb), sym.diff(b, a, bb)
            out.append((ia, ib,
                        None if dG == 0 else sym.lambdify(var, dG, 'numpy'),
                        None if db == 0 else sym.lambdify(var, db, 'numpy')))
    return out


def expected(case, N, free):
    """The independent answer: dense ``(H, A)``, ``H = d2 f / d free^2`` (the
    full symmetric matrix) and ``A`` the sum of the ABSOLUTE values of the
    terms that add into each entry (the basis of the tolerance)."""
    n, q, r = dims(case)
    nz, h = n + q, case['h']
    nf = num_free(case, N)
    H, A = np.zeros((nf, nf)), np.zeros((nf, nf))
    traj = free[:nz*N].reshape(nz, N)
    pars = list(free[nz*N:])
    mid = case['method'] == MID
    pts = np.arange(N - 1)
    at = (traj[:, :-1] + traj[:, 1:])/2 if mid else traj[:, 1:]
    # (node, weight of d point / d node) of every point
    sides = [(pts, 0.5), (pts + 1, 0.5)] if mid else [(pts + 1, 1.0)]

    def index(var, node):
        return var*N + node if var < nz else nz*N + (var - nz) + 0*node

    for a, b, dG, db in _second_partials(case['name']):
        if dG is not None:
            val = h*np.broadcast_to(dG(*(list(at) + pars)), (N - 1,))
            for na, wa in (sides if a < nz else [(pts, 1.0)]):
                for nb, wb in (sides if b < nz else [(pts, 1.0)]):
                    np.add.at(H, (index(a, na), index(b, nb)), wa*wb*val)
                    np.add.at(A, (index(a, na), index(b, nb)),
                              np.abs(wa*wb*val))
        if db is not None:
            val = float(db(*([0.0]*nz + pars)))
            H[index(a, 0), index(b, 0)] += val
            A[index(a, 0), index(b, 0)] += abs(val)
    return H, A


def check(case, N, free, rows, cols, values, factor=1.0):
    """Holds the triplets to the independent answer: lower triangle, in
    range, the SUM of the triplets equal to ``factor * tril(H)`` to ``1e-12``
    (``1e-11`` for parameter-parameter entries: sums over all points) of the
    absolute terms of each entry; structural zeros of the expected matrix
    exactly ``0.0``.  Returns the worst error over its tolerance."""
    import scipy.sparse
    n, q, r = dims(case)
    nf = num_free(case, N)
    rows, cols, values = (np.asarray(a) for a in (rows, cols, values))
    assert rows.shape == cols.shape == values.shape, case['name']
    assert np.all(rows >= cols), case['name']
    assert np.all((cols >= 0) & (rows < nf)), case['name']
    got = scipy.sparse.coo_matrix((values, (rows, cols)),
                                  shape=(nf, nf)).toarray()
    H, A = expected(case, N, free)
    want, A = factor*np.tril(H), abs(factor)*np.tril(A)
    tol = 1e-12*A
    tail = (n + q)*N
    tol[tail:, tail:] = 1e-11*A[tail:, tail:]
    err = np.abs(got - want)
    print('%s N=%d factor=%g: nnz %d, max error %.3g, max error/tolerance '
          '%.3g' % (case['name'], N, factor, len(values), err.max(initial=0),
                    (err[A > 0]/tol[A > 0]).max(initial=0)))
    assert np.all(got[A == 0] == 0.0), case['name']
    assert np.all(err <= tol), (case['name'], float(err.max()))
    return float((err[A > 0]/tol[A > 0]).max(initial=0))


def interpreted(case, N, free, factor=1.0):
    """``(rows, cols, values)`` of the objective Hessian PROGRAM through the
    CPU interpreter (``tests/dag_interp.py``), assembled by its pattern with
    the host's closed-form indices."""
    import dag_interp
    from opty_amd import objective
    states, inputs, unknowns = case['args']
    dag, roots, n, q, r = objective.build_objective_hessian_program(
        case['expr'], states, inputs, unknowns, case['method'], t)
    point_roots, pattern, tail_quad, tail_const, tail_pairs = roots
    nz, h = n + q, case['h']
    base = 1 if case['method'] == BE else 0
    traj = free[:nz*N].reshape(nz, N)

    def values_of(kind, i):
        if kind == 'par':
            return free[nz*N + i]
        off = base + (kind == 'adj')
        return traj[i, off:off + N - 1]
    ones = np.ones(N - 1)
    point = [h*val*ones for val in
             dag_interp.evaluate(dag, list(point_roots), values_of)]
    quad = dag_interp.evaluate(dag, list(tail_quad), values_of)
    const = dag_interp.evaluate(dag, list(tail_const), values_of)
    tail = [h*np.sum(g*ones) + float(b) for g, b in zip(quad, const)]
    rows, cols = objective.objective_hessian_indices(
        pattern, tail_pairs, n, q, N, case['method'])
    values = factor*np.concatenate(point + [np.array(tail, dtype=float)])
    return rows, cols, values


def build_args(case, N):
    states, inputs, unknowns = case['args']
    return dict(objective=case['expr'], state_symbols=states,
                unknown_input_trajectories=inputs,
                unknown_parameters=unknowns, num_collocation_nodes=N,
                integration_method=case['method'], time_symbol=t)


def compile_case(case):
    """``(code object, program)`` of a case (``compile_objective_hessian``)."""
    from opty_amd.objective import compile_objective_hessian
    return compile_objective_hessian(**build_args(case, 20))


@functools.lru_cache(maxsize=None)
def function(name, N, device=0):
    """``(rows, cols, values)`` of ``create_objective_hessian_function`` for
    the case ``name`` (made once per session)."""
    import opty_amd
    case = BY_NAME[name]
    return opty_amd.create_objective_hessian_function(
        node_time_interval=case['h'], device=device, **build_args(case, N))


def pendulum_problem(N=41, method=BE, obj_hessian='device'):
    """A ``Problem`` of the pendulum swing-up (``examples/problems.py``) with
    the symbolic effort objective ``Integral(T(t)**2, t)`` -> ``(problem,
    (rows, cols, values))``; ``obj_hessian='hand'``: the same Hessian from a
    hand-written host callable."""
    import opty_amd
    from examples import problems
    kw = problems.pendulum_swing_up(num_nodes=N, method=method)
    tt = kw['time_symbol']
    torque = sym.Function('T')(tt)
    h = kw['node_time_interval']
    args = (sym.Integral(torque**2, tt), kw['state_symbols'], [torque], [],
            N, h)
    okw = dict(integration_method=method, time_symbol=tt)
    obj, obj_grad = opty_amd.create_objective_function(*args, **okw)
    hess = opty_amd.create_objective_hessian_function(*args, **okw)
    if obj_hessian == 'hand':
        rows, cols, values = hess
        hess = (rows, cols, lambda free: np.asarray(values(free)))
    prob = opty_amd.Problem(obj, obj_grad, obj_hessian=hess, **kw)
    return prob, hess


def prebuild_jobs():
    """Thunks that build the code objects of the objective Hessian tests
    (``__graft_entry__.build`` runs them side by side): one per objective and
    method -- the code does not depend on N -- and the modules of the
    ``Problem`` test."""
    from opty_amd.objective import compile_objective, \
        compile_objective_hessian

    def objgrad():
        # the module of test_c_abi_errors' "missing kernel"
        case = BY_NAME['trig_mid']
        states, inputs, unknowns = case['args']
        compile_objective(case['expr'], states, inputs, unknowns, 20,
                          case['method'], t)

    def one(case):
        compile_case(case)

    def pendulum():
        from examples import problems
        import opty_amd
        kw = problems.pendulum_swing_up(num_nodes=41, method=BE)
        tt = kw['time_symbol']
        torque = sym.Function('T')(tt)
        args = (sym.Integral(torque**2, tt), kw['state_symbols'], [torque],
                [], 41)
        okw = dict(integration_method=BE, time_symbol=tt)
        compile_objective(*args, **okw)
        compile_objective_hessian(*args, **okw)
        col = opty_amd.ConstraintCollocator(**kw)
        col.prebuild()
        col._build_hessian_code_object()
    return [lambda case=case: one(case) for case in CASES] + [pendulum,
                                                              objgrad]
