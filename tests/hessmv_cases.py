"""What the Hessian-operator test files share: the INDEPENDENT answer --
``scipy.sparse`` on the triplets and the project's index functions, nothing
of the kernel or of its host statement --, the derived tolerance, the index
tables of the cases and the one code object that ``__graft_entry__.build``
prebuilds for them."""
import functools

import numpy as np
import sympy as sm

import hessian_cases as hc
import objective_hessian_cases as ohc

#: N - 1 of the CPU comparison
CPU_EDGES = (1, 2, 63, 64, 65, 127)
#: (label, N - 1) of the GPU block-edge cases: blocks of 64 lanes advance by
#: 63 nodes, so 63 / 64 / 65 and 127 / 128 sit on both sides of a block edge
GPU_EDGES = ([(k, m) for k in 'AE' for m in (1, 2, 63, 64, 65, 127, 128)] +
             [('C', m) for m in (1, 64, 65)] + [('D', m) for m in (65, 129)])
#: node count of the objective-only handle: N - 1 = 129 = 2*63 + 3, three
#: blocks of tail partials
OBJECTIVE_ONLY_NODES = 130


def reference(num_free, rows, cols, values, v):
    """``(y_ref, tol, k)``: ``H = L + L.T - diag(L)`` for ``L`` the sum of
    the triplets, ``y_ref = H v`` in float64 on the host; ``tol_r = 4 (k_r +
    2) 2**-53 (|H| |v|)_r`` with ``k_r`` the number of triplets that touch
    row ``r``."""
    import scipy.sparse as sp
    rows, cols = np.asarray(rows), np.asarray(cols)
    values = np.asarray(values, dtype=float)
    L = sp.coo_matrix((values, (rows, cols)),
                      shape=(num_free, num_free)).tocsr()
    H = (L + L.T - sp.diags(L.diagonal())).tocsr()
    y_ref = H @ v
    k = np.bincount(rows, minlength=num_free) + np.bincount(
        cols[rows != cols], minlength=num_free)
    tol = 4.0*(k + 2)*2.0**-53*(abs(H) @ np.abs(v))
    return y_ref, tol, k


def check(what, y, num_free, rows, cols, values, v):
    """Holds ``y`` to :func:`reference`; no entry is excused and a row that
    no triplet touches is exactly ``0.0``.  Returns the worst error over its
    tolerance."""
    y = np.asarray(y)
    y_ref, tol, k = reference(num_free, rows, cols, values, v)
    assert y.shape == y_ref.shape, what
    err = np.abs(y - y_ref)
    live = tol > 0
    worst = float((err[live]/tol[live]).max(initial=0.0))
    print('%s: %d triplets, %d rows without one, max error %.3g, max '
          'error/tolerance %.3g' % (what, len(values), int((k == 0).sum()),
                                    err.max(initial=0.0), worst))
    assert np.all(np.isfinite(y)), what
    assert np.all(y[k == 0] == 0.0), what
    assert np.all(err <= tol), (what, float(err.max()), worst)
    return worst


@functools.lru_cache(maxsize=None)
def _program(label):
    """Hessian program of a kernel problem without instance constraints (it
    does not depend on N)."""
    return hc.collocator(label, 65)._build_hessian_program()


def node_tables(label, ncn):
    """``(N, n + q, r + s, pattern, rows, cols)`` of the constraint Hessian
    of ``hc.KERNEL_PROBLEMS[label]`` at ``ncn`` constraint nodes, or of a
    named problem of the zoo (then ``ncn`` is None: its own node count)."""
    from opty_amd.codegen.program import hessian_indices
    if label in 'ABDE':
        prog = _program(label)
        rows, cols = hessian_indices(prog, ncn + 1, [])
        N = ncn + 1
    else:
        import opty_amd
        from examples import problems
        col = hc.collocator(label, ncn) if ncn is not None else \
            opty_amd.ConstraintCollocator(**problems.build(label))
        prog = col._build_hessian_program()
        rows, cols = col.hessian_indices_closed_form()
        N = col.num_collocation_nodes
    return (N, prog.n + prog.q, prog.r + prog.s,
            np.array(prog.index_pattern(), dtype=np.int32).reshape(-1, 4),
            rows, cols)


@functools.lru_cache(maxsize=None)
def objective_program(name):
    """``(n + q, r, pattern, tail_pairs, base)`` of an objective case."""
    from opty_amd import objective
    case = ohc.BY_NAME[name]
    states, inputs, unknowns = case['args']
    dag, roots, n, q, r = objective.build_objective_hessian_program(
        case['expr'], states, inputs, unknowns, case['method'], ohc.t)
    pattern, pairs = roots[1], roots[4]
    return (n + q, r, np.array(pattern, dtype=np.int32).reshape(-1, 4),
            np.array(pairs, dtype=np.int64).reshape(-1, 2),
            1 if case['method'] == ohc.BE else 0)


def objective_tables(name, N):
    """... and ``(rows, cols)`` of its values for ``N`` nodes."""
    from opty_amd import objective
    nz, r, pattern, pairs, base = objective_program(name)
    case = ohc.BY_NAME[name]
    n, q, _ = ohc.dims(case)
    return objective.objective_hessian_indices(pattern, pairs, n, q, N,
                                               case['method'])


def carrier_problem(num_nodes=OBJECTIVE_ONLY_NODES):
    """A problem with the sizes of the objective case ``all_mid`` -- two
    states, two unknown input trajectories, three unknown parameters --
    whose handle an objective-only product handle borrows."""
    m, c, k, t = sm.symbols('m, c, k, t')
    x, v, f1, f2 = [s(t) for s in sm.symbols('x, v, f1, f2',
                                             cls=sm.Function)]
    eom = sm.Matrix([x.diff() - v, m*v.diff() + c*v + k*x - f1 - f2])
    return dict(equations_of_motion=eom, state_symbols=(x, v),
                num_collocation_nodes=num_nodes, node_time_interval=0.3,
                time_symbol=t, integration_method='midpoint')


def kkt_problem(num_nodes=20):
    from examples import kkt_minres
    return kkt_minres.problem(num_nodes)


def prebuild_jobs():
    """Thunks that build the code objects of tests/test_hessmv_gpu.py which
    no other list builds (``__graft_entry__.build`` runs them side by side):
    the carrier problem's module and the modules of the example."""
    import opty_amd

    def carrier():
        opty_amd.ConstraintCollocator(**carrier_problem()).prebuild()

    def example():
        from examples import kkt_minres
        kkt_minres.prebuild(20)
    return [carrier, example]
