"""CPU tests of the objective's exact Hessian (``opty_amd.objective.
build_objective_hessian_program`` and its emitter): the program through the
DAG interpreter against an independent SymPy answer, the index pattern, the
refusals, and what ``hipcc`` makes of every generated source."""
import numpy as np
import pytest
import sympy as sym

import objective_hessian_cases as ohc
from opty_amd import hip_backend as hb
from opty_amd import objective

NAMES = [case['name'] for case in ohc.CASES]


def _program(case):
    states, inputs, unknowns = case['args']
    return objective.build_objective_hessian_program(
        case['expr'], states, inputs, unknowns, case['method'], ohc.t)


@pytest.mark.parametrize('name', NAMES)
def test_program_against_the_independent_answer(name):
    """Every case at N = 7: the program's values, assembled by its pattern,
    sum to the lower triangle of the SymPy Hessian."""
    case, N = ohc.BY_NAME[name], 7
    free = ohc.make_free(case, N)
    rows, cols, values = ohc.interpreted(case, N, free)
    ohc.check(case, N, free, rows, cols, values)
    rows, cols, values = ohc.interpreted(case, N, free, factor=-2.5)
    ohc.check(case, N, free, rows, cols, values, factor=-2.5)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('N', [2, 7])
def test_host_closed_form_indices(name, N):
    """Lower-triangular and in range at every point, N = 2 included (the
    orientation rule is valid for N >= 2); the layout is entry-major."""
    case = ohc.BY_NAME[name]
    dag, roots, n, q, r = _program(case)
    point_roots, pattern, tail_quad, tail_const, tail_pairs = roots
    rows, cols = objective.objective_hessian_indices(
        pattern, tail_pairs, n, q, N, case['method'])
    E, T = len(point_roots), len(tail_pairs)
    assert rows.dtype == cols.dtype == np.int64
    assert len(rows) == len(cols) == E*(N - 1) + T
    assert np.all(rows >= cols) and np.all(cols >= 0)
    assert np.all(rows < ohc.num_free(case, N))
    base = 1 if case['method'] == ohc.BE else 0
    for e, (rv, ro, cv, co) in enumerate(pattern):
        # orientation: lexicographic on (var, off), parameters last
        assert (rv < 0, rv, ro) >= (cv < 0, cv, co) or rv < 0
        if rv >= 0:
            assert np.array_equal(rows[e*(N - 1):(e + 1)*(N - 1)],
                                  rv*N + np.arange(N - 1) + base + ro)
        assert np.array_equal(cols[e*(N - 1):(e + 1)*(N - 1)],
                              cv*N + np.arange(N - 1) + base + co)
    assert np.all(rows[E*(N - 1):] >= (n + q)*N)


def test_expected_shapes_of_the_cases():
    """E and T of the cases that exist for their shape."""
    def shape(name):
        roots = _program(ohc.BY_NAME[name])[1]
        return len(roots[0]), len(roots[2])
    assert shape('effort_be') == (1, 0)
    assert shape('effort_mid') == (3, 0)
    assert shape('param_only_be') == shape('param_only_mid') == (0, 1)
    assert shape('linear_be') == shape('linear_mid') == (0, 0)
    # x-x, v-x, v-v, u-u, p-u and p-p
    assert shape('trig_be') == (5, 1)
    assert shape('trig_mid') == (3 + 4 + 3 + 3 + 2, 1)


def test_midpoint_pairs_yield_four_and_three_triplets():
    """A pair k != l of trajectory variables: four triplets per point, a pair
    k == l three -- (0,0), (1,1), (1,0) -- all from ONE root; a
    parameter-trajectory pair: both offsets."""
    dag, roots, n, q, r = _program(ohc.BY_NAME['trig_mid'])
    point_roots, pattern = roots[0], roots[1]
    groups = {}
    for node, (rv, ro, cv, co) in zip(point_roots, pattern):
        groups.setdefault((rv, cv), []).append((ro, co, node))
    assert sorted(groups) == [(-1, 2), (0, 0), (1, 0), (1, 1), (2, 2)]
    for (rv, cv), members in groups.items():
        offs = [(ro, co) for ro, co, _ in members]
        if rv < 0:
            assert offs == [(0, 0), (0, 1)]
        elif rv != cv:
            assert offs == [(0, 0), (0, 1), (1, 0), (1, 1)]
        else:
            assert offs == [(0, 0), (1, 1), (1, 0)]
        assert len({node for _, _, node in members}) == 1
    # backward Euler: one triplet per pair
    roots = _program(ohc.BY_NAME['trig_be'])[1]
    assert all(ro == 0 and co == 0 for rv, ro, _, co in roots[1] if rv >= 0)


def test_refusals_are_those_of_the_objective_program():
    t, x, m = ohc.t, ohc.x, ohc.m
    build = objective.build_objective_hessian_program
    first = objective.build_objective_program
    bad = [sym.Integral(sym.Integral(x, t)*x, t),           # nested
           sym.Integral(x**2, (t, 0, 1)),                   # definite limits
           sym.Integral(x**2, t)**2,                        # nonlinear
           x**2]                                            # outside integral
    for expr in bad:
        with pytest.raises(NotImplementedError) as want:
            first(expr, [x], [], [m], time_symbol=t)
        with pytest.raises(NotImplementedError) as got:
            build(expr, [x], [], [m], time_symbol=t)
        assert str(got.value) == str(want.value)
    with pytest.raises(NotImplementedError, match='simpson'):
        build(sym.Integral(x**2, t), [x], [], [m], 'simpson', t)


def _sources():
    out = {}
    for case in ohc.CASES:
        states, inputs, unknowns = case['args']
        source, program = objective.objective_hessian_source(
            case['expr'], states, inputs, unknowns, case['method'], ohc.t)
        out.setdefault(source, (case, program))
    return out


def test_every_generated_source_compiles_clean_for_gfx950():
    """Every distinct source: compiles for gfx950, exports ``opty_objhess``
    and -- only with parameter-parameter entries -- ``opty_objhess_fin``,
    spills no vector register, and does not depend on N."""
    sources = _sources()
    assert len(sources) > 1
    for source, (case, program) in sources.items():
        T = len(program[1][2])
        assert 'atomic' not in source
        assert source.count('__launch_bounds__(64)') == (2 if T else 1)
        hsaco = hb.compile_module(source)
        res = hb.cached_kernel_resources(hsaco)
        assert set(res) == ({'opty_objhess', 'opty_objhess_fin'} if T
                            else {'opty_objhess'}), case['name']
        assert hb.vgpr_spills(hsaco, objective.OBJHESS_KERNELS) == {}
        for kernel in res.values():
            assert kernel['.group_segment_fixed_size'] == 0     # no LDS
        # one code object for every node count
        paths = {objective.compile_objective_hessian(
            **ohc.build_args(case, N))[0] for N in (20, 100003)}
        assert paths == {hsaco}, case['name']
