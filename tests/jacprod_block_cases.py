"""What tests/test_jacprod_block_cpu.py and tests/test_jacprod_block_gpu.py
share with ``__graft_entry__.build``: the problem lists of the block products
``J V`` / ``J^T W`` and the code objects they load."""
from test_hessian_cpu import _nonlinear_instance_pendulum

from examples import problems

#: the problems of tests/test_jacprod_gpu.py (parity per problem)
PARITY = ['msd_be_small', 'msd_mid_small', 'vardur_pendulum_small',
          'pend2_link_vardur_unkmass_small', 'config2_pendulum_small',
          'config3_10link_small', 'piecewise_be_small', 'c99_be_small',
          'biped_small', 'biped_mid_small', 'one_legged_small',
          'implicit_traj_be_small', 'implicit_traj_mid_small']
#: problems with tail columns (partials per column): every column count
TAILED = ['vardur_pendulum_small', 'pend2_link_vardur_unkmass_small']
#: column counts of TAILED: none, the single path, partial and full passes of
#: either width, a full pass and a remainder, two full passes
COLUMN_COUNTS = [0, 1, 2, 3, 4, 5, 7, 8]
#: N of the variable-duration pendulum: ``N - 1`` below, at and off the
#: multiples of 63 and 64, and the smallest
EDGE_NODES = [2, 3, 64, 65, 127, 128, 130, 200]
EDGE_METHODS = ['backward euler', 'midpoint']
#: the modules the CPU test cross-compiles
CROSS_COMPILED = ['config3_10link_small', 'vardur_pendulum_small',
                  'biped_small']
#: node count of the nonlinear-instance pendulum
INSTANCE_NODES = 11


def collocator(name, **extra):
    import opty_amd
    if name == 'nonlinear_instance':
        kw = _nonlinear_instance_pendulum(num_nodes=INSTANCE_NODES)
    else:
        kw = problems.build(name)
    return opty_amd.ConstraintCollocator(**dict(kw, **extra))


def edge_collocator(num_nodes, method):
    import opty_amd
    return opty_amd.ConstraintCollocator(
        **problems.variable_duration_pendulum(num_nodes=num_nodes,
                                              method=method))


def _prebuild(col):
    col.prebuild()
    col._build_jacprod_code_object()
    col._build_jacprod_block_code_object()


def prebuild_jobs():
    """Thunks that build the code objects the block-product tests load
    (``__graft_entry__.build`` runs them side by side): per problem the
    problem module, the single product module and the block module.  The
    module sources do not depend on N: one build per method serves every
    node count of the edge cases."""
    def small():
        for name in PARITY + ['nonlinear_instance']:
            if name not in ('biped_small', 'biped_mid_small',
                            'one_legged_small'):
                _prebuild(collocator(name))
        for method in EDGE_METHODS:
            for num_nodes in EDGE_NODES:
                col = edge_collocator(num_nodes, method)
                col.prebuild()
                if num_nodes == EDGE_NODES[0]:
                    _prebuild(col)

    def large(name):
        return lambda: _prebuild(collocator(name))

    def example():
        from examples import jacobian_sketch
        jacobian_sketch.prebuild()
    return [small, example] + [large(name) for name in (
        'biped_small', 'biped_mid_small', 'one_legged_small')]


def interpreted_block(col, free, V, W, width):
    """``(J V, J^T W, bounds of J V, bounds of J^T W)`` through the NumPy
    interpreter of the program the device runs: for ``width`` > 1 the block
    program of that width, pass by pass (a short pass repeats its first
    column, as the kernels' clamped loads do); for width 1, or one column,
    the single program.  Bounds in units of round-off, assembled like the
    values."""
    import numpy as np
    import dag_interp
    from test_jacprod_cpu import interpreted_products
    from opty_amd.codegen.program import assemble_jvp, assemble_vjp
    k = V.shape[1]
    out = [np.zeros((n, k)) for n in (col.num_constraints, col.num_free)*2]
    if width == 1 or k == 1:
        for c in range(k):
            for dst, src in zip(out, interpreted_products(
                    col, free, V[:, c], W[:, c], with_bounds=True)):
                dst[:, c] = src
        return out
    prog = col._build_jacprod_block_program(width)
    N = col.num_collocation_nodes
    nodes = np.arange(N - 1)
    atoms = col._atom_free_index()
    ev = dag_interp.evaluate_with_error_bound
    for c0 in range(0, k, width):
        pick = [c0 + c if c0 + c < k else c0 for c in range(width)]
        fin = col._jacprod_block_inputs(free, V[:, pick], nodes, 'jvp')
        rin = col._jacprod_block_inputs(free, W[:, pick], nodes, 'vjp')
        inst, ib = ev(prog.dag, prog.inst_jac_out, fin)
        inst = [float(x) for x in inst]
        ib = [abs(float(x)) for x in ib]
        for c in range(min(width, k - c0)):
            tan, tb = ev(prog.dag, prog.tan_out[c], fin)
            adj, ab = ev(prog.dag, prog.adj_out[c], rin)
            v, w = V[:, c0 + c], W[:, c0 + c]
            out[0][:, c0 + c] = assemble_jvp(prog, N, tan, inst, v, atoms)
            out[1][:, c0 + c] = assemble_vjp(prog, N, adj, inst, w, atoms)
            out[2][:, c0 + c] = assemble_jvp(
                prog, N, [np.abs(x) for x in tb], ib, np.abs(v), atoms)
            out[3][:, c0 + c] = assemble_vjp(
                prog, N, [np.abs(x) for x in ab], ib, np.abs(w), atoms)
    return out
