"""What tests/test_jacprod_shard_cpu.py and tests/test_jacprod_shard_gpu.py
share with ``__graft_entry__.build``: the problem and window lists of the
node-sharded Jacobian products and the code objects they load."""
import numpy as np

from jacprod_block_cases import collocator

from examples import problems

#: the window tests' problem: the variable-duration pendulum (free ``h`` and an
#: unknown parameter: tail columns; instance constraints at both ends) at
#: ``N - 1`` = 200 constraint nodes
EDGE_NODES = 201
EDGE_METHODS = ['backward euler', 'midpoint']
#: windows ``[a, b)`` of the 200 constraint nodes: the first node alone, one
#: node short of / exactly / one past a block from either start (blocks of
#: ``opty_jvp`` hold 64 nodes, of ``opty_vjp`` 63 behind a halo node), windows
#: that end with the trajectory (they own time node N - 1), the last node
#: alone, the whole problem and an empty window
WINDOWS = [(0, 1), (0, 63), (0, 64), (1, 2), (1, 64), (1, 65), (62, 126),
           (63, 127), (64, 200), (137, 200), (199, 200), (0, 200), (5, 5)]
#: ranks the 200 nodes are partitioned over (200: one node per rank)
WORLDS = [1, 2, 3, 7, 200]
#: one 3-way partition each: midpoint (lo and hi swapped), two tail columns,
#: instance atoms at both ends (owned by different ranks), known trajectories
#: of ``free``, the largest row count, several strips and ``forget`` builds
COVERAGE = ['msd_mid_small', 'pend2_link_vardur_unkmass_small',
            'config2_pendulum_small', 'nonlinear_instance',
            'implicit_traj_be_small', 'config3_10link_small', 'biped_small']
#: problems of the NumPy model of the windowed sums (CPU)
MODELLED = ['msd_be_small', 'msd_mid_small',
            'pend2_link_vardur_unkmass_small', 'config2_pendulum_small']
#: ranks of the process tests, and the problem they shard
RANKS = 2


def edge_kwargs(method):
    return problems.variable_duration_pendulum(num_nodes=EDGE_NODES,
                                               method=method)


def edge_collocator(method, **extra):
    import opty_amd
    return opty_amd.ConstraintCollocator(**dict(edge_kwargs(method),
                                                **extra))


def owned(a, b, N):
    """Time nodes ``[a, end)`` the window ``[a, b)`` of an ``N``-node problem
    owns in ``J^T w``: its own, and node ``N - 1`` behind the last constraint
    node."""
    return a, b + (1 if b == N - 1 and b > a else 0)


def draw_inputs(seed, col):
    """``(free, v, w)`` as tests/test_jacprod_gpu.py draws them."""
    from test_jacprod_cpu import draw
    rng = np.random.default_rng(seed)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.02
    return free, draw(rng, col.num_free), draw(rng, col.num_constraints)


def prebuild_jobs():
    """Thunks that build the code objects the sharded-product tests load
    (``__graft_entry__.build`` runs them side by side).  The product modules
    do not depend on N: one per problem and method; the problem module per
    node count and launch size (the whole problem, and the halves the two
    ranks of the process tests launch)."""
    from opty_amd.sharded import partition_nodes

    def edges():
        for method in EDGE_METHODS:
            col = edge_collocator(method)
            col.prebuild()
            col._build_jacprod_code_object()
            half = max(b - a for a, b in partition_nodes(EDGE_NODES - 1,
                                                         RANKS))
            edge_collocator(method, launch_nodes=half).prebuild()
            edge_collocator(method, launch_nodes=EDGE_NODES - 1).prebuild()

    def coverage():
        for name in COVERAGE:
            col = collocator(name)
            col.prebuild()
            col._build_jacprod_code_object()

    def example():
        from examples import sharded_lsmr
        sharded_lsmr.prebuild()
    return [edges, coverage, example]
