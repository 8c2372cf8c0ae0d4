"""What tests/test_hessian_shard_cpu.py and tests/test_hessian_shard_gpu.py
share with ``__graft_entry__.build``: the problems, windows and worlds of the
node-sharded exact Hessian, the problem and objective of the process test,
and the code objects they load."""
import hessian_cases as hc

#: constraint nodes of every problem of the window tests
NCN = 200
#: ``hessian_cases.KERNEL_PROBLEMS``: A -- even PH 52, two tail parameters;
#: C -- PH 30 plus one instance entry, midpoint; E -- odd PH 21, the 8-byte
#: flush
PROBLEMS = ('A', 'C', 'E')
#: two strips; one 3-way partition only
TWO_STRIPS = 'D'
#: windows ``[a, b)`` of the 200 nodes: one node; one node short of, exactly
#: and one past a 64-lane block, from an even and from an odd start; a last
#: block with one valid lane; the last node alone; the whole problem; an
#: empty window
WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (1, 2), (1, 65), (1, 66),
           (63, 127), (64, 128), (64, 200), (137, 200), (199, 200), (0, 200),
           (5, 5)]
#: ranks the 200 nodes are partitioned over (200: one node per rank)
WORLDS = [1, 2, 3, 7, 200]
#: ranks of the process test, which shards problem A
RANKS = 2
PROCESS_PROBLEM = 'A'


def collocator(label, **extra):
    return hc.collocator(label, NCN, **extra)


def process_kwargs():
    return hc.KERNEL_PROBLEMS[PROCESS_PROBLEM](NCN + 1)


def process_objective(kw):
    """``(expression, arguments of create_objective_hessian_function)`` of the
    process test's objective on problem A: the cart force and a state under
    the integral, both unknown masses outside it -- per-point entries and
    parameter-parameter entries."""
    import sympy as sm
    import opty_amd
    col = opty_amd.ConstraintCollocator(**kw)
    t = kw['time_symbol']
    force = col.unknown_input_trajectories[0]
    angle = kw['state_symbols'][1]
    m_a, m_b = col.unknown_parameters
    expr = sm.Integral(force**2 + m_a*sm.cos(angle), t) + m_a**2*m_b
    return expr, dict(
        state_symbols=kw['state_symbols'],
        unknown_input_trajectories=col.unknown_input_trajectories,
        unknown_parameters=col.unknown_parameters,
        num_collocation_nodes=kw['num_collocation_nodes'],
        integration_method=kw['integration_method'], time_symbol=t)


def process_obj_hessian(kw):
    """``obj_hessian`` of the process test (needs a GPU)."""
    import opty_amd
    expr, args = process_objective(kw)
    return opty_amd.create_objective_hessian_function(
        expr, node_time_interval=kw['node_time_interval'], **args)


def prebuild_jobs():
    """Thunks that build the code objects the sharded-Hessian tests load
    (``__graft_entry__.build`` runs them side by side).  The Hessian module
    does not depend on N: one per problem; the problem module per node count
    and launch size (the whole problem, and the halves the two ranks of the
    process test launch); the objective Hessian module of the process
    test."""
    from opty_amd.objective import compile_objective_hessian
    from opty_amd.sharded import partition_nodes

    def windows():
        for label in PROBLEMS + (TWO_STRIPS,):
            col = collocator(label)
            col.prebuild()
            col._build_hessian_code_object()

    def process():
        half = max(b - a for a, b in partition_nodes(NCN, RANKS))
        collocator(PROCESS_PROBLEM, launch_nodes=half).prebuild()
        collocator(PROCESS_PROBLEM, launch_nodes=NCN).prebuild()
        kw = process_kwargs()
        expr, args = process_objective(kw)
        compile_objective_hessian(expr, **args)

    def example():
        from examples import sharded_exact_hessian
        sharded_exact_hessian.prebuild()
    return [windows, process, example]
