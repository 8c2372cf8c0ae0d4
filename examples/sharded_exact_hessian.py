#!/usr/bin/env python
"""The exact Hessian of the Lagrangian of ONE node-sharded problem: a 3-link
pendulum on a cart, minimum effort, as ``opty_amd.ShardedProblem(obj_hessian=
...)`` over the GPUs of a node.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \\
        --master-addr 127.0.0.1 examples/sharded_exact_hessian.py [num_nodes]

Rank 0 plays the solver: it asks for ``hessianstructure()`` and ``hessian(free,
lagrange, obj_factor)`` (IPOPT would, through ``prob.solve(x0)``, once
``cyipopt`` is installed; without ``obj_hessian`` it keeps its limited-memory
quasi-Newton default), the other ranks ``serve()``.  Every rank evaluates the
constraint triplets of its own nodes and returns its slice over its own PCIe
link through one page-locked host vector shared by all processes; the root
alone evaluates the objective's.  The root then
builds a single-GPU ``opty_amd.Problem`` with the same arguments and compares
the two answers: the constraint section bit for bit.
"""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                '..')))

import numpy as np

import opty_amd
from examples import problems

NUM_NODES = 2001
#: worlds whose launch sizes :func:`prebuild` builds the problem module for
WORLDS = (1, 2)


def _kwargs(num_nodes):
    return problems.n_link_cart_pendulum(num_links=3, num_nodes=num_nodes,
                                         interval=0.005)


def _objective(kw):
    """``(expression, arguments of create_objective_hessian_function)``: the
    integral of the squared cart force."""
    import sympy as sm
    col = opty_amd.ConstraintCollocator(**kw)
    t = kw['time_symbol']
    force = col.unknown_input_trajectories[0]
    return sm.Integral(force**2, t), dict(
        state_symbols=kw['state_symbols'],
        unknown_input_trajectories=col.unknown_input_trajectories,
        unknown_parameters=col.unknown_parameters,
        num_collocation_nodes=kw['num_collocation_nodes'],
        integration_method=kw['integration_method'], time_symbol=t)


def prebuild(num_nodes=NUM_NODES):
    """Builds the code objects of the default run (no GPU needed): the
    problem module at the launch size of every world in ``WORLDS``, the
    Hessian module and the objective Hessian module."""
    from opty_amd.objective import compile_objective_hessian
    from opty_amd.sharded import partition_nodes
    kw = _kwargs(num_nodes)
    for world in WORLDS:
        nodes = max(b - a for a, b in partition_nodes(num_nodes - 1, world))
        opty_amd.ConstraintCollocator(launch_nodes=nodes, **kw).prebuild()
    col = opty_amd.ConstraintCollocator(**kw)
    col.prebuild()
    col._build_hessian_code_object()
    expr, args = _objective(kw)
    compile_objective_hessian(expr, **args)


def main():
    import torch
    import torch.distributed as dist
    num_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else NUM_NODES
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    shared_gpu = int(os.environ.get('WORLD_SIZE', 1)) > \
        torch.cuda.device_count()
    if shared_gpu:            # development: several ranks on one GPU
        local %= torch.cuda.device_count()
        dist.init_process_group('gloo')
    else:
        dist.init_process_group('nccl',
                                device_id=torch.device('cuda', local))
    torch.cuda.set_device(local)
    kw = _kwargs(num_nodes)
    expr, args = _objective(kw)
    obj_hessian = opty_amd.create_objective_hessian_function(
        expr, node_time_interval=kw['node_time_interval'], device=local,
        **args)

    def obj(free):
        return float(free @ free)

    def grad(free):
        return 2.0*free

    # (any objective value / gradient: the callbacks shown are the Hessian's)
    prob = opty_amd.ShardedProblem(obj, grad, device=local,
                                   obj_hessian=obj_hessian, **kw)
    if rank != 0:
        prob.serve()
        dist.destroy_process_group()
        return
    rows, cols = prob.hessianstructure()
    rng = np.random.default_rng(3)
    free = rng.uniform(-1.0, 1.0, prob.num_free)
    lagrange = rng.uniform(-1.0, 1.0, prob.num_constraints)
    values = np.array(prob.hessian(free, lagrange, 0.7))
    ncon = prob.sharded.hessian_nnz
    print('%d ranks, N = %d: the Hessian of the Lagrangian has %d triplets '
          '(lower triangle; %d of the constraints, PH = %d per node, %d of '
          'the objective) in %d free variables'
          % (dist.get_world_size(), num_nodes, len(rows), ncon,
             prob.sharded.PH, len(rows) - ncon, prob.num_free))
    assert len(values) == len(rows) == len(cols) and np.all(rows >= cols)
    prob.shutdown()
    dist.destroy_process_group()
    # the same arguments on this rank's GPU alone
    single = opty_amd.Problem(obj, grad, device=local,
                              obj_hessian=obj_hessian, **kw)
    srows, scols = single.hessianstructure()
    want = np.array(single.hessian(free, lagrange, 0.7))
    assert np.array_equal(rows, srows) and np.array_equal(cols, scols)
    same = np.array_equal(values[:ncon].view(np.int64),
                          want[:ncon].view(np.int64))
    print('constraint section bit for bit the single-GPU Problem.hessian: %s; '
          'objective section max difference %.3g'
          % (same, np.abs(values[ncon:] - want[ncon:]).max(initial=0.0)))
    assert same


if __name__ == '__main__':
    main()
