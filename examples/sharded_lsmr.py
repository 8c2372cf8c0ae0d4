#!/usr/bin/env python
"""``examples/feasible_guess_lsmr.py`` on a node-sharded problem: Gauss-Newton
steps ``dx = lsmr(J, -c)`` on the 1-link pendulum swing-up, where ``J`` is the
matrix-free operator of ``ShardedProblem.jacobian_operator(free)`` -- every
``matvec`` (``J v``) and ``rmatvec`` (``J^T w``) is evaluated by all ranks,
each on its window of the constraint nodes, and only vectors of ``num_free``
doubles at the most cross PCIe.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \\
        --master-addr 127.0.0.1 examples/sharded_lsmr.py [num_nodes]

Rank 0 iterates and prints ``||c||`` per iteration; the other ranks
``serve()``.  With more ranks than GPUs (development: several ranks on one
GPU) the rendezvous is gloo.  Exits non-zero if the norm did not fall."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                '..')))

import numpy as np

import opty_amd
from examples import problems

#: node count of the default run, and the world sizes whose launch sizes
#: :func:`prebuild` compiles the problem module for
NUM_NODES = 101
WORLDS = (1, 2)


def _kwargs(num_nodes):
    return problems.pendulum_swing_up(num_nodes=num_nodes, duration=10.0)


def prebuild(num_nodes=NUM_NODES):
    """Builds the code objects of the default run (no GPU needed): the
    problem module at the launch size of every world in ``WORLDS`` and the
    product module."""
    from opty_amd.sharded import partition_nodes
    for world in WORLDS:
        nodes = max(b - a for a, b in partition_nodes(num_nodes - 1, world))
        col = opty_amd.ConstraintCollocator(launch_nodes=nodes,
                                            **_kwargs(num_nodes))
        col.prebuild()
    col._build_jacprod_code_object()


def iterate(prob, num_nodes, iterations=6, verbose=True):
    """The root's side: ``(free, norms)``."""
    from scipy.sparse.linalg import lsmr
    free = np.zeros(prob.num_free)
    free[:num_nodes] = np.linspace(0.0, np.pi, num_nodes)
    norms = []
    for it in range(iterations + 1):
        c = np.array(prob.constraints(free))
        norms.append(float(np.linalg.norm(c)))
        if verbose:
            print('iteration %d: ||c|| = %.6e' % (it, norms[-1]))
        if it == iterations or norms[-1] < 1e-10:
            break
        J = prob.jacobian_operator(free)
        dx = lsmr(J, -c, atol=1e-12, btol=1e-12, maxiter=4*prob.num_free)[0]
        free = free + dx
    return free, norms


def main():
    import torch
    import torch.distributed as dist
    num_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else NUM_NODES
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    os.environ.setdefault('WORLD_SIZE', '1')
    os.environ.setdefault('RANK', '0')
    if int(os.environ['WORLD_SIZE']) > torch.cuda.device_count():
        local %= torch.cuda.device_count()
        dist.init_process_group('gloo')
    else:
        dist.init_process_group('nccl',
                                device_id=torch.device('cuda', local))
    torch.cuda.set_device(local)
    prob = opty_amd.ShardedProblem(lambda free: float(free @ free),
                                   lambda free: 2.0*free, device=local,
                                   **_kwargs(num_nodes))
    norms = [1.0, 0.0]
    try:
        if rank != 0:
            prob.serve()
        else:
            _, norms = iterate(prob, num_nodes)
            prob.shutdown()
    finally:
        dist.destroy_process_group()
    return norms


if __name__ == '__main__':
    norms = main()
    sys.exit(0 if norms[-1] < norms[0] else 1)
