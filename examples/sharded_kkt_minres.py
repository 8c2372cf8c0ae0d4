#!/usr/bin/env python
"""The Newton step of examples/kkt_minres.py over the GPUs of a node: the same
pendulum swing-up with the effort objective, as ONE node-sharded problem whose
KKT operator

    [[H, J^T],     H = obj_factor d2 f + sum_k lagrange_k d2 c_k
     [J,  0 ]]     J = d c / d free

is built from ``ShardedProblem.resident_hessian_operator`` (H v from values
that stay in every rank's device memory) and ``ShardedProblem.
jacobian_operator`` and handed to ``scipy.sparse.linalg.minres`` on rank 0.  A
product moves ``num_free`` / ``num_constraints`` doubles each way; nothing of
the size of a matrix leaves a device.  Prints the residual history.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \\
        --master-addr 127.0.0.1 examples/sharded_kkt_minres.py [num_nodes]

``OPTY_HISTORY=<file.npy>``: rank 0 also saves the history there.
"""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__),
                                                '..')))

import numpy as np

from examples import kkt_minres

NUM_NODES = 20
#: worlds whose launch sizes :func:`prebuild` builds the problem module for
WORLDS = (1, 2)


def prebuild(num_nodes=NUM_NODES):
    """Builds the code objects of the default run (no GPU needed): what
    ``kkt_minres.prebuild`` builds, and the problem module at the launch size
    of every world in ``WORLDS``."""
    import opty_amd
    from opty_amd.sharded import partition_nodes
    kkt_minres.prebuild(num_nodes)
    kw = kkt_minres._arguments(num_nodes)[0]
    for world in WORLDS:
        nodes = max(b - a for a, b in partition_nodes(num_nodes - 1, world))
        opty_amd.ConstraintCollocator(launch_nodes=nodes, **kw).prebuild()


def problem(num_nodes=NUM_NODES, device=0):
    """The ``ShardedProblem`` of ``kkt_minres.problem``; every rank builds
    it."""
    import opty_amd
    kw, args, okw = kkt_minres._arguments(num_nodes)
    obj, obj_grad = opty_amd.create_objective_function(*args, **okw)
    hess = opty_amd.create_objective_hessian_function(*args, device=device,
                                                      **okw)
    return opty_amd.ShardedProblem(obj, obj_grad, obj_hessian=hess,
                                   device=device, **kw)


def kkt_operator(prob, free, lagrange, obj_factor=1.0):
    """``(K, H, J)`` as ``kkt_minres.kkt_operator``, every product served by
    all ranks."""
    from scipy.sparse.linalg import LinearOperator
    H = prob.resident_hessian_operator(free, lagrange, obj_factor)
    J = prob.jacobian_operator(free)
    n, m = prob.num_free, prob.num_constraints

    def matvec(z):
        z = np.asarray(z, dtype=float).reshape(-1)
        x, w = z[:n], z[n:]
        return np.concatenate((H.matvec(x) + J.rmatvec(w), J.matvec(x)))
    K = LinearOperator((n + m, n + m), dtype=np.float64, matvec=matvec,
                       rmatvec=matvec)
    return K, H, J


def newton_step(prob, maxiter=400, verbose=True):
    """Rank 0: ``kkt_minres.main``'s step on the sharded problem."""
    from scipy.sparse.linalg import minres
    rng = np.random.default_rng(0)
    free = 0.1*rng.standard_normal(prob.num_free)
    lagrange = np.zeros(prob.num_constraints)
    K, H, J = kkt_operator(prob, free, lagrange)
    rhs = -np.concatenate((prob.gradient(free) + J.rmatvec(lagrange),
                           prob.constraints(free)))
    history = []

    def callback(z):
        history.append(float(np.linalg.norm(K.matvec(z) - rhs)))
        if verbose and (len(history) % 20 == 1):
            print('iteration %4d   |K z - rhs| = %.3e'
                  % (len(history), history[-1]))
    step, info = minres(K, rhs, maxiter=maxiter, callback=callback)
    if verbose:
        print('minres: info %d after %d iterations, |rhs| = %.3e, final '
              'residual %.3e' % (info, len(history), np.linalg.norm(rhs),
                                 history[-1] if history else float('nan')))
    return step, history


def main():
    import torch
    import torch.distributed as dist
    num_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else NUM_NODES
    maxiter = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29500')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    shared_gpu = int(os.environ['WORLD_SIZE']) > torch.cuda.device_count()
    if shared_gpu:            # development: several ranks on one GPU
        local %= torch.cuda.device_count()
        dist.init_process_group('gloo')
    else:
        dist.init_process_group('nccl',
                                device_id=torch.device('cuda', local))
    torch.cuda.set_device(local)
    prob = problem(num_nodes, local)
    if rank != 0:
        prob.serve()
        dist.destroy_process_group()
        return
    print('%d ranks, N = %d: KKT system of %d + %d unknowns'
          % (dist.get_world_size(), num_nodes, prob.num_free,
             prob.num_constraints))
    step, history = newton_step(prob, maxiter)
    if os.environ.get('OPTY_HISTORY'):
        np.save(os.environ['OPTY_HISTORY'], np.array(history))
    prob.shutdown()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
