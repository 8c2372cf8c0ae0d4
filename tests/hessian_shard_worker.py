"""One rank of tests/test_hessian_shard_gpu.py's process test:

    hessian_shard_worker.py <backend> <rank> <world> <port> <out.npz>

Every rank builds problem A of ``hessian_shard_cases`` as an
``opty_amd.ShardedProblem`` with a device-backed ``obj_hessian`` on
``cuda:0``; rank 0 asks for the structure and the values of the Hessian of the
Lagrangian and saves what it got, the others serve until the root's
``shutdown()``.  Prints ``rank <r> of <w> ok`` at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np


def main(backend, rank, world, port, out):
    import torch
    import torch.distributed as dist
    import opty_amd
    import hessian_cases as hc
    import hessian_shard_cases as cases
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    kw = dict(rank=rank, world_size=world)
    if backend == 'nccl':
        kw['device_id'] = torch.device('cuda', 0)
    dist.init_process_group(backend, **kw)
    try:
        torch.cuda.set_device(0)
        pkw = cases.process_kwargs()
        prob = opty_amd.ShardedProblem(
            lambda f: 0.0, lambda f: 0.0*f,
            obj_hessian=cases.process_obj_hessian(pkw), **pkw)
        assert prob.callbacks._rccl == (backend == 'nccl')
        # nothing of the Hessian is held before the first call
        assert prob.sharded.hess_local is None
        assert prob.callbacks.hess_host is None
        if rank != 0:
            prob.serve()        # returns after the root's shutdown()
        else:
            free, lam = hc.inputs(31, prob.collocator)
            con0 = prob.constraints(free)
            rows, cols = prob.hessianstructure()
            first = np.array(prob.hessian(free, lam, 0.7))
            # multipliers per call, back to back: no rank may read the
            # previous ones (a power of two scales the values exactly)
            double = np.array(prob.hessian(free, 2.0*lam, 1.4))
            again = np.array(prob.hessian(free, lam, 0.7))
            con1 = prob.constraints(free)
            np.savez(out, free=free, lam=lam, rows=rows, cols=cols,
                     first=first, double=double, again=again, con0=con0,
                     con1=con1, ncon=prob.sharded.hessian_nnz,
                     ab=np.array([prob.sharded.a, prob.sharded.b]))
            prob.shutdown()
    finally:
        dist.destroy_process_group()
    print('rank %d of %d ok' % (rank, world))


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]),
         sys.argv[5])
