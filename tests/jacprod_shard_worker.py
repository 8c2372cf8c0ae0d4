"""One rank of tests/test_jacprod_shard_gpu.py's process tests:

    jacprod_shard_worker.py <backend> <rank> <world> <port> <out.npz>

Every rank builds the variable-duration pendulum of ``jacprod_shard_cases`` as
an ``opty_amd.ShardedProblem`` on ``cuda:0``; rank 0 applies the sharded
Jacobian operator and saves what it got, the others serve until the root's
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
    import jacprod_shard_cases as cases
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    kw = dict(rank=rank, world_size=world)
    if backend == 'nccl':
        kw['device_id'] = torch.device('cuda', 0)
    dist.init_process_group(backend, **kw)
    try:
        torch.cuda.set_device(0)
        prob = opty_amd.ShardedProblem(lambda f: 0.0, lambda f: 0.0*f,
                                       **cases.edge_kwargs('backward euler'))
        assert prob.callbacks._rccl == (backend == 'nccl')
        if rank != 0:
            prob.serve()        # returns after the root's shutdown()
        else:
            free, v, w = cases.draw_inputs(6, prob.collocator)
            _, v2, w2 = cases.draw_inputs(12, prob.collocator)
            con0 = prob.constraints(free)
            op = prob.jacobian_operator(free)
            assert op.shape == (prob.collocator.num_constraints,
                                prob.num_free)
            assert op.dtype == np.float64
            jv, jtw = op.matvec(v), op.rmatvec(w)
            JV = op.matmat(np.stack([v, v2], axis=1))
            JTW = op.rmatmat(np.stack([w, w2], axis=1))
            again = op.matvec(v), op.rmatvec(w)
            # a direction per call, back to back: no rank may read the
            # previous one (a power of two scales the product exactly)
            split = prob.sharded.num_rows*prob.sharded.N
            for k in range(1, 13):
                assert np.array_equal(op.matvec(2.0**k*v), 2.0**k*jv), k
                assert np.array_equal(op.rmatvec(2.0**-k*w)[:split],
                                      2.0**-k*jtw[:split]), k
            con1 = prob.constraints(free)
            np.savez(out, free=free, v=v, w=w, v2=v2, w2=w2, jv=jv, jtw=jtw,
                     JV=JV, JTW=JTW, jv_again=again[0], jtw_again=again[1],
                     con0=con0, con1=con1,
                     ab=np.array([prob.sharded.a, prob.sharded.b]))
            prob.shutdown()
    finally:
        dist.destroy_process_group()
    print('rank %d of %d ok' % (rank, world))


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]),
         sys.argv[5])
