"""One rank of tests/test_hessmv_shard_gpu.py's process test:

    hessmv_shard_worker.py <backend> <rank> <world> <port> <out.npz>

Every rank builds problem A of ``hessian_shard_cases`` as an
``opty_amd.ShardedProblem`` with a device-backed ``obj_hessian`` on
``cuda:0``; rank 0 applies the resident Hessian operator and saves what it
got, the others serve until the root's ``shutdown()``.  Prints ``rank <r> of
<w> ok`` at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np


def main(backend, rank, world, port, out):
    import pytest
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
        sh, cb = prob.sharded, prob.callbacks
        assert cb._rccl == (backend == 'nccl')
        # nothing of the operator is held before the first load
        assert sh.hmv_values is None and sh._hmv_handle is None
        assert cb.hy_host is None
        with pytest.raises(NotImplementedError, match='hessian_operator'):
            prob.hessian_operator(None, None)
        if rank != 0:
            prob.serve()        # returns after the root's shutdown()
            # the resident values: this rank's nodes and one halo node
            assert sh.hmv_values.numel() == (sh.b - sh.halo_begin)*sh.PH
            assert sh.hess_local is None and cb.hess_host is None
        else:
            free, lam = hc.inputs(31, prob.collocator)
            n = prob.num_free
            v, u = np.random.default_rng(32).uniform(-1.0, 1.0, (2, n))
            con0 = prob.constraints(free)
            # host arrays only, refused before any collective
            with pytest.raises(TypeError, match='host arrays'):
                prob.resident_hessian_operator(
                    torch.from_numpy(free).cuda(), lam)
            op = prob.resident_hessian_operator(free, lam, 0.7)
            assert op.shape == (n, n) and op.dtype == np.float64
            hv, hu = op.matvec(v), op.rmatvec(u)
            HV = op.matmat(np.stack([v, u], axis=1))
            again = op.matvec(v)
            # nothing of the size of the Hessian went to the host
            assert sh.hess_local is None and cb.hess_host is None
            # one set is resident: a second operator replaces the first
            doubled = prob.resident_hessian_operator(free, 2.0*lam, 1.4)
            with pytest.raises(RuntimeError, match='replaced'):
                op.matvec(v)
            hv2 = doubled.matvec(v)
            con1 = prob.constraints(free)
            np.savez(out, free=free, lam=lam, v=v, u=u, hv=hv, hu=hu, HV=HV,
                     again=again, hv2=hv2, con0=con0, con1=con1,
                     ab=np.array([sh.a, sh.b]))
            prob.shutdown()
    finally:
        dist.destroy_process_group()
    print('rank %d of %d ok' % (rank, world))


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]),
         sys.argv[5])
