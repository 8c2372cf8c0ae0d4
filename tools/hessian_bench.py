"""Times ``opty_hip_eval_hess`` (the exact Hessian of the constraint
Lagrangian) at config 3 -- the 10-link pendulum on a cart, N = 100 000 --
with device input and output, and the host callback
(``generate_hessian_function()(free, lagrange)``, host arrays in and out).

Algorithmic bytes: ``8*((n+q)*N + M*(N-1) + PH*(N-1))`` (free read once,
multipliers read once, Hessian values written once); the fraction is of the
8 TB/s HBM peak.  Prints one JSON line.

    python tools/hessian_bench.py [--problem config3_10link] [--iters 50]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    hess = col.generate_hessian_function()
    handle = hess.handle
    prog = col._build_hessian_program()
    N, ncn = col.num_collocation_nodes, col.num_collocation_nodes - 1
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    lam = rng.uniform(-1.0, 1.0, col.num_constraints)
    d_free = torch.from_numpy(free).cuda()
    d_lam = torch.from_numpy(lam).cuda()
    d_out = torch.empty(handle.nnz, dtype=torch.float64, device='cuda')
    hip = col.hip
    for _ in range(5):
        handle.evaluate(d_free, d_lam, d_out, hb.DEVICE)
    hip.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        handle.evaluate(d_free, d_lam, d_out, hb.DEVICE)
    hip.synchronize()
    us = (time.perf_counter() - t0)/args.iters*1e6
    nbytes = 8*((prog.n + prog.q)*N + prog.M*ncn + prog.PH*ncn)
    for _ in range(3):
        hess(free, lam)
    t0 = time.perf_counter()
    reps = max(1, args.iters//10)
    for _ in range(reps):
        hess(free, lam)
    host_us = (time.perf_counter() - t0)/reps*1e6
    print(json.dumps(dict(
        problem=args.problem, N=N, PH=prog.PH,
        strips=col._hessian_meta['strips'], device_us=round(us, 2),
        algorithmic_bytes=nbytes,
        tb_per_s=round(nbytes/us*1e-6, 3),
        fraction_of_8tbs=round(nbytes/us*1e-6/8.0, 3),
        host_callback_us=round(host_us, 1))))


if __name__ == '__main__':
    main()
