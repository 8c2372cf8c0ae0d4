"""Times the matrix-free Jacobian products at config 3 -- the 10-link
pendulum on a cart, N = 100 000 -- on one process, next to the Jacobian they
replace, all in ONE run:

* device times of ``opty_jvp``, of ``opty_vjp`` + ``opty_vjp_fin`` and of the
  Jacobian evaluation (``opty_hip_eval_jac``, device in / device out): a host
  clock around ``--iters`` back-to-back enqueues that ends in a device
  synchronise, repeated ``--rounds`` times with the three ALTERNATING inside
  every round (median, minimum and maximum over the rounds);
* host-path times of ``jvp(free, v)`` / ``vjp(free, w)`` beside
  ``jacobian(free)`` (host arrays in and out: they depend on the box's PCIe
  link; reported, not gated).

Algorithmic bytes of a product: ``free`` and one vector read, one vector
written.  Exits non-zero when a product is not faster than the Jacobian.

    python tools/jacprod_bench.py [--problem config3_10link] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=9)
    args = ap.parse_args()
    import numpy as np
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    jac = col.generate_jacobian_function()
    handle, hip = jvp.handle, col.hip
    N = col.num_collocation_nodes
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    v = rng.uniform(-1.0, 1.0, col.num_free)
    w = rng.uniform(-1.0, 1.0, col.num_constraints)
    d_free, d_v, d_w = (torch.from_numpy(x).cuda() for x in (free, v, w))
    d_jv = torch.empty(col.num_constraints, dtype=torch.float64, device='cuda')
    d_jtw = torch.empty(col.num_free, dtype=torch.float64, device='cuda')
    d_jac = torch.empty(hip.nnz, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    device = dict(
        opty_jvp=lambda: handle.jvp(d_free, d_v, d_jv, hb.DEVICE),
        opty_vjp_fin=lambda: handle.vjp(d_free, d_w, d_jtw, hb.DEVICE),
        opty_jac=lambda: hip.eval_jac(d_free, d_jac, hb.DEVICE))
    host = dict(jvp=lambda: jvp(free, v), vjp=lambda: vjp(free, w),
                jacobian=lambda: jac(free))

    def timed(fn, iters, sync):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        if sync:
            hip.synchronize()
        return (time.perf_counter() - t0)/iters*1e6

    def measure(group, iters, sync):
        for fn in group.values():         # warm-up: every shape, every path
            timed(fn, 3, sync)
        runs = {k: [] for k in group}
        for _ in range(args.rounds):
            for k, fn in group.items():   # alternating inside a round
                runs[k].append(timed(fn, iters, sync))
        return {k: dict(median_us=round(statistics.median(t), 2),
                        min_us=round(min(t), 2), max_us=round(max(t), 2))
                for k, t in runs.items()}

    dev = measure(device, args.iters, True)
    hst = measure(host, max(1, args.iters//10), False)
    nfree, ncon = col.num_free, col.num_constraints
    nbytes = dict(opty_jvp=8*(2*nfree + ncon), opty_vjp_fin=8*(2*nfree + ncon),
                  opty_jac=8*(nfree + hip.nnz))
    for k, b in nbytes.items():
        dev[k]['algorithmic_bytes'] = b
        dev[k]['tb_per_s'] = round(b/dev[k]['median_us']*1e-6, 3)
    base = dev['opty_jac']['median_us']
    meta = col._jacprod_meta
    out = dict(
        problem=args.problem, N=N, iters=args.iters, rounds=args.rounds,
        jvp_strips=meta['jvp_strips'], vjp_strips=meta['vjp_strips'],
        device=dev, host_path=hst,
        jvp_over_jac=round(dev['opty_jvp']['median_us']/base, 4),
        vjp_over_jac=round(dev['opty_vjp_fin']['median_us']/base, 4),
        jacobian_kernel=str(hip.routing().get('flavour')))
    print(json.dumps(out))
    ok = dev['opty_jvp']['median_us'] < base and \
        dev['opty_vjp_fin']['median_us'] < base
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
