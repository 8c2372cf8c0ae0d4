"""Times the block products ``J V`` and ``J^T W`` at config 3 -- the 10-link
pendulum on a cart, N = 100 000 -- device to device, for k = 2, 4 and 8
columns, next to their yardstick in the SAME process: k single products
through the unchanged ``opty_jvp`` / ``opty_vjp``.

A host clock around ``--iters`` back-to-back enqueues that ends in a device
synchronise, repeated ``--rounds`` times with ALL entries alternating inside
every round; median (minimum .. maximum) over the rounds, microseconds per
call (a call: all k columns).  Reported, not gated.

    python tools/jacprod_block_bench.py [--problem config3_10link]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COLUMNS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=9)
    args = ap.parse_args()
    import numpy as np
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    jvp = col.generate_jvp_function()
    jmm = col.generate_jvp_block_function()
    single, block, hip = jvp.handle, jmm.handle, col.hip
    if block is None:
        print(json.dumps(dict(problem=args.problem, width=1,
                              tried=col._jacprod_block_meta['tried'])))
        return 0
    nfree, ncon = col.num_free, col.num_constraints
    kmax = max(COLUMNS)
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, nfree)
    d_free = torch.from_numpy(free).cuda()
    # column-major blocks: column c is row c of these
    d_V = torch.from_numpy(rng.uniform(-1.0, 1.0, (kmax, nfree))).cuda()
    d_W = torch.from_numpy(rng.uniform(-1.0, 1.0, (kmax, ncon))).cuda()
    d_Y = torch.empty((kmax, ncon), dtype=torch.float64, device='cuda')
    d_G = torch.empty((kmax, nfree), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    def singles(call, X, out, k):
        def run():
            for c in range(k):
                call(d_free, X[c], out[c], hb.DEVICE)
        return run

    entries = {}
    for k in COLUMNS:
        entries['jvp_block k=%d' % k] = lambda k=k: block.jvp_block(
            d_free, d_V, nfree, d_Y, ncon, k, hb.DEVICE)
        entries['jvp singles k=%d' % k] = singles(single.jvp, d_V, d_Y, k)
        entries['vjp_block k=%d' % k] = lambda k=k: block.vjp_block(
            d_free, d_W, ncon, d_G, nfree, k, hb.DEVICE)
        entries['vjp singles k=%d' % k] = singles(single.vjp, d_W, d_G, k)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        hip.synchronize()
        return (time.perf_counter() - t0)/args.iters*1e6

    for fn in entries.values():           # warm-up: every shape, every path
        fn()
        fn()
    hip.synchronize()
    runs = {name: [] for name in entries}
    for _ in range(args.rounds):
        for name, fn in entries.items():  # alternating inside a round
            runs[name].append(timed(fn))
    stats = {name: dict(median_us=round(statistics.median(t), 2),
                        min_us=round(min(t), 2), max_us=round(max(t), 2))
             for name, t in runs.items()}
    ratios = {}
    for k in COLUMNS:
        for which in ('jvp', 'vjp'):
            ratios['%s k=%d' % (which, k)] = round(
                stats['%s_block k=%d' % (which, k)]['median_us'] /
                stats['%s singles k=%d' % (which, k)]['median_us'], 4)
    bmeta, smeta = col._jacprod_block_meta, col._jacprod_meta
    res = hb.cached_kernel_resources(bmeta['hsaco'])
    print(json.dumps(dict(
        problem=args.problem, N=col.num_collocation_nodes, iters=args.iters,
        rounds=args.rounds, width=bmeta['width'],
        block_strips=[bmeta['jvp_strips'], bmeta['vjp_strips']],
        block_strip_ops=bmeta['strip_ops'], block_forget=bmeta['forget'],
        single_strips=[smeta['jvp_strips'], smeta['vjp_strips']],
        vgprs={name: [res[name]['.vgpr_count'],
                      res[name].get('.agpr_count', 0)]
               for name in col._JACPROD_BLOCK_KERNELS},
        device=stats, block_over_singles=ratios)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
