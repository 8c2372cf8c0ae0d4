"""Times the Hessian operator at config 3 -- the 10-link pendulum on a cart,
N = 100 000, 285 stored entries per node -- on one process, in ONE run:

* (a) device time of K single products ``y = H v`` from the stored triplets
  (``opty_hessmv`` + ``opty_hessmv_fin``, device in / device out), K = 1, 2,
  4, 8, on K distinct columns;
* (b) device time of ONE block product ``Y = H V`` of K columns
  (``opty_hip_hessmv_apply_block``: ``ceil(K / block_width)`` passes of
  ``opty_hessmv_block``), K = 2, 4, 8 -- the yardstick of (b) is (a) at the
  same K, in the same run;
* (c) device time of ``opty_hess`` of the same problem, for scale;
* (d) the host alternative: ``hessian(free, lagrange)`` to NumPy, then ``L =
  coo_matrix(triplets)``, ``H = L + L.T - diag(L)``, ``H @ v`` on the CPU
  (the first ``--host-rounds`` rounds only: it takes seconds).

(a) to (c): a host clock around ``--iters`` back-to-back enqueues that ends
in a device synchronise; (d): one call.  ``--rounds`` rounds that ALTERNATE
all of them; median (min .. max) over the rounds.  Algorithmic bytes of a
product: the node section read once, ``v`` read and ``y`` written; a block
product reads the node section once per pass.  Every column of the block
products must have the bits of its single product.  Reported, not gated.

    python tools/hessmv_bench.py [--problem config3_10link] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TB_PER_S = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--host-rounds', type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    hess = col.generate_hessian_function()
    hmv = col.generate_hessian_product_function()
    rows, cols = col.hessian_indices_closed_form()
    hip, N, nfree = col.hip, col.num_collocation_nodes, col.num_free
    PH = col._build_hessian_program().PH
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, nfree)
    lam = rng.uniform(-1.0, 1.0, col.num_constraints)
    v = rng.uniform(-1.0, 1.0, nfree)
    d_free, d_lam, d_v = (torch.from_numpy(x).cuda() for x in (free, lam, v))
    d_val = hess(d_free, d_lam)
    d_y = torch.empty(nfree, dtype=torch.float64, device='cuda')
    # the columns of the block products: row c of a (K, num_free) tensor
    widths = (2, 4, 8)
    V = rng.uniform(-1.0, 1.0, (max(widths), nfree))
    V[0] = v
    d_V = torch.from_numpy(V).cuda()
    d_Y = torch.empty_like(d_V)
    d_Y1 = torch.empty_like(d_V)
    handle = hmv.handle
    d_out = torch.empty_like(d_val)
    torch.cuda.synchronize()
    col.sync_known()

    def host_alternative():
        values = hess(free, lam)
        L = sp.coo_matrix((values, (rows, cols)), shape=(nfree, nfree)).tocsr()
        return (L + L.T - sp.diags(L.diagonal())) @ v

    def enqueued(fn):
        def run():
            for _ in range(args.iters):
                fn()
            hip.synchronize()
            return args.iters
        return run

    def once():
        host_alternative()
        return 1

    def singles(K):
        def run():
            for c in range(K):
                handle.apply(d_val, d_V[c], d_Y1[c], hb.DEVICE)
        return run

    def block(K):
        return lambda: handle.apply_block(d_val, d_V, nfree, d_Y, nfree, K,
                                          hb.DEVICE)
    group = dict(
        hessmv=enqueued(lambda: handle.apply(d_val, d_v, d_y, hb.DEVICE)))
    for K in widths:
        group['singles_%d' % K] = enqueued(singles(K))
        group['block_%d' % K] = enqueued(block(K))
    group.update(
        opty_hess=enqueued(lambda: hess.handle.evaluate(d_free, d_lam, d_out,
                                                        hb.DEVICE)),
        host_alternative=once)
    for fn in group.values():             # warm-up: every path once
        fn()
    # every column of the widest block product: the bits of its single one
    same_bits = bool(torch.equal(d_Y.view(torch.int64),
                                 d_Y1.view(torch.int64)))
    runs = {k: [] for k in group}
    for r in range(args.rounds):
        for k, fn in group.items():       # alternating inside a round
            if k == 'host_alternative' and r >= args.host_rounds:
                continue
            t0 = time.perf_counter()
            count = fn()
            runs[k].append((time.perf_counter() - t0)/count*1e6)
    out = {k: dict(median_us=round(statistics.median(t), 1),
                   min_us=round(min(t), 1), max_us=round(max(t), 1))
           for k, t in runs.items()}
    # the product is the reference's to rounding
    y_ref = host_alternative()
    err = float(np.abs(d_y.cpu().numpy() - y_ref).max())
    nbytes = 8*(PH*(N - 1) + 2*nfree)
    tbs = nbytes/out['hessmv']['median_us']*1e-6
    sides, ntraj = hmv.handle.sides()
    Kb = handle.block_width
    blocks = {}
    for K in widths:
        one, many = out['singles_%d' % K], out['block_%d' % K]
        passes = -(-K//Kb)
        moved = 8*(passes*PH*(N - 1) + 2*K*nfree)
        blocks[K] = dict(
            passes=passes, block_over_singles=round(
                many['median_us']/one['median_us'], 3),
            algorithmic_bytes=moved,
            tb_per_s=round(moved/many['median_us']*1e-6, 3))
    print('%-18s %12s   (%s .. %s) us' % ('', 'median', 'min', 'max'))
    for k, t in out.items():
        print('%-18s %12.1f   (%.1f .. %.1f)' % (k, t['median_us'],
                                                 t['min_us'], t['max_us']))
    for K in widths:
        print('block_%d / singles_%d = %.3f   (%d passes of at most %d '
              'columns)' % (K, K, blocks[K]['block_over_singles'],
                            blocks[K]['passes'], Kb))
    print(json.dumps(dict(
        problem=args.problem, N=N, PH=PH, num_free=nfree, sides=len(sides),
        lds_bytes_per_block=64*33*8 + len(sides)*2*64*8,
        block_width=Kb,
        lds_bytes_per_block_of_a_pass={
            w: 64*33*8 + len(sides)*w*2*64*8 for w in range(2, Kb + 1)},
        block_columns_have_the_bits_of_the_single_products=same_bits,
        block_products=blocks,
        iters=args.iters, rounds=args.rounds, times=out,
        algorithmic_bytes=nbytes, tb_per_s=round(tbs, 3),
        fraction_of_peak=round(tbs/PEAK_TB_PER_S, 4),
        hessmv_over_opty_hess=round(out['hessmv']['median_us'] /
                                    out['opty_hess']['median_us'], 3),
        max_abs_difference_from_host=err)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
