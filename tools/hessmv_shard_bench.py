"""Times the node-sharded Hessian operator on ONE GPU: ``opty_hip_hessmv_apply``
(the whole problem, device in / device out) and the windows a rank of 2, 4 and
8 multiplies (``opty_hip_hessmv_apply_shard`` from resident values into a
dense rank-local block), a first and a middle window each, all in ONE run --
what one rank of a node-sharded problem spends on a product ``H v``, without
the broadcast of ``v`` and the copy of its slice to the host.  Nothing here
runs on several physical GPUs.

Method of ``tools/hessian_shard_bench.py``: a host clock around ``--iters``
back-to-back enqueues that ends in a device synchronise, repeated ``--rounds``
times with all entries ALTERNATING inside every round; median (minimum ..
maximum) over the rounds.  Reported, not gated.  ``--prebuild`` builds the
code objects (no GPU) and exits.

    python tools/hessmv_shard_bench.py [--problem config3_10link]
        [--worlds 2,4,8] [--iters 30] [--rounds 9] [--out table.txt]
        [--label TEXT] [--prebuild]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--worlds', default='2,4,8')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--label', default='')
    ap.add_argument('--prebuild', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import opty_amd
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.program import hessmv_window_blocks
    from opty_amd.sharded import partition_nodes
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    if args.prebuild:
        col.prebuild()
        _, cut, meta = col._build_hessian_code_object()
        print('%s: built, %d strips' % (args.problem, len(cut)))
        return 0
    import torch
    hess = col.generate_hessian_function()
    handle, hip = col._ensure_hessmv(), col.hip
    prog = col._build_hessian_program()
    N, nfree = col.num_collocation_nodes, col.num_free
    ncn, PH = N - 1, prog.PH
    nrows, ntail = prog.n + prog.q, prog.r + prog.s
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, nfree)
    if col._variable_duration:
        free[-1] = 0.01
    lam = rng.uniform(-1.0, 1.0, col.num_constraints)
    d_free, d_lam, d_v = (torch.from_numpy(x).cuda() for x in (
        free, lam, rng.uniform(-1.0, 1.0, nfree)))
    d_val = hess(d_free, d_lam)     # builds, verifies, installs the knowns
    d_inst = d_val[ncn*PH:] if len(prog.inst_hess_out) else None
    d_y = torch.empty(nfree, dtype=torch.float64, device='cuda')
    d_tail = torch.empty(max(1, ntail), dtype=torch.float64, device='cuda') \
        if ntail else None
    torch.cuda.synchronize()

    def window(a, b):
        # (the rank's resident values: a view from its halo node on; the
        # rank-local block is dense, rows `owned` apart)
        first = a - (1 if a > 0 else 0)
        owned = b - a + (1 if b == ncn else 0)
        values = d_val[first*PH:]
        return lambda: handle.apply_shard(values, d_inst, d_v, d_y, owned,
                                          d_tail, a, b, b == ncn)

    whole = 'whole (hessmv_apply)'
    entries = {whole: (0, ncn), 'whole window': (0, ncn)}
    group = {whole: lambda: handle.apply(d_val, d_v, d_y, hb.DEVICE)}
    for world in (int(x) for x in args.worlds.split(',')):
        ranges = partition_nodes(ncn, world)
        entries['1/%d middle' % world] = ranges[world//2]
        entries['1/%d first' % world] = ranges[0]
    for label, (a, b) in entries.items():
        if label not in group:
            group[label] = window(a, b)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        hip.synchronize()
        return (time.perf_counter() - t0)/args.iters*1e6

    for fn in group.values():           # warm-up: every shape
        for _ in range(3):
            fn()
    hip.synchronize()
    runs = {k: [] for k in group}
    for _ in range(args.rounds):
        for k, fn in group.items():     # alternating inside a round
            runs[k].append(timed(fn))
    med = {k: statistics.median(t) for k, t in runs.items()}
    sides, _ = handle.sides()
    lines = ['%s%s, N = %d (PH = %d, %d instance entries, %d sides); one GPU; '
             '%d rounds of %d calls, alternating'
             % (args.label + ': ' if args.label else '', args.problem, N, PH,
                len(prog.inst_hess_out), len(sides), args.rounds, args.iters),
             '%-22s %8s %7s  %-34s %s' % ('window', 'nodes', 'blocks',
                                          'us per call: median (min .. max)',
                                          'over whole')]
    for k, t in runs.items():
        a, b = entries[k]
        lines.append('%-22s %8d %7d  %9.2f (%9.2f .. %9.2f)%6s %.3f'
                     % (k, b - a, hessmv_window_blocks(N, a, b), med[k],
                        min(t), max(t), '', med[k]/med[whole]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
