"""Times the node-sharded Jacobian products on ONE GPU: the whole products
and the windows a rank of 2, 4 and 8 evaluates (``opty_hip_jacprod_jvp_shard``
/ ``opty_hip_jacprod_vjp_shard``, device in / device out into dense rank-local
blocks), all in ONE run -- what one rank of a node-sharded problem spends on a
product, without the exchange.

Method of ``tools/jacprod_bench.py``: a host clock around ``--iters``
back-to-back enqueues that ends in a device synchronise, repeated ``--rounds``
times with all entries ALTERNATING inside every round; median (minimum ..
maximum) over the rounds.  A window of ``J^T w`` that does not start the
trajectory evaluates one halo node more than it owns: the middle rank's
window (with the halo) stands next to rank 0's (without) at every world size.

    python tools/jacprod_shard_bench.py [--problem config3_10link]
        [--worlds 2,4,8] [--iters 30] [--rounds 9] [--out table.txt]
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
    args = ap.parse_args()
    import numpy as np
    import torch
    import opty_amd
    from opty_amd.sharded import partition_nodes
    from examples import problems
    col = opty_amd.ConstraintCollocator(**problems.build(args.problem))
    jvp = col.generate_jvp_function()
    handle, hip = jvp.handle, col.hip
    N = col.num_collocation_nodes
    ncn = N - 1
    prog = col._build_jacprod_program()
    M, R, T = prog.M, prog.n + prog.q, prog.r + prog.s
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.01
    v = rng.uniform(-1.0, 1.0, col.num_free)
    w = rng.uniform(-1.0, 1.0, col.num_constraints)
    jvp(free, v)                # builds, verifies, installs the known values
    d_free, d_v, d_w = (torch.from_numpy(x).cuda() for x in (free, v, w))
    d_jv = torch.empty(M*ncn, dtype=torch.float64, device='cuda')
    d_jtw = torch.empty(R*N, dtype=torch.float64, device='cuda')
    d_tail = torch.empty(max(1, T), dtype=torch.float64, device='cuda')
    tail = d_tail if T else None
    torch.cuda.synchronize()

    def window(a, b):
        own = b - a + (1 if b == ncn else 0)
        return (lambda: handle.jvp_shard(d_free, d_v, d_jv, b - a, a, b),
                lambda: handle.vjp_shard(d_free, d_w, d_jtw, own, tail, a, b))

    entries = {'whole': (0, ncn)}
    for world in (int(x) for x in args.worlds.split(',')):
        ranges = partition_nodes(ncn, world)
        entries['1/%d middle' % world] = ranges[world//2]
        entries['1/%d first' % world] = ranges[0]
    group = {}
    for label, (a, b) in entries.items():
        group['jvp ' + label], group['vjp ' + label] = window(a, b)

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
    meta = col._jacprod_meta
    lines = ['%s, N = %d (M = %d, %d free rows, %d tail columns); jvp strips '
             '%d, vjp strips %d; %d rounds of %d calls, alternating'
             % (args.problem, N, M, R, T, meta['jvp_strips'],
                meta['vjp_strips'], args.rounds, args.iters),
             '%-16s %8s  %-34s %s' % ('window', 'nodes',
                                      'us per call: median (min .. max)',
                                      'over whole')]
    for k, t in runs.items():
        a, b = entries[k[4:]]
        lines.append('%-16s %8d  %9.2f (%9.2f .. %9.2f)%6s %.3f'
                     % (k, b - a, med[k], min(t), max(t), '',
                        med[k]/med[k[:4] + 'whole']))
    for world in (int(x) for x in args.worlds.split(',')):
        lines.append('halo node of vjp at 1/%d: middle - first = %+.2f us'
                     % (world, med['vjp 1/%d middle' % world] -
                        med['vjp 1/%d first' % world]))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
