"""Times the node-sharded exact Hessian on ONE GPU: ``opty_hip_eval_hess`` (the
whole problem, device in / device out) and the windows a rank of 2, 4 and 8
evaluates (``opty_hip_eval_hess_shard`` into a dense rank-local block), all in
ONE run -- what one rank of a node-sharded problem spends on the constraint
triplets, without the copy to the host.

Method of ``tools/jacprod_shard_bench.py``: a host clock around ``--iters``
back-to-back enqueues that ends in a device synchronise, repeated ``--rounds``
times with all entries ALTERNATING inside every round; median (minimum ..
maximum) over the rounds.

``--whole-only`` times ``opty_hip_eval_hess`` alone and uses nothing that an
older checkout lacks; ``--tree DIR`` imports the package from that checkout
(built there) instead of this one, so that two commits can be timed in turns
in one session.  ``--prebuild`` builds the code objects (no GPU) and exits.

    python tools/hessian_shard_bench.py [--problem config3_10link]
        [--worlds 2,4,8] [--iters 30] [--rounds 9] [--out table.txt]
        [--whole-only] [--tree DIR] [--label TEXT] [--prebuild]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='config3_10link')
    ap.add_argument('--worlds', default='2,4,8')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--whole-only', action='store_true')
    ap.add_argument('--tree', default=REPO)
    ap.add_argument('--label', default='')
    ap.add_argument('--prebuild', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import opty_amd
    from opty_amd import hip_backend as hb
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
    handle, hip = hess.handle, col.hip
    prog = col._build_hessian_program()
    N = col.num_collocation_nodes
    ncn, PH = N - 1, prog.PH
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.01
    lam = rng.uniform(-1.0, 1.0, col.num_constraints)
    hess(free, lam)             # builds, verifies, installs the known values
    d_free, d_lam = (torch.from_numpy(x).cuda() for x in (free, lam))
    d_out = torch.empty(handle.nnz, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    entries = {'whole (eval_hess)': (0, ncn)}
    group = {'whole (eval_hess)':
             lambda: handle.evaluate(d_free, d_lam, d_out, hb.DEVICE)}
    if not args.whole_only:
        def window(a, b):
            return lambda: handle.eval_shard(d_free, d_lam, d_out, a, b)
        entries['whole window'] = (0, ncn)
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
    meta = col._hessian_meta
    lines = ['%s%s, N = %d (PH = %d, %d instance entries); %d strips; %d '
             'rounds of %d calls, alternating'
             % (args.label + ': ' if args.label else '', args.problem, N, PH,
                len(prog.inst_hess_out), meta['strips'], args.rounds,
                args.iters),
             '%-18s %8s  %-34s %s' % ('window', 'nodes',
                                      'us per call: median (min .. max)',
                                      'over whole')]
    for k, t in runs.items():
        a, b = entries[k]
        lines.append('%-18s %8d  %9.2f (%9.2f .. %9.2f)%6s %.3f'
                     % (k, b - a, med[k], min(t), max(t), '',
                        med[k]/med['whole (eval_hess)']))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
