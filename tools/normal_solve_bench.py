"""Times the direct solver with the constraint normal matrix ``S = Jc D^-1
Jc^T + delta_c I`` (``ConstraintCollocator.generate_normal_solver``) on one
process, in ONE run per problem:

* (a) ``blocks`` (``opty_normal_blocks`` into caller's buffers), ``factor``
  (the blocks again into the handle's storage, then ``opty_normal_elim`` /
  ``opty_normal_update`` per level) and ``solve`` (one right-hand side: the
  forward and backward kernels per level), each between two device events on
  the stream the handle runs on (device pointers in and out);
* (b) the host route on the same ``S``: the blocks to NumPy,
  ``scipy.linalg.cholesky_banded`` and ``cho_solve_banded`` on the lower band
  of the node-ordered matrix (the first ``--host-rounds`` rounds only);
* (c) the iteration it replaces: ``--lsmr-iters`` iterations of
  ``scipy.sparse.linalg.lsmr`` on ``ConstraintCollocator.jacobian_operator``
  for the minimum-norm step ``J dx = -c`` (``examples/feasible_guess_lsmr.py``
  gives it ``4*num_free``), against ``dx = -D^-1 J^T S^-1 c`` by the solver.

``--rounds`` rounds that ALTERNATE all of them; median (min .. max) over the
rounds.  Reported, not gated.

    python tools/normal_solve_bench.py [--problems config3_10link] [--prebuild]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def build(spec, nodes):
    from examples import problems
    parts = spec.split(':')
    prune = parts[-1] == 'prune'
    if prune:
        parts = parts[:-1]
    if parts[0] == 'pendulum':
        kw = problems.n_link_cart_pendulum(
            num_links=int(parts[1]), num_nodes=nodes,
            method={'be': 'backward euler'}.get(parts[2], parts[2]))
    else:
        kw = problems.build(parts[0])
    return dict(kw, prune_zeros=prune)


def prebuild(spec, nodes):
    """The code objects :func:`measure` loads (no GPU needed)."""
    import opty_amd
    col = opty_amd.ConstraintCollocator(**build(spec, nodes))
    col.prebuild()
    col._build_jacprod_code_object()


def banded(A, B):
    """The lower band of the node-ordered matrix in LAPACK's layout,
    ``ab[k, j] = S[j + k, j]``, from the blocks."""
    import numpy as np
    n, M = A.shape[0], A.shape[1]
    ab = np.zeros((2*M, n*M))
    for b in range(M):
        for a in range(b, M):
            ab[a - b, b::M] = A[:, a, b]
        for a in range(M):
            ab[M + a - b, b::M][:n - 1] = B[:, a, b]
    return ab


def measure(spec, args):
    import numpy as np
    import torch
    from scipy.linalg import cho_solve_banded, cholesky_banded
    from scipy.sparse.linalg import lsmr
    import opty_amd
    from opty_amd import hip_backend as hb
    col = opty_amd.ConstraintCollocator(**build(spec, args.nodes))
    ns = col.generate_normal_solver()
    handle, hip = ns.handle, col.hip
    hip.use_torch_stream()              # events and launches on one stream
    N, n = col.num_collocation_nodes, col.num_free
    M, ncn, m = ns.M, ns.num_nodes, ns.size
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, n)
    d_free = torch.from_numpy(free).cuda()
    d_jval = torch.empty(hip.nnz, dtype=torch.float64, device='cuda')
    d_A = torch.empty((ncn, M, M), dtype=torch.float64, device='cuda')
    d_B = torch.empty((ncn - 1, M, M), dtype=torch.float64, device='cuda')
    con = np.array(col.generate_constraint_function()(free))
    d_r = torch.from_numpy(np.ascontiguousarray(con[:m])).cuda()
    d_y = torch.empty_like(d_r)
    torch.cuda.synchronize()
    col.sync_known()
    hip.eval_jac(d_free, d_jval, hb.DEVICE)
    hip.synchronize()
    delta_c = args.delta_c

    def timed(fn):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)*1e3

    def blocks():
        return timed(lambda: handle.blocks(d_jval, None, delta_c, d_A, d_B,
                                           hb.DEVICE))

    def factor():
        us = timed(lambda: handle.factor(d_jval, None, delta_c, hb.DEVICE))
        assert handle.status() is None
        return us

    def solve():
        return timed(lambda: handle.solve(d_r, d_y, 1, m, hb.DEVICE))

    host = {}

    def host_route():
        A, B = d_A.cpu().numpy(), d_B.cpu().numpy()
        t0 = time.perf_counter()
        ab = banded(A, B)
        t1 = time.perf_counter()
        cb = cholesky_banded(ab, lower=True, overwrite_ab=True,
                             check_finite=False)
        t2 = time.perf_counter()
        rhs = con[:m].reshape(M, ncn).T.ravel()         # node-major
        y = cho_solve_banded((cb, True), rhs, check_finite=False)
        t3 = time.perf_counter()
        host['y'] = y.reshape(ncn, M).T.ravel()
        return dict(host_band_layout=(t1 - t0)*1e6,
                    host_cholesky_banded=(t2 - t1)*1e6,
                    host_cho_solve_banded=(t3 - t2)*1e6)

    J = col.jacobian_operator(free)

    def lsmr_route():
        t0 = time.perf_counter()
        out = lsmr(J, -con, atol=1e-12, btol=1e-12, maxiter=args.lsmr_iters)
        host['lsmr'] = out
        return (time.perf_counter() - t0)*1e6

    group = dict(blocks=blocks, factor=factor, solve=solve)
    for fn in group.values():             # warm-up: every path once
        fn()
    names = list(group) + ['host_band_layout', 'host_cholesky_banded',
                           'host_cho_solve_banded', 'lsmr']
    runs = {k: [] for k in names}
    for r in range(args.rounds):
        for k, fn in group.items():       # alternating inside a round
            runs[k].append(fn())
        if r < args.host_rounds:
            for k, t in host_route().items():
                runs[k].append(t)
            runs['lsmr'].append(lsmr_route())
    out = {k: dict(median_us=round(statistics.median(t), 1),
                   min_us=round(min(t), 1), max_us=round(max(t), 1))
           for k, t in runs.items() if t}
    y = d_y.cpu().numpy()
    same = float(np.abs(y - host['y']).max()/np.abs(host['y']).max())
    # the minimum-norm step of the collocation rows by the solver (D = I)
    w = np.zeros(col.num_constraints)
    w[:m] = y
    dx = -J.rmatvec(w)
    cnorm = float(np.linalg.norm(con[:m]))
    direct = float(np.linalg.norm((J.matvec(dx) + con)[:m])/cnorm)
    step = host['lsmr'][0]
    iterative = float(np.linalg.norm((J.matvec(step) + con)[:m])/cnorm)
    levels = 1
    k = ncn
    while k > 1:
        k, levels = (k + 1)//2, levels + 1
    flops = 0
    k = ncn
    while True:                 # Cholesky, two solves; three products
        elim, surv = (1, 0) if k == 1 else (k//2, (k + 1)//2)
        flops += elim*(M**3/3 + 2*M**3) + surv*6*M**3
        if k == 1:
            break
        k = (k + 1)//2
    print('%s, N = %d: S %d x %d in %d blocks of %d x %d, %d levels, '
          'workspace %.3f GB, about %.1f GFlop per factorisation'
          % (spec, N, m, m, ncn, M, M, levels, ns.workspace_bytes/1e9,
             flops/1e9))
    print('%-24s %12s   (%s .. %s) us' % ('', 'median', 'min', 'max'))
    for k, t in out.items():
        print('%-24s %12.1f   (%.1f .. %.1f)' % (k, t['median_us'],
                                                 t['min_us'], t['max_us']))
    print('|y - y_banded|/|y| = %.3g; |J dx + c|/|c| on the collocation '
          'rows: solver %.3g, lsmr after %d iterations %.3g'
          % (same, direct, host['lsmr'][2], iterative))
    return dict(
        problem=spec, N=N, M=M, rows=m, levels=levels,
        workspace_bytes=ns.workspace_bytes, flops=flops, delta_c=delta_c,
        rounds=args.rounds, times=out,
        factor_gflops=round(flops/out['factor']['median_us']*1e-3, 1),
        against_banded=same, residual_solver=direct,
        residual_lsmr=iterative, lsmr_iterations=int(host['lsmr'][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems', default='config3_10link')
    ap.add_argument('--nodes', type=int, default=100000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=2)
    ap.add_argument('--lsmr-iters', type=int, default=50)
    ap.add_argument('--delta-c', type=float, default=1e-8)
    ap.add_argument('--prebuild', action='store_true')
    args = ap.parse_args()
    from opty_amd import hip_backend as hb
    for spec in args.problems.split(','):
        if args.prebuild:
            prebuild(spec, args.nodes)
            continue
        try:
            print(json.dumps(measure(spec, args)), flush=True)
        except hb.HipBackendError as e:
            print(json.dumps(dict(problem=spec, refused=str(e))), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
