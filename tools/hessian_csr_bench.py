"""Times the CSR Hessian -- the stored triplets compressed to the unique lower
triangle on the GPU -- on one process, in ONE run per problem:

* (a) device time of ``opty_hesscsr`` + ``opty_hesscsr_fin`` alone (``opty_hip_
  hesscsr_compress``, device in / device out);
* (b) device time of ``opty_hess`` of the same problem, the yardstick;
* (c) the host alternative: ``hessian(free, lagrange)`` to NumPy, then
  ``coo_matrix(triplets).tocsr()`` on the CPU (the first ``--host-rounds``
  rounds only: it takes seconds).

(a) and (b): a host clock around ``--iters`` back-to-back enqueues that ends
in a device synchronise; (c): one call.  ``--rounds`` rounds that ALTERNATE
all of them; median (min .. max) over the rounds.  The kernel's floor is its
algorithmic traffic, one read of the triplets plus one write of the distinct
values; the achieved fraction of the 8 TB/s peak is printed next to the time.
The result must equal SciPy's to the bound of ``tests/hessian_csr_cases.py``.
Reported, not gated.

A problem is a name of ``examples/problems.py`` or ``pendulum:LINKS:METHOD``
(the n-link pendulum on a cart at ``--nodes`` nodes).

    python tools/hessian_csr_bench.py [--problems config3_10link,pendulum:10:midpoint]
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


def build(spec, nodes):
    from examples import problems
    if spec.startswith('pendulum:'):
        _, links, method = spec.split(':')
        return problems.n_link_cart_pendulum(
            num_links=int(links), num_nodes=nodes,
            method={'be': 'backward euler'}.get(method, method))
    return problems.build(spec)


def measure(spec, args):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    col = opty_amd.ConstraintCollocator(**build(spec, args.nodes))
    hess = col.generate_hessian_function()
    hcsr = col.generate_hessian_csr_function()
    rows, cols = col.hessian_indices_closed_form()
    hip, N, nfree = col.hip, col.num_collocation_nodes, col.num_free
    PH = col._build_hessian_program().PH
    handle = hcsr.handle
    nnz, nu = handle.nnz, handle.nnz_unique
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, nfree)
    lam = rng.uniform(-1.0, 1.0, col.num_constraints)
    d_free, d_lam = (torch.from_numpy(x).cuda() for x in (free, lam))
    d_val = hess(d_free, d_lam)
    d_data = torch.empty(nu, dtype=torch.float64, device='cuda')
    d_out = torch.empty_like(d_val)
    torch.cuda.synchronize()
    col.sync_known()

    def host_alternative():
        values = hess(free, lam)
        return sp.coo_matrix((values, (rows, cols)),
                             shape=(nfree, nfree)).tocsr()

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
    group = dict(
        hesscsr=enqueued(lambda: handle.compress(d_val, d_data, hb.DEVICE)),
        opty_hess=enqueued(lambda: hess.handle.evaluate(d_free, d_lam, d_out,
                                                        hb.DEVICE)),
        host_alternative=once)
    for fn in group.values():             # warm-up: every path once
        fn()
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
    # the result is SciPy's: structure equal, values within (k - 1) u sum|a|
    ref = host_alternative()
    ref.sum_duplicates()
    ref.sort_indices()
    indptr, indices = col.hessian_csr_structure()
    same_structure = bool(np.array_equal(indptr, ref.indptr) and
                          np.array_equal(indices, ref.indices))
    values = hess(free, lam)
    key = rows*nfree + cols
    _, group_of = np.unique(key, return_inverse=True)
    count = np.bincount(group_of)
    tol = (count - 1)*2.0**-53*np.bincount(group_of, weights=np.abs(values))
    err = np.abs(d_data.cpu().numpy() - ref.data)
    nbytes = 8*(nnz + nu)
    tbs = nbytes/out['hesscsr']['median_us']*1e-6
    print('%s, N = %d: %d triplets, %d distinct pairs' % (spec, N, nnz, nu))
    print('%-18s %12s   (%s .. %s) us' % ('', 'median', 'min', 'max'))
    for k, t in out.items():
        print('%-18s %12.1f   (%.1f .. %.1f)' % (k, t['median_us'],
                                                 t['min_us'], t['max_us']))
    return dict(
        problem=spec, N=N, PH=PH, num_free=nfree, nnz=nnz, nnz_unique=nu,
        iters=args.iters, rounds=args.rounds, times=out,
        algorithmic_bytes=nbytes, tb_per_s=round(tbs, 3),
        fraction_of_peak=round(tbs/PEAK_TB_PER_S, 4),
        hesscsr_over_opty_hess=round(out['hesscsr']['median_us'] /
                                     out['opty_hess']['median_us'], 3),
        host_over_hesscsr=round(out['host_alternative']['median_us'] /
                                out['hesscsr']['median_us'], 1),
        structure_equals_scipy=same_structure,
        values_within_tolerance=bool(np.all(err <= tol)),
        max_abs_difference_from_scipy=float(err.max(initial=0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems',
                    default='config3_10link,pendulum:10:midpoint')
    ap.add_argument('--nodes', type=int, default=100000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--host-rounds', type=int, default=2)
    args = ap.parse_args()
    from opty_amd import hip_backend as hb
    for spec in args.problems.split(','):
        try:
            print(json.dumps(measure(spec, args)))
        except hb.HipBackendError as e:
            # (a pattern the handle refuses is part of the report)
            print(json.dumps(dict(problem=spec, refused=str(e))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
