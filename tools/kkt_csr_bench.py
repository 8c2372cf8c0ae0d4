"""Times the assembly of the augmented system as CSR -- the Hessian's triplets
and the CSR Jacobian's values laid out as one lower triangle on the GPU -- on
one process, in ONE run per problem:

* (a) the whole ``opty_hip_kktcsr_assemble`` (device in / device out): a host
  clock around ``--iters`` back-to-back enqueues that ends in a device
  synchronise;
* (b) its four stages by device events (``opty_hip_kktcsr_assemble_timed``):
  the compression, ``opty_kkt_diag``, ``opty_kkt_jrows``, ``opty_kkt_inst``;
* (c) a plain device-to-device copy of the Jacobian's bytes in the same
  process (torch's contiguous same-device ``copy_``: ``hipMemcpyAsync``), the
  rate a plain copy reaches on that machine at that moment;
* (d) the host route of ``examples/kkt_direct.py``: the CSR Hessian and the
  Jacobian to NumPy, then ``scipy.sparse.bmat`` (the first ``--host-rounds``
  rounds only: it takes seconds).

``--rounds`` rounds that ALTERNATE all of them; median (min .. max) over the
rounds.  The floor traffic of ``opty_kkt_jrows`` is one read of the Jacobian's
block values plus one write of its rows in ``K`` (a diagonal more per row), of
the whole assembly that plus one read of the triplets and one write of the
``W`` block; the achieved TB/s are printed next to the times.  Reported, not
gated.

A problem is ``NAME[:prune]`` of ``examples/problems.py`` or
``pendulum:LINKS:METHOD[:prune]`` (the n-link pendulum on a cart at
``--nodes`` nodes); the Jacobian is in the CSR layout.

    python tools/kkt_csr_bench.py [--problems config3_10link,config3_10link:prune,pendulum:10:midpoint]
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
    return dict(kw, jacobian_layout='csr', prune_zeros=prune)


def measure(spec, args):
    import numpy as np
    import scipy.sparse as sp
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    col = opty_amd.ConstraintCollocator(**build(spec, args.nodes))
    hess = col.generate_hessian_function()
    hcsr = col.generate_hessian_csr_function()
    jac = col.generate_jacobian_function()
    kkt = col.generate_kkt_csr_function()
    handle, hip = kkt.handle, col.hip
    N, n, m = col.num_collocation_nodes, col.num_free, col.num_constraints
    prog = col._build_program()
    P, M = len(prog.pattern), prog.M
    rng = np.random.default_rng(0)
    free = rng.uniform(-1.0, 1.0, n)
    lam = rng.uniform(-1.0, 1.0, m)
    d_free, d_lam = (torch.from_numpy(x).cuda() for x in (free, lam))
    d_hval = hess(d_free, d_lam)
    d_jval = torch.empty(hip.nnz, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    col.sync_known()
    hip.eval_jac(d_free, d_jval, hb.DEVICE)
    hip.synchronize()
    d_data = torch.empty(handle.nnz_kkt, dtype=torch.float64, device='cuda')
    d_copy = torch.empty_like(d_jval)
    torch.cuda.synchronize()
    hptr, hidx = col.hessian_csr_structure()
    jptr, jidx = col.jacobian_csr_structure()

    def host_route():
        H = sp.csr_matrix((np.array(hcsr(free, lam)), hidx, hptr),
                          shape=(n, n))
        J = sp.csr_matrix((np.array(jac(free)), jidx, jptr), shape=(m, n))
        return sp.bmat([[H, None], [J, sp.csr_matrix((m, m))]], format='csr')

    def assemble():
        for _ in range(args.iters):
            handle.assemble(d_hval, d_jval, None, 1e-4, 1e-8, d_data,
                            hb.DEVICE)
        hip.synchronize()
        return args.iters

    def copy():
        for _ in range(args.iters):
            d_copy.copy_(d_jval)
        torch.cuda.synchronize()
        return args.iters

    def once():
        host_route()
        return 1
    group = dict(assemble=assemble, memcpy_d2d=copy, host_route=once)
    stages = ('compression', 'opty_kkt_diag', 'opty_kkt_jrows',
              'opty_kkt_inst')
    for fn in group.values():             # warm-up: every path once
        fn()
    runs = {k: [] for k in list(group) + list(stages)}
    for r in range(args.rounds):
        for k, fn in group.items():       # alternating inside a round
            if k == 'host_route' and r >= args.host_rounds:
                continue
            t0 = time.perf_counter()
            count = fn()
            runs[k].append((time.perf_counter() - t0)/count*1e6)
        ms = handle.assemble_timed(d_hval, d_jval, None, 1e-4, 1e-8, d_data)
        for k, t in zip(stages, ms):
            runs[k].append(t*1e3)
    out = {k: dict(median_us=round(statistics.median(t), 1),
                   min_us=round(min(t), 1), max_us=round(max(t), 1))
           for k, t in runs.items()}
    # the result is the host route's (stored zeros included) with every
    # diagonal and the regularisation on it, bit for bit
    indptr, indices = col.kkt_csr_structure()
    data = d_data.cpu().numpy()
    ref = host_route()
    ref.sort_indices()
    size = n + m
    rrow = np.repeat(np.arange(size), np.diff(ref.indptr))
    key = np.repeat(np.arange(size), np.diff(indptr))*size + indices
    at = np.searchsorted(key, rrow*size + ref.indices)
    expect = np.zeros(len(data))
    expect[at] = ref.data
    wdiag, cdiag = indptr[1:n + 1] - 1, indptr[n + 1:] - 1
    expect[wdiag] = (expect[wdiag] + 0.0) + 1e-4
    expect[cdiag] = 0.0 - 1e-8
    hit = np.zeros(len(data), dtype=bool)
    hit[at] = hit[wdiag] = hit[cdiag] = True
    same = bool(np.array_equal(key[at], rrow*size + ref.indices) and
                hit.all() and
                np.array_equal(expect.view(np.int64), data.view(np.int64)))
    ncn = N - 1
    jrows_bytes = 8*(P*ncn + (P + M)*ncn)
    all_bytes = jrows_bytes + 8*(handle.nnz + handle.nnz_hessian) + \
        8*(hip.nnz - P*ncn)*2 + 24*n
    copy_bytes = 16*hip.nnz

    def rate(nbytes, key):
        return round(nbytes/out[key]['median_us']*1e-6, 3)
    print('%s, N = %d: K %d x %d, %d stored values (W block %d of %d '
          'triplets, Jacobian %d)' % (spec, N, n + m, n + m, handle.nnz_kkt,
                                      handle.nnz_hessian, handle.nnz,
                                      hip.nnz))
    print('%-18s %12s   (%s .. %s) us' % ('', 'median', 'min', 'max'))
    for k, t in out.items():
        print('%-18s %12.1f   (%.1f .. %.1f)' % (k, t['median_us'],
                                                 t['min_us'], t['max_us']))
    return dict(
        problem=spec, N=N, num_free=n, num_constraints=m,
        nnz_kkt=handle.nnz_kkt, nnz_hessian_block=handle.nnz_hessian,
        hessian_triplets=handle.nnz, jacobian_values=hip.nnz,
        iters=args.iters, rounds=args.rounds, times=out,
        jrows_floor_bytes=jrows_bytes,
        jrows_tb_per_s=rate(jrows_bytes, 'opty_kkt_jrows'),
        assemble_floor_bytes=all_bytes,
        assemble_tb_per_s=rate(all_bytes, 'assemble'),
        memcpy_bytes=copy_bytes,
        memcpy_tb_per_s=rate(copy_bytes, 'memcpy_d2d'),
        host_over_assemble=round(out['host_route']['median_us'] /
                                 out['assemble']['median_us'], 1),
        equals_host_route=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problems',
                    default='config3_10link,config3_10link:prune,'
                            'pendulum:10:midpoint')
    ap.add_argument('--nodes', type=int, default=100000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=2)
    args = ap.parse_args()
    from opty_amd import hip_backend as hb
    for spec in args.problems.split(','):
        try:
            print(json.dumps(measure(spec, args)), flush=True)
        except hb.HipBackendError as e:
            print(json.dumps(dict(problem=spec, refused=str(e))), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
