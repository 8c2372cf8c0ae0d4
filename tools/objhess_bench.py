"""Times the objective Hessian kernels next to the objective gradient's, for
the ``effort`` objective (``Integral(u**2, t)``) and for ``trig``
(``Integral(p*u**2 + cos(x)*v**2, t) + 3*p**2``) at N = 100 000, both
integration methods, all in ONE run:

* ``opty_objhess`` (+ ``opty_objhess_fin``): device in, device out, a host
  clock around ``--iters`` back-to-back enqueues that ends in a device
  synchronise ("enqueued"), and the same with a synchronise after EVERY call
  ("per call");
* ``opty_objgrad`` + ``opty_objfin`` of the same objective: device in, device
  out; ``opty_hip_objective_eval`` waits for its value on every call, so it
  has a "per call" figure only -- the one to read next to the Hessian's.

The candidates alternate inside every round; median and minimum .. maximum
over ``--rounds`` rounds.  Reported, not gated: the algorithmic bytes,
``8*((n+q)*N + nnz)``, are so few that the launch decides the time.

    python tools/objhess_bench.py [--nodes 100000] [--iters 50]
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
    ap.add_argument('--nodes', type=int, default=100000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=9)
    args = ap.parse_args()
    import numpy as np
    import sympy as sym
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    t = sym.symbols('t')
    x, v, u = [f(t) for f in sym.symbols('x, v, u', cls=sym.Function)]
    p = sym.symbols('p')
    N, h = args.nodes, 0.01
    objectives = dict(
        effort=(sym.Integral(u**2, t), [x, v], [u], []),
        trig=(sym.Integral(p*u**2 + sym.cos(x)*v**2, t) + 3*p**2, [x, v],
              [u], [p]))
    cand, info = {}, {}
    keep = []
    for name, spec in objectives.items():
        for method, tag in (('backward euler', 'be'), ('midpoint', 'mid')):
            kw = dict(integration_method=method, time_symbol=t)
            obj, obj_grad = opty_amd.create_objective_function(
                *spec, N, h, **kw)
            rows, cols, values = opty_amd.create_objective_hessian_function(
                *spec, N, h, **kw)
            num_free = 3*N + len(spec[3])
            free = torch.from_numpy(np.random.default_rng(0).uniform(
                -1.0, 1.0, num_free)).cuda()
            grad = torch.empty(num_free, dtype=torch.float64, device='cuda')
            out = torch.empty(len(rows), dtype=torch.float64, device='cuda')
            keep.append((free, grad, out))
            hess, first = values.handle, obj.handle
            hess.use_torch_stream()
            first.use_torch_stream()
            key = '%s_%s' % (name, tag)
            cand['objhess ' + key] = (
                lambda hess=hess, free=free, out=out:
                hess.evaluate(free, 1.0, out, hb.DEVICE))
            cand['objgrad ' + key] = (
                lambda first=first, free=free, grad=grad:
                first.evaluate(free, grad, hb.DEVICE))
            info[key] = dict(E=hess.desc['E'], T=hess.desc['T'],
                             nnz=int(hess.nnz),
                             objhess_algorithmic_bytes=8*(3*N +
                                                          int(hess.nnz)),
                             objgrad_algorithmic_bytes=8*2*num_free)
    torch.cuda.synchronize()

    def timed(fn, iters, every):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            if every:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0)/iters*1e6

    def measure(group, every):
        for fn in group.values():
            timed(fn, 3, every)
        runs = {k: [] for k in group}
        for _ in range(args.rounds):
            for k, fn in group.items():         # alternating inside a round
                runs[k].append(timed(fn, args.iters, every))
        return {k: dict(median_us=round(statistics.median(ts), 2),
                        min_us=round(min(ts), 2), max_us=round(max(ts), 2))
                for k, ts in runs.items()}

    per_call = measure(cand, True)
    enqueued = measure({k: fn for k, fn in cand.items()
                        if k.startswith('objhess')}, False)
    print(json.dumps(dict(N=N, iters=args.iters, rounds=args.rounds,
                          objectives=info, per_call=per_call,
                          enqueued=enqueued), indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
