#!/usr/bin/env python
"""Developer tool (GPU box): the two forms of the restricted Jacobian kernels
(``EmitOptions.var_order``: None = one workgroup per block and strip, 'run' =
persistent waves over contiguous strip runs) of one workload, A/B in ONE
process, and traced.

    python tools/restricted_runs.py <workload> [--nodes N] [--rounds R]
        [--persist W] [--trace] [--build-only]

Per round and form, interleaved: ``opty_jac_var``, ``opty_conjac_var`` and
``opty_con`` by events (``opty_hip_time_eval`` into a registered output, the
plan's routing: the kernel that is named is the kernel that runs), and the
full kernels ``opty_jac`` / ``opty_conjac`` of the same two modules into an
unregistered buffer.  With
``--trace``: one traced launch of ``opty_jac_var`` and of ``opty_conjac_var``
per form (``EmitOptions(trace=1)``) -- wave / item durations per strip class,
the share of them spent before the first strip entry (slab fill; run form:
fill and trig stage, on the items that change block), per-SIMD busy share and
gaps.  ``--build-only`` compiles the code objects (no device needed).
"""
import argparse
import copy
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, REPO)

import numpy as np                                            # noqa: E402
import opty_amd                                               # noqa: E402
from opty_amd import hip_backend as hb                        # noqa: E402
from opty_amd.codegen.emit_hip import TRACE_OFFSET            # noqa: E402
from examples import problems                                 # noqa: E402

TICK_US = 0.01          # wall_clock64: 100 MHz
FORMS = (('dispatch', None), ('run', 'run'))


def collocator(workload, nodes, form, persist, trace):
    factory, fkw = problems.CONFIGS[workload]
    if nodes:
        fkw = dict(fkw, num_nodes=nodes)
    kw = factory(**fkw)
    opts = copy.copy(opty_amd.ConstraintCollocator(**kw)._printer_options())
    opts.var_order = form
    if persist:
        opts.var_persist = persist
    opts.trace = int(trace)
    return opty_amd.ConstraintCollocator(emit_options=opts, **kw)


def report_trace(rec, label):
    rec = rec[rec[:, 1] != 0]
    t0 = rec[:, 0].min()
    start, end = (rec[:, 0] - t0)*TICK_US, (rec[:, 1] - t0)*TICK_US
    grp = rec[:, 2] >> 40
    stage = ((rec[:, 2] >> 24) & 0xffff)*TICK_US
    hw = rec[:, 3] & 0xffffff
    dur = end - start
    print('%s: %d records, span %.1f us' % (label, len(rec), end.max()))
    for g in np.unique(grp):
        m = grp == g
        s = stage[m]
        hit = s > 0
        print('  class %2d: %5d items  dur med %5.2f p90 %5.2f max %5.2f us; '
              'fill/stage on %5d of them: med %4.2f p90 %4.2f us; share of '
              'the class\'s time %4.1f %%'
              % (g, m.sum(), np.median(dur[m]), np.percentile(dur[m], 90),
                 dur[m].max(), hit.sum(),
                 np.median(s[hit]) if hit.any() else 0.0,
                 np.percentile(s[hit], 90) if hit.any() else 0.0,
                 100*s.sum()/dur[m].sum()))
    print('  all: time before the first strip entry %.1f %% of the summed '
          'item time (%.0f of %.0f us)'
          % (100*stage.sum()/dur.sum(), stage.sum(), dur.sum()))
    simd = hw & 0xf7f3f
    gaps, busy = [], []
    for k in np.unique(simd):
        m = np.flatnonzero(simd == k)
        m = m[np.argsort(start[m])]
        gaps.extend(start[m][1:] - end[m][:-1])
        busy.append(dur[m].sum())
    gaps = np.array(gaps) if gaps else np.zeros(1)
    print('  per SIMD (%d): busy mean %.1f us of %.1f (%.0f %%), items %.1f, '
          'gap med %.2f p90 %.2f us, sum %.1f us'
          % (len(busy), np.mean(busy), end.max(),
             100*np.mean(busy)/end.max(), len(rec)/len(busy), np.median(gaps),
             np.percentile(gaps, 90), gaps.sum()/len(busy)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload')
    ap.add_argument('--nodes', type=int, default=0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--persist', type=int, default=0)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--build-only', action='store_true')
    a = ap.parse_args()
    os.environ.setdefault('OPTY_CROSS_CHECK', 'off')
    os.environ['OPTY_HIP_ROUTING'] = 'plan'
    cols = {}
    for traced in ([0, 1] if a.trace else [0]):
        for name, form in FORMS:
            col = collocator(a.workload, a.nodes, form, a.persist, traced)
            hsaco, meta = col._build_code_object()
            k = meta['kernels']
            print('%s%s: %s restricted_ok %s; %s' % (
                name, ' traced' if traced else '', os.path.basename(hsaco),
                meta.get('restricted_ok'), {
                    n: (r['.vgpr_count'] + r['.agpr_count'],
                        r['.vgpr_spill_count'], r['.sgpr_spill_count'])
                    for n, r in hb.cached_kernel_resources(
                        meta.get('run_hsaco') or hsaco).items()
                    if n.endswith('_var')}), flush=True)
            if not meta.get('restricted_ok') or \
                    bool(meta.get('run_hsaco')) != (form == 'run'):
                # (a run form that fails a build gate is replaced by the
                # dispatch form: nothing to compare)
                print('%s form not built: %s' % (
                    name, meta.get('restricted_refused') or
                    col._run_form_refused), flush=True)
                return
            cols[name, traced] = col
    if a.build_only:
        return
    import torch
    dev = torch.device('cuda:0')
    f64 = dict(dtype=torch.float64, device=dev)
    state = {}
    for key, col in cols.items():
        hip = col.hip
        hip.use_torch_stream()
        d = hip.desc
        ncn = col.num_collocation_nodes - 1
        nblk8 = ((ncn + 63)//64 + 7)//8*8
        # (every Jacobian kernel of a traced module leaves records: room
        # for the widest launch)
        nrec = max((nblk8*d[k + '_wgs_per_block'] + 1)*d[k + '_waves_per_wg']
                   for k in ('jac', 'fused', 'var_jac', 'var_fused'))
        frees = []
        for seed in (11, 12):
            fh = problems.make_free(col.num_free, seed=seed)
            col._sync_known(hip, fh)
            frees.append(torch.from_numpy(fh).to(dev))
        con = torch.empty(col.num_constraints, **f64)
        jac = torch.zeros(hip.nnz + (TRACE_OFFSET + 4*nrec + 64
                                     if key[1] else 0), **f64)
        hip.output_register(jac)
        hip.eval_con_jac(frees[0], con, jac, hb.DEVICE)     # written whole
        torch.cuda.synchronize()
        state[key] = (hip, frees, con, jac, ncn, nrec)
    # (the full kernels share the module, and with it the compiler flags of
    # the run form's loops: timed into an unregistered buffer)
    kernels = (('opty_jac_var', hb.EVAL_JAC),
               ('opty_conjac_var', hb.EVAL_FUSED_KERNEL),
               ('opty_con', hb.EVAL_CON),
               ('opty_jac', hb.EVAL_JAC),
               ('opty_conjac', hb.EVAL_FUSED_KERNEL))
    plain = torch.empty(state['run', 0][0].nnz, **f64)
    times = {(f, k): [] for f, _ in FORMS for k, _ in kernels}
    for r in range(a.rounds):
        for name, _ in FORMS:
            hip, frees, con, jac, ncn, _ = state[name, 0]
            for kname, what in kernels:
                out = jac if kname.endswith('_var') else plain
                hip.time_eval(what, frees[1], con, out, 20)
                ms = hip.time_eval(what, frees[1], con, out, a.iters)
                if what != hb.EVAL_CON:
                    assert hip.routing()['flavour'] == (
                        'restricted' if out is jac else 'full')
                times[name, kname].append(ms)
    for (name, kname), ms in sorted(times.items()):
        print('%-9s %-16s ms per launch: %s  (min %.4f max %.4f)'
              % (name, kname, ' '.join('%.4f' % m for m in ms), min(ms),
                 max(ms)), flush=True)
    # the two forms compute the same values
    ja = state['dispatch', 0][3].cpu().numpy()
    jb = state['run', 0][3].cpu().numpy()
    print('largest difference between the forms\' buffers: %.3g (largest '
          'entry %.3g)' % (np.abs(ja - jb).max(), np.abs(ja).max()),
          flush=True)
    if not a.trace:
        return
    for name, _ in FORMS:
        hip, frees, con, jac, ncn, nrec = state[name, 1]
        P = hip.desc['P']
        for kname, what in kernels[:2]:
            hip.time_eval(what, frees[1], con, jac, 20)
            jac[hip.nnz:].zero_()
            torch.cuda.synchronize()
            hip.time_eval(what, frees[1], con, jac, 1)
            torch.cuda.synchronize()
            assert hip.routing()['flavour'] == 'restricted'
            rec = jac[ncn*P + TRACE_OFFSET:ncn*P + TRACE_OFFSET + 4*nrec] \
                .view(torch.int64).cpu().numpy().reshape(-1, 4)
            report_trace(rec, '%s %s' % (name, kname))


if __name__ == '__main__':
    main()
