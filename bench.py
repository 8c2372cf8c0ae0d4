#!/usr/bin/env python
"""Benchmark of the hot path: constraint + Jacobian evaluations per second of
the 10-link pendulum on a cart at N = 100 000 collocation nodes (BASELINE.json
metric, ``configs[2]`` on one GPU, ``configs[3]`` on several), inputs resident
in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline.
``--full`` adds everything else the benchmark measures or checks: the
per-kernel times and the roofline, the check of the benched launch against
the reference's golden record, the serial pair, the other configurations,
the host path, the CPU baseline and (N > 1) the re-assembly variants.
``--dump-outputs DIR`` writes what the last timed step computed under DIR
(:func:`dump_outputs`).

One *step* = one ``constraints(free)`` + one ``jacobian(free)`` on a free
vector that differs from the previous step's (rotating set of synthetic
vectors already in HBM), evaluated through the C ABI (``libopty_hip.so``) with
device pointers on torch's current stream.  Both outputs of a step come from
ONE launch (``opty_hip_eval_con_jac`` / ``opty_hip_eval_shard``: the Jacobian
waves plus one constraint wave per 64-node block); ``--serial`` issues two
launches (constraints, then Jacobian -- the order IPOPT calls them in)
instead, and ``--full`` also reports that figure as
``config.serial_evals_per_s``.

Multi-GPU (``--gpus N`` under ``torch.distributed.run``) is BASELINE config 4:
the 100 000 nodes of ONE problem are sharded over the ranks, one contiguous
node range each with a one-node halo (``opty_amd.sharded``) --
**strong scaling**, ``value`` = evaluations of the whole problem per second
with every rank's slice of the outputs left in its own HBM (no data-path
collective).  With ``--full`` the same K steps are then re-timed with the
two re-assembly variants SURVEY.md 8(e) lists, reported in
``config.variants``:
``gather`` (+ RCCL point-to-point gather-v of constraints and Jacobian to rank
0) and ``to_host`` (+ every rank copying its shard over its own PCIe link
into one page-locked host vector shared by all ranks).  ``--weak`` instead
gives every rank its own ``--nodes``-node problem.

Timing: an untimed clock-ramp phase (``--prewarm-ms`` of the same step; an
idle GPU starts at its lowest clock), W untimed warm-up steps, then exactly K
steps between barrier + ``torch.cuda.synchronize()`` pairs, max over ranks.

Prints ONE JSON line (rank 0).
"""

import argparse
import json
import os
import sys
import time

# The CPU baseline's OpenMP team is pinned.  libgomp reads
# OMP_PROC_BIND / OMP_PLACES when it is loaded and then binds the thread that
# loaded it -- which would also pin the GPU process's host threads -- so the
# baseline runs in a child process of its own (`--cpu-baseline-only`).
CPU_BASELINE_ENV = {'OMP_PROC_BIND': 'close', 'OMP_PLACES': 'cores'}

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
WORKLOAD = 'config3_10link'


def host_cpu():
    """CPU model, sockets, physical cores, logical CPUs and NUMA nodes of this
    box (for ``cpu_baseline.sample``)."""
    model, phys, logical = '?', set(), 0
    try:
        pid = cid = None
        with open('/proc/cpuinfo') as f:
            for line in f:
                k, _, v = line.partition(':')
                k, v = k.strip(), v.strip()
                if k == 'model name':
                    model = v
                elif k == 'processor':
                    logical += 1
                elif k == 'physical id':
                    pid = v
                elif k == 'core id':
                    cid = v
                elif not k and pid is not None:
                    phys.add((pid, cid))
                    pid = cid = None
    except OSError:
        pass
    try:
        numa = len([d for d in os.listdir('/sys/devices/system/node')
                    if d.startswith('node') and d[4:].isdigit()])
    except OSError:
        numa = 0
    return dict(model=model, sockets=len({p for p, _ in phys}) or 1,
                physical_cores=len(phys) or logical,
                logical_cpus=logical or (os.cpu_count() or 1),
                numa_nodes=numa)


def _cpu_baseline_impl(kw, budget_s=24.0):
    """The oracle's C/OpenMP restatement of the reference's generated code
    (validated against the real reference's wall time on the same cores by
    ``tests/golden/_gen/time_reference.py``), timed on this box's host cores
    on the same N = 100 000 workload: OpenMP team sizes 1 and a few up to the
    physical core count, threads bound (``OMP_PROC_BIND=close``,
    ``OMP_PLACES=cores``), fresh ``free`` each repetition, min and median per
    team.  ``value`` is the best team's *reference-shaped* pair (fresh
    constraint array + transpose copy, as ``opty/direct_collocation.py:
    2444-2446``); the persistent-buffer variant is reported beside it."""
    import numpy as np
    from oracle.collocation_oracle import OracleCollocator, split_free
    from examples import problems
    cpu = host_cpu()
    cores = cpu['physical_cores']
    orc = OracleCollocator(name='config3_10link', parallel=True, **kw)
    con = orc.generate_constraint_function()
    jac = orc.generate_jacobian_function()
    frees = [problems.make_free(orc.num_free, seed=s) for s in range(3)]
    con(frees[0]), jac(frees[0])                   # warm-up / page-in

    # persistent-buffer variant: the compiled loops called directly on
    # preallocated outputs (no fresh array, no transpose copy)
    pcon = np.empty((orc.N - 1, orc.M))
    pjac = np.empty((orc.N - 1, orc.M*orc.C))
    consts = [float(orc.known_parameter_map[p]) for p in orc.parameters]

    def persistent(free):
        states, spec, _, _ = split_free(free, orc.n, orc.q, orc.N, False)
        vec = orc._node_vectors(states, np.atleast_2d(spec))
        orc._c_con(pcon, *vec, *consts, orc.node_time_interval)
        orc._c_jac(pjac, *vec, *consts, orc.node_time_interval)

    def shaped(free):
        con(free)
        jac(free)

    teams = sorted({t for t in (1, 8, 16, 32, cores//2, cores) if 1 <= t <=
                    max(1, cores)})
    results = {}
    per_team = budget_s/(2*len(teams))
    for threads in teams:
        orc._c_con.parallel = orc._c_jac.parallel = threads
        for label, fn in (('shaped', shaped), ('persistent', persistent)):
            for k in range(3):
                fn(frees[k])                       # 3 warm-ups
            ts = []
            t_end = time.perf_counter() + per_team
            while len(ts) < 20 or (time.perf_counter() < t_end and
                                   len(ts) < 60):
                f = frees[len(ts) % 3]
                t0 = time.perf_counter()
                fn(f)
                ts.append(time.perf_counter() - t0)
                if len(ts) >= 5 and time.perf_counter() > t_end + per_team:
                    break                          # a very slow team
            ts.sort()
            results[(threads, label)] = (ts[0], ts[len(ts)//2], len(ts))
    best = min(teams, key=lambda t: results[(t, 'shaped')][1])
    best_p = min(teams, key=lambda t: results[(t, 'persistent')][1])
    detail = '; '.join(
        '%d thr: shaped min %.1f / med %.1f ms, persistent min %.1f / med '
        '%.1f ms (%d reps)' % (
            t, 1e3*results[(t, 'shaped')][0], 1e3*results[(t, 'shaped')][1],
            1e3*results[(t, 'persistent')][0],
            1e3*results[(t, 'persistent')][1], results[(t, 'shaped')][2])
        for t in teams)
    return dict(
        value=1.0/results[(best, 'shaped')][1], unit='evals/s', cores=best,
        kind='port', stat='median',
        min_ms=1e3*results[(best, 'shaped')][0],
        median_ms=1e3*results[(best, 'shaped')][1],
        persistent_buffers={'evals_per_s':
                            1.0/results[(best_p, 'persistent')][1],
                            'cores': best_p,
                            'min_ms': 1e3*results[(best_p, 'persistent')][0],
                            'median_ms':
                            1e3*results[(best_p, 'persistent')][1]},
        host=cpu,
        sample='constraint+Jacobian evaluations of the full N=%d 10-link '
               'problem (same workload as the GPU line), OpenMP over nodes '
               '(gcc -O2 -fopenmp, OMP_PROC_BIND=%s OMP_PLACES=%s), 3 '
               'warm-ups then >= 20 repetitions per team, fresh free each; '
               'value = 1/median of the reference-shaped pair of the best '
               'team; CPU: %s, %d socket(s), %d physical cores, %d logical, '
               '%d NUMA node(s); %s' % (
                   orc.N, os.environ.get('OMP_PROC_BIND'),
                   os.environ.get('OMP_PLACES'), cpu['model'],
                   cpu['sockets'], cpu['physical_cores'],
                   cpu['logical_cpus'], cpu['numa_nodes'], detail))


def cpu_baseline(nodes):
    """Runs :func:`_cpu_baseline_impl` in a child process with the OpenMP
    binding environment and returns its dictionary."""
    import subprocess
    env = dict(os.environ, **CPU_BASELINE_ENV)
    proc = subprocess.run([sys.executable, os.path.abspath(__file__),
                           '--cpu-baseline-only', '--nodes', str(nodes)],
                          capture_output=True, text=True, env=env, cwd=REPO)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    if proc.returncode != 0 or not lines:
        return {'error': proc.stderr[-2000:]}
    return json.loads(lines[-1])


def lookup_traffic(kernel_sha):
    """HBM bytes per launch from the PMC passes (FETCH_SIZE x2 + WRITE_SIZE,
    collected separately with rocprofv3 as the microarch guide prescribes;
    summaries under profiles/), keyed on the sha-256 of the generated source
    of the kernel the counters were collected on (N = 100 000 launch): a
    changed kernel yields ``None``."""
    try:
        with open(os.path.join(REPO, 'profiles', 'traffic.json')) as f:
            return json.load(f)[kernel_sha]['hbm_bytes_per_launch']
    except (OSError, KeyError, ValueError, TypeError):
        return None


#: ``--dump-outputs``: bytes all files of a run may take, and constraint nodes
#: of the fixed, seeded sample of the Jacobian (the whole Jacobian of the
#: benchmark is 792 MB)
DUMP_BYTES = 64 << 20
DUMP_NODES = 4096


def dump_outputs(path, con2d, jac2d, a, b, ncn, suffix=''):
    """``--dump-outputs``: what the last timed step computed, as float64
    ``.npy`` files under ``path``.  ``con2d`` (M, b-a) / ``jac2d`` (b-a, P)
    are the outputs of the launch's constraint nodes [a, b) of ``ncn``
    (device tensors or arrays).  Written: ``jac_sample`` (k, P), the Jacobian
    blocks of a fixed, seeded sample of the ``ncn`` nodes (the first and the
    last node included; the part of it in [a, b)), their global node indices
    ``jac_sample_nodes``, and ``con`` (M, b-a), the constraints whole -- or,
    where they would take more than half of :data:`DUMP_BYTES`,
    ``con_sample`` (M, k) at the same nodes.  ``suffix`` tells the ranks of a
    multi-GPU run apart."""
    import numpy as np
    rng = np.random.default_rng(0)
    nodes = np.unique(np.concatenate([
        rng.choice(ncn, min(DUMP_NODES, ncn), replace=False), [0, ncn - 1]]))
    nodes = nodes[(nodes >= a) & (nodes < b)]
    sel = nodes - a
    whole_con = 8*con2d.shape[0]*ncn <= DUMP_BYTES//2
    if isinstance(jac2d, np.ndarray):
        jac = jac2d[sel]
        con = con2d if whole_con else con2d[:, sel]
    else:
        import torch
        idx = torch.from_numpy(sel).to(jac2d.device)
        jac = jac2d[idx].cpu().numpy()
        con = (con2d if whole_con else con2d[:, idx]).cpu().numpy()
    os.makedirs(path, exist_ok=True)
    for name, arr in (('con' if whole_con else 'con_sample', con),
                      ('jac_sample', jac), ('jac_sample_nodes', nodes)):
        np.save(os.path.join(path, name + suffix + '.npy'),
                np.ascontiguousarray(arr, dtype=np.float64))


#: entries of ``other_configs`` that are also timed with parameter-specialised
#: kernels (blocks bound by their arithmetic)
SPECIALISED_ENTRIES = ('config5_one_legged', 'config5_biped')


def other_configs(dev, iters):
    """Kernel times and HBM fractions of BASELINE config 2 and of the
    config-5 stand-in on this GPU (hipEvent-timed, single GPU)."""
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems
    out = {}
    for name in ('config2_pendulum', 'config5_standin_24link',
                 'config5_gaitlike_24link', 'config5_one_legged',
                 'config5_biped'):
        try:
            _other_config(name, dev, iters, out, torch, opty_amd, hb,
                          problems)
        except Exception as exc:     # noqa: the headline line must survive
            # (a build that the verification of DESIGN.md 4.1 refuses, a
            # problem that does not fit ...): recorded, not fatal
            out[name] = {'error': '%s: %s' % (type(exc).__name__,
                                             str(exc)[:600])}
            torch.cuda.empty_cache()
    return out


def config3_shards(kw, dev, iters, whole_ms):
    """BASELINE config 4's launches on THIS GPU: one of 2 / 4 / 8 node
    shards of the benchmark problem (what each GPU of a node launches: its own
    launch geometry from the launch plans, the global free vector, a node
    range from the middle), hipEvent-timed like the headline, with the
    verdict of the build verification of every shard's code object.
    ``speedup_vs_whole`` = headline launch time / shard launch time: the
    strong scaling of the evaluation with the outputs left distributed."""
    import torch
    import opty_amd
    from opty_amd import hip_backend as hb
    from opty_amd.sharded import partition_nodes
    from examples import problems
    out = {}
    base = opty_amd.ConstraintCollocator(device=dev.index, **kw)
    prog = base._build_program()
    ncn = base.num_collocation_nodes - 1
    free = torch.from_numpy(problems.make_free(base.num_free)).to(dev)
    for world in (2, 4, 8):
        try:
            a, b = partition_nodes(ncn, world)[world//2]
            shard = opty_amd.ConstraintCollocator(
                device=dev.index, launch_nodes=b - a, **kw)
            shard._program = prog
            sh = shard.hip
            sh.use_torch_stream()
            scon = torch.empty((prog.M, b - a), dtype=torch.float64,
                               device=dev)
            sjac = torch.empty((b - a)*prog.P, dtype=torch.float64,
                               device=dev)
            sh.time_eval_shard(hb.EVAL_FUSED, free, scon, b - a, sjac, a, b,
                               max(3, iters//4))
            ms = min(sh.time_eval_shard(hb.EVAL_FUSED, free, scon, b - a,
                                        sjac, a, b, iters) for _ in range(3))
            out['shard_1of%d' % world] = dict(
                nodes=b - a, fused_ms=ms, speedup_vs_whole=whole_ms/ms,
                build_check=_build_check(shard), **_routing(sh, b - a))
            sh.close()
            del scon, sjac
        except Exception as exc:         # noqa: the headline must survive
            out['shard_1of%d' % world] = {'error': '%s: %s' % (
                type(exc).__name__, str(exc)[:400])}
        torch.cuda.empty_cache()
    return out


def _build_check(col):
    """What the verification of the code object in use said (every build is
    held to its expression DAG, run as an instruction tape on the GPU, before
    its handle exists: DESIGN.md 4.1)."""
    v = getattr(col, '_build_verdict', None)
    if not v:
        return None
    # (isa_exec_copies: what the static ISA check found in the build in
    # use, {} = clean; isa_replaced: it replaced a build with such copies;
    # vector_spills_in_service: spilling kernels an entry point can launch
    # -- must be {}; banned_kernels: spilling kernels no entry point
    # launches)
    return {k: v.get(k) for k in (
        'ok', 'referee', 'referee_version', 'worst', 'nodes', 'replacement',
        'isa_exec_copies', 'isa_replaced', 'banned_kernels',
        'vector_spills_in_service') if v.get(k) is not None}


def _routing(hip, nodes=None):
    """What the handle's entry points launch for this launch size, as the
    handle measured it on this device (``opty_hip_routing``)."""
    r = hip.routing(nodes)
    out = dict(routing=r['routing'], fused_pays=not r['fused_loses'],
               jac_via_fused=r['jac_via_fused'])
    if 'ms' in r:
        out['calibration_ms'] = {k: round(float(v), 6)
                                 for k, v in r['ms'].items()}
    return out


def _other_config(name, dev, iters, out, torch, opty_amd, hb, problems):
    pkw = problems.build(name)
    col = opty_amd.ConstraintCollocator(device=dev.index, **pkw)
    hip = col.hip
    hip.use_torch_stream()
    free = torch.from_numpy(problems.make_free(
        col.num_free, variable_duration=col._variable_duration)).to(dev)
    con = torch.empty(col.num_constraints, dtype=torch.float64,
                      device=dev)
    jac = torch.empty(hip.nnz, dtype=torch.float64, device=dev)
    res = {}
    # 'opty_conjac' is what OPTY_HIP_EVAL_FUSED / opty_hip_eval_con_jac issue
    # for this problem: the fused kernel, or -- when the launch plan measured
    # it slower (opty_hip_desc.fused_loses) -- opty_con followed by opty_jac;
    # 'opty_conjac_kernel' is the fused kernel itself in that case
    whats = [(hb.EVAL_CON, 'opty_con'), (hb.EVAL_JAC, 'opty_jac'),
             (hb.EVAL_FUSED, 'opty_conjac')]
    for what, label in whats:
        ms0 = hip.time_eval(what, free, con, jac, max(3, iters//4))
        # (best of three batches of at least ~4 ms each: the entries are
        # compared with each other to a per cent -- fused against the pair,
        # opty_jac against fused -- and twenty launches of a 30 us kernel do
        # not resolve a per cent)
        n = min(2000, max(iters, int(4.0/max(ms0, 1e-4)) + 1))
        res[label] = min(hip.time_eval(what, free, con, jac, n)
                         for _ in range(3))
    route = _routing(hip)
    if not route['fused_pays'] and not hip.desc['routing'] & \
            hb.ROUTE_NO_FUSED_KERNEL:
        hip.time_eval(hb.EVAL_FUSED_KERNEL, free, con, jac,
                      max(3, iters//4))
        res['opty_conjac_kernel'] = hip.time_eval(
            hb.EVAL_FUSED_KERNEL, free, con, jac, iters)
    nbytes = 8.0*(col.num_free + col.num_constraints + hip.nnz)
    serial = res['opty_con'] + res['opty_jac']
    out[name] = dict(
        nodes=col.num_collocation_nodes, nnz=hip.nnz, kernel_ms=res,
        fused_algorithmic_bytes=nbytes,
        fused_hbm_frac=nbytes/(res['opty_conjac']*1e-3)/1e9/HBM_PEAK_GBS,
        evals_per_s=1e3/res['opty_conjac'],
        serial_evals_per_s=1e3/serial,
        # (every launch of this entry reads ONE free vector; the headline
        # rotates four -- 1-2 % of the bytes of a write stream)
        free_vectors=1,
        # (True: the generic module of this problem spills hundreds of scalar
        # registers, so the collocator printed its known parameters into
        # the kernels as literals on its own -- the default since r06,
        # ConstraintCollocator(specialize_parameters=None); rebuilt when the
        # known parameter map changes)
        auto_specialised=bool(col._auto_specialized),
        build_check=_build_check(col), **route)
    if name in SPECIALISED_ENTRIES:
        # opt-in: node-invariant values as literals of the kernels
        # (ConstraintCollocator(specialize_parameters=True): for solves with
        # fixed known parameters; rebuilt when they change)
        spec = opty_amd.ConstraintCollocator(
            device=dev.index, specialize_parameters=True, **pkw)
        spec._program = col._program
        sp = spec.hip
        sp.use_torch_stream()
        sres = {}
        for what, label in whats[:3]:
            sp.time_eval(what, free, con, jac, max(3, iters//4))
            sres[label] = sp.time_eval(what, free, con, jac, iters)
        out[name]['specialised_parameters'] = dict(
            kernel_ms=sres,
            fused_hbm_frac=nbytes/(sres['opty_conjac']*1e-3)/1e9 /
            HBM_PEAK_GBS,
            build_check=_build_check(spec))
        sp.close()
    if name.startswith('config5'):
        # one of eight node shards of the same problem (what each GPU of
        # an 8-GPU node launches): its own launch geometry, the global
        # free vector, a node range from the middle
        from opty_amd.sharded import partition_nodes
        ncn = col.num_collocation_nodes - 1
        a, b = partition_nodes(ncn, 8)[3]
        shard = opty_amd.ConstraintCollocator(
            device=dev.index, launch_nodes=b - a, **pkw)
        shard._program = col._program            # same equations
        sh = shard.hip
        sh.use_torch_stream()
        prog = col._build_program()
        scon = torch.empty((prog.M, b - a), dtype=torch.float64,
                           device=dev)
        sh.time_eval_shard(hb.EVAL_FUSED, free, scon, b - a, jac, a, b,
                           max(3, iters//4))
        ms = min(sh.time_eval_shard(hb.EVAL_FUSED, free, scon, b - a,
                                    jac, a, b, iters) for _ in range(3))
        out[name]['shard_1of8'] = dict(
            nodes=b - a, fused_ms=ms,
            speedup_vs_whole=res['opty_conjac']/ms,
            build_check=_build_check(shard), **_routing(sh, b - a))
        sh.close()
        del scon
    if name == 'config2_pendulum':
        # the cyipopt-callback path of the small config (NumPy in / out,
        # PCIe and sync latency inclusive); the reference's compiled C
        # takes 140 us + 189 us on one core
        import numpy as np
        hip.set_stream(None)
        cf = col.generate_constraint_function(recycle=True)
        jf = col.generate_jacobian_function()
        hf = [problems.make_free(col.num_free, seed=s) for s in range(3)]
        lat = {}
        for label, fn in (('con', cf), ('jac', jf)):
            fn(hf[0])
            ts = []
            for k in range(50):
                t0 = time.perf_counter()
                fn(hf[k % 3])
                ts.append(time.perf_counter() - t0)
            lat[label] = 1e6*float(np.median(ts))
        out[name]['host_path_us'] = lat
    hip.close()
    del con, jac, free
    torch.cuda.empty_cache()


def host_path(kw, dev_index, reps=15):
    """Wall time of the host (cyipopt-callback) path of config 3: NumPy in,
    NumPy out through ``generate_*_function`` (PCIe inclusive): the
    reference's dense-block contract as the callbacks serve it (``jac``:
    after the first call only the entries that can change cross PCIe,
    ``opty_hip_eval_jac_persistent``), the same vector copied whole every call
    (``jac_dense_copy``), ``prune_zeros=True`` and
    ``jacobian_layout='varying_first'`` (the same triplets, ordered so that
    no host scatter is needed)."""
    import opty_amd
    from opty_amd import hip_backend as hb
    from examples import problems

    def med(fn, frees, warm=1):
        for k in range(warm):
            fn(frees[k % len(frees)])
        ts = []
        for k in range(reps):
            t0 = time.perf_counter()
            fn(frees[k % len(frees)])
            ts.append(time.perf_counter() - t0)
        # (the hosts are shared: the median of 15 calls -- 70 ms -- rides out
        # a burst of somebody else's load that the median of 7 did not; the
        # fastest call is recorded next to it)
        best[0] = 1e3*min(ts)
        return 1e3*sorted(ts)[len(ts)//2]

    best = [0.0]
    out = {}
    for label, extra in (('', {}), ('_pruned', {'prune_zeros': True}),
                         ('_varying_first',
                          {'jacobian_layout': 'varying_first'})):
        col = opty_amd.ConstraintCollocator(device=dev_index, **extra, **kw)
        frees = [problems.make_free(col.num_free, seed=s) for s in range(3)]
        if not label:
            out['con'] = med(col.generate_constraint_function(recycle=True),
                             frees)
            dense = hb.pinned_empty(col.hip.nnz)
            out['jac_dense_copy'] = med(
                lambda f: col.hip.eval_jac(f, dense, hb.HOST), frees)
            del dense
            from opty_amd.codegen.program import (varying_copies,
                                                   scaled_copies)
            unique, copies = varying_copies(col._build_program())
            out['varying_entries_per_block'] = len(unique) + len(copies)
            # ... of which only the distinct expressions cross PCIe (r05),
            # and of those only one per group of node-invariant multiples
            # of the same per-node expression (r06)
            out['moved_entries_per_block_r05'] = len(unique)
            moved = len(scaled_copies(col._build_program())[0]) \
                if getattr(col, '_copy_chains', None) else len(unique)
            out['moved_entries_per_block'] = moved
            out['host_threads'] = hb.host_threads()
            ncn = col.num_collocation_nodes - 1
            pcie = {'h2d_bytes': 8*col.num_free, 'd2h_bytes': 8*moved*ncn}
        # (the host scatter verifies its thread placement over the first
        # calls with every new vector -- csrc/host_scatter.cpp ScatterPool::feedback;
        # they are warm-up, for each of the three collocators)
        jf = col.generate_jacobian_function()
        out['jac' + label] = med(jf, frees, warm=14)
        out['jac' + label + '_min'] = best[0]
        if not label:
            # where the bytes and the threads are (so that a slow line can be
            # read): NUMA node of the persistent vector, of the scatter
            # workers, of the device
            w, d, verified = hb.host_placement()
            out['placement'] = {
                'vector_node': hb.host_numa_node(jf(frees[0])),
                'workers_node': w, 'device_node': d,
                'verified_by_measurement': verified}
        out['nnz' + label] = col.hip.nnz
        col.hip.close()
    # regression guard: the reference-ordered default layout
    # must stay within 15 % of the scatter-free opt-in layout, which sits on
    # the PCIe link
    # The host path's own roofline: the bytes one jacobian(free) moves over
    # the link against what the link does on THIS box (page-locked
    # hipMemcpy of 256 MB either way, best of 5); `frac` and
    # `frac_download_only` below.
    try:
        n = 32 << 20
        hbuf = hb.pinned_empty(n)
        hbuf[:] = 1.0
        dbuf = hb.DeviceVector(hbuf[:1], dev_index)
        dbuf.close()
        lib = hb.load_library()
        dptr = lib.opty_hip_device_alloc(dev_index, 8*n)
        rates = {}
        for tag, kind, dst, src in (('h2d', 0, dptr, hbuf.ctypes.data),
                                    ('d2h', 1, hbuf.ctypes.data, dptr)):
            ts = []
            for _ in range(6):
                t0 = time.perf_counter()
                hb._check(lib.opty_hip_memcpy(dst, src, 8*n, kind))
                ts.append(time.perf_counter() - t0)
            rates[tag] = 8*n/min(ts[1:])/1e9
        lib.opty_hip_device_free(dptr)
        del hbuf
        pcie['link_GBps'] = rates
        pcie['d2h_GBps_achieved'] = pcie['d2h_bytes']/(out['jac']*1e-3)/1e9
        # `frac` as VERDICT r05 item 3 defines it: the bytes a call moves,
        # BOTH ways, over the median call, against the measured (one-way)
        # link rate.  The link is full duplex and the upload rides in the
        # shadow of the download, so the stricter reading is the download
        # alone: `frac_download_only`
        moved = pcie['h2d_bytes'] + pcie['d2h_bytes']
        pcie['GBps_achieved'] = moved/(out['jac']*1e-3)/1e9
        pcie['frac'] = pcie['GBps_achieved']/rates['d2h']
        pcie['frac_download_only'] = pcie['d2h_GBps_achieved']/rates['d2h']
        pcie['frac_download_only_best_call'] = pcie['d2h_bytes']/(
            out['jac_min']*1e-3)/1e9/rates['d2h']
        pcie['bound_ms'] = 1e3*pcie['d2h_bytes']/(rates['d2h']*1e9)
    except Exception as exc:             # noqa: secondary figure
        pcie['error'] = '%s: %s' % (type(exc).__name__, str(exc)[:200])
    out['pcie'] = pcie
    out['jac_guard'] = {
        'ok': bool(out['jac'] <= 1.15*out['jac_varying_first']),
        'ratio': out['jac']/out['jac_varying_first'], 'limit': 1.15}
    out['pair_evals_per_s'] = 1e3/(out['con'] + out['jac'])
    out['pair_pruned_evals_per_s'] = 1e3/(out['con'] + out['jac_pruned'])
    # the reference's triplets in another order (opt-in): the entries that
    # can change stream into the head of the persistent array, no scatter
    out['pair_varying_first_evals_per_s'] = 1e3/(
        out['con'] + out['jac_varying_first'])
    return out


class _Verifier(object):
    """Checks outputs of the benched launches against the REFERENCE's golden
    record of this workload (``tests/golden/config3_10link.npz``: full blocks
    at a strided node sample, per-entry / per-equation sums over ALL nodes,
    recorded from csu-hmc/opty's compiled path by
    ``tests/golden/_gen/make_golden.py``; ``frees[0]`` is its seed-0 vector).
    Runs after the timed region, never inside it.

    Tolerance: 1e-10 relative per sampled entry, an entry that cancels to
    (nearly) nothing being held to 1e-10 of the largest entry of its own
    equation row at its own node; sums to 1e-9 of the mean absolute entry
    times the node count."""

    def __init__(self, M, P, N, dev):
        import numpy as np
        with open(os.path.join(REPO, 'tests', 'golden',
                               'MANIFEST.json')) as f:
            self.meta = json.load(f)[WORKLOAD]
        self.z = np.load(os.path.join(REPO, 'tests', 'golden',
                                      WORKLOAD + '.npz'))
        assert (self.meta['N'], self.meta['M'], self.meta['M'] *
                self.meta['C']) == (N, M, P)
        self.M, self.P, self.N, self.dev = M, P, N, dev
        self.C = P//M
        self.worst = 0.0
        self.failed = []
        self.checked = []

    def _entries(self, got, want, rowmax, label):
        import numpy as np
        err = np.abs(got - want)
        ref = np.maximum(np.abs(want), rowmax)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.where(ref > 0, err/ref, err)
        worst = float(np.nanmax(rel)) if rel.size else 0.0
        if not np.isfinite(got).all():
            worst = float('inf')
        self.worst = max(self.worst, worst)
        if not worst <= 1e-10:
            self.failed.append('%s: worst relative error %.3g' % (label,
                                                                  worst))

    def nodes(self, con2d, jac2d, a, b, label):
        """``con2d`` (M, b-a) / ``jac2d`` (b-a, P) tensors or arrays of the
        constraint nodes [a, b): the reference's sampled nodes among them."""
        import numpy as np
        nodes = self.z['nodes']
        pick = (nodes >= a) & (nodes < b)
        sel = nodes[pick] - a
        if not len(sel):
            return
        want_j = self.z['jac_nodes'][pick]
        rowmax = np.abs(want_j.reshape(len(sel), self.M, self.C)).max(axis=2)
        if not isinstance(jac2d, np.ndarray):       # device tensors
            import torch
            idx = torch.from_numpy(sel).to(jac2d.device)
            got_j = jac2d[idx].cpu().numpy()
            got_c = con2d[:, idx].cpu().numpy()
        else:
            got_j, got_c = jac2d[sel], con2d[:, sel]
        self._entries(got_j, want_j, np.repeat(rowmax, self.C, axis=1),
                      label + ' jac nodes')
        self._entries(got_c, self.z['con_nodes'][:, pick], rowmax.T,
                      label + ' con nodes')
        self.checked.append('%s: %d sampled nodes' % (label, len(sel)))

    def sums(self, jac_sum, con_sum, jac_abs, con_abs, label):
        """Sums over ALL constraint nodes (already reduced over the ranks):
        per block entry (P,), per equation (M,), of |jac| and of |con| (the
        scale of the constraint sums)."""
        import numpy as np
        scale = float(self.z['jac_abs_sum'][0])
        for got, want, ref, tag in (
                (jac_sum, self.z['jac_entry_sums'], scale/self.P,
                 'jac entry sums'),
                (con_sum, self.z['con_eq_sums'], float(con_abs)/self.M,
                 'con sums'),
                (np.array([jac_abs]), self.z['jac_abs_sum'], scale,
                 'jac abs sum')):
            got = np.asarray(got, dtype=float)
            rel = np.abs(got - want)/np.maximum(np.abs(want), ref)
            worst = float(np.nanmax(rel)) if np.isfinite(got).all() \
                else float('inf')
            self.worst = max(self.worst, worst*0.1)     # bar is 1e-9
            if not worst <= 1e-9:
                self.failed.append('%s %s: %.3g' % (label, tag, worst))
        self.checked.append(label + ': checksums over all nodes')


def main_no_torch(args):
    """``bench.py --no-torch``: the headline step driven through ctypes
    alone (BASELINE.json north_star: "Python host code calls, through a thin
    ctypes C-ABI layer ...").  Same workload, same K / W / prewarm contract,
    same JSON keys for the headline and its roofline; the secondary figures
    are the torch line's.  N > 1: launch one process per GPU with the usual
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* environment (torch.distributed
    .run exports it; no torch process group is created)."""
    os.environ['OPTY_HIP_NO_TORCH'] = '1'
    import numpy as np
    from opty_amd import hip_backend as hb
    from opty_amd.shard_host import (NodeShard, RcclTransport,
                                     SocketTransport, launch_env)
    from examples import problems
    rank, world, local_rank, addr, port = launch_env()
    assert world == max(1, args.gpus), 'one process per GPU (WORLD_SIZE)'
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    oversub = os.environ.get('OPTY_BENCH_OVERSUBSCRIBE') == '1'
    ndev = hb.load_library().opty_hip_device_count()
    if oversub:
        local_rank %= max(1, ndev)
    side = SocketTransport(rank, world, addr, port)
    transport = None
    if world > 1 and not oversub:
        transport = RcclTransport(side, device=local_rank)
    strong = not args.weak
    factory, fkw = problems.CONFIGS[WORKLOAD]
    kw = factory(**dict(fkw, num_nodes=args.nodes))
    sh = NodeShard(rank=rank if strong else 0,
                   world_size=world if strong else 1,
                   transport=(transport or side) if strong and world > 1
                   else None, device=local_rank, **kw)
    col = sh.collocator
    hip = col.hip
    a, b, M, P, N = sh.a, sh.b, sh.M, sh.P, sh.N
    cnt = b - a
    frees = [hb.DeviceVector(problems.make_free(
        sh.num_free, seed=s + (0 if strong else 1000*rank)), local_rank)
        for s in range(4)]
    from opty_amd.shard_host import _device_empty
    con, jac = _device_empty(M*cnt, local_rank), \
        _device_empty(cnt*P, local_rank)
    what = hb.EVAL_PAIR if args.serial else hb.EVAL_FUSED
    lib, h = hb.load_library(), hip._h
    fp = [f.data_ptr() for f in frees]
    cp, jp = con.data_ptr(), jac.data_ptr()

    def step(k):
        hb._check(lib.opty_hip_eval_shard(h, what, fp[k % 4], cp, cnt, jp, a,
                                          b))

    def barrier():
        hip.synchronize()
        side.barrier()
        hip.synchronize()

    t_ramp = time.perf_counter()
    k = 0
    while (time.perf_counter() - t_ramp)*1e3 < args.prewarm_ms:
        for _ in range(16):
            step(k)
            k += 1
        hip.synchronize()
    for k in range(args.warmup):
        step(k)
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    barrier()
    el = time.perf_counter() - t0
    parts = side.gather_bytes(repr(el).encode(), 0)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, con.numpy().reshape(M, cnt),
                     jac.numpy().reshape(cnt, P), a, b, N - 1,
                     '' if world == 1 else '_rank%d' % rank)
    if args.full:
        jac_ms = hip.time_eval_shard(hb.EVAL_JAC, frees[0], None, cnt, jac,
                                     a, b, args.steps)
        con_ms = hip.time_eval_shard(hb.EVAL_CON, frees[1], con, cnt, None,
                                     a, b, args.steps)
        fused_ms = hip.time_eval_shard(hb.EVAL_FUSED, frees[2], con, cnt,
                                       jac, a, b, args.steps)
    # what was benched, against the reference's golden record
    verify = {'ok': None, 'skipped': 'no reference golden for N = %d'
              % args.nodes}
    if not args.full:
        verify = {'ok': None, 'skipped': 'checked with --full'}
    elif args.nodes == 100000 and strong:
        step(0)
        hip.synchronize()
        ver = _Verifier(M, P, N, None)
        ver.nodes(con.numpy().reshape(M, cnt), jac.numpy().reshape(cnt, P),
                  a, b, 'benched launch (rank %d)' % rank)
        fails = side.gather_bytes(json.dumps(
            [ver.failed, ver.checked, ver.worst]).encode(), 0)
        if rank == 0:
            got = [json.loads(f) for f in fails]
            verify = {'ok': not any(g[0] for g in got),
                      'worst_rel': max(g[2] for g in got), 'ranks': world,
                      'checked': sum((g[1] for g in got), []),
                      'failed': sum((g[0] for g in got), []),
                      'golden': 'tests/golden/%s.npz' % WORKLOAD}
    route = _routing(hip, cnt)
    build = _build_check(col)
    loaded_torch = 'torch' in sys.modules
    side.barrier()
    if rank == 0:
        elapsed = max(float(p.decode()) for p in parts)
        free_bytes = 8.0*((col.num_states +
                           col.num_unknown_input_trajectories)*(cnt + 1))
        if args.serial or not route['fused_pays']:
            dom = 'opty_jac'
            dom_bytes = free_bytes + 8.0*P*cnt
        else:
            dom = 'opty_conjac'
            dom_bytes = free_bytes + 8.0*M*cnt + 8.0*P*cnt
        kmeta = col._kernel_meta['kernels'][
            'jac' if dom == 'opty_jac' and not route['jac_via_fused']
            else 'conjac']
        line = {
            'metric': 'constraint+Jacobian evals/sec at N=100k nodes '
                      '(10-link pendulum on cart, backward Euler)',
            'value': args.steps*(1 if strong else world)/elapsed,
            'unit': 'evals/s', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': 1e3*elapsed/args.steps,
            'higher_is_better': True,
            'scaling': 'strong' if strong else 'weak', 'vs_baseline': None,
            'dtype': 'f64', 'data': 'synthetic',
            'config': {
                'workload': '10-link inverted pendulum on cart, %d nodes, '
                            'backward Euler, n=M=22, q=1, C=45, nnz=%d'
                            % (N, P*(N - 1)),
                'host': 'ctypes through include/opty_hip.h, no torch in the '
                        'process (torch imported: %s)' % loaded_torch,
                'step': 'constraints and Jacobian of one free vector from '
                        'one opty_hip_eval_shard call',
                'sharding': 'ONE problem, constraint nodes [%d, %d) of %d on '
                            'rank 0; outputs left distributed, no data-path '
                            'collective' % (a, b, N - 1),
                'oversubscribed': bool(oversub),
                'prewarm_ms': args.prewarm_ms, 'build_check': build,
                'routing': route, 'kernel_sha': kmeta['sha'][:16],
                'nodes_per_launch': cnt, 'verify': verify},
        }
        if args.full:
            dom_ms = jac_ms if dom == 'opty_jac' else fused_ms
            achieved = dom_bytes/(dom_ms*1e-3)/1e9
            line['config']['kernel_ms'] = {
                'opty_jac': jac_ms, 'opty_con': con_ms,
                'opty_conjac': fused_ms}
            line['roofline'] = {
                'bound': 'hbm', 'kernel': dom, 'achieved': achieved,
                'algorithmic_bytes_per_launch': dom_bytes,
                'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                'frac': achieved/HBM_PEAK_GBS,
                'traffic': lookup_traffic(kmeta['sha'])
                if (world == 1 and args.nodes == 100000) else None}
        print(json.dumps(line))
    assert not loaded_torch, 'torch was imported in --no-torch mode'
    for v in frees + [con, jac]:
        v.close()
    sh.close()
    if transport is not None:
        transport.close()
    side.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--nodes', type=int, default=100000,
                    help='collocation nodes of the problem (sharded over the '
                         'ranks; per rank with --weak)')
    ap.add_argument('--weak', action='store_true',
                    help='weak scaling: every rank evaluates its own '
                         '--nodes-node problem (default: strong scaling, ONE '
                         '--nodes-node problem sharded over the ranks = '
                         'BASELINE config 4)')
    ap.add_argument('--serial', action='store_true',
                    help='two launches per step (constraints, then Jacobian) '
                         'instead of the fused one')
    ap.add_argument('--prewarm-ms', type=float, default=150.0,
                    help='untimed clock-ramp phase before the warm-up steps '
                         '(wall milliseconds of the same step; 0 disables)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, everything else the benchmark '
                         'measures or checks: per-kernel times and roofline, '
                         'the check against the reference\'s golden record, '
                         'the secondary figures and the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write what the last timed step computed as .npy '
                         'files under DIR (constraints whole, a fixed sample '
                         'of the Jacobian\'s node blocks)')
    ap.add_argument('--no-cpu-baseline', action='store_true',
                    help='with --full: skip the CPU baseline')
    ap.add_argument('--cpu-baseline-only', action='store_true',
                    help='(internal) time the CPU baseline in this process '
                         'and print its JSON')
    ap.add_argument('--no-extras', action='store_true',
                    help='with --full: skip the secondary figures (serial '
                         'pair, host path, other configs, re-assembly '
                         'variants)')
    ap.add_argument('--no-torch', action='store_true',
                    help='the same step and line from a process that never '
                         'imports torch: device memory, launches, hipEvent '
                         'timing and (N > 1) the RCCL communicator through '
                         'the C ABI, rendezvous over a TCP side channel '
                         '(opty_amd.shard_host)')
    args = ap.parse_args()

    if args.no_torch:
        return main_no_torch(args)

    if args.cpu_baseline_only:
        from examples import problems
        factory, fkw = problems.CONFIGS[WORKLOAD]
        print(json.dumps(_cpu_baseline_impl(
            factory(**dict(fkw, num_nodes=args.nodes)))))
        return

    import torch
    import torch.distributed as dist
    from opty_amd import hip_backend as hb
    from examples import problems
    from opty_amd.sharded import ShardedCollocator, SharedHostVector

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    # Development aid: OPTY_BENCH_OVERSUBSCRIBE=1 lets several ranks share one
    # GPU (gloo rendezvous; RCCL refuses duplicate devices) so that the
    # multi-process launch path can be exercised on a 1-GPU box.  The result
    # is flagged in `config` and is not a scaling measurement.
    oversub = os.environ.get('OPTY_BENCH_OVERSUBSCRIBE') == '1' and \
        world > torch.cuda.device_count()
    if oversub:
        local_rank %= torch.cuda.device_count()
    if args.gpus > 1 or world > 1:
        assert world == args.gpus, 'launch with torch.distributed.run'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # ONE node by contract: RCCL's bootstrap socket on the loopback
        # interface, not whichever the container has (data goes over xGMI)
        os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
        if oversub:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=torch.device(
                'cuda', local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    strong = not args.weak

    factory, fkw = problems.CONFIGS[WORKLOAD]
    kw = factory(**dict(fkw, num_nodes=args.nodes))
    # Strong scaling: the handle is built for the global problem and
    # evaluates this rank's node range of it.  Weak scaling (and one GPU):
    # the rank's range is the whole problem.
    sh = ShardedCollocator(rank=rank if strong else 0,
                           world_size=world if strong else 1,
                           device=dev, **kw)
    col = sh.collocator
    hip = col.hip
    hip.use_torch_stream()
    a, b = sh.a, sh.b
    M, P, N = sh.M, sh.P, sh.N
    nfree = col.num_free

    frees = [torch.from_numpy(problems.make_free(
        nfree, seed=s + (0 if strong else 1000*rank))).to(dev)
        for s in range(4)]
    con, jac = sh.con_local, sh.jac_local           # (M, b-a), ((b-a)*P,)
    cs = con.stride(0)
    # raw addresses: the step is one ctypes call
    fp = [f.data_ptr() for f in frees]
    cp, jp = con.data_ptr(), jac.data_ptr()

    def step(k, serial=args.serial):
        f = fp[k % 4]
        if serial:
            hip.eval_shard(hb.EVAL_CON, f, cp, cs, None, a, b)
            hip.eval_shard(hb.EVAL_JAC, f, None, cs, jp, a, b)
        else:
            hip.eval_shard(hb.EVAL_FUSED, f, cp, cs, jp, a, b)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, warmup):
        for k in range(warmup):
            fn(k)
        barrier()
        t0 = time.perf_counter()
        for k in range(steps):
            fn(k)
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = t.item()
        return el

    # Clock ramp: an idle MI355X sits at its lowest shader clock and needs a
    # few tens of milliseconds of work to reach the sustained one.  The same
    # step is run untimed for `--prewarm-ms` of wall time before the W
    # warm-up steps, so that the K timed steps measure the steady state
    # whatever K and W are.
    t_ramp = time.perf_counter()
    k = 0
    while (time.perf_counter() - t_ramp)*1e3 < args.prewarm_ms:
        for _ in range(16):
            step(k)
            k += 1
        torch.cuda.synchronize()
    elapsed = timed(step, args.steps, args.warmup)
    if args.dump_outputs:
        # (before anything else is launched: the buffers hold the last
        # timed step's outputs)
        dump_outputs(args.dump_outputs, con, jac.view(b - a, P), a, b, N - 1,
                     '' if world == 1 else '_rank%d' % rank)

    def headline(extras, verify, kernel_ms=None):
        """The JSON line (rank 0); ``kernel_ms``: the per-kernel times of
        ``--full`` (and with them the roofline), None in a plain run."""
        cnt = b - a
        free_bytes = 8.0*((col.num_states +
                           col.num_unknown_input_trajectories)*(cnt + 1))
        # algorithmic bytes of one launch: read the free
        # columns of the launch's nodes once, write the outputs once
        jac_bytes = free_bytes + 8.0*P*cnt
        con_bytes = free_bytes + 8.0*M*cnt
        route = _routing(hip, cnt)
        if args.serial or not route['fused_pays']:
            # (two launches per step -- asked for, or because the handle
            # measured opty_con + opty_jac faster than the fused kernel on
            # this device: the Jacobian kernel is the dominant one)
            dom, dom_bytes = 'opty_jac', jac_bytes
        else:
            dom = 'opty_conjac'
            dom_bytes = free_bytes + 8.0*M*cnt + 8.0*P*cnt
        kmeta = col._kernel_meta['kernels'][
            'jac' if dom == 'opty_jac' and not route['jac_via_fused']
            else 'conjac']
        value = args.steps*(1 if strong else world)/elapsed
        nnz_total = P*(N - 1)*(1 if strong else world)
        out = {
            'metric': 'constraint+Jacobian evals/sec at N=100k nodes '
                      '(10-link pendulum on cart, backward Euler)',
            'value': value, 'unit': 'evals/s', 'n_gpus': world,
            'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': 1e3*elapsed/args.steps,
            'higher_is_better': True,
            'scaling': 'strong' if strong else 'weak',
            'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {
                'workload': (
                    '10-link inverted pendulum on cart, %d nodes%s, backward '
                    'Euler, n=M=22, q=1, C=45, nnz=%d' % (
                        N, ' per GPU' if not strong else
                        (' sharded over %d GPUs (BASELINE config 4)' % world
                         if world > 1 else ''), nnz_total)),
                'step': ('constraints then Jacobian, two launches'
                         if args.serial else
                         'constraints and Jacobian of one free vector from '
                         'one launch (opty_hip_eval_shard / '
                         'opty_hip_eval_con_jac)'),
                'sharding': (
                    'ONE problem, constraint nodes [%d, %d) of %d on rank 0 '
                    '(contiguous ranges, one-node halo); outputs left '
                    'distributed, no data-path collective' % (a, b, N - 1)
                    if strong else
                    'independent %d-node problems, one per GPU' % N),
                'oversubscribed': bool(oversub),
                'prewarm_ms': args.prewarm_ms,
                'code_object_sha': col._kernel_meta['sha'][:16],
                'build_check': _build_check(col),
                'routing': route,
                'kernel_sha': kmeta['sha'][:16],
                'jac_waves_per_block': hip.desc['jac_wgs_per_block'] *
                hip.desc['jac_waves_per_wg'],
                'nodes_per_launch': cnt,
            },
        }
        if kernel_ms is not None:
            dom_ms = kernel_ms[dom]
            achieved = dom_bytes/(dom_ms*1e-3)/1e9
            traffic = lookup_traffic(kmeta['sha']) \
                if (world == 1 and args.nodes == 100000) else None
            out['config']['GBps_nnz_written'] = \
                8.0*P*cnt/(kernel_ms['opty_jac']*1e-3)/1e9
            out['config']['kernel_ms'] = kernel_ms
            out['roofline'] = {
                'bound': 'hbm', 'kernel': dom, 'achieved': achieved,
                'algorithmic_bytes_per_launch': dom_bytes,
                'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                'frac': achieved/HBM_PEAK_GBS, 'traffic': traffic}
        out['config'].update(extras)
        out['config']['verify'] = verify
        if args.full and not args.no_cpu_baseline and world == 1:
            out['cpu_baseline'] = cpu_baseline(args.nodes)
        return out

    if not args.full:
        if rank == 0:
            print(json.dumps(headline({}, {'ok': None,
                                           'skipped': 'checked with --full'})))
        if world > 1:
            dist.destroy_process_group()
        return

    # Kernel durations, measured live with HIP events on the launch stream.
    jac_ms = hip.time_eval_shard(hb.EVAL_JAC, frees[0], None, cs, jac, a, b,
                                 args.steps)
    con_ms = hip.time_eval_shard(hb.EVAL_CON, frees[1], con, cs, None, a, b,
                                 args.steps)
    fused_ms = hip.time_eval_shard(hb.EVAL_FUSED, frees[2], con, cs, jac, a,
                                   b, args.steps)
    kernel_ms = {'opty_jac': jac_ms, 'opty_con': con_ms,
                 'opty_conjac': fused_ms}
    barrier()

    # ---- verification of what was benched (after the timed region) ----------
    # frees[0] is the seed-0 vector the reference's golden record of this
    # workload was made with; the check runs the very launch that was timed.
    verifier = None
    verify = {'ok': None, 'skipped': 'no reference golden for N = %d'
              % args.nodes}
    if args.nodes == 100000:
        verifier = _Verifier(M, P, N, dev)

    def reduce_sum(t):
        if world > 1 and strong:
            if oversub:
                h = t.cpu()
                dist.all_reduce(h)
                return h
            dist.all_reduce(t)
        return t.cpu()

    def check_sums(con2d, jac2d, label, reduce=True):
        part = torch.cat([jac2d.sum(0), con2d.sum(1),
                          jac2d.abs().sum().view(1),
                          con2d.abs().sum().view(1)])
        part = (reduce_sum(part) if reduce else part.cpu()).numpy()
        verifier.sums(part[:P], part[P:P + M], part[P + M], part[P + M + 1],
                      label)

    if verifier is not None:
        step(0)
        torch.cuda.synchronize()
        jac2d = jac.view(b - a, P)
        if strong or rank == 0:
            verifier.nodes(con, jac2d, a, b, 'benched launch')
        if strong or world == 1:
            check_sums(con, jac2d, 'benched launch')

    extras = {}
    if not args.no_extras:
        if not args.serial:
            el = timed(lambda k: step(k, True), args.steps, args.warmup)
            extras['serial_evals_per_s'] = args.steps*(
                1 if strong else world)/el
        if world > 1 and strong:
            # The re-assembly variants are secondary figures, and the only
            # part of this program that exchanges data between ranks: if they
            # hang on a node this build has never seen (RCCL point-to-point
            # over xGMI, eight processes page-locking one mapping), the
            # headline line -- already measured and verified -- must still
            # appear.  A watchdog prints it from rank 0 and ends every rank.
            import threading
            limit = float(os.environ.get('OPTY_BENCH_VARIANTS_TIMEOUT',
                                         '240'))

            def give_up():
                if rank == 0:
                    local = {
                        'ok': bool(verifier is None or
                                   (not verifier.failed and
                                    verifier.worst <= 1e-10)),
                        'worst_rel': None if verifier is None
                        else verifier.worst, 'ranks': world,
                        'backend': dist.get_backend(),
                        'checked': [] if verifier is None
                        else verifier.checked,
                        'failed': [] if verifier is None else verifier.failed,
                        'note': 'rank 0 only: the run was ended by the '
                                'watchdog before the verdicts were reduced'}
                    extras['variants_error'] = (
                        'watchdog: the re-assembly variants did not finish '
                        'within %.0f s' % limit)
                    print(json.dumps(headline(extras, local, kernel_ms)),
                          flush=True)
                os._exit(0)
            watchdog = threading.Timer(limit + (0.0 if rank == 0 else 10.0),
                                       give_up)
            watchdog.daemon = True
            watchdog.start()
            try:
                # re-assembly variants of SURVEY.md 8(e); rank 0 is where IPOPT
                # would run and evaluates its own shard in place
                variants = {}
                ncn = N - 1

                def gather_step(k):
                    sh.evaluate(frees[k % 4], in_place=(rank == 0))
                    sh.gather(0)
                el = timed(gather_step, args.steps, args.warmup)
                if verifier is not None:
                    sh.evaluate(frees[0], in_place=(rank == 0))
                    got = sh.gather(0)
                    if rank == 0:
                        gc = got[0][:M*ncn].view(M, ncn)
                        gj = got[1][:P*ncn].view(ncn, P)
                        verifier.nodes(gc, gj, 0, ncn, 'gather')
                        check_sums(gc, gj, 'gather', reduce=False)
                variants['gather'] = {
                    'evals_per_s': args.steps/el, 'ms_per_step': 1e3*el/args.steps,
                    'what': 'eval + point-to-point gather-v of con and jac to '
                            'rank 0 (%s)' % dist.get_backend()}
                if not oversub or os.environ.get('OPTY_HIP_RCCL_LIBRARY'):
                    # (oversubscribed ranks share one GPU: only with the test
                    # transport of tests/fake_rccl in librccl's place --
                    # tools/scale_rehearsal.sh)
                    # the same gather through the C ABI's own RCCL
                    # communicator (opty_hip_comm_create / opty_hip_gather_v:
                    # grouped ncclSend / ncclRecv issued by libopty_hip.so on
                    # the handle's stream, no PyTorch process group on the data
                    # path); RCCL refuses duplicate devices, so not when the
                    # ranks share one GPU
                    try:
                        sh.comm = hb.HipComm.from_process_group(
                            None, device=local_rank)
                        el = timed(gather_step, args.steps, args.warmup)
                        if verifier is not None:
                            sh.evaluate(frees[0], in_place=(rank == 0))
                            got = sh.gather(0)
                            if rank == 0:
                                gc = got[0][:M*ncn].view(M, ncn)
                                gj = got[1][:P*ncn].view(ncn, P)
                                verifier.nodes(gc, gj, 0, ncn, 'gather_c_abi')
                                check_sums(gc, gj, 'gather_c_abi',
                                           reduce=False)
                        variants['gather_c_abi'] = {
                            'evals_per_s': args.steps/el,
                            'ms_per_step': 1e3*el/args.steps,
                            'what': 'eval + opty_hip_gather_v to rank 0 (the '
                                    'library\'s own RCCL communicator)'}
                    except Exception as err:    # noqa: first contact with RCCL
                        variants['gather_c_abi'] = {'error': repr(err)[:400]}
                    finally:
                        sh.comm = None
                # a /dev/shm too small for the 810 MB is the one failure that
                # must not take the headline line down: probe it on rank 0 first
                # and let every rank know
                st = os.statvfs('/dev/shm')
                room = torch.tensor([float(st.f_bavail*st.f_frsize)],
                                    dtype=torch.float64,
                                    device=dev if not oversub else 'cpu')
                dist.broadcast(room, 0)
                if room.item() > 8.0*(M + P)*ncn*1.05:
                    con_host = SharedHostVector(
                        'opty_bench_con_%d' % os.getppid(), M*ncn, rank)
                    jac_host = SharedHostVector(
                        'opty_bench_jac_%d' % os.getppid(), P*ncn, rank,
                        pin=(a*P, b*P))     # the slice this rank writes

                    def host_step(k):
                        sh.evaluate(frees[k % 4])
                        sh.to_host(con_host, jac_host)
                    el = timed(host_step, args.steps, args.warmup)

                    def check_host(cvec, jvec, label):
                        hc = torch.from_numpy(cvec[:M*ncn]).view(M, ncn)
                        hj = torch.from_numpy(jvec[:P*ncn]).view(ncn, P)
                        verifier.nodes(hc.numpy(), hj.numpy(), 0, ncn, label)
                        check_sums(hc, hj, label, reduce=False)
                    if verifier is not None:
                        con_host.array[:] = float('nan')
                        barrier()
                        host_step(0)
                        barrier()
                        if rank == 0:
                            check_host(con_host.array, jac_host.array,
                                       'to_host')
                    variants['to_host'] = {
                        'evals_per_s': args.steps/el,
                        'ms_per_step': 1e3*el/args.steps,
                        'what': 'eval + every rank copies its shard over its '
                                'own PCIe link into one page-locked host vector '
                                'shared by all ranks'}
                    # the same through the solver-facing service: rank 0 calls
                    # constraints(free) then jacobian(free) with NumPy arrays
                    # (H2D of `free` on every rank, evaluation, every shard to
                    # the shared host vectors, host barrier), the others serve
                    from opty_amd.sharded import ShardedCallbacks
                    cb = ShardedCallbacks(sh, name='opty_bench_cb_%d' %
                                          os.getppid(), jac_host=jac_host)
                    if rank == 0:
                        hf = [f.cpu().numpy() for f in frees[:2]]
                        c0, j0 = cb.constraints(hf[0]), cb.jacobian(hf[0])
                        if verifier is not None:
                            check_host(c0, j0, 'callbacks')
                        reps = max(5, args.steps//10)
                        t0 = time.perf_counter()
                        for k in range(reps):
                            cb.constraints(hf[k % 2])
                            cb.jacobian(hf[k % 2])
                        el = (time.perf_counter() - t0)/reps
                        variants['callbacks'] = {
                            'evals_per_s': 1.0/el, 'ms_per_pair': 1e3*el,
                            'what': 'opty_amd.ShardedCallbacks: constraints(free) '
                                    '+ jacobian(free) with NumPy arrays on rank '
                                    '0, served by all ranks (the cyipopt '
                                    'callback pattern on N GPUs)'}
                        cb.shutdown()
                    else:
                        cb.serve()
                    con_host.close()
                    jac_host.close()
                else:
                    variants['to_host'] = {
                        'skipped': '/dev/shm has %.0f MB free, the shared host '
                                   'vectors need %.0f MB' % (
                                       room.item()/1e6, 8.0*(M + P)*ncn/1e6)}
                extras['variants'] = variants
            except Exception as err:      # the headline line must survive
                extras['variants_error'] = repr(err)
            # (the watchdog stays armed until the verdicts below are reduced:
            # a rank that left the variants early must not wait for ever for
            # one that hangs in them)
        if world == 1:
            extras['other_configs'] = other_configs(dev, max(20,
                                                             args.steps//4))
            # BASELINE config 4's launches (1/2, 1/4, 1/8 of the benchmark
            # problem's nodes) on this GPU, next to the headline launch
            extras['other_configs']['config3_shards'] = config3_shards(
                kw, dev, max(20, args.steps//4), fused_ms)
            extras['host_path_ms'] = host_path(kw, local_rank)

    if verifier is not None:
        # every rank's verdict: worst error and number of failed checks
        st = torch.tensor([verifier.worst if verifier.worst == verifier.worst
                           else float('inf'), float(len(verifier.failed))],
                          dtype=torch.float64)
        if world > 1:
            st = st.to(dev) if not oversub else st
            try:
                dist.all_reduce(st, op=dist.ReduceOp.MAX)
            except RuntimeError:
                # a peer that the watchdog has ended already (its connection
                # is gone): same ending here, not a traceback
                if strong and not args.no_extras:
                    watchdog.cancel()
                    give_up()
                raise
            st = st.cpu()
        verify = {
            'ok': bool(st[1].item() == 0 and st[0].item() <= 1e-10),
            'worst_rel': st[0].item(), 'ranks': world,
            'backend': (dist.get_backend() if world > 1 else None),
            'golden': 'tests/golden/%s.npz (reference: %s)' % (
                WORKLOAD, verifier.meta['reference']),
            'checked': verifier.checked, 'failed': verifier.failed}
    if world > 1 and strong and not args.no_extras:
        watchdog.cancel()

    if rank == 0:
        print(json.dumps(headline(extras, verify, kernel_ms)))
    if world > 1:
        dist.destroy_process_group()
    if verify['ok'] is False:
        # a fast launch whose results differ from the reference's is not a
        # result: the line above carries the details
        sys.exit(3)


if __name__ == '__main__':
    main()
