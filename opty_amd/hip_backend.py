"""Host side of the HIP backend: build the per-problem gfx950 code object and
drive ``libopty_hip.so`` (``include/opty_hip.h``) through ``ctypes``.

Counterpart of the build/import half of the reference's ``ufuncify_matrix``
(``opty/utils.py:814-928``: write files, run ``setup.py build_ext`` in a
subprocess, import the module, SHA-256 cache keyed on the generated code).
Here: write ``<sha>.hip``, run ``hipcc --genco`` in a subprocess, keep
``<sha>.hsaco`` in a cache directory keyed on the source hash.

There is no CPU fallback: if the runtime library or a HIP device is missing
the constructors raise.
"""

import ctypes
import hashlib
import logging
import os
import shutil
import subprocess

import numpy as np

logger = logging.getLogger(__name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PKG, 'csrc')
LIB_PATH = os.path.join(_PKG, 'libopty_hip.so')
DEFAULT_CACHE = os.path.join(_PKG, '_cache')
ARCH = 'gfx950'

#: OPTY_HIP_ABI_VERSION of include/opty_hip.h these bindings were written for
ABI_VERSION = 12
HOST, DEVICE = 0, 1
#: hipStreamLegacy: the null / legacy default stream (torch's default)
STREAM_LEGACY = 1
EVAL_CON, EVAL_JAC, EVAL_PAIR, EVAL_FUSED, EVAL_FUSED_KERNEL = 0, 1, 2, 3, 4
#: opty_hip_desc.routing bits (include/opty_hip.h: OPTY_HIP_ROUTE_*)
ROUTE_CALIBRATE, ROUTE_NO_JAC_KERNEL, ROUTE_NO_FUSED_KERNEL = 1, 2, 4


class HipBackendError(RuntimeError):
    pass


class BuildRejected(HipBackendError):
    """A code object whose kernels disagree with the expression DAG on the
    verification nodes (``ConstraintCollocator._verify_build``); ``verdict``
    holds the per-kernel errors."""

    def __init__(self, message, verdict=None):
        HipBackendError.__init__(self, message)
        self.verdict = verdict


def torch_stream_pointer(stream=None):
    """``hipStream_t`` of a ``torch.cuda.Stream`` (default: the current one)
    for the ``set_stream`` calls.  torch's default stream is the legacy null
    stream, whose handle is 0 -- which ``opty_hip_*_set_stream`` reads as
    "back to the handle's own stream"; it is passed as ``hipStreamLegacy``
    (``OPTY_HIP_STREAM_LEGACY``) instead, so that the kernels really are
    ordered with the torch operations around them."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream or STREAM_LEGACY


def _hipcc():
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(exe):
        raise HipBackendError('hipcc not found; cannot build HIP kernels')
    return exe


#: translation units of libopty_hip.so (csrc/opty_internal.h says what is
#: where) and of the build referee's own library
RUNTIME_SOURCES = ('runtime.cpp', 'programs.cpp', 'host_scatter.cpp',
                   'comm.cpp', 'hessian.cpp', 'jacprod.cpp', 'hessmv.cpp',
                   'hesscsr.cpp', 'kktcsr.cpp', 'normal.cpp')
REFEREE_SOURCES = ('referee.cpp',)
REFEREE_PATH = os.path.join(_PKG, 'libopty_hip_referee.so')


def _build_shared(target, sources, extra_deps, force):
    srcs = [os.path.join(CSRC, f) for f in sources]
    deps = srcs + [os.path.join(_PKG, '..', 'include', 'opty_hip.h')] + [
        os.path.join(CSRC, f) for f in extra_deps]
    if (not force and os.path.exists(target) and
            all(os.path.getmtime(target) >= os.path.getmtime(d)
                for d in deps)):
        return target
    tmp = target + '.%d.tmp' % os.getpid()
    base = [_hipcc(), '--offload-arch=' + ARCH, '-O3', '-std=c++17',
            '-Wno-unused-value', '-fPIC']
    # one hipcc per translation unit, side by side (each takes ~20 s)
    from concurrent.futures import ThreadPoolExecutor
    import tempfile
    with tempfile.TemporaryDirectory() as work:
        objs = [os.path.join(work, os.path.basename(f) + '.o') for f in srcs]

        def one(job):
            src, obj = job
            return subprocess.run(base + ['-c', src, '-o', obj],
                                  capture_output=True, text=True)
        with ThreadPoolExecutor(len(srcs)) as pool:
            procs = list(pool.map(one, zip(srcs, objs)))
        bad = [p for p in procs if p.returncode != 0]
        if bad:
            raise HipBackendError('building %s failed:\n%s' % (
                os.path.basename(target), '\n'.join(p.stderr for p in bad)))
        proc = subprocess.run(base + ['-shared'] + objs + ['-o', tmp],
                              capture_output=True, text=True)
    if proc.returncode != 0:
        raise HipBackendError('linking %s failed:\n%s' % (
            os.path.basename(target), proc.stderr))
    os.replace(tmp, target)
    return target


def build_runtime_library(force=False):
    """Compiles ``csrc/*.cpp`` into ``libopty_hip.so`` and the build
    referee's ``libopty_hip_referee.so`` (in-tree)."""
    _build_shared(REFEREE_PATH, REFEREE_SOURCES, ('opty_poison.inc',), force)
    return _build_shared(LIB_PATH, RUNTIME_SOURCES, ('opty_internal.h',),
                         force)


def compile_module(source, cache_dir=None, show_compile_output=False,
                   extra_flags=(), opt_level=None):
    """``hipcc --genco`` of a generated module; returns the ``.hsaco`` path.

    Cached on the SHA-256 of (source, device header, flags) the way the
    reference caches on ``opty_code_hash`` (``opty/utils.py:759-770``).
    """
    cache_dir = os.path.abspath(cache_dir or DEFAULT_CACHE)
    os.makedirs(cache_dir, exist_ok=True)
    with open(os.path.join(CSRC, 'opty_device.h')) as f:
        header = f.read()
    # -O2, not -O3: identical kernel times (10-link and 24-link systems).  In
    # round 1 a hipcc 7.2 -O3 build of one generated kernel (24-link
    # pendulum, row-sorted layout) returned 1e16 in two entries of equation 47
    # at every node while -O1/-O2/-Os agreed with the reference; round 2 could
    # not reproduce it.  Round 3 met the same kind of failure twice more --
    # wrong, run-to-run different values confined to one strip of a 24-link
    # kernel -- and every such build spilled VECTOR registers (512 VGPRs next
    # to hundreds of SGPR spills); no spill-free build has misbehaved.  That is
    # what is enforced now (vgpr_spills below; ConstraintCollocator.
    # _build_code_object never uses a spilling build); -O2 stays the default
    # because it costs nothing, and tests/test_hip_parity.py::
    # test_optimisation_levels_agree cross-checks -O1 against the default on
    # every run.  OPTY_HIPCC_OPT / OPTY_HIPCC_FLAGS override for experiments.
    flags = ['--offload-arch=' + ARCH,
             opt_level or os.environ.get('OPTY_HIPCC_OPT', '-O2'),
             '-std=c++17'] + \
        os.environ.get('OPTY_HIPCC_FLAGS', '').split() + list(extra_flags)
    digest = hashlib.sha256(
        (source + '\0' + header + '\0' + ' '.join(flags)).encode()
    ).hexdigest()[:24]
    base = os.path.join(cache_dir, 'opty_' + digest)
    hsaco = base + '.hsaco'
    manifest = os.environ.get('OPTY_CACHE_MANIFEST')
    if manifest:
        # which code objects a run asks for (tools/prune_cache.py keeps
        # those and drops the leftovers of experiments)
        with open(manifest, 'a') as f:
            f.write(os.path.basename(hsaco) + '\n')
    if os.path.exists(hsaco):
        logger.info('code object cache hit: %s', hsaco)
        return hsaco
    # several ranks (or threads) may build the same module at once: private
    # temp names, atomic renames
    import threading
    tag = '.%d.%d.tmp' % (os.getpid(), threading.get_ident())
    src_tmp = base + tag + '.hip'
    with open(src_tmp, 'w') as f:
        f.write(source)
    # compressed offload bundle (zstd; hipModuleLoad and the bundler read it
    # as they read a plain one): 4x smaller in the in-tree cache that travels
    # with every GPU lease.  Not part of the digest: the code is the same.
    cmd = [_hipcc()] + flags + list(COMPRESS_FLAGS) + [
        '--genco', '-I', CSRC, src_tmp, '-o', hsaco + tag]
    logger.info('compiling %s', base + '.hip')
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if show_compile_output:
        print(proc.stdout)
        print(proc.stderr)
    if proc.returncode != 0:
        # mirrors the reference surfacing compiler stderr in an ImportError
        # (opty/utils.py:912-916)
        raise ImportError('Unable to build the HIP code object {}, '
                          'compilation failed. STDERR output from '
                          'compilation:\n{}'.format(src_tmp, proc.stderr))
    # the printed source is kept next to the code object only on request
    # (OPTY_KEEP_SOURCES=1: disassembly sessions); 0.8 GB of them travelled
    # with every GPU lease in r04.  A failed compile leaves its source behind
    # (the ImportError above names it).
    if os.environ.get('OPTY_KEEP_SOURCES') == '1':
        os.replace(src_tmp, base + '.hip')
    else:
        os.remove(src_tmp)
    os.replace(hsaco + tag, hsaco)
    return hsaco


#: how a code object is stored (OPTY_HIPCC_COMPRESS=0: plain bundles)
COMPRESS_FLAGS = () if os.environ.get('OPTY_HIPCC_COMPRESS') == '0' else (
    '--offload-compress', '--offload-compression-level=19')

#: hipcc switches of the last-resort build of a module whose kernels spill
#: vector registers whatever the cut: without the scheduler stage that the
#: wrong values of round 3 followed (profiles/r03_spill_incident.txt)
SAFE_SCHEDULER_FLAGS = ('-mllvm',
                        '-amdgpu-disable-unclustered-high-rp-reschedule')

#: hipcc switch of ``ConstraintCollocator(deterministic=True)``: every
#: floating-point operation rounds on its own (no mul + add -> fma), so an
#: entry's value does not depend on which wave's straight-line code holds it
DETERMINISTIC_FLAGS = ('-ffp-contract=off',)

#: hipcc switches of a module with persistent kernels (dispatch order 'list':
#: loops over (block, strip) items): without MachineLICM, which would move
#: the materialised constants of every strip out of the item loops and keep
#: them alive (in spilled SGPRs) through all of them
LOOP_FLAGS = ('-mllvm', '-disable-machine-licm')

_RESOURCE_KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count',
                  '.vgpr_spill_count', '.sgpr_spill_count',
                  '.private_segment_fixed_size', '.group_segment_fixed_size')


def kernel_resources(hsaco_path):
    """``{kernel: {'.vgpr_count': ..., '.vgpr_spill_count': ...,
    '.private_segment_fixed_size': ..., ...}}`` from the AMDGPU metadata note
    of a code object built by :func:`compile_module`.  Raises
    :class:`HipBackendError` when the tools fail or the note has no kernel
    records -- a guard built on this must not pass because nothing was
    read."""
    import re
    import tempfile
    llvm = os.path.join(os.path.dirname(os.path.dirname(
        os.path.realpath(_hipcc()))), 'lib', 'llvm', 'bin')
    if not os.path.isdir(llvm):
        llvm = '/opt/rocm/lib/llvm/bin'
    try:
        with tempfile.NamedTemporaryFile(suffix='.elf') as elf:
            # `hipcc --genco` writes an offload bundle: take the gfx950 ELF
            # out
            subprocess.run([os.path.join(llvm, 'clang-offload-bundler'),
                            '--unbundle', '--type=o',
                            '--input=' + hsaco_path,
                            '--targets=hipv4-amdgcn-amd-amdhsa--' + ARCH,
                            '--output=' + elf.name], check=True,
                           capture_output=True)
            txt = subprocess.run([os.path.join(llvm, 'llvm-readelf'),
                                  '--notes', elf.name], capture_output=True,
                                 text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError) as err:
        raise HipBackendError('cannot read the kernel metadata of %s: %s'
                              % (hsaco_path, err)) from err
    out = {}
    for blk in txt.split('- .agpr_count')[1:]:
        blk = '.agpr_count' + blk
        name = re.search(r'\.name:\s+(\S+)', blk)
        vals = {k: re.search(re.escape(k) + r':\s+(\d+)', blk)
                for k in _RESOURCE_KEYS}
        if name is None or any(v is None for v in vals.values()):
            raise HipBackendError('unexpected kernel metadata in %s:\n%s'
                                  % (hsaco_path, blk[:400]))
        out[name.group(1)] = {k: int(v.group(1)) for k, v in vals.items()}
    if not out:
        raise HipBackendError('no kernel records in the metadata of %s'
                              % hsaco_path)
    return out


def vgpr_spills(hsaco_path, kernels=('opty_con', 'opty_jac', 'opty_conjac')):
    """``{kernel: spilled vector registers}`` for the kernels that spill
    VECTOR registers to scratch memory.  The generated kernels are not allowed
    to: at 512 VGPRs next to hundreds of SGPR spills hipcc 7.2 has produced
    code objects whose results were wrong and differed from run to run (the
    24-link stand-in with 19 strips: 32 spilled VGPRs, 100 B of scratch);
    every such case seen so far spilled vector registers, none of the
    spill-free builds misbehaved.

    The verdict (all resource counts of the named kernels) is cached next to
    the code object (``<hsaco>.resources.json``), so a cache hit of
    :func:`compile_module` costs no subprocess.  A code object that holds
    NONE of the named kernels is an error, not "no spills"."""
    res = cached_kernel_resources(hsaco_path)
    if not any(k in res for k in kernels):
        raise HipBackendError('%s holds none of the kernels %s (found %s)'
                              % (hsaco_path, list(kernels), sorted(res)))
    return {k: res[k]['.vgpr_spill_count'] for k in kernels
            if k in res and (res[k]['.vgpr_spill_count'] > 0 or
                             res[k]['.private_segment_fixed_size'] > 0)}


def cached_kernel_resources(hsaco_path):
    """:func:`kernel_resources`, remembered in ``<hsaco>.resources.json``."""
    import json
    side = hsaco_path + '.resources.json'
    try:
        if os.path.getmtime(side) >= os.path.getmtime(hsaco_path):
            with open(side) as f:
                res = json.load(f)
            if isinstance(res, dict) and res:
                return res
    except (OSError, ValueError):
        pass
    res = kernel_resources(hsaco_path)
    try:
        tmp = side + '.%d.tmp' % os.getpid()
        with open(tmp, 'w') as f:
            json.dump(res, f)
        os.replace(tmp, side)
    except OSError:                         # read-only cache: recompute later
        pass
    return res


def high_pressure_kernels(hsaco_path, vgpr_limit=480,
                          kernels=('opty_con', 'opty_jac', 'opty_conjac')):
    """Kernels at the edge of the register file: ``>= vgpr_limit`` vector
    registers or any spilled scalar registers -- the builds whose schedules
    go through the compiler's high-register-pressure stages.
    ``{kernel: (vgprs, sgpr spills)}``."""
    res = cached_kernel_resources(hsaco_path)
    return {k: (res[k]['.vgpr_count'], res[k]['.sgpr_spill_count'])
            for k in kernels if k in res and
            (res[k]['.vgpr_count'] >= vgpr_limit or
             res[k]['.sgpr_spill_count'] > 0)}


class _Desc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int64)] + [
        (name, ctypes.c_int32) for name in (
            'n', 'M', 'm_known', 'q', 'p_known', 'r', 's', 'C', 'P', 'method',
            'num_inst', 'nnz_inst', 'num_inst_atoms', 'jac_wgs_per_block',
            'jac_waves_per_wg', 'fused_wgs_per_block', 'con_wgs_per_block',
            'num_uniform', 'uniform_dynamic', 'device', 'fused_waves_per_wg',
            'con_waves_per_wg', 'layout', 'inst_folded', 'fused_loses',
            'jac_via_fused', 'jac_persist', 'fused_persist', 'routing')] + [
        ('jac_class_cost', ctypes.c_float*32),
        ('fused_class_cost', ctypes.c_float*32)] + [
        (name, ctypes.c_int32) for name in (
            'var_jac_wgs_per_block', 'var_jac_waves_per_wg',
            'var_fused_wgs_per_block', 'var_fused_waves_per_wg')]

    def __init__(self, **kw):
        # (arguments of opty_hip_set_restricted_runs, not fields)
        for key in HipProblem._RUN_KEYS:
            kw.pop(key, None)
        for key in ('jac_class_cost', 'fused_class_cost'):
            cost = list(kw.pop(key, ()))
            setattr(self, key, (ctypes.c_float*32)(*cost[:32]))
        super().__init__(**kw)


#: what the build referee leaves in the register files before every kernel
#: it checks: a quiet NaN as either half of a double
POISON = 0x7ff80000
#: ... once with each of these (ConstraintCollocator._verify_build)
POISONS = (0x00000000, 0x7ff80000, 0xffffffff)


def poison_registers(pattern=POISON):
    """``opty_hip_poison_registers`` on the current device."""
    _check_referee(load_referee().opty_hip_poison_registers(pattern))


def run_schedule(persist, node_blocks, class_cost):
    """``opty_hip_run_schedule``: the same, for a restricted kernel in run
    form (contiguous, cost-balanced runs per XCD)."""
    return list_schedule(persist, node_blocks, class_cost,
                         entry='opty_hip_run_schedule')


def list_schedule(persist, node_blocks, class_cost,
                  entry='opty_hip_list_schedule'):
    """``opty_hip_list_schedule``: ``[[(class, block), ...] per workgroup]``
    of a persistent kernel's launch over ``node_blocks`` 64-node blocks."""
    import numpy as np
    lib = load_library()
    build = getattr(lib, entry)
    cost = (ctypes.c_float*len(class_cost))(*class_cost)
    count = ctypes.c_int64()
    _check(build(persist, node_blocks, len(class_cost), cost, None, 0,
                 ctypes.byref(count)))
    table = np.zeros(count.value, dtype=np.int32)
    _check(build(
        persist, node_blocks, len(class_cost), cost,
        table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(table),
        ctypes.byref(count)))
    npw = int(table[0])
    off, items = table[1:npw + 2], table[npw + 2:]
    return [[(int(v) >> 24, (int(v) & 0xffffff)*8 + w % 8)
             for v in items[off[w]:off[w + 1]]] for w in range(npw)]


class _MatDesc(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'num_vec', 'num_const', 'rows', 'cols', 'wgs_per_block',
        'waves_per_wg', 'num_uniform', 'device')]


class _HessDesc(ctypes.Structure):
    _fields_ = [('PH', ctypes.c_int32), ('nnz_inst', ctypes.c_int32),
                ('strips', ctypes.c_int32), ('pattern', ctypes.c_void_p),
                ('inst_rows', ctypes.c_void_p), ('inst_cols', ctypes.c_void_p)]


class _HessmvDesc(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'PH', 'nnz_inst', 'E', 'obj_base', 'T')] + [
        (name, ctypes.c_void_p) for name in (
            'pattern', 'inst_rows', 'inst_cols', 'obj_pattern', 'tail_rows',
            'tail_cols')]


class _NormalDesc(ctypes.Structure):
    _fields_ = [('M', ctypes.c_int32), ('P', ctypes.c_int32),
                ('layout', ctypes.c_int32), ('pattern', ctypes.c_void_p)]


class _JacprodDesc(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'jvp_strips', 'vjp_strips', 'num_tail', 'nnz_inst')]


class _JacprodBlockDesc(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        'width', 'jvp_strips', 'vjp_strips', 'num_tail', 'nnz_inst')]


class _ObjDesc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int64), ('n', ctypes.c_int32),
                ('q', ctypes.c_int32), ('r', ctypes.c_int32),
                ('device', ctypes.c_int32), ('h', ctypes.c_double)]


class _ObjHessDesc(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int64), ('n', ctypes.c_int32),
                ('q', ctypes.c_int32), ('r', ctypes.c_int32),
                ('device', ctypes.c_int32), ('h', ctypes.c_double),
                ('base', ctypes.c_int32), ('E', ctypes.c_int32),
                ('T', ctypes.c_int32)]


_lib = None

#: every symbol ``include/opty_hip.h`` declares: (restype, argtypes)
_P = ctypes.c_void_p
_SIGNATURES = {
    'opty_hip_list_schedule': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_int64, ctypes.c_int,
        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32),
        ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    'opty_hip_run_schedule': (ctypes.c_int, [
        ctypes.c_int, ctypes.c_int64, ctypes.c_int,
        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32),
        ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    'opty_hip_set_restricted_runs': (ctypes.c_int, [
        _P, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
        ctypes.POINTER(ctypes.c_float),
        ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    'opty_hip_create': (ctypes.c_int, [ctypes.POINTER(_Desc),
                                       ctypes.c_char_p,
                                       ctypes.POINTER(_P)]),
    'opty_hip_destroy': (ctypes.c_int, [_P]),
    'opty_hip_set_stream': (ctypes.c_int, [_P, _P]),
    'opty_hip_synchronize': (ctypes.c_int, [_P]),
    'opty_hip_set_known_parameters': (ctypes.c_int, [_P, _P, ctypes.c_int32]),
    'opty_hip_set_interval': (ctypes.c_int, [_P, ctypes.c_double]),
    'opty_hip_set_known_trajectories': (ctypes.c_int,
                                        [_P, _P, ctypes.c_int32]),
    'opty_hip_set_instance_indices': (ctypes.c_int, [_P, _P, _P, _P]),
    'opty_hip_set_block_pattern': (ctypes.c_int, [_P, _P]),
    'opty_hip_set_segments': (ctypes.c_int, [_P, _P, _P, _P]),
    'opty_hip_num_free': (ctypes.c_int64, [_P]),
    'opty_hip_num_constraints': (ctypes.c_int64, [_P]),
    'opty_hip_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_eval_con': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_eval_jac': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_eval_con_jac': (ctypes.c_int, [_P, _P, _P, _P,
                                             ctypes.c_int32]),
    'opty_hip_jacobian_indices': (ctypes.c_int, [_P, _P, _P,
                                                 ctypes.c_int32]),
    'opty_hip_jacobian_indices_shard': (ctypes.c_int, [
        _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int32]),
    'opty_hip_jacobian_indices_range': (ctypes.c_int, [
        _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int32]),
    'opty_hip_time_eval': (ctypes.c_int, [_P, ctypes.c_int32, _P, _P, _P,
                                          ctypes.c_int32,
                                          ctypes.POINTER(ctypes.c_float)]),
    'opty_hip_eval_shard': (ctypes.c_int, [
        _P, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, ctypes.c_int64,
        ctypes.c_int64]),
    'opty_hip_eval_instance': (ctypes.c_int, [_P, _P, _P, _P]),
    'opty_hip_set_varying_entries': (ctypes.c_int, [_P, _P, ctypes.c_int32]),
    'opty_hip_set_entry_copies': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_set_entry_copies_scaled': (ctypes.c_int, [_P, _P, _P, _P,
                                                        ctypes.c_int32]),
    'opty_hip_eval_jac_persistent': (ctypes.c_int, [_P, _P, _P,
                                                    ctypes.c_int32]),
    'opty_hip_pack_ratio': (ctypes.c_double, []),
    'opty_hip_shard_jac_to_host': (ctypes.c_int, [
        _P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]),
    'opty_hip_set_host_threads': (ctypes.c_int, [ctypes.c_int32]),
    'opty_hip_host_threads': (ctypes.c_int, []),
    'opty_hip_host_numa_node': (ctypes.c_int, [_P]),
    'opty_hip_host_placement': (ctypes.c_int, [_P, _P, _P]),
    'opty_hip_routing': (ctypes.c_int, [
        _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_float)]),
    'opty_hip_time_eval_shard': (ctypes.c_int, [
        _P, ctypes.c_int32, _P, _P, ctypes.c_int64, _P, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]),
    'opty_hip_host_register': (ctypes.c_int, [_P, ctypes.c_size_t]),
    'opty_hip_host_unregister': (ctypes.c_int, [_P]),
    'opty_hip_matrix_create': (ctypes.c_int, [ctypes.POINTER(_MatDesc),
                                              ctypes.c_char_p,
                                              ctypes.POINTER(_P)]),
    'opty_hip_matrix_destroy': (ctypes.c_int, [_P]),
    'opty_hip_matrix_set_stream': (ctypes.c_int, [_P, _P]),
    'opty_hip_matrix_eval': (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64,
                                            ctypes.c_int32]),
    'opty_hip_objective_create': (ctypes.c_int, [ctypes.POINTER(_ObjDesc),
                                                 ctypes.c_char_p,
                                                 ctypes.POINTER(_P)]),
    'opty_hip_objective_destroy': (ctypes.c_int, [_P]),
    'opty_hip_objective_set_stream': (ctypes.c_int, [_P, _P]),
    'opty_hip_objective_eval': (ctypes.c_int, [_P, _P, _P, _P,
                                               ctypes.c_int32]),
    'opty_hip_objhess_create': (ctypes.c_int, [ctypes.POINTER(_ObjHessDesc),
                                               _P, ctypes.c_char_p,
                                               ctypes.POINTER(_P)]),
    'opty_hip_objhess_destroy': (ctypes.c_int, [_P]),
    'opty_hip_objhess_set_stream': (ctypes.c_int, [_P, _P]),
    'opty_hip_objhess_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_objhess_indices': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_objhess_eval': (ctypes.c_int, [_P, _P, ctypes.c_double, _P,
                                             ctypes.c_int32]),
    'opty_hip_host_alloc': (ctypes.c_void_p, [ctypes.c_size_t]),
    'opty_hip_host_free': (ctypes.c_int, [_P]),
    'opty_hip_device_alloc': (ctypes.c_void_p, [ctypes.c_int32,
                                                 ctypes.c_size_t]),
    'opty_hip_device_free': (ctypes.c_int, [_P]),
    'opty_hip_memcpy': (ctypes.c_int, [_P, _P, ctypes.c_size_t,
                                       ctypes.c_int32]),
    'opty_hip_comm_unique_id': (ctypes.c_int, [_P]),
    'opty_hip_comm_create': (ctypes.c_int, [_P, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(_P)]),
    'opty_hip_comm_destroy': (ctypes.c_int, [_P]),
    'opty_hip_comm_rank': (ctypes.c_int, [_P]),
    'opty_hip_comm_world': (ctypes.c_int, [_P]),
    'opty_hip_bcast_free': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_gather_v': (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P,
                                         ctypes.c_int32, ctypes.c_int32]),
    'opty_hip_hessian_create': (ctypes.c_int, [_P, ctypes.POINTER(_HessDesc),
                                               ctypes.c_char_p,
                                               ctypes.POINTER(_P)]),
    'opty_hip_hessian_destroy': (ctypes.c_int, [_P]),
    'opty_hip_hessian_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_eval_hess': (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int32]),
    'opty_hip_hessian_indices': (ctypes.c_int, [_P, _P, _P, ctypes.c_int32]),
    'opty_hip_eval_hess_shard': (ctypes.c_int, [
        _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64]),
    'opty_hip_eval_hess_instance': (ctypes.c_int, [_P, _P, _P, _P]),
    'opty_hip_hessian_indices_range': (ctypes.c_int, [
        _P, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_int32]),
    'opty_hip_jacprod_create': (ctypes.c_int,
                                [_P, ctypes.POINTER(_JacprodDesc),
                                 ctypes.c_char_p, ctypes.POINTER(_P)]),
    'opty_hip_jacprod_destroy': (ctypes.c_int, [_P]),
    'opty_hip_jacprod_jvp': (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int32]),
    'opty_hip_jacprod_vjp': (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int32]),
    'opty_hip_jacprod_jvp_shard': (ctypes.c_int, [
        _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'opty_hip_jacprod_jvp_instance': (ctypes.c_int, [_P, _P, _P, _P]),
    'opty_hip_jacprod_vjp_shard': (ctypes.c_int, [
        _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64]),
    'opty_hip_jacprod_block_create': (ctypes.c_int,
                                      [_P, ctypes.POINTER(_JacprodBlockDesc),
                                       ctypes.c_char_p, ctypes.POINTER(_P)]),
    'opty_hip_jacprod_block_destroy': (ctypes.c_int, [_P]),
    'opty_hip_jacprod_block_width': (ctypes.c_int32, [_P]),
    'opty_hip_jacprod_block_jvp': (ctypes.c_int,
                                   [_P, _P, _P, ctypes.c_int64, _P,
                                    ctypes.c_int64, ctypes.c_int32,
                                    ctypes.c_int32]),
    'opty_hip_jacprod_block_vjp': (ctypes.c_int,
                                   [_P, _P, _P, ctypes.c_int64, _P,
                                    ctypes.c_int64, ctypes.c_int32,
                                    ctypes.c_int32]),
    'opty_hip_hessmv_create': (ctypes.c_int,
                               [_P, ctypes.POINTER(_HessmvDesc),
                                ctypes.POINTER(_P)]),
    'opty_hip_hessmv_destroy': (ctypes.c_int, [_P]),
    'opty_hip_hessmv_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_hessmv_sides': (ctypes.c_int32, [_P, _P, ctypes.c_int32, _P]),
    'opty_hip_hessmv_apply': (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int32]),
    'opty_hip_hessmv_apply_block': (ctypes.c_int,
                                    [_P, _P, _P, ctypes.c_int64, _P,
                                     ctypes.c_int64, ctypes.c_int32,
                                     ctypes.c_int32]),
    'opty_hip_hessmv_block_width': (ctypes.c_int32, [_P]),
    'opty_hip_hessmv_apply_shard': (ctypes.c_int, [
        _P, _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_int32]),
    'opty_hip_hesscsr_create': (ctypes.c_int,
                                [_P, ctypes.POINTER(_HessmvDesc),
                                 ctypes.POINTER(_P)]),
    'opty_hip_hesscsr_destroy': (ctypes.c_int, [_P]),
    'opty_hip_hesscsr_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_hesscsr_nnz_unique': (ctypes.c_int64, [_P]),
    'opty_hip_hesscsr_structure': (ctypes.c_int, [_P, _P, _P,
                                                  ctypes.c_int32]),
    'opty_hip_hesscsr_compress': (ctypes.c_int, [_P, _P, _P,
                                                 ctypes.c_int32]),
    'opty_hip_hesscsr_create_with_diagonal': (
        ctypes.c_int, [_P, ctypes.POINTER(_HessmvDesc), ctypes.POINTER(_P)]),
    'opty_hip_kktcsr_create': (ctypes.c_int,
                               [_P, ctypes.POINTER(_HessmvDesc),
                                ctypes.POINTER(_P)]),
    'opty_hip_kktcsr_destroy': (ctypes.c_int, [_P]),
    'opty_hip_kktcsr_nnz': (ctypes.c_int64, [_P]),
    'opty_hip_kktcsr_nnz_hessian': (ctypes.c_int64, [_P]),
    'opty_hip_kktcsr_nnz_triplets': (ctypes.c_int64, [_P]),
    'opty_hip_kktcsr_structure': (ctypes.c_int, [_P, _P, _P,
                                                 ctypes.c_int32]),
    'opty_hip_kktcsr_assemble': (ctypes.c_int,
                                 [_P, _P, _P, _P, ctypes.c_double,
                                  ctypes.c_double, _P, ctypes.c_int32]),
    'opty_hip_kktcsr_assemble_timed': (ctypes.c_int,
                                       [_P, _P, _P, _P, ctypes.c_double,
                                        ctypes.c_double, _P, _P]),
    'opty_hip_normal_create': (ctypes.c_int,
                               [_P, ctypes.POINTER(_NormalDesc),
                                ctypes.POINTER(_P)]),
    'opty_hip_normal_destroy': (ctypes.c_int, [_P]),
    'opty_hip_normal_workspace_bytes': (ctypes.c_int64, [_P]),
    'opty_hip_normal_max_equations': (ctypes.c_int32, [_P]),
    'opty_hip_normal_blocks': (ctypes.c_int,
                               [_P, _P, _P, ctypes.c_double, _P, _P,
                                ctypes.c_int32]),
    'opty_hip_normal_factor': (ctypes.c_int,
                               [_P, _P, _P, ctypes.c_double, ctypes.c_int32]),
    'opty_hip_normal_factor_status': (ctypes.c_int, [_P, _P, _P]),
    'opty_hip_normal_solve': (ctypes.c_int,
                              [_P, _P, _P, ctypes.c_int32, ctypes.c_int64,
                               ctypes.c_int32]),
    'opty_hip_output_register': (ctypes.c_int, [_P, _P, ctypes.c_int64,
                                                ctypes.c_int64]),
    'opty_hip_output_unregister': (ctypes.c_int, [_P, _P]),
    'opty_hip_output_invalidate': (ctypes.c_int, [_P, _P]),
    'opty_hip_abi_version': (ctypes.c_int, []),
    'opty_hip_device_count': (ctypes.c_int, []),
    'opty_hip_last_error': (ctypes.c_char_p, []),
}


#: entry points of libopty_hip_referee.so (include/opty_hip_referee.h)
_REFEREE_SIGNATURES = {
    'opty_hip_poison_registers': (ctypes.c_int, [ctypes.c_uint]),
    'opty_hip_tape_run': (ctypes.c_int, [ctypes.c_int32, _P, ctypes.c_int64,
                                         _P, ctypes.c_int64, ctypes.c_int64]),
    'opty_hip_referee_last_error': (ctypes.c_char_p, []),
}
_referee = None


def load_referee():
    """Loads ``libopty_hip_referee.so`` -- the build verification's device
    side (instruction tape, register poisoner), kept out of the runtime
    library -- on first use."""
    global _referee
    if _referee is None:
        load_library()          # one HIP runtime per process, loaded first
        if not os.path.exists(REFEREE_PATH):
            build_runtime_library()
        lib = ctypes.CDLL(REFEREE_PATH)
        for name, (res, args) in _REFEREE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _referee = lib
    return _referee


def _check_referee(rc):
    if rc != 0:
        raise HipBackendError(
            load_referee().opty_hip_referee_last_error().decode())


def load_library():
    """Loads ``libopty_hip.so`` and binds every declared entry point."""
    global _lib
    if _lib is None:
        # PyTorch wheels bundle their own libamdhip64; if torch is going to
        # live in this process it must load first so that both share ONE HIP
        # runtime (two runtimes in a process see no devices).
        # (OPTY_HIP_NO_TORCH=1: a torch-free process -- opty_amd.shard_host,
        # bench.py --no-torch -- must not pay the import either)
        if os.environ.get('OPTY_HIP_NO_TORCH') != '1':
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(LIB_PATH):
            # not built yet (fresh checkout): build it from source with hipcc;
            # there is no CPU fallback, so a missing compiler is an error
            try:
                build_runtime_library()
            except HipBackendError as err:
                raise HipBackendError(
                    '%s is missing and could not be built (%s): run `python '
                    '-c "import __graft_entry__ as g; g.build()"`'
                    % (LIB_PATH, err))
        lib = ctypes.CDLL(LIB_PATH)
        # the bindings below mirror ONE version of include/opty_hip.h: a
        # library built from another one would read the descriptor / the
        # trailing arguments wrongly without any error
        try:
            version = lib.opty_hip_abi_version()
        except AttributeError:
            version = None
        if version != ABI_VERSION:
            raise HipBackendError(
                '%s implements version %s of the C ABI, these bindings '
                'version %d (include/opty_hip.h: OPTY_HIP_ABI_VERSION): '
                'rebuild it -- `python -c "import __graft_entry__ as g; '
                'g.build()"`' % (LIB_PATH, version, ABI_VERSION))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        raise HipBackendError(load_library().opty_hip_last_error().decode())


def tape_run(tape, vals, device=0):
    """Runs an instruction tape (:mod:`opty_amd.codegen.tape`) on the device
    over the value table ``vals`` (``(nslots, nodes)`` float64, C order;
    constant and input slots filled) -- ``opty_hip_tape_run``, the referee of
    builds at the register limit.  Fills ``vals`` in place and returns it."""
    code = np.ascontiguousarray(tape.code, dtype=np.int32)
    assert vals.dtype == np.float64 and vals.flags.c_contiguous
    assert vals.shape[0] == tape.nslots
    _check_referee(load_referee().opty_hip_tape_run(
        int(device), code.ctypes.data, code.shape[0], vals.ctypes.data,
        vals.shape[0], vals.shape[1]))
    return vals


def _ptr(x):
    """Raw address of a NumPy array, a torch tensor, an int or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if hasattr(x, 'data_ptr'):
        return x.data_ptr()
    return int(x)


class DeviceVector(object):
    """float64 device memory through the C ABI alone (``opty_hip_device_
    alloc`` / ``opty_hip_memcpy``; no torch): what the build referee hands
    the kernels, so that every output starts as NaN on the DEVICE -- a store
    that never happens cannot hide behind what an earlier kernel left in a
    buffer of the handle."""

    def __init__(self, values, device=0):
        self._lib = load_library()
        host = np.ascontiguousarray(values, dtype=np.float64)
        self.size = host.size
        self.ptr = self._lib.opty_hip_device_alloc(device,
                                                   max(8, host.nbytes))
        if not self.ptr:
            raise HipBackendError(self._lib.opty_hip_last_error().decode())
        if host.size:
            _check(self._lib.opty_hip_memcpy(self.ptr, host.ctypes.data,
                                             host.nbytes, 0))

    def data_ptr(self):
        return self.ptr

    def assign(self, values):
        """Overwrites the vector with ``size`` host values."""
        host = np.ascontiguousarray(values, dtype=np.float64)
        assert host.size == self.size
        if host.size:
            _check(self._lib.opty_hip_memcpy(self.ptr, host.ctypes.data,
                                             host.nbytes, 0))

    def read_into(self, out):
        """Copies the vector into the contiguous float64 host array
        ``out`` of ``size`` values."""
        assert out.size == self.size and out.dtype == np.float64
        if self.size:
            _check(self._lib.opty_hip_memcpy(out.ctypes.data, self.ptr,
                                             out.nbytes, 1))
        return out

    def numpy(self):
        return self.read_into(np.empty(self.size))

    def close(self):
        if self.ptr:
            self._lib.opty_hip_device_free(self.ptr)
            self.ptr = None

    __del__ = close


class _PinnedBlock(object):
    """Owner of one ``opty_hip_host_alloc`` block (freed with the last NumPy
    view of it)."""

    def __init__(self, nbytes):
        self._lib = load_library()
        self.ptr = self._lib.opty_hip_host_alloc(nbytes)
        if not self.ptr:
            raise HipBackendError(self._lib.opty_hip_last_error().decode())
        self.nbytes = nbytes

    def __del__(self):
        if getattr(self, 'ptr', None):
            self._lib.opty_hip_host_free(self.ptr)
            self.ptr = None


def pinned_empty(count, dtype=np.float64):
    """``np.empty(count, dtype)`` in page-locked host memory."""
    dtype = np.dtype(dtype)
    block = _PinnedBlock(max(1, count)*dtype.itemsize)
    buf = (ctypes.c_char*block.nbytes).from_address(block.ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=count)
    # keep the block alive as long as any view of the array is
    _PINNED_OWNERS[id(buf)] = block
    import weakref
    weakref.finalize(buf, _PINNED_OWNERS.pop, id(buf), None)
    return arr


_PINNED_OWNERS = {}


def set_host_threads(count=0):
    """Host threads that scatter the varying Jacobian entries into the
    caller's dense vector (0 = default)."""
    _check(load_library().opty_hip_set_host_threads(int(count)))


def host_threads():
    return load_library().opty_hip_host_threads()


def pack_ratio():
    """Largest varying fraction of a block for which the host-visible
    Jacobian moves only the varying entries (``opty_hip_pack_ratio``)."""
    return float(load_library().opty_hip_pack_ratio())


def host_numa_node(array):
    """NUMA node that holds the first page of a NumPy array (-1: unknown)."""
    return load_library().opty_hip_host_numa_node(array.ctypes.data)


def host_placement():
    """``(scatter workers' NUMA node, the device's NUMA node, verified by
    measurement)`` -- ``opty_hip_host_placement``."""
    w, d, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(load_library().opty_hip_host_placement(
        ctypes.addressof(w), ctypes.addressof(d), ctypes.addressof(v)))
    return w.value, d.value, bool(v.value)


def host_register(array):
    """Page-locks the memory of a NumPy array the caller owns (e.g. a
    shared-memory mapping); pair with :func:`host_unregister`."""
    _check(load_library().opty_hip_host_register(array.ctypes.data,
                                                 array.nbytes))


def host_unregister(array):
    _check(load_library().opty_hip_host_unregister(array.ctypes.data))


class HipProblem(object):
    """One ``opty_hip_problem`` handle."""

    def __init__(self, desc, hsaco_path):
        self._lib = load_library()
        if self._lib.opty_hip_device_count() == 0:
            raise HipBackendError('no HIP device is visible: the HIP '
                                  'backend has no CPU fallback')
        self._h = self._create(desc, hsaco_path)
        self.desc = dict(desc)
        self.num_free = self._lib.opty_hip_num_free(self._h)
        self.num_constraints = self._lib.opty_hip_num_constraints(self._h)
        self.nnz = self._lib.opty_hip_nnz(self._h)

    #: descriptor keys of the restricted kernels' run form: not fields of
    #: ``opty_hip_desc`` but arguments of ``opty_hip_set_restricted_runs``
    _RUN_KEYS = ('var_jac_persist', 'var_fused_persist',
                 'var_jac_class_cost', 'var_fused_class_cost',
                 'var_run_code_object')

    def _create(self, desc, hsaco_path):
        """A new C handle for ``desc``; where the build carries the run form
        of the restricted kernels (``var_run_code_object``: a code object of
        its own) the handle takes it before anything can launch them."""
        desc = dict(desc)
        run = {k: desc.pop(k, None) for k in self._RUN_KEYS}
        h = _P()
        d = _Desc(**desc)
        _check(self._lib.opty_hip_create(ctypes.byref(d),
                                         hsaco_path.encode(),
                                         ctypes.byref(h)))
        if run['var_run_code_object']:
            jp, fp = (int(run[k] or 0) for k in self._RUN_KEYS[:2])
            jc, fc = (list(run[k] or ()) for k in self._RUN_KEYS[2:4])
            rc = self._lib.opty_hip_set_restricted_runs(
                h, run['var_run_code_object'].encode(),
                jp, len(jc), (ctypes.c_float*max(1, len(jc)))(*jc),
                fp, len(fc), (ctypes.c_float*max(1, len(fc)))(*fc))
            if rc:
                self._lib.opty_hip_destroy(h)
                _check(rc)
        return h

    def close(self):
        # Hessian handles borrow this one: they go first
        for dep in list(getattr(self, '_dependents', ())):
            dep.release()
        if getattr(self, '_h', None):
            self._lib.opty_hip_destroy(self._h)
            self._h = None

    __del__ = close

    def reload(self, desc, hsaco_path):
        """Replaces the C handle behind this object by one for another code
        object of the same problem (kernels specialised for new parameter
        values); tables and stream have to be installed again."""
        new = self._create(desc, hsaco_path)
        self.close()
        self._h = new
        self.desc = dict(desc)
        if getattr(self, '_stream_ptr', None):
            self.set_stream(self._stream_ptr)
        # the owners' word holds for the object, not for the C handle
        for ptr, (a, b) in list(getattr(self, '_outputs', {}).items()):
            _check(self._lib.opty_hip_output_register(self._h, ptr, a, b))

    # -- configuration -------------------------------------------------------
    def set_stream(self, stream_ptr):
        _check(self._lib.opty_hip_set_stream(self._h, stream_ptr))
        self._stream_ptr = stream_ptr

    def use_torch_stream(self, stream=None):
        """Run this handle's work on a torch stream (default: the current
        one), ordered with the torch operations issued there."""
        self.set_stream(torch_stream_pointer(stream))

    def synchronize(self):
        _check(self._lib.opty_hip_synchronize(self._h))

    #: ``(known parameter values, fixed interval or None)`` that the loaded
    #: kernels carry as LITERALS (parameter-specialised modules), else None
    literals = None

    def _refuse_other_literals(self, what, same):
        if self.literals is not None and not same:
            raise HipBackendError(
                'the kernels of this handle carry the %s as literals '
                '(parameter-specialised module): change the collocator\'s '
                'known_parameter_map / node_time_interval and call '
                'col.sync_known() -- it rebuilds them -- or build with '
                'specialize_parameters=False' % what)

    def set_known_parameters(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if self.literals is not None:
            self._refuse_other_literals(
                'known parameters', tuple(float(x) for x in v) ==
                tuple(self.literals[0]))
        _check(self._lib.opty_hip_set_known_parameters(
            self._h, _ptr(v), len(v)))

    def set_interval(self, h):
        if self.literals is not None and self.literals[1] is not None:
            self._refuse_other_literals('node time interval',
                                        float(h) == float(self.literals[1]))
        _check(self._lib.opty_hip_set_interval(self._h, float(h)))

    def set_known_trajectories(self, values):
        if hasattr(values, 'data_ptr'):
            _check(self._lib.opty_hip_set_known_trajectories(
                self._h, _ptr(values), DEVICE))
            return
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.size == self.desc['m_known']*self.desc['N']
        _check(self._lib.opty_hip_set_known_trajectories(
            self._h, _ptr(v), HOST))

    def set_block_pattern(self, pattern):
        jk = np.ascontiguousarray(pattern, dtype=np.int32).reshape(-1, 2)
        assert len(jk) == self.desc['P']
        _check(self._lib.opty_hip_set_block_pattern(self._h, _ptr(jk)))

    def set_segments(self, order, seg_len, copy_source):
        """``opty_hip_set_segments`` (``OPTY_HIP_LAYOUT_SEGMENTED``):
        ``order``: the block entries in stored order, ``seg_len``: lengths of
        the varying / repeated / invariant segments, ``copy_source``: for
        every entry of segment 1 its source's position in segment 0."""
        o = np.ascontiguousarray(order, dtype=np.int32)
        n = np.ascontiguousarray(seg_len, dtype=np.int32)
        c = np.ascontiguousarray(copy_source, dtype=np.int32)
        assert len(o) == self.desc['P'] and len(n) == 3
        _check(self._lib.opty_hip_set_segments(self._h, _ptr(o), _ptr(n),
                                               _ptr(c)))

    def set_instance_indices(self, atom_index, rows, cols):
        a = np.ascontiguousarray(atom_index, dtype=np.int64)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        c = np.ascontiguousarray(cols, dtype=np.int64)
        _check(self._lib.opty_hip_set_instance_indices(
            self._h, _ptr(a), _ptr(r), _ptr(c)))

    # -- evaluation ------------------------------------------------------------
    def eval_con(self, free, con, mem):
        _check(self._lib.opty_hip_eval_con(self._h, _ptr(free), _ptr(con),
                                           mem))

    def eval_jac(self, free, jac, mem):
        _check(self._lib.opty_hip_eval_jac(self._h, _ptr(free), _ptr(jac),
                                           mem))

    def set_varying_entries(self, entries):
        """Block entries that can change from call to call (ascending); see
        ``opty_hip_set_varying_entries``."""
        e = np.ascontiguousarray(entries, dtype=np.int32)
        _check(self._lib.opty_hip_set_varying_entries(self._h, _ptr(e),
                                                      len(e)))

    def set_entry_copies(self, copies, scales=None):
        """``[(dst, src), ...]``: block entries filled on the host from a
        varying entry of the same block (``scales``: times that factor);
        see ``opty_hip_set_entry_copies`` / ``..._scaled``."""
        dst = np.ascontiguousarray([c[0] for c in copies], dtype=np.int32)
        src = np.ascontiguousarray([c[1] for c in copies], dtype=np.int32)
        if scales is None:
            _check(self._lib.opty_hip_set_entry_copies(
                self._h, _ptr(dst), _ptr(src), len(dst)))
            return
        scl = np.ascontiguousarray(scales, dtype=np.float64)
        assert scl.shape == dst.shape
        _check(self._lib.opty_hip_set_entry_copies_scaled(
            self._h, _ptr(dst), _ptr(src), _ptr(scl), len(dst)))

    def eval_jac_persistent(self, free, jac, fresh):
        """``opty_hip_eval_jac_persistent``: host ``free``, page-locked
        persistent host ``jac``; ``fresh``: ``jac`` is a new allocation (or
        was written to) since this handle last filled it."""
        _check(self._lib.opty_hip_eval_jac_persistent(
            self._h, _ptr(free), _ptr(jac), int(bool(fresh))))

    def shard_jac_to_host(self, d_jac_shard, host_jac, node_begin, node_end,
                          fresh):
        """``opty_hip_shard_jac_to_host``: the blocks of a node shard from
        device memory into the dense page-locked host vector of the global
        problem (only what changed after the first time with this mapping of
        the vector: ``fresh`` says when it is a new one)."""
        _check(self._lib.opty_hip_shard_jac_to_host(
            self._h, _ptr(d_jac_shard), _ptr(host_jac), node_begin, node_end,
            int(bool(fresh))))

    def eval_con_jac(self, free, con, jac, mem):
        _check(self._lib.opty_hip_eval_con_jac(
            self._h, _ptr(free), _ptr(con), _ptr(jac), mem))

    def jacobian_indices(self, rows, cols, mem):
        _check(self._lib.opty_hip_jacobian_indices(
            self._h, _ptr(rows), _ptr(cols), mem))

    def jacobian_indices_shard(self, num_nodes_global, node_offset, rows,
                               cols, mem):
        _check(self._lib.opty_hip_jacobian_indices_shard(
            self._h, num_nodes_global, node_offset, _ptr(rows), _ptr(cols),
            mem))

    def jacobian_indices_range(self, node_begin, node_end, rows, cols, mem):
        _check(self._lib.opty_hip_jacobian_indices_range(
            self._h, node_begin, node_end, _ptr(rows), _ptr(cols), mem))

    def eval_shard(self, what, free, con, con_stride, jac, node_begin,
                   node_end):
        """Constraint nodes ``[node_begin, node_end)`` from the global device
        ``free``; see ``opty_hip_eval_shard`` in ``include/opty_hip.h``."""
        _check(self._lib.opty_hip_eval_shard(
            self._h, what, _ptr(free), _ptr(con), con_stride, _ptr(jac),
            node_begin, node_end))

    def output_register(self, jac, node_begin=0, node_end=None):
        """``opty_hip_output_register``: the caller OWNS the device buffer
        ``jac`` (tensor or address), passes it for the constraint nodes
        ``[node_begin, node_end)`` (default: all) and nobody else writes to
        it between two evaluations -- which may then leave the
        node-invariant entries as the previous evaluation wrote them.  Kept
        across :meth:`reload`.  Unregister before the memory is released."""
        if node_end is None:
            node_end = self.desc['N'] - 1
        _check(self._lib.opty_hip_output_register(
            self._h, _ptr(jac), int(node_begin), int(node_end)))
        if not hasattr(self, '_outputs'):
            self._outputs = {}
        self._outputs[_ptr(jac)] = (int(node_begin), int(node_end))

    def output_unregister(self, jac):
        """``opty_hip_output_unregister``."""
        _check(self._lib.opty_hip_output_unregister(self._h, _ptr(jac)))
        getattr(self, '_outputs', {}).pop(_ptr(jac), None)

    def output_invalidate(self, jac=None):
        """``opty_hip_output_invalidate``: the next evaluation into the
        registered buffer ``jac`` (None: into any) writes everything."""
        _check(self._lib.opty_hip_output_invalidate(self._h, _ptr(jac)))

    def eval_instance(self, free, con_tail, jac_tail):
        """The instance-constraint values / partials from the global device
        ``free`` into device buffers (either may be None); see
        ``opty_hip_eval_instance``."""
        _check(self._lib.opty_hip_eval_instance(
            self._h, _ptr(free), _ptr(con_tail), _ptr(jac_tail)))

    def time_eval_shard(self, what, free, con, con_stride, jac, node_begin,
                        node_end, iters):
        ms = ctypes.c_float()
        _check(self._lib.opty_hip_time_eval_shard(
            self._h, what, _ptr(free), _ptr(con), con_stride, _ptr(jac),
            node_begin, node_end, iters, ctypes.byref(ms)))
        return ms.value

    def routing(self, nodes=None):
        """What the entry points launch for launches of ``nodes`` constraint
        nodes (default: the whole problem): ``opty_hip_routing`` -- a dict
        with ``routing`` ('calibrated' once the handle has measured that
        launch size on its device, else 'plan'), ``fused_loses``,
        ``jac_via_fused`` and, when calibrated, the measured ``ms`` of
        ``opty_conjac`` / ``opty_con`` / ``opty_jac``; ``flavour`` is
        ``'restricted'`` when the last Jacobian launch of that size was
        served by ``opty_conjac_var`` / ``opty_jac_var`` (a registered
        output, :meth:`output_register`: flags and times are then those
        kernels'), else ``'full'``."""
        if nodes is None:
            nodes = self.desc['N'] - 1
        cal, fl, jv = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        ms = (ctypes.c_float*3)()
        _check(self._lib.opty_hip_routing(
            self._h, int(nodes), ctypes.byref(cal), ctypes.byref(fl),
            ctypes.byref(jv), ms))
        banned = self.desc.get('routing', 0) & (ROUTE_NO_JAC_KERNEL |
                                                ROUTE_NO_FUSED_KERNEL)
        restricted, cal.value = bool(cal.value & 2), cal.value & 1
        out = dict(routing='calibrated' if cal.value else (
                       'fixed: a spilling kernel is banned' if banned
                       else 'plan'),
                   fused_loses=bool(fl.value), jac_via_fused=bool(jv.value),
                   flavour='restricted' if restricted else 'full')
        if cal.value:
            out['ms'] = dict(opty_conjac=ms[0], opty_con=ms[1], opty_jac=ms[2])
        return out

    def time_eval(self, what, free, con, jac, iters):
        ms = ctypes.c_float()
        _check(self._lib.opty_hip_time_eval(
            self._h, what, _ptr(free), _ptr(con), _ptr(jac), iters,
            ctypes.byref(ms)))
        return ms.value


class HipComm(object):
    """One ``opty_hip_comm``: this process's rank in an RCCL communicator
    of one-process-per-GPU ranks (``include/opty_hip.h``).  The collective
    calls go through the C ABI -- grouped ``ncclSend`` / ``ncclRecv`` issued by
    the library on the problem handle's stream -- not through a PyTorch
    process group."""

    ID_BYTES = 128

    def __init__(self, unique_id, rank, world, device=0):
        self._lib = load_library()
        if len(unique_id) != self.ID_BYTES:
            raise ValueError('unique_id must be %d bytes' % self.ID_BYTES)
        self._h = _P()
        buf = ctypes.create_string_buffer(bytes(unique_id), self.ID_BYTES)
        _check(self._lib.opty_hip_comm_create(
            ctypes.addressof(buf), int(rank), int(world), int(device),
            ctypes.byref(self._h)))
        self.rank, self.world, self.device = int(rank), int(world), device

    @staticmethod
    def unique_id():
        """``ncclGetUniqueId`` as bytes (one rank calls this and hands the
        result to the others)."""
        buf = ctypes.create_string_buffer(HipComm.ID_BYTES)
        _check(load_library().opty_hip_comm_unique_id(ctypes.addressof(buf)))
        return buf.raw

    @classmethod
    def from_process_group(cls, group=None, device=0):
        """Bootstraps the communicator over an initialised
        ``torch.distributed`` group of any backend (the 128-byte id travels
        as an object broadcast); the data path afterwards is this library's
        own RCCL communicator."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0)
                                   if group is not None else 0, group=group)
        return cls(box[0], rank, world, device)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.opty_hip_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def bcast_free(self, hip, free, root=0):
        """``opty_hip_bcast_free``: the global free vector (device tensor /
        pointer) from ``root`` to every rank, on ``hip``'s stream."""
        _check(self._lib.opty_hip_bcast_free(self._h, hip._h, _ptr(free),
                                             int(root)))

    def gather_v(self, hip, bounds, con_shard, jac_shard, con_global,
                 jac_global, root=0, what=EVAL_PAIR):
        """``opty_hip_gather_v``: node shards to ``root`` (Jacobian slices
        in place, constraint blocks through one strided copy per peer)."""
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        assert len(b) == self.world + 1
        _check(self._lib.opty_hip_gather_v(
            self._h, hip._h, _ptr(b), _ptr(con_shard), _ptr(jac_shard),
            _ptr(con_global), _ptr(jac_global), int(root), int(what)))


class HipMatrix(object):
    """One ``opty_hip_matrix`` handle: a matrix of expressions evaluated for
    n argument rows (the ``ufuncify_matrix`` call shape)."""

    def __init__(self, desc, hsaco_path):
        self._lib = load_library()
        if self._lib.opty_hip_device_count() == 0:
            raise HipBackendError('no HIP device is visible: the HIP '
                                  'backend has no CPU fallback')
        self._h = _P()
        d = _MatDesc(**desc)
        _check(self._lib.opty_hip_matrix_create(
            ctypes.byref(d), hsaco_path.encode(), ctypes.byref(self._h)))
        self.desc = dict(desc)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.opty_hip_matrix_destroy(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream_ptr):
        _check(self._lib.opty_hip_matrix_set_stream(self._h, stream_ptr))

    def use_torch_stream(self, stream=None):
        """Run this handle's work on a torch stream (default: the current
        one), ordered with the torch operations issued there."""
        self.set_stream(torch_stream_pointer(stream))

    def evaluate(self, result, vec_args, const_args, n, mem):
        ptrs = (ctypes.c_void_p*max(1, len(vec_args)))(
            *[_ptr(v) for v in vec_args])
        cst = np.ascontiguousarray(const_args, dtype=np.float64)
        _check(self._lib.opty_hip_matrix_eval(
            self._h, _ptr(result), ctypes.addressof(ptrs), _ptr(cst), n, mem))


class HipObjective(object):
    """One ``opty_hip_objective`` handle (objective value + gradient)."""

    def __init__(self, desc, hsaco_path):
        self._lib = load_library()
        if self._lib.opty_hip_device_count() == 0:
            raise HipBackendError('no HIP device is visible: the HIP '
                                  'backend has no CPU fallback')
        self._h = _P()
        d = _ObjDesc(**desc)
        _check(self._lib.opty_hip_objective_create(
            ctypes.byref(d), hsaco_path.encode(), ctypes.byref(self._h)))
        self.desc = dict(desc)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.opty_hip_objective_destroy(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream_ptr):
        _check(self._lib.opty_hip_objective_set_stream(self._h, stream_ptr))

    def use_torch_stream(self, stream=None):
        """Run this handle's work on a torch stream (default: the current
        one), ordered with the torch operations issued there."""
        self.set_stream(torch_stream_pointer(stream))

    def evaluate(self, free, grad, mem):
        """Returns the objective value; fills ``grad`` when it is given."""
        value = ctypes.c_double()
        _check(self._lib.opty_hip_objective_eval(
            self._h, _ptr(free), ctypes.addressof(value), _ptr(grad), mem))
        return value.value


class HipObjectiveHessian(object):
    """One ``opty_hip_objhess`` handle: the exact Hessian of the objective
    (lower triangle, triplets; ``include/opty_hip.h``).  ``pattern``: ``(row
    var, row off, col var, col off)`` per per-point entry, ``tail_pairs``:
    the parameters ``(a, b)`` per parameter-parameter entry."""

    def __init__(self, desc, pattern, tail_pairs, hsaco_path):
        self._lib = load_library()
        if self._lib.opty_hip_device_count() == 0:
            raise HipBackendError('no HIP device is visible: the HIP '
                                  'backend has no CPU fallback')
        self._h = _P()
        table = np.ascontiguousarray(np.concatenate((
            np.asarray(pattern, dtype=np.int32).reshape(-1),
            np.asarray(tail_pairs, dtype=np.int32).reshape(-1))))
        assert len(table) == 4*desc['E'] + 2*desc['T']
        #: the index pattern and the parameter pairs the handle was made from
        self.pattern = np.asarray(pattern, dtype=np.int32).reshape(-1, 4)
        self.tail_pairs = np.asarray(tail_pairs,
                                     dtype=np.int32).reshape(-1, 2)
        d = _ObjHessDesc(**desc)
        _check(self._lib.opty_hip_objhess_create(
            ctypes.byref(d), _ptr(table) if len(table) else None,
            hsaco_path.encode(), ctypes.byref(self._h)))
        self.desc = dict(desc)
        self.nnz = self._lib.opty_hip_objhess_nnz(self._h)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.opty_hip_objhess_destroy(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream_ptr):
        _check(self._lib.opty_hip_objhess_set_stream(self._h, stream_ptr))

    def use_torch_stream(self, stream=None):
        """Run this handle's work on a torch stream (default: the current
        one), ordered with the torch operations issued there."""
        self.set_stream(torch_stream_pointer(stream))

    def indices(self, rows, cols, mem):
        _check(self._lib.opty_hip_objhess_indices(self._h, _ptr(rows),
                                                  _ptr(cols), mem))

    def evaluate(self, free, obj_factor, out, mem):
        """Fills ``out`` (``nnz`` values) with ``obj_factor`` times the
        Hessian's values; enqueued on the handle's stream for ``DEVICE``."""
        _check(self._lib.opty_hip_objhess_eval(
            self._h, _ptr(free), float(obj_factor), _ptr(out), mem))


class _DerivedHandle(object):
    """A C handle that borrows the device data of a :class:`HipProblem`.
    When the problem's C handle is replaced (:meth:`HipProblem.reload`) or
    closed, this handle is released first and created again for the new one
    on the next call.  Subclasses name their ``_create`` / ``_destroy``
    symbols and build their descriptor in ``_descriptor()``."""

    def __init__(self, problem, hsaco_path):
        self._lib = load_library()
        self._problem = problem
        self._hsaco = hsaco_path
        self._h = None
        import weakref
        deps = problem.__dict__.setdefault('_dependents', weakref.WeakSet())
        deps.add(self)
        self._handle()

    def _handle(self):
        if self._h is None:
            if not getattr(self._problem, '_h', None):
                raise HipBackendError('the problem handle is closed')
            d = self._descriptor()
            h = _P()
            # (a handle without a code object of its own: ``hsaco_path`` None)
            code = () if self._hsaco is None else (self._hsaco.encode(),)
            _check(getattr(self._lib, self._create)(
                self._problem._h, ctypes.byref(d), *code, ctypes.byref(h)))
            self._h = h
        return self._h

    def release(self):
        if getattr(self, '_h', None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    __del__ = release


class HipHessian(_DerivedHandle):
    """One ``opty_hip_hessian`` handle: the exact Hessian of the constraint
    Lagrangian of a :class:`HipProblem`, whose device data it borrows.  When
    the problem's C handle is replaced (:meth:`HipProblem.reload`) or closed,
    this handle is released first and created again for the new one on the
    next call."""

    _create, _destroy = 'opty_hip_hessian_create', 'opty_hip_hessian_destroy'

    def __init__(self, problem, desc, hsaco_path):
        self._desc = dict(desc)
        self._pattern = np.ascontiguousarray(desc['pattern'],
                                             dtype=np.int32).reshape(-1)
        self._irows = np.ascontiguousarray(desc['inst_rows'], dtype=np.int64)
        self._icols = np.ascontiguousarray(desc['inst_cols'], dtype=np.int64)
        super().__init__(problem, hsaco_path)
        self.nnz = self._lib.opty_hip_hessian_nnz(self._h)

    def _descriptor(self):
        return _HessDesc(PH=self._desc['PH'], nnz_inst=self._desc['nnz_inst'],
                         strips=self._desc['strips'],
                         pattern=_ptr(self._pattern),
                         inst_rows=_ptr(self._irows),
                         inst_cols=_ptr(self._icols))

    def evaluate(self, free, lagrange, hess, mem):
        _check(self._lib.opty_hip_eval_hess(self._handle(), _ptr(free),
                                            _ptr(lagrange), _ptr(hess), mem))

    def indices(self, rows, cols, mem):
        _check(self._lib.opty_hip_hessian_indices(self._handle(), _ptr(rows),
                                                  _ptr(cols), mem))

    def eval_shard(self, free, lagrange, hess_shard, node_begin, node_end):
        """The values of the constraint nodes ``[node_begin, node_end)`` from
        the global device ``free`` / ``lagrange`` into the ``(node_end -
        node_begin)*PH`` doubles ``hess_shard``; see
        ``opty_hip_eval_hess_shard`` in ``include/opty_hip.h``."""
        _check(self._lib.opty_hip_eval_hess_shard(
            self._handle(), _ptr(free), _ptr(lagrange), _ptr(hess_shard),
            int(node_begin), int(node_end)))

    def eval_instance(self, free, lagrange, inst_out):
        """The ``nnz_inst`` instance values into the device buffer
        ``inst_out`` (``opty_hip_eval_hess_instance``)."""
        _check(self._lib.opty_hip_eval_hess_instance(
            self._handle(), _ptr(free), _ptr(lagrange), _ptr(inst_out)))

    def indices_range(self, node_begin, node_end, rows, cols, mem):
        """Global indices of the values of the nodes ``[node_begin,
        node_end)`` (``opty_hip_hessian_indices_range``)."""
        _check(self._lib.opty_hip_hessian_indices_range(
            self._handle(), int(node_begin), int(node_end), _ptr(rows),
            _ptr(cols), mem))


class HipJacobianProduct(_DerivedHandle):
    """One ``opty_hip_jacprod`` handle: ``J(free) v`` and ``J(free)^T w`` of a
    :class:`HipProblem`, whose device data it borrows.  When the problem's C
    handle is replaced (:meth:`HipProblem.reload`) or closed, this handle is
    released first and created again for the new one on the next call."""

    _create, _destroy = 'opty_hip_jacprod_create', 'opty_hip_jacprod_destroy'

    def __init__(self, problem, desc, hsaco_path):
        self._desc = dict(desc)
        super().__init__(problem, hsaco_path)

    def _descriptor(self):
        return _JacprodDesc(**self._desc)

    def jvp(self, free, v, out, mem):
        _check(self._lib.opty_hip_jacprod_jvp(self._handle(), _ptr(free),
                                              _ptr(v), _ptr(out), mem))

    def vjp(self, free, w, out, mem):
        _check(self._lib.opty_hip_jacprod_vjp(self._handle(), _ptr(free),
                                              _ptr(w), _ptr(out), mem))

    def jvp_shard(self, free, v, out, out_stride, node_begin, node_end):
        """``J v`` of the constraint nodes ``[node_begin, node_end)`` from the
        global device ``free`` / ``v``; see ``opty_hip_jacprod_jvp_shard``
        in ``include/opty_hip.h``."""
        _check(self._lib.opty_hip_jacprod_jvp_shard(
            self._handle(), _ptr(free), _ptr(v), _ptr(out), int(out_stride),
            int(node_begin), int(node_end)))

    def jvp_instance(self, free, v, out_tail):
        """The ``o`` instance rows of ``J v`` into the device buffer
        ``out_tail`` (``opty_hip_jacprod_jvp_instance``)."""
        _check(self._lib.opty_hip_jacprod_jvp_instance(
            self._handle(), _ptr(free), _ptr(v), _ptr(out_tail)))

    def vjp_shard(self, free, w, out, out_stride, tail_part, node_begin,
                  node_end):
        """``J^T w`` on the time nodes the window ``[node_begin, node_end)``
        owns and the window's share ``tail_part`` of the tail entries; see
        ``opty_hip_jacprod_vjp_shard``."""
        _check(self._lib.opty_hip_jacprod_vjp_shard(
            self._handle(), _ptr(free), _ptr(w), _ptr(out), int(out_stride),
            _ptr(tail_part), int(node_begin), int(node_end)))


class HipJacobianBlockProduct(_DerivedHandle):
    """One ``opty_hip_jacprod_block`` handle: ``J(free) V`` and ``J(free)^T
    W`` of a :class:`HipProblem` for several columns per pass, over a block
    module of its own; borrows and follows the problem's C handle as
    :class:`HipJacobianProduct` does."""

    _create, _destroy = ('opty_hip_jacprod_block_create',
                         'opty_hip_jacprod_block_destroy')

    def __init__(self, problem, desc, hsaco_path):
        self._desc = dict(desc)
        super().__init__(problem, hsaco_path)

    def _descriptor(self):
        return _JacprodBlockDesc(**self._desc)

    @property
    def width(self):
        """Columns per pass."""
        return int(self._lib.opty_hip_jacprod_block_width(self._handle()))

    def jvp_block(self, free, V, ldv, Y, ldy, ncols, mem):
        _check(self._lib.opty_hip_jacprod_block_jvp(
            self._handle(), _ptr(free), _ptr(V), ldv, _ptr(Y), ldy, ncols,
            mem))

    def vjp_block(self, free, W, ldw, G, ldg, ncols, mem):
        _check(self._lib.opty_hip_jacprod_block_vjp(
            self._handle(), _ptr(free), _ptr(W), ldw, _ptr(G), ldg, ncols,
            mem))


class _HessianTripletsHandle(_DerivedHandle):
    """A handle over the stored triplets of the Hessian of the Lagrangian,
    made from an ``opty_hip_hessmv_desc``: ``desc`` holds ``PH, pattern,
    inst_rows, inst_cols`` and, with an objective section, ``E, obj_pattern,
    obj_base, tail_rows, tail_cols`` (``include/opty_hip.h``).  It borrows
    its :class:`HipProblem` for sizes, device and stream (no code object: the
    kernels are the runtime library's) and is released and created again
    with the problem's C handle, as the other derived handles are.
    Subclasses name ``_nnz``, the symbol that counts the triplets."""

    def __init__(self, problem, desc):
        def table(key, dtype, width):
            return np.ascontiguousarray(desc.get(key, ()),
                                        dtype=dtype).reshape(-1, width)
        self._pattern = table('pattern', np.int32, 4)
        self._obj_pattern = table('obj_pattern', np.int32, 4)
        self._irows, self._icols, self._trows, self._tcols = (
            table(key, np.int64, 1) for key in
            ('inst_rows', 'inst_cols', 'tail_rows', 'tail_cols'))
        # (explicit counts: what the error-path tests hand over on purpose)
        self._counts = dict(
            PH=desc.get('PH', len(self._pattern)),
            nnz_inst=desc.get('nnz_inst', len(self._irows)),
            E=desc.get('E', len(self._obj_pattern)),
            obj_base=desc.get('obj_base', 0),
            T=desc.get('T', len(self._trows)))
        super().__init__(problem, None)
        self.nnz = getattr(self._lib, self._nnz)(self._h)

    def _descriptor(self):
        def ptr(a):
            return _ptr(a) if a.size else None
        return _HessmvDesc(
            pattern=ptr(self._pattern), inst_rows=ptr(self._irows),
            inst_cols=ptr(self._icols), obj_pattern=ptr(self._obj_pattern),
            tail_rows=ptr(self._trows), tail_cols=ptr(self._tcols),
            **{k: int(v) for k, v in self._counts.items()})


class HipHessianProduct(_HessianTripletsHandle):
    """One ``opty_hip_hessmv`` handle: ``y = H v`` from the stored triplets of
    the Hessian of the Lagrangian of a :class:`HipProblem`
    (:class:`_HessianTripletsHandle`)."""

    _create, _destroy = 'opty_hip_hessmv_create', 'opty_hip_hessmv_destroy'
    _nnz = 'opty_hip_hessmv_nnz'

    def sides(self):
        """``(sides, number of trajectory sides)`` of the handle's side
        table: ``(row, slot)`` pairs, ``(-1, offset)`` for a tail side."""
        ntraj = ctypes.c_int32()
        count = self._lib.opty_hip_hessmv_sides(self._handle(), None, 0,
                                                ctypes.addressof(ntraj))
        out = np.zeros((count, 2), dtype=np.int32)
        self._lib.opty_hip_hessmv_sides(self._handle(), _ptr(out), count,
                                        None)
        return [tuple(int(x) for x in row) for row in out], ntraj.value

    def apply(self, values, v, y, mem):
        _check(self._lib.opty_hip_hessmv_apply(
            self._handle(), _ptr(values), _ptr(v), _ptr(y), mem))

    @property
    def block_width(self):
        """Columns one pass of :meth:`apply_block` takes (1 .. 4): the widest
        ``opty_hessmv_block`` whose LDS fits the device's limit per block
        (``codegen.program.hessian_block_width``)."""
        return int(self._lib.opty_hip_hessmv_block_width(self._handle()))

    def apply_block(self, values, V, ldv, Y, ldy, ncols, mem):
        """``Y = H V`` for ``ncols`` contiguous columns, column ``c`` of
        ``V`` at ``c*ldv`` and of ``Y`` at ``c*ldy`` doubles: bit for bit
        what :meth:`apply` gives column by column."""
        _check(self._lib.opty_hip_hessmv_apply_block(
            self._handle(), _ptr(values), _ptr(V), int(ldv), _ptr(Y),
            int(ldy), int(ncols), mem))

    def apply_shard(self, values_shard, inst_values, v, out, out_stride,
                    tail_part, node_begin, node_end, tail_owner):
        """The share of ``H v`` of the constraint nodes ``[node_begin,
        node_end)`` from the global device ``v`` and the window's values (one
        halo node in front when ``node_begin > 0``): the owned time nodes
        into ``out``, the share of the tail entries into ``tail_part``; see
        ``opty_hip_hessmv_apply_shard`` in ``include/opty_hip.h``."""
        _check(self._lib.opty_hip_hessmv_apply_shard(
            self._handle(), _ptr(values_shard), _ptr(inst_values), _ptr(v),
            _ptr(out), int(out_stride), _ptr(tail_part), int(node_begin),
            int(node_end), int(bool(tail_owner))))


class HipHessianCsr(_HessianTripletsHandle):
    """One ``opty_hip_hesscsr`` handle: the stored triplets of the Hessian of
    the Lagrangian of a :class:`HipProblem` compressed to the CSR lower
    triangle, every pair once, duplicates summed in a fixed order
    (:class:`_HessianTripletsHandle`; ``include/opty_hip.h``, "Hessian as
    CSR")."""

    _create, _destroy = 'opty_hip_hesscsr_create', 'opty_hip_hesscsr_destroy'
    _nnz = 'opty_hip_hesscsr_nnz'

    @property
    def nnz_unique(self):
        """Distinct ``(row, col)`` pairs: the length of ``data``."""
        return int(self._lib.opty_hip_hesscsr_nnz_unique(self._handle()))

    def structure(self, indptr, indices, mem):
        _check(self._lib.opty_hip_hesscsr_structure(
            self._handle(), _ptr(indptr), _ptr(indices), mem))

    def compress(self, values, data, mem):
        _check(self._lib.opty_hip_hesscsr_compress(
            self._handle(), _ptr(values), _ptr(data), mem))


class HipKktCsr(_HessianTripletsHandle):
    """One ``opty_hip_kktcsr`` handle: the lower triangle of the augmented
    system ``[[W + diag(sigma) + delta_w I, J^T], [J, -delta_c I]]`` of a
    :class:`HipProblem` with ``jacobian_layout='csr'`` as one canonical CSR
    matrix, every diagonal stored, assembled on the device from the
    Hessian's triplets and the Jacobian's values
    (:class:`_HessianTripletsHandle`; ``include/opty_hip.h``, "Augmented
    system as CSR").  ``nnz`` counts the Hessian's triplets."""

    _create, _destroy = 'opty_hip_kktcsr_create', 'opty_hip_kktcsr_destroy'
    _nnz = 'opty_hip_kktcsr_nnz_triplets'

    @property
    def nnz_kkt(self):
        """Stored values of ``K``: the length of ``indices`` and ``data``."""
        return int(self._lib.opty_hip_kktcsr_nnz(self._handle()))

    @property
    def nnz_hessian(self):
        """Stored values of the ``W`` block, diagonals included."""
        return int(self._lib.opty_hip_kktcsr_nnz_hessian(self._handle()))

    def structure(self, indptr, indices, mem):
        _check(self._lib.opty_hip_kktcsr_structure(
            self._handle(), _ptr(indptr), _ptr(indices), mem))

    def assemble(self, hess_values, jac_values, sigma, delta_w, delta_c,
                 data, mem):
        _check(self._lib.opty_hip_kktcsr_assemble(
            self._handle(), _ptr(hess_values), _ptr(jac_values),
            None if sigma is None else _ptr(sigma), float(delta_w),
            float(delta_c), _ptr(data), mem))

    def assemble_timed(self, hess_values, jac_values, sigma, delta_w,
                       delta_c, data):
        """The same for device pointers, synchronous: ``(compression,
        opty_kkt_diag, opty_kkt_jrows, opty_kkt_inst)`` in milliseconds by
        device events (``opty_hip_kktcsr_assemble_timed``)."""
        ms = np.zeros(4, dtype=np.float32)
        _check(self._lib.opty_hip_kktcsr_assemble_timed(
            self._handle(), _ptr(hess_values), _ptr(jac_values),
            None if sigma is None else _ptr(sigma), float(delta_w),
            float(delta_c), _ptr(data), _ptr(ms)))
        return tuple(float(x) for x in ms)


class HipNormalSolver(_DerivedHandle):
    """One ``opty_hip_normal`` handle: the block-tridiagonal normal matrix
    ``S = Jc[:, :T] diag(1/d[:T]) Jc[:, :T]^T + delta_c I`` of a
    :class:`HipProblem`, formed from the Jacobian's values, factorised by
    block cyclic reduction with Cholesky factors and solved with, all on the
    device (``include/opty_hip.h``, "Normal matrix").  ``desc`` holds ``M``,
    ``layout`` (``'coo'`` / ``'csr'``) and ``pattern``, the ``(j, k)`` of the
    stored block entries.  It borrows its problem for sizes, method, device
    and stream (no code object: the kernels are the runtime library's) and
    is released and created again with the problem's C handle, as the other
    derived handles are."""

    _create, _destroy = 'opty_hip_normal_create', 'opty_hip_normal_destroy'
    _LAYOUTS = {'coo': 0, 'csr': 1}

    def __init__(self, problem, desc):
        self._pattern = np.ascontiguousarray(
            desc['pattern'], dtype=np.int32).reshape(-1, 2)
        self.M = int(desc['M'])
        # (an explicit count: what the error-path tests hand over on purpose)
        self.P = int(desc.get('P', len(self._pattern)))
        layout = desc.get('layout', 'coo')
        self._layout = self._LAYOUTS.get(layout, layout)
        super().__init__(problem, None)

    def _descriptor(self):
        return _NormalDesc(
            M=self.M, P=self.P, layout=int(self._layout),
            pattern=_ptr(self._pattern) if self._pattern.size else None)

    @property
    def workspace_bytes(self):
        """Device memory the handle owns for the levels and its tables."""
        return int(self._lib.opty_hip_normal_workspace_bytes(self._handle()))

    @property
    def max_equations(self):
        """The largest ``M`` a handle on this device takes."""
        return int(self._lib.opty_hip_normal_max_equations(self._handle()))

    def blocks(self, jac_values, d, delta_c, A, B, mem):
        _check(self._lib.opty_hip_normal_blocks(
            self._handle(), _ptr(jac_values), None if d is None else _ptr(d),
            float(delta_c), _ptr(A), _ptr(B), mem))

    def factor(self, jac_values, d, delta_c, mem):
        """Enqueues (``DEVICE``) or runs (``HOST``) the factorisation;
        :meth:`status` says how it went."""
        _check(self._lib.opty_hip_normal_factor(
            self._handle(), _ptr(jac_values), None if d is None else _ptr(d),
            float(delta_c), mem))

    def status(self):
        """``None`` after a factorisation whose pivots were all positive and
        finite, else ``(level, row)`` of the first one that was not; waits
        for the factorisation."""
        level, row = ctypes.c_int32(), ctypes.c_int64()
        _check(self._lib.opty_hip_normal_factor_status(
            self._handle(), ctypes.addressof(level), ctypes.addressof(row)))
        return None if level.value < 0 else (level.value, row.value)

    def solve(self, r, y, ncols, ld, mem):
        _check(self._lib.opty_hip_normal_solve(
            self._handle(), _ptr(r), _ptr(y), int(ncols), int(ld), mem))
