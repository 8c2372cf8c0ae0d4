"""CPU tests of the node-sharded exact Hessian (the constraint triplets of a
node-sharded problem, every rank its own nodes): the header, the bindings and
the library agree; the emitted kernels carry the window and keep their
flushes; a lane-by-lane model of ``opty_hess`` stores every node of a window
once; two gloo ranks serve ``ShardedCallbacks.hessian`` with the interpreter
injected; and ``ShardedProblem`` takes ``obj_hessian``.  No GPU is needed."""
import os
import re
import socket

import numpy as np
import pytest

import hessian_cases as hc
import hessian_shard_cases as cases
from test_jacprod_shard_cpu import CTYPES, _declaration

from examples import problems
from opty_amd import hip_backend as hb
from opty_amd.sharded import partition_nodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    'opty_hip_eval_hess_shard': (
        'int', ['*', '*', '*', '*', 'int64_t', 'int64_t']),
    'opty_hip_eval_hess_instance': ('int', ['*', '*', '*', '*']),
    'opty_hip_hessian_indices_range': (
        'int', ['*', 'int64_t', 'int64_t', '*', '*', 'int32_t'])}

#: ``hessian_cases.flush_calls`` of the default module of each problem, as
#: the commit before the window arguments emitted them
FLUSHES = {
    'A': [(16, 16, 0, 52), (16, 16, 16, 52), (16, 16, 32, 52),
          (16, 4, 48, 52)],
    'C': [(16, 16, 0, 30), (16, 14, 16, 30)],
    'E': [(8, 16, 0, 21), (8, 5, 16, 21)]}
KERNELS = {'A': ['opty_hess'], 'C': ['opty_hess', 'opty_hess_inst'],
           'E': ['opty_hess']}


def test_header_bindings_and_library_agree():
    hb.build_runtime_library()
    lib = hb.load_library()
    for name, want in DECLARED.items():
        res, args = _declaration(name)
        assert (res, args) == want, name
        have_res, have_args = hb._SIGNATURES[name]
        assert have_res == CTYPES[res] and len(have_args) == len(args), name
        for have, a in zip(have_args, args):
            assert have == (hb._P if a == '*' else CTYPES[a]), (name, have, a)
        assert hasattr(lib, name), name
    for method in ('eval_shard', 'eval_instance', 'indices_range'):
        assert hasattr(hb.HipHessian, method)
    # additive: the version is the one the existing clients were built for
    assert hb.ABI_VERSION == 12
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        header = f.read()
    assert re.search(r'#define OPTY_HIP_ABI_VERSION 12\b', header)
    # ... and the version comment names them
    comment = header[:header.index('#define OPTY_HIP_ABI_VERSION')]
    for name in DECLARED:
        assert name in comment, name


@pytest.mark.parametrize('label', cases.PROBLEMS)
def test_emitted_source_carries_the_window_and_keeps_its_flushes(label):
    from opty_amd.codegen import emit_hessian as eh
    prog = hc.collocator(label, 7)._build_hessian_program()
    source, _ = eh.emit_hessian_module(prog)
    kernels = re.findall(r'__launch_bounds__\(64\)\s+(\w+)\(', source)
    assert kernels == KERNELS[label]
    assert source.count('__global__') == len(kernels)
    assert source.count('long long wa, long long wb, double *__restrict__ '
                        'tail)') == len(kernels)
    assert eh.HESS_PARAMS.endswith(
        'double h, long long N, long long wa, long long wb, '
        'double *__restrict__ tail')
    # values are addressed from the window's origin
    assert 'hess + (i0 - wa)*%dLL' % prog.PH in source
    assert 'atomic' not in source.lower() and 'asm' not in source
    assert hc.flush_calls(source) == FLUSHES[label]
    if 'opty_hess_inst' in kernels:
        inst = source[source.index('opty_hess_inst('):]
        assert 'tail[0] = ' in inst and 'hess[' not in inst


def test_window_preamble_is_one_function_and_the_products_keep_theirs():
    """``block_preamble`` has a window form, not a fork: without it the text
    is what the block product kernels were emitted with."""
    from opty_amd.codegen.emit_strips import block_preamble
    assert block_preamble(63) == [
        'const int lane = threadIdx.x;',
        'const long long ncn = N - 1;',
        'const long long i0 = (long long)blockIdx.x*63;',
        'if (i0 >= ncn) return;',
        'const long long i = i0 + lane;',
        'const long long ic = i < ncn ? i : ncn - 1;']
    assert block_preamble(window=True) == [
        'const int lane = threadIdx.x;',
        'const long long ncn = N - 1;',
        'const long long i0 = wa + (long long)blockIdx.x*64;',
        'if (i0 >= wb) return;',
        'const long long i = i0 + lane;',
        'const long long ic = i < wb ? i : wb - 1;']


def _hess_lanes(wa, wb):
    """What ``opty_hess`` does with the window ``[wa, wb)``, lane by lane, in
    the kernel's and the launch's own terms: ``[(node, row of hess it is
    stored to)]``; a flush writes rows ``0 .. nv - 1`` of the block's tile
    to ``hrow + row*PH``, ``hrow = hess + (i0 - wa)*PH``."""
    stores = []
    nblk = (wb - wa + 63)//64           # csrc/hessian.cpp, launch_hess
    for blk in range(nblk):
        i0 = wa + 64*blk
        assert i0 < wb, 'a block with nothing to do was launched'
        nv = min(64, wb - i0)
        assert 1 <= nv <= 64
        for lane in range(64):
            i = i0 + lane
            ic = i if i < wb else wb - 1
            assert wa <= ic < wb        # every load is a node of the window
            if lane < nv:
                assert ic == i
                stores.append((i, (i0 - wa) + lane))
    return stores


@pytest.mark.parametrize('window', cases.WINDOWS,
                         ids=['%d-%d' % w for w in cases.WINDOWS])
def test_every_node_of_a_window_is_stored_once(window):
    a, b = window
    stores = _hess_lanes(a, b)
    assert [i for i, _ in stores] == list(range(a, b))
    assert [row for _, row in stores] == list(range(b - a))
    assert all(row == i - a for i, row in stores)


@pytest.mark.parametrize('world', cases.WORLDS)
def test_partitions_tile_the_value_vector(world):
    PH = 52
    seen = np.zeros(cases.NCN*PH, dtype=int)
    for a, b in partition_nodes(cases.NCN, world):
        for i, row in _hess_lanes(a, b):
            seen[a*PH + row*PH:a*PH + (row + 1)*PH] += 1
    assert (seen == 1).all()


# -- two gloo ranks --------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _unused(*args, **kwargs):
    raise AssertionError('only the Hessian is asked for')


class _Interpreter(object):
    """``hessian_evaluator``: the CPU interpreter of the Hessian DAG
    (``hessian_cases.interpreted``) at the window's nodes."""

    col = None
    calls = 0

    def __call__(self, free, lagrange, hess1d, inst_out, a, b):
        import torch
        self.calls += 1
        block, inst, _ = hc.interpreted(self.col, free.numpy(),
                                        lagrange.numpy(), np.arange(a, b))
        hess1d.copy_(torch.from_numpy(np.ascontiguousarray(block).ravel()))
        if inst_out is not None:
            inst_out.copy_(torch.from_numpy(inst))


#: constraint nodes of the gloo tests (the interpreter is Python)
SMALL = 9


def _callbacks_worker(rank, world, port, label, out):
    import torch.distributed as dist
    from opty_amd.sharded import ShardedCallbacks, ShardedCollocator
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        ev = _Interpreter()
        sh = ShardedCollocator(
            evaluator=_unused, instance_evaluator=_unused,
            hessian_evaluator=ev, **hc.KERNEL_PROBLEMS[label](SMALL + 1))
        ev.col = sh.collocator
        # a collocator that is never asked holds nothing new
        assert sh.hess_local is None and sh.hess_inst is None
        assert sh._hessian_handle is None
        assert getattr(sh.collocator, '_hessian_program', None) is None
        cb = ShardedCallbacks(sh, name='opty_t_hs_%d' % port)
        assert cb.hess_host is None and cb.lam_host is None
        if rank != 0:
            cb.serve()
            assert cb.hess_host is not None and ev.calls == 3
            return
        free, lam = hc.inputs(21, sh.collocator)
        got = cb.hessian(free, lam)
        assert got is cb.hess_host.array            # persistent
        first = np.array(got)
        # multipliers per call, back to back: no rank may read the previous
        # ones (a power of two scales the values exactly)
        second = np.array(cb.hessian(free, 2.0*lam))
        third = np.array(cb.hessian(free, lam))
        with pytest.raises(ValueError):
            cb.hessian(free, lam[:-1])
        with pytest.raises(ValueError):
            cb.hessian(free[:-1], lam)
        np.savez(out, free=free, lam=lam, first=first, second=second,
                 third=third, nnz=sh.hessian_nnz,
                 ab=np.array([sh.a, sh.b]))
        cb.shutdown()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('label', ['C', 'A'])
def test_two_ranks_serve_the_hessian(tmp_path, label):
    """``ShardedCallbacks.hessian`` on the root with the interpreter injected
    as ``hessian_evaluator``: exactly the interpreter's whole-problem values,
    with (C) and without (A) instance entries."""
    import torch.multiprocessing as mp
    out = str(tmp_path/'root.npz')
    mp.spawn(_callbacks_worker, args=(2, _free_port(), label, out), nprocs=2,
             join=True)
    z = np.load(out)
    col = hc.collocator(label, SMALL)
    block, inst, _ = hc.interpreted(col, z['free'], z['lam'])
    assert (len(inst) > 0) == (label == 'C')
    want = np.concatenate((block.ravel(), inst))
    assert int(z['nnz']) == len(want)
    assert tuple(z['ab']) == partition_nodes(SMALL, 2)[0]
    assert np.array_equal(z['first'].view(np.int64), want.view(np.int64))
    assert np.array_equal(z['second'], 2.0*want)
    assert np.array_equal(z['third'].view(np.int64), want.view(np.int64))


def _problem_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    import opty_amd
    from opty_amd import direct_collocation as dc
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        # the Jacobian's structure comes from the device and is not what
        # this test is about
        none = np.zeros(0, dtype=np.int64)
        dc.ConstraintCollocator.jacobian_indices = lambda self: (none, none)

        def make(kw, ev, obj_hessian):
            return opty_amd.ShardedProblem(
                lambda f: 0.0, lambda f: 0.0*f, torch_device='cpu',
                obj_hessian=obj_hessian,
                sharded_kwargs=dict(evaluator=_unused,
                                    instance_evaluator=_unused,
                                    hessian_evaluator=ev), **kw)

        # refused at construction, on every rank, before any collective:
        # implicit known trajectories ...
        implicit = problems.build('implicit_traj_be_small')
        with pytest.raises(NotImplementedError):
            make(implicit, _unused, ([0], [0], lambda f: np.ones(1)))
        # ... and known trajectories that are functions of free
        kw = hc.KERNEL_PROBLEMS['C'](SMALL + 1)
        sym = next(iter(kw['known_trajectory_map']))
        called = dict(kw, known_trajectory_map={
            sym: lambda free: np.ones(SMALL + 1)})
        with pytest.raises(NotImplementedError, match='functions of'):
            make(called, _unused, ([0], [0], lambda f: np.ones(1)))
        # Problem's checks
        with pytest.raises(ValueError, match='lower triangle'):
            make(kw, _unused, ([0], [1], lambda f: np.ones(1)))

        nf = opty_amd.ConstraintCollocator(**kw).num_free
        orows = np.array([0, nf - 1, nf - 1], dtype=np.int64)
        ocols = np.array([0, 0, nf - 1], dtype=np.int64)
        seen = []

        def values(free):
            seen.append(rank)
            return np.array([1.0, 2.0, 3.0])*free[0]

        ev = _Interpreter()
        prob = make(kw, ev, (orows, ocols, values))
        ev.col = prob.collocator
        assert prob.callbacks.hessian_extra == 3
        with pytest.raises(NotImplementedError, match='hessian_operator'):
            prob.hessian_operator(None, None)
        if rank != 0:
            assert not hasattr(prob, 'hessian')
            prob.serve()
            assert seen == []
            return
        free, lam = hc.inputs(22, prob.collocator)
        with pytest.raises(TypeError, match='host arrays'):
            prob.hessian(torch.from_numpy(free), lam, 1.0)
        rows, cols = prob.hessianstructure()
        got = prob.hessian(free, lam, 0.7)
        assert got is prob.callbacks.hess_host.array
        crows, ccols = prob.collocator.hessian_indices_closed_form()
        np.savez(out, free=free, lam=lam, got=np.array(got), rows=rows,
                 cols=cols, crows=crows, ccols=ccols, orows=orows,
                 ocols=ocols)
        assert seen == [0]
        prob.shutdown()
    finally:
        dist.destroy_process_group()


def test_sharded_problem_takes_an_objective_hessian(tmp_path):
    """``ShardedProblem(obj_hessian=...)`` (refused before the Hessian was
    sharded): the ``[constraint | objective]`` structure of ``Problem``, the
    constraint section from all ranks, the objective's from the root
    alone."""
    import torch.multiprocessing as mp
    out = str(tmp_path/'root.npz')
    mp.spawn(_problem_worker, args=(2, _free_port(), out), nprocs=2,
             join=True)
    z = np.load(out)
    col = hc.collocator('C', SMALL)
    block, inst, _ = hc.interpreted(col, z['free'], z['lam'])
    want = np.concatenate((block.ravel(), inst,
                           0.7*(np.array([1.0, 2.0, 3.0])*z['free'][0])))
    assert np.array_equal(z['got'].view(np.int64), want.view(np.int64))
    assert np.array_equal(z['rows'], np.concatenate((z['crows'],
                                                     z['orows'])))
    assert np.array_equal(z['cols'], np.concatenate((z['ccols'],
                                                     z['ocols'])))
    assert np.all(z['rows'] >= z['cols'])


def test_obj_hessian_without_a_process_group_is_refused():
    """No ``torch.distributed`` group, no ranks to serve the Hessian: refused
    at construction, before anything else is looked at."""
    import torch.distributed as dist
    import opty_amd
    assert not dist.is_initialized()
    kw = hc.KERNEL_PROBLEMS['C'](SMALL + 1)
    with pytest.raises(NotImplementedError, match='process group'):
        opty_amd.ShardedProblem(lambda f: 0.0, lambda f: 0.0*f,
                                obj_hessian=([0], [0], lambda f: np.ones(1)),
                                **kw)
