"""GPU tests of the node-sharded exact Hessian (C ABI
``opty_hip_eval_hess_shard`` / ``opty_hip_eval_hess_instance`` /
``opty_hip_hessian_indices_range``: ``opty_hess`` over a window of the
constraint nodes; ``ShardedProblem(obj_hessian=...)``).  The contract:

1. the union of the windows of any partition, written in place, has the BITS
   of ``opty_hip_eval_hess`` of the same handle (the instance values by
   ``eval_instance``);
2. nothing outside a window's slice is written (outputs start as NaN);
3. a second call gives the same bits;
4. ``indices_range`` is the slice of ``hessian_indices()``;
5. the whole-problem values still meet the criterion of
   tests/test_hessian_kernel_gpu.py against the CPU interpreter."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import hessian_cases as hc
import hessian_shard_cases as cases
from golden_util import assert_close

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GUARD = 8               # doubles of NaN on either side of a dense block
_CACHE = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


class _Case(object):
    """A collocator, its Hessian handle, inputs on the device and the
    whole-problem values of the same handle (``opty_hip_eval_hess`` with
    device pointers)."""

    def __init__(self, label, seed):
        import torch
        from opty_amd import hip_backend as hb
        self.label = label
        self.col = col = cases.collocator(label)
        self.handle = col.generate_hessian_function().handle
        prog = col._build_hessian_program()
        self.PH, self.nnz_inst = prog.PH, len(prog.inst_hess_out)
        self.ncn = col.num_collocation_nodes - 1
        assert self.ncn == cases.NCN
        self.nnz = self.handle.nnz
        assert self.nnz == self.ncn*self.PH + self.nnz_inst
        self.free, self.lam = hc.inputs(seed, col)
        col.hip.use_torch_stream()
        self.dev = torch.device('cuda', col._device)
        self.dfree, self.dlam = (torch.from_numpy(x).to(self.dev)
                                 for x in (self.free, self.lam))
        col.sync_known()
        whole = self.nan(self.nnz)
        self.handle.evaluate(self.dfree, self.dlam, whole, hb.DEVICE)
        torch.cuda.synchronize()
        self.whole = whole.cpu().numpy()
        assert np.isfinite(self.whole).all()

    def nan(self, count):
        import torch
        return torch.full((count,), np.nan, dtype=torch.float64,
                          device=self.dev)

    def partition(self, ranges):
        """Every window of ``ranges`` written IN PLACE into a NaN-filled
        global vector, the instance values by ``eval_instance``."""
        import torch
        PH = self.PH
        g = self.nan(self.nnz)
        for a, b in ranges:
            self.handle.eval_shard(self.dfree, self.dlam, g[a*PH:], a, b)
        self.handle.eval_instance(self.dfree, self.dlam, g[self.ncn*PH:])
        torch.cuda.synchronize()
        return g.cpu().numpy()

    def check_partition(self, ranges, what):
        """Contract points 1 and 3 for the partition ``ranges``."""
        got = self.partition(ranges)
        assert np.array_equal(_bits(got), _bits(self.whole)), what
        again = self.partition(ranges)
        assert np.array_equal(_bits(again), _bits(got)), what


def _case(label):
    if label not in _CACHE:
        _CACHE[label] = _Case(label, 23)
    return _CACHE[label]


@pytest.mark.parametrize('label', cases.PROBLEMS)
@pytest.mark.parametrize('window', cases.WINDOWS,
                         ids=['%d-%d' % w for w in cases.WINDOWS])
def test_window_edges_into_dense_blocks(label, window):
    """A window through the C ABI into a NaN-filled dense block between guard
    bands: the whole evaluation's bits on the slice, NaN everywhere else, the
    same bits again, and the window's indices."""
    import torch
    from opty_amd import hip_backend as hb
    c = _case(label)
    a, b = window
    count = (b - a)*c.PH
    want = c.whole[a*c.PH:b*c.PH]
    for attempt in range(2):
        buf = c.nan(GUARD + count + GUARD)
        c.handle.eval_shard(c.dfree, c.dlam, buf[GUARD:], a, b)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[-GUARD:]).all()
        assert np.array_equal(_bits(got[GUARD:GUARD + count]), _bits(want))
    rows = np.full(count + 2, -7, dtype=np.int64)
    cols = np.full(count + 2, -7, dtype=np.int64)
    c.handle.indices_range(a, b, rows[1:], cols[1:], hb.HOST)
    r0, c0 = c.col.hessian_indices()
    assert np.array_equal(rows[1:-1], r0[a*c.PH:b*c.PH])
    assert np.array_equal(cols[1:-1], c0[a*c.PH:b*c.PH])
    assert rows[0] == rows[-1] == cols[0] == cols[-1] == -7


@pytest.mark.parametrize('label', cases.PROBLEMS)
@pytest.mark.parametrize('world', cases.WORLDS)
def test_partitions_in_place(label, world):
    import torch
    from opty_amd.sharded import partition_nodes
    c = _case(label)
    ranges = partition_nodes(c.ncn, world)
    c.check_partition(ranges, '%s over %d ranks' % (label, world))
    # one rank alone: nothing but its slice is written
    a, b = ranges[world//2]
    g = c.nan(c.nnz)
    c.handle.eval_shard(c.dfree, c.dlam, g[a*c.PH:], a, b)
    torch.cuda.synchronize()
    mine = np.zeros(c.nnz, dtype=bool)
    mine[a*c.PH:b*c.PH] = True
    assert np.array_equal(~np.isnan(g.cpu().numpy()), mine)
    # ... and the instance values alone
    g = c.nan(c.nnz)
    c.handle.eval_instance(c.dfree, c.dlam, g[c.ncn*c.PH:])
    torch.cuda.synchronize()
    mine = np.zeros(c.nnz, dtype=bool)
    mine[c.ncn*c.PH:] = True
    assert np.array_equal(~np.isnan(g.cpu().numpy()), mine)
    if label == 'C':
        assert c.nnz_inst > 0


def test_three_way_partition_of_two_strips():
    from opty_amd.sharded import partition_nodes
    c = _Case(cases.TWO_STRIPS, 24)
    assert c.col._hessian_meta['strips'] == 2
    c.check_partition(partition_nodes(c.ncn, 3), 'D over 3 ranks')
    c.col.hip.set_stream(None)


@pytest.mark.parametrize('label', cases.PROBLEMS)
def test_whole_problem_values_against_the_interpreter(label):
    """The whole-problem kernel is the windowed kernel over ``[0, N-1)``: the
    criterion of tests/test_hessian_kernel_gpu.py."""
    c = _case(label)
    block, inst, bnd = hc.interpreted(c.col, c.free, c.lam)
    split = c.ncn*c.PH
    assert_close(c.whole[:split], block.ravel(), rtol=1e-12,
                 bound=bnd.ravel(), what=label)
    np.testing.assert_allclose(c.whole[split:], inst, rtol=1e-12,
                               atol=1e-300)


def test_c_abi_rejections():
    """Bad windows, null pointers and a misaligned base return an error with
    the offending number in the message, before anything is enqueued; an odd
    base is accepted for an odd PH; the handle still works."""
    import torch
    from opty_amd import hip_backend as hb
    lib = hb.load_library()
    c = _case('A')
    h, ncn, PH = c.handle, c.ncn, c.PH
    assert PH % 2 == 0
    out = c.nan(c.nnz)
    idx = np.full(c.nnz, -7, dtype=np.int64)
    for (a, b), number in (((-1, 5), '-1'), ((0, ncn + 1), str(ncn + 1)),
                           ((7, 6), '7')):
        with pytest.raises(hb.HipBackendError, match=number):
            h.eval_shard(c.dfree, c.dlam, out, a, b)
        with pytest.raises(hb.HipBackendError, match=number):
            h.indices_range(a, b, idx, idx, hb.HOST)
    for args in ((None, c.dlam, out), (c.dfree, None, out),
                 (c.dfree, c.dlam, None)):
        with pytest.raises(hb.HipBackendError, match='null'):
            h.eval_shard(*args, 0, 10)
    for args in ((None, idx), (idx, None)):
        with pytest.raises(hb.HipBackendError, match='null'):
            h.indices_range(0, 10, *args, hb.HOST)
    P = hb._ptr
    assert lib.opty_hip_eval_hess_shard(None, P(c.dfree), P(c.dlam), P(out),
                                        0, 10) != 0
    assert b'null' in lib.opty_hip_last_error()
    assert lib.opty_hip_eval_hess_instance(None, P(c.dfree), P(c.dlam),
                                           P(out)) != 0
    assert b'null' in lib.opty_hip_last_error()
    assert lib.opty_hip_hessian_indices_range(None, 0, 10, P(idx), P(idx),
                                              hb.HOST) != 0
    assert b'null' in lib.opty_hip_last_error()
    # an even PH is written with 16-byte stores: a base at 8 mod 16 is refused
    odd = out[1:]
    assert odd.data_ptr() % 16 == 8
    with pytest.raises(hb.HipBackendError, match='aligned') as err:
        h.eval_shard(c.dfree, c.dlam, odd, 0, 10)
    assert '%x' % odd.data_ptr() in str(err.value) and \
        '(%d)' % PH in str(err.value)
    # no instance entries: succeeds and writes nothing, whatever the pointer
    assert c.nnz_inst == 0
    h.eval_instance(c.dfree, c.dlam, None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()           # nothing was enqueued
    assert (idx == -7).all()
    # with instance entries a null destination is refused
    ci = _case('C')
    assert ci.nnz_inst > 0
    with pytest.raises(hb.HipBackendError, match='null'):
        ci.handle.eval_instance(ci.dfree, ci.dlam, None)
    # an odd PH takes 8-byte stores: the same base is accepted
    e = _case('E')
    assert e.PH % 2 == 1
    buf = e.nan(GUARD + 1 + 10*e.PH + GUARD)
    base = buf[GUARD + 1:]
    assert base.data_ptr() % 16 == 8
    e.handle.eval_shard(e.dfree, e.dlam, base, 3, 13)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[:GUARD + 1]).all() and np.isnan(got[-GUARD:]).all()
    assert np.array_equal(_bits(got[GUARD + 1:-GUARD]),
                          _bits(e.whole[3*e.PH:13*e.PH]))
    # the handle still works
    c.check_partition([(0, ncn)], 'after the rejections')


# -- ShardedProblem(obj_hessian=...): processes that share the one GPU -----------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(backend, world, out, limit=240):
    """Starts the ranks, each under its own time limit, and checks every exit
    status."""
    port = _free_port()
    worker = os.path.join(REPO, 'tests', 'hessian_shard_worker.py')
    procs = [subprocess.Popen(
        [sys.executable, worker, backend, str(r), str(world), str(port),
         out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=limit)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, text) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, 'rank %d:\n%s' % (r, text[-3000:])
        # (a serving rank gets here only when shutdown() released it)
        assert 'rank %d of %d ok' % (r, world) in text


@pytest.mark.parametrize('backend,world', [('gloo', cases.RANKS),
                                           ('nccl', 1)])
def test_sharded_problem_hessian_equals_the_single_gpu_problem(tmp_path,
                                                               backend,
                                                               world):
    """``ShardedProblem(obj_hessian=create_objective_hessian_function(...))``
    on problem A: the root's ``hessianstructure()`` and ``hessian(free,
    lagrange, 0.7)``, served by all ranks, against a single-GPU ``Problem``
    with the same arguments -- bit for bit, both sections (the same kernels
    on the same GPU)."""
    import opty_amd
    out = str(tmp_path/'root.npz')
    _run_ranks(backend, world, out)
    z = np.load(out)
    assert tuple(z['ab']) == (0, -(-cases.NCN//world))
    kw = cases.process_kwargs()
    single = opty_amd.Problem(lambda f: 0.0, lambda f: 0.0*f,
                              obj_hessian=cases.process_obj_hessian(kw),
                              **kw)
    rows, cols = single.hessianstructure()
    assert np.array_equal(z['rows'], rows) and np.array_equal(z['cols'], cols)
    ncon = int(z['ncon'])
    assert 0 < ncon < len(rows)             # both sections are there
    want = np.array(single.hessian(z['free'], z['lam'], 0.7))
    assert np.array_equal(_bits(z['first'][:ncon]), _bits(want[:ncon]))
    assert np.array_equal(_bits(z['first'][ncon:]), _bits(want[ncon:]))
    assert np.array_equal(_bits(z['again']), _bits(z['first']))
    assert np.array_equal(z['double'], 2.0*want)
    np.testing.assert_array_equal(z['con0'], z['con1'])
