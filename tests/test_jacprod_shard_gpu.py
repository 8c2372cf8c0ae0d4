"""GPU tests of the node-sharded Jacobian products (C ABI
``opty_hip_jacprod_jvp_shard`` / ``opty_hip_jacprod_jvp_instance`` /
``opty_hip_jacprod_vjp_shard``, the four product kernels over a window of the
constraint nodes; ``ShardedProblem.jacobian_operator``).  The contract:

1. ``J v``: the union of the windows of any partition has the BITS of the
   whole-problem product of the same handle;
2. ``J^T w``, trajectory entries (instance terms included): the same;
3. ``J^T w``, tail entries: the same bits from call to call, the whole
   product's bits for the one-window partition, otherwise the project's
   criterion ``assert_close(rtol=1e-12, bound=...)`` with the interpreter's
   bounds;
4. nothing outside a window's slice is written (outputs start as NaN)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import jacprod_shard_cases as cases
from golden_util import assert_close
from jacprod_block_cases import collocator

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GUARD = 8               # doubles of NaN on either side of a dense block
_CACHE = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


class _Case(object):
    """A collocator, its product handle, inputs on the device, the
    whole-problem products of the same handle and the interpreter's values
    and bounds."""

    def __init__(self, col, seed):
        import torch
        import dag_interp
        from test_jacprod_cpu import interpreted_products
        from opty_amd.codegen.program import assemble_vjp
        self.col = col
        jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
        self.handle = jvp.handle
        self.free, self.v, self.w = cases.draw_inputs(seed, col)
        prog = self.prog = col._build_jacprod_program()
        self.N = col.num_collocation_nodes
        self.ncn = self.N - 1
        self.M, self.R, self.T = prog.M, prog.n + prog.q, prog.r + prog.s
        self.o = col.num_instance_constraints
        # the whole problem, the same handle (this also installs the known
        # values of this free vector on the device)
        self.jv = np.array(jvp(self.free, self.v))
        self.jtw = np.array(vjp(self.free, self.w))
        self.interp = interpreted_products(col, self.free, self.v, self.w,
                                           with_bounds=True)
        # the adjoint roots per node, for the tail shares of a window
        nodes = np.arange(self.ncn)
        rin = col._jacprod_inputs(self.free, self.w, nodes, 'vjp')
        adj, ab = dag_interp.evaluate_with_error_bound(prog.dag, prog.adj_out,
                                                       rin)
        wide = [np.broadcast_to(np.asarray(x, dtype=float), (self.ncn,))
                for x in adj]
        wide_b = [np.abs(np.broadcast_to(np.asarray(x, dtype=float),
                                         (self.ncn,))) for x in ab]
        none = [0.0]*len(prog.inst_jac_out)
        atoms = col._atom_free_index()

        def tail_share(a, b):
            """``(values, bounds)`` of a window's tail share: the assembly of
            the whole product over the window's nodes alone."""
            inside = (nodes >= a) & (nodes < b)
            val = assemble_vjp(prog, self.N, [np.where(inside, x, 0.0)
                                              for x in wide], none, self.w,
                               atoms)
            bnd = assemble_vjp(prog, self.N, [np.where(inside, x, 0.0)
                                              for x in wide_b], none,
                               np.abs(self.w), atoms)
            return val[self.R*self.N:], bnd[self.R*self.N:]
        self.tail_share = tail_share
        col.hip.use_torch_stream()
        dev = torch.device('cuda', col._device)
        self.dev = dev
        self.dfree, self.dv, self.dw = (torch.from_numpy(x).to(dev)
                                        for x in (self.free, self.v, self.w))

    def nan(self, *shape):
        import torch
        return torch.full(shape, np.nan, dtype=torch.float64, device=self.dev)

    def partition(self, ranges):
        """Every window of ``ranges`` written IN PLACE into NaN-filled global
        vectors, the instance rows by the last: ``(J v, J^T w with its tail
        left as the windows left it, (world, T) tail shares)``."""
        import torch
        jv = self.nan(self.col.num_constraints)
        jtw = self.nan(self.col.num_free)
        parts = self.nan(len(ranges), max(1, self.T))
        for g, (a, b) in enumerate(ranges):
            self.handle.jvp_shard(self.dfree, self.dv, jv[a:], self.ncn, a, b)
            self.handle.vjp_shard(self.dfree, self.dw, jtw[a:], self.N,
                                  parts[g] if self.T else None, a, b)
        self.handle.jvp_instance(self.dfree, self.dv, jv[self.M*self.ncn:])
        torch.cuda.synchronize()
        return (jv.cpu().numpy(), jtw.cpu().numpy(),
                parts.cpu().numpy()[:, :self.T])

    def check_partition(self, ranges, what):
        """Contract points 1 to 3 for the partition ``ranges``."""
        from opty_amd.sharded import ShardedCollocator
        jv, jtw, parts = self.partition(ranges)
        split = self.R*self.N
        assert np.array_equal(_bits(jv), _bits(self.jv)), what
        assert np.array_equal(_bits(jtw[:split]), _bits(self.jtw[:split])), \
            what
        # the windows leave the tail of the vector to whoever adds the shares
        assert np.isnan(jtw[split:]).all(), what
        if self.T:
            tail = ShardedCollocator.sum_tail_parts(parts)
            print('%s: tail %s, whole product %s' % (what, tail,
                                                     self.jtw[split:]))
            if len(ranges) == 1:
                assert np.array_equal(_bits(tail), _bits(self.jtw[split:]))
            _, wjtw, _, bw = self.interp
            assert_close(tail, wjtw[split:], rtol=1e-12, bound=bw[split:],
                         what=what + ' vjp tail')
        # the same bits from call to call
        jv2, jtw2, parts2 = self.partition(ranges)
        assert np.array_equal(_bits(jv2), _bits(jv)), what
        assert np.array_equal(_bits(jtw2[:split]), _bits(jtw[:split])), what
        assert np.array_equal(_bits(parts2), _bits(parts)), what


def _edge(method):
    if method not in _CACHE:
        _CACHE[method] = _Case(cases.edge_collocator(method), 6)
    return _CACHE[method]


@pytest.mark.parametrize('method', cases.EDGE_METHODS)
@pytest.mark.parametrize('window', cases.WINDOWS,
                         ids=['%d-%d' % w for w in cases.WINDOWS])
def test_window_edges_into_dense_blocks(method, window):
    """A window through the C ABI into NaN-filled dense blocks between guard
    bands: the whole product's bits on the slice, NaN everywhere else; the
    tail share against the interpreter's sum over the window's nodes."""
    import torch
    c = _edge(method)
    a, b = window
    cnt = b - a
    lo, hi = cases.owned(a, b, c.N)
    own = hi - lo
    jv = c.nan(GUARD + c.M*cnt + GUARD)
    jtw = c.nan(GUARD + c.R*own + GUARD)
    tail = c.nan(GUARD + c.T + GUARD)
    c.handle.jvp_shard(c.dfree, c.dv, jv[GUARD:], cnt, a, b)
    c.handle.vjp_shard(c.dfree, c.dw, jtw[GUARD:], own, tail[GUARD:], a, b)
    torch.cuda.synchronize()
    jv, jtw, tail = (x.cpu().numpy() for x in (jv, jtw, tail))
    for buf in (jv, jtw, tail):
        assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[-GUARD:]).all()
    want = c.jv[:c.M*c.ncn].reshape(c.M, c.ncn)[:, a:b]
    assert np.array_equal(_bits(jv[GUARD:-GUARD]), _bits(want).ravel())
    want = c.jtw[:c.R*c.N].reshape(c.R, c.N)[:, lo:hi]
    assert np.array_equal(_bits(jtw[GUARD:-GUARD]), _bits(want).ravel())
    share, bound = c.tail_share(a, b)
    got = tail[GUARD:-GUARD]
    print('window [%d, %d) %s: tail share %s, interpreter %s'
          % (a, b, method, got, share))
    if cnt == 0:
        assert np.array_equal(got, np.zeros(c.T))
    assert_close(got, share, rtol=1e-12, bound=bound,
                 what='window [%d, %d) tail share' % window)
    if (a, b) == (0, c.ncn):
        assert np.array_equal(_bits(got), _bits(c.jtw[c.R*c.N:]))


@pytest.mark.parametrize('method', cases.EDGE_METHODS)
@pytest.mark.parametrize('world', cases.WORLDS)
def test_partitions_in_place(method, world):
    import torch
    from opty_amd.sharded import partition_nodes
    c = _edge(method)
    ranges = partition_nodes(c.ncn, world)
    c.check_partition(ranges, '%s over %d ranks' % (method, world))
    # one rank alone: nothing but its slices is written
    g = world//2
    a, b = ranges[g]
    lo, hi = cases.owned(a, b, c.N)
    jv, jtw = c.nan(c.col.num_constraints), c.nan(c.col.num_free)
    part = c.nan(c.T)
    c.handle.jvp_shard(c.dfree, c.dv, jv[a:], c.ncn, a, b)
    c.handle.vjp_shard(c.dfree, c.dw, jtw[a:], c.N, part, a, b)
    torch.cuda.synchronize()
    mine = np.zeros(c.col.num_constraints, dtype=bool)
    mine[:c.M*c.ncn].reshape(c.M, c.ncn)[:, a:b] = True
    assert np.array_equal(~np.isnan(jv.cpu().numpy()), mine)
    mine = np.zeros(c.col.num_free, dtype=bool)
    mine[:c.R*c.N].reshape(c.R, c.N)[:, lo:hi] = True
    assert np.array_equal(~np.isnan(jtw.cpu().numpy()), mine)
    assert np.isfinite(part.cpu().numpy()).all()


@pytest.mark.parametrize('name', cases.COVERAGE)
def test_three_way_partition_per_problem(name):
    from opty_amd.sharded import partition_nodes
    c = _Case(collocator(name), 7)
    if name in ('config2_pendulum_small', 'nonlinear_instance'):
        # instance atoms at both ends of the trajectory: other ranks' entries
        atoms = np.array(c.col._atom_free_index()) % c.N
        assert atoms.min() == 0 and atoms.max() == c.N - 1
    if name == 'pend2_link_vardur_unkmass_small':
        assert c.T >= 2
    c.check_partition(partition_nodes(c.ncn, 3), name)
    c.col.hip.set_stream(None)


def test_c_abi_rejections():
    """Bad windows and null pointers return an error with a message, before
    anything is enqueued; nothing aborts and the handle still works."""
    from opty_amd import hip_backend as hb
    c = _edge('backward euler')
    h, ncn, N = c.handle, c.ncn, c.N
    jv, jtw, tail = c.nan(c.M*ncn), c.nan(c.R*N), c.nan(c.T)
    assert c.T > 0
    for a, b in ((-1, 5), (0, ncn + 1), (7, 6)):
        with pytest.raises(hb.HipBackendError, match='window'):
            h.jvp_shard(c.dfree, c.dv, jv, ncn, a, b)
        with pytest.raises(hb.HipBackendError, match='window'):
            h.vjp_shard(c.dfree, c.dw, jtw, N, tail, a, b)
    with pytest.raises(hb.HipBackendError, match='out_stride'):
        h.jvp_shard(c.dfree, c.dv, jv, 9, 0, 10)
    with pytest.raises(hb.HipBackendError, match='out_stride'):
        h.vjp_shard(c.dfree, c.dw, jtw, 10, tail, ncn - 10, ncn)
    for args in ((None, c.dv, jv), (c.dfree, None, jv), (c.dfree, c.dv, None)):
        with pytest.raises(hb.HipBackendError, match='null'):
            h.jvp_shard(*args, ncn, 0, 10)
    for args in ((None, c.dw, jtw), (c.dfree, None, jtw),
                 (c.dfree, c.dw, None)):
        with pytest.raises(hb.HipBackendError, match='null'):
            h.vjp_shard(*args, N, tail, 0, 10)
    with pytest.raises(hb.HipBackendError, match='tail_part'):
        h.vjp_shard(c.dfree, c.dw, jtw, N, None, 0, 10)
    with pytest.raises(hb.HipBackendError, match='null'):
        h.jvp_instance(c.dfree, c.dv, None)
    lib = hb.load_library()
    assert lib.opty_hip_jacprod_jvp_shard(None, hb._ptr(c.dfree),
                                          hb._ptr(c.dv), hb._ptr(jv), ncn, 0,
                                          10) != 0
    assert b'null' in lib.opty_hip_last_error()
    import torch
    torch.cuda.synchronize()
    for buf in (jv, jtw, tail):
        assert torch.isnan(buf).all()           # nothing was enqueued
    # without tail columns a null tail_part is fine
    plain = _Case(collocator('config3_10link_small'), 8)
    assert plain.T == 0
    out = plain.nan(plain.R*plain.N)
    plain.handle.vjp_shard(plain.dfree, plain.dw, out, plain.N, None, 0,
                           plain.ncn)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(plain.jtw))
    plain.col.hip.set_stream(None)
    # the handle still works
    c.check_partition([(0, ncn)], 'after the rejections')


def test_known_parameter_change_between_windowed_calls_is_seen():
    import torch
    from opty_amd.sharded import partition_nodes
    from examples import problems
    kw = problems.build('config3_10link_small')
    c = _Case(collocator('config3_10link_small'), 5)
    ranges = partition_nodes(c.ncn, 3)
    first = c.partition(ranges)
    col = c.col
    vals = np.array([float(col.known_parameter_map[p])
                     for p in col.known_parameters])
    at = [str(p) for p in col.known_parameters].index('g')
    vals[at] = 3.5
    col.hip.set_known_parameters(vals)
    second = c.partition(ranges)
    torch.cuda.synchronize()
    import opty_amd
    kw2 = dict(kw, known_parameter_map=dict(kw['known_parameter_map']))
    g = [p for p in kw2['known_parameter_map'] if str(p) == 'g'][0]
    kw2['known_parameter_map'][g] = 3.5
    fresh = opty_amd.ConstraintCollocator(**kw2)
    want = (np.array(fresh.generate_jvp_function()(c.free, c.v)),
            np.array(fresh.generate_vjp_function()(c.free, c.w)))
    for a, b, d in zip(first[:2], second[:2], want):
        assert not np.array_equal(a, b)
        np.testing.assert_allclose(b, d, rtol=1e-13, atol=1e-300)
    col.hip.set_stream(None)


# -- ShardedProblem.jacobian_operator: processes that share the one GPU --------
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
    worker = os.path.join(REPO, 'tests', 'jacprod_shard_worker.py')
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
def test_sharded_operator_equals_the_single_process_operator(tmp_path,
                                                             backend, world):
    """``ShardedProblem.jacobian_operator(free)``: ``matvec``, ``rmatvec``
    and two-column ``matmat`` / ``rmatmat`` on the root, served by all ranks,
    against the operator of a single-process collocator: bit for bit on every
    entry but the tail of ``J^T w``, which is held to the interpreter's
    bounds (and, with one rank, has the single product's bits too)."""
    out = str(tmp_path/'root.npz')
    _run_ranks(backend, world, out)
    z = np.load(out)
    c = _edge('backward euler')
    assert tuple(z['ab']) == (0, -(-c.ncn//world))
    np.testing.assert_array_equal(z['free'], c.free)
    op = c.col.jacobian_operator(z['free'])
    split = c.R*c.N
    from test_jacprod_cpu import interpreted_products
    for v, w, jv, jtw in ((z['v'], z['w'], z['jv'], z['jtw']),
                          (z['v'], z['w'], z['JV'][:, 0], z['JTW'][:, 0]),
                          (z['v2'], z['w2'], z['JV'][:, 1], z['JTW'][:, 1]),
                          (z['v'], z['w'], z['jv_again'], z['jtw_again'])):
        want_v, want_w = op.matvec(v), op.rmatvec(w)
        assert np.array_equal(_bits(jv), _bits(want_v))
        assert np.array_equal(_bits(jtw[:split]), _bits(want_w[:split]))
        _, wjtw, _, bw = interpreted_products(c.col, z['free'], v, w,
                                              with_bounds=True)
        print('%s x %d: tail %s, single process %s'
              % (backend, world, jtw[split:], want_w[split:]))
        assert_close(jtw[split:], wjtw[split:], rtol=1e-12, bound=bw[split:],
                     what='sharded operator vjp tail')
        if world == 1:
            assert np.array_equal(_bits(jtw[split:]), _bits(want_w[split:]))
    assert np.array_equal(_bits(z['jtw_again']), _bits(z['jtw']))
    np.testing.assert_array_equal(z['con0'], z['con1'])
    want = c.col.generate_constraint_function()(z['free'])
    np.testing.assert_allclose(z['con0'], want, rtol=1e-12, atol=1e-12)
