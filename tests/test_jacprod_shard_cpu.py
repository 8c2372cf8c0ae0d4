"""CPU tests of the node-sharded Jacobian products (``J v`` and ``J^T w`` over
the ranks of a node-sharded problem): the header, the bindings and the library
agree; the emitted kernels carry the window; the ownership rule tiles the time
nodes; a NumPy model of the windowed sums reproduces both products; and two
gloo ranks serve them through ``ShardedCallbacks``.  No GPU is needed."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

import jacprod_shard_cases as cases
from jacprod_block_cases import collocator
from test_jacprod_cpu import U, draw, reference_matrix

from examples import problems
from opty_amd import hip_backend as hb
from opty_amd.sharded import partition_nodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64,
          'int': ctypes.c_int}
DECLARED = {
    'opty_hip_jacprod_jvp_shard': (
        'int', ['*', '*', '*', '*', 'int64_t', 'int64_t', 'int64_t']),
    'opty_hip_jacprod_jvp_instance': ('int', ['*', '*', '*', '*']),
    'opty_hip_jacprod_vjp_shard': (
        'int', ['*', '*', '*', '*', 'int64_t', '*', 'int64_t', 'int64_t'])}


def _declaration(name):
    """``(result type, [argument types])`` of ``name`` in the header, a
    pointer of any kind as ``'*'``."""
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        header = f.read()
    m = re.search(r'^(\w+)\s+%s\(([^)]*)\);' % name, header, re.M)
    assert m, name
    args = []
    for arg in m.group(2).split(','):
        arg = re.sub(r'/\*.*?\*/', ' ', arg, flags=re.S)
        words = arg.replace('const', ' ').split()
        args.append('*' if '*' in arg else words[0])
    return m.group(1), args


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
    for method in ('jvp_shard', 'jvp_instance', 'vjp_shard'):
        assert hasattr(hb.HipJacobianProduct, method)
    # additive: the version is the one the existing clients were built for
    assert hb.ABI_VERSION == 12
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        assert re.search(r'#define OPTY_HIP_ABI_VERSION 12\b', f.read())


def test_emitted_source_has_the_four_kernels_and_the_window():
    from opty_amd.codegen import emit_jacprod as ej
    for name in ('config3_10link_small', 'vardur_pendulum_small'):
        prog = collocator(name)._build_jacprod_program()
        source, _ = ej.emit_jacprod_module(prog)
        kernels = re.findall(r'__launch_bounds__\(64\)\s+(\w+)\(', source)
        assert kernels == ['opty_jvp', 'opty_jvp_inst', 'opty_vjp',
                           'opty_vjp_fin'], (name, kernels)
        assert source.count('__global__') == 4
        # every kernel takes the window, the stride and the tail pointer
        assert source.count('long long wa, long long wb, long long ostride, '
                            'double *__restrict__ tail)') == 4
        assert 'atomic' not in source.lower() and 'asm' not in source
        # entries are addressed from the window's origin
        assert '*ostride + (i - wa)]' in source
    # the block kernels keep their argument list
    assert ej.JACPROD_BLOCK_PARAMS.endswith(
        'double h, long long N, long long ldv, long long ldo, int ncols')
    assert 'wa' not in ej.JACPROD_BLOCK_PARAMS.replace('known', '')
    assert ej.JACPROD_PARAMS.startswith(
        ej.JACPROD_BLOCK_PARAMS[:ej.JACPROD_BLOCK_PARAMS.index(', long long '
                                                               'ldv')])


@pytest.mark.parametrize('n', [1, 2, 63, 64, 200])
@pytest.mark.parametrize('world', [1, 2, 3, 7])
def test_owned_time_nodes_tile_the_trajectory(n, world):
    N = n + 1
    seen = np.zeros(N, dtype=int)
    for a, b in partition_nodes(n, world):
        lo, hi = cases.owned(a, b, N)
        seen[lo:hi] += 1
    assert (seen == 1).all(), (n, world, seen)


def _vjp_lanes(wa, wb, N):
    """What ``opty_vjp`` does with the window ``[wa, wb)``, lane by lane, in
    the kernel's own terms: ``(entries written, constraint nodes counted,
    nodes evaluated)`` as lists."""
    from opty_amd.codegen.emit_jacprod import VJP_STRIDE, vjp_window_blocks
    ncn = N - 1
    pend = wb + (1 if wb == ncn else 0)
    written, counted, evaluated = [], [], []
    for blk in range(vjp_window_blocks(wa, wb, N)):
        i0 = wa - (1 if wa > 0 else 0) + blk*VJP_STRIDE
        assert i0 < wb, 'a block with nothing to do was launched'
        for lane in range(64):
            i = i0 + lane
            first = lane > 0 or (blk == 0 and wa == 0)
            valid = i < wb
            if valid:
                evaluated.append(i)
                assert 0 <= i < ncn
            if valid and first:
                counted.append(i)
            if i < pend and first:
                # lo(i) of a valid lane, hi(i - 1) from the lane before
                assert valid or i == ncn
                assert lane == 0 or (i - 1) in evaluated
                written.append(i)
    return written, counted, evaluated


@pytest.mark.parametrize('N', [2, 3, 64, 65, 127, 128, 130, 201])
def test_every_owned_entry_has_one_writer(N):
    """The lane logic of ``opty_vjp`` over windows at every block edge: every
    owned entry is written once, every node of the window counted once, and
    nothing else is written."""
    ncn = N - 1
    edges = sorted({x for x in (0, 1, 2, 62, 63, 64, 65, 125, 126, 127, 128,
                                ncn - 64, ncn - 63, ncn - 1, ncn)
                    if 0 <= x <= ncn})
    windows = [(a, b) for a in edges for b in edges if a < b]
    if N == cases.EDGE_NODES:
        windows += [w for w in cases.WINDOWS if w[0] < w[1]]
    for wa, wb in windows:
        written, counted, _ = _vjp_lanes(wa, wb, N)
        lo, hi = cases.owned(wa, wb, N)
        assert written == list(range(lo, hi)), (wa, wb)
        assert counted == list(range(wa, wb)), (wa, wb)


# -- a NumPy model of the windowed sums ----------------------------------------
class Model(object):
    """The windowed products from the reference matrix ``J`` of a problem (at
    the reference's ``free``): what a rank's kernels compute, as sparse
    products over the window's rows."""

    def __init__(self, name):
        self.col = col = collocator(name)
        self.free, self.J, self.A, _, _ = reference_matrix(name, col)
        prog = col._build_jacprod_program()
        self.N = col.num_collocation_nodes
        self.M, self.rows, self.T = prog.M, prog.n + prog.q, prog.r + prog.s
        self.ncn = self.N - 1

    def window_rows(self, a, b):
        return (np.arange(self.M)[:, None]*self.ncn +
                np.arange(a, b)[None, :]).ravel()

    def jvp(self, free, v, out2d, inst_out, a, b):
        """The rows of the window's nodes."""
        v = np.asarray(v)
        out2d[...] = _like(out2d, (self.J[self.window_rows(a, b)] @ v)
                           .reshape(self.M, b - a))
        if inst_out is not None:
            inst_out[...] = _like(inst_out, self.J[self.M*self.ncn:] @ v)

    def vjp(self, free, w, out2d, tail_part, a, b):
        """``J^T w`` on the owned columns; the tail from the window's rows
        alone."""
        w = np.asarray(w)
        lo, hi = cases.owned(a, b, self.N)
        g = self.J.T @ w
        out2d[...] = _like(out2d, g[:self.rows*self.N].reshape(
            self.rows, self.N)[:, lo:hi])
        rows = self.window_rows(a, b)
        tail_part[...] = _like(tail_part, (self.J[rows].T @ w[rows])[
            self.rows*self.N:])


def _like(dst, values):
    if hasattr(dst, 'numpy'):
        import torch
        return torch.from_numpy(np.ascontiguousarray(values))
    return values


@pytest.mark.parametrize('name', cases.MODELLED)
@pytest.mark.parametrize('world', [1, 2, 3, 7])
def test_windowed_sums_reproduce_the_products(name, world):
    m = Model(name)
    rng = np.random.default_rng(41)
    v, w = draw(rng, m.col.num_free), draw(rng, m.col.num_constraints)
    jv = np.full(m.col.num_constraints, np.nan)
    jtw = np.full(m.col.num_free, np.nan)
    parts = np.full((world, m.T), np.nan)
    ranges = partition_nodes(m.ncn, world)
    for g, (a, b) in enumerate(ranges):
        lo, hi = cases.owned(a, b, m.N)
        m.jvp(m.free, v, jv[:m.M*m.ncn].reshape(m.M, m.ncn)[:, a:b],
              jv[m.M*m.ncn:] if g == world - 1 else None, a, b)
        m.vjp(m.free, w, jtw[:m.rows*m.N].reshape(m.rows, m.N)[:, lo:hi],
              parts[g], a, b)
    from opty_amd.sharded import ShardedCollocator
    jtw[m.rows*m.N:] = ShardedCollocator.sum_tail_parts(parts)
    want_v, want_w = m.J @ v, m.J.T @ w
    # the same sparse rows times the same vector
    np.testing.assert_array_equal(jv, want_v)
    np.testing.assert_array_equal(jtw[:m.rows*m.N], want_w[:m.rows*m.N])
    # a sum of N-1 terms in another order: N-1 units of round-off of the sum
    # of the magnitudes at the most
    bound = m.ncn*U*(m.A.T @ np.abs(w))[m.rows*m.N:]
    assert np.all(np.abs(jtw[m.rows*m.N:] - want_w[m.rows*m.N:]) <= bound)


# -- two gloo ranks ------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, name, out):
    import torch.distributed as dist
    from test_sharded_gloo import _OracleShard
    from opty_amd.sharded import ShardedCallbacks, ShardedCollocator
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        kw = problems.build(name)
        model = Model(name)
        a, b = partition_nodes(model.ncn, world)[rank]
        ev = _OracleShard(dict(kw), a, b)
        ev.o.known_parameter_map = dict(ev.o.known_parameter_map)
        sh = ShardedCollocator(evaluator=ev, instance_evaluator=ev.instance,
                               block_shape=(ev.o.M, ev.o.M*ev.o.C),
                               product_evaluator=(model.jvp, model.vjp), **kw)
        ev.sh = sh
        assert sh.jv_local is None and sh.tail_part is None
        cb = ShardedCallbacks(sh, name='opty_t_jp_%d' % port)
        assert cb.jv_host is None and cb.jtw_host is None
        if rank != 0:
            cb.serve()
            return
        rng = np.random.default_rng(43)
        v = draw(rng, sh.collocator.num_free)
        w = draw(rng, sh.num_constraints)
        c0 = cb.constraints(model.free)
        jv = cb.jvp(model.free, v)
        jtw = cb.vjp(model.free, w)
        jv2, jtw2 = cb.jvp(model.free, 2.0*v), cb.vjp(model.free, 2.0*w)
        # a direction per call, back to back: no rank may read the previous
        # one (a power of two scales the product exactly)
        split = model.rows*model.N
        for k in range(1, 25):
            assert np.array_equal(cb.jvp(model.free, 2.0**k*v), 2.0**k*jv), k
            assert np.array_equal(cb.vjp(model.free, 2.0**-k*w)[:split],
                                  2.0**-k*jtw[:split]), k
        with pytest.raises(ValueError):
            cb.jvp(model.free, w[:-1])
        with pytest.raises(ValueError):
            cb.vjp(model.free, np.r_[w, 1.0])
        c1 = cb.constraints(model.free)
        j1 = np.array(cb.jacobian(model.free))
        np.savez(out, v=v, w=w, jv=jv, jtw=jtw, jv2=jv2, jtw2=jtw2, c0=c0,
                 c1=c1, j1=j1)
        cb.shutdown()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('name', ['pend2_link_vardur_unkmass_small',
                                  'config2_pendulum_small'])
def test_two_ranks_serve_the_products(tmp_path, name):
    """``ShardedCallbacks.jvp`` / ``vjp`` on the root with the model injected
    as ``product_evaluator``: the reference products; ``constraints`` and
    ``jacobian`` work before and after."""
    import torch.multiprocessing as mp
    from oracle.collocation_oracle import OracleCollocator
    out = str(tmp_path/'root.npz')
    mp.spawn(_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
    z = np.load(out)
    m = Model(name)
    split = m.rows*m.N
    want_v, want_w = m.J @ z['v'], m.J.T @ z['w']
    np.testing.assert_array_equal(z['jv'], want_v)
    np.testing.assert_array_equal(z['jtw'][:split], want_w[:split])
    bound = m.ncn*U*(m.A.T @ np.abs(z['w']))[split:]
    assert np.all(np.abs(z['jtw'][split:] - want_w[split:]) <= bound)
    np.testing.assert_array_equal(z['jv2'], 2.0*want_v)
    np.testing.assert_array_equal(z['jtw2'][:split], 2.0*want_w[:split])
    full = OracleCollocator(name='shard', **problems.build(name))
    con = full.generate_constraint_function()(m.free)
    jac = np.asarray(full.generate_jacobian_function()(m.free))
    for got in (z['c0'], z['c1']):
        np.testing.assert_allclose(got, con, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(z['j1'], jac, rtol=1e-13, atol=1e-13)
