"""GPU tests of the node-sharded Hessian operator (C ABI
``opty_hip_hessmv_apply_shard``: ``opty_hessmv`` / ``opty_hessmv_fin`` over a
window of the constraint nodes; ``ShardedProblem.resident_hessian_operator``).
The contract:

1. for every partition of the nodes the windows' trajectory entries of ``y``,
   instance terms included, have the BITS of ``opty_hip_hessmv_apply`` on the
   same handle and the values ``opty_hip_eval_hess`` gives;
2. the tail shares have the same bits from call to call, the whole product's
   bits for the one-window partition, and for every other partition their sum
   in window order meets ``hessmv_cases.check`` (``4 (k_r + 2) 2**-53 (|H|
   |v|)_r``, which holds for any order of the same sum);
3. nothing outside a window's slice is written (outputs start as NaN, between
   guard bands)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import hessian_cases as hc
import hessian_shard_cases as hs
import hessian_synth_cases as sc
import hessmv_cases as mc
import hessmv_shard_cases as cases

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GUARD = 8               # doubles of NaN on either side of a vector
_CACHE = {}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


class _Case(object):
    """A problem handle, a product handle of the constraint section, the
    whole-problem values on the device (``opty_hip_eval_hess``, or random
    ones for a synthetic descriptor), a direction and the whole product of
    the same handle.  ``hessian``: the Hessian handle that evaluates windows
    of values (None: windows are views of the whole values)."""

    def __init__(self, col, product, hessian, values, rows, cols, seed):
        import torch
        from opty_amd import hip_backend as hb
        self.col, self.product, self.hessian = col, product, hessian
        self.N = col.num_collocation_nodes
        self.ncn = self.N - 1
        self.rows, self.cols = rows, cols
        self.num_free = col.num_free
        prog = col._build_hessian_program()
        self.nrows, self.ntail = prog.n + prog.q, prog.r + prog.s
        self.split = self.nrows*self.N
        assert self.num_free == self.split + self.ntail
        self.nnz = product.nnz
        assert len(rows) == self.nnz
        self.PH = (self.nnz - product._counts['nnz_inst'])//self.ncn
        self.nnz_inst = self.nnz - self.PH*self.ncn
        col.hip.use_torch_stream()
        self.dev = torch.device('cuda', col._device)
        rng = np.random.default_rng(seed)
        self.v = rng.uniform(-1.0, 1.0, self.num_free)
        self.dv = torch.from_numpy(self.v).to(self.dev)
        if hessian is not None:
            self.free, self.lam = hc.inputs(seed, col)
            self.dfree, self.dlam = (torch.from_numpy(x).to(self.dev)
                                     for x in (self.free, self.lam))
            col.sync_known()
            self.dvalues = self.nan(self.nnz)
            hessian.evaluate(self.dfree, self.dlam, self.dvalues, hb.DEVICE)
        else:
            self.dvalues = torch.from_numpy(values).to(self.dev)
        whole = self.nan(self.num_free)
        product.apply(self.dvalues, self.dv, whole, hb.DEVICE)
        torch.cuda.synchronize()
        self.values = self.dvalues.cpu().numpy()
        self.whole = whole.cpu().numpy()
        assert np.isfinite(self.values).all()
        mc.check('whole product', self.whole, self.num_free, rows, cols,
                 self.values, self.v)

    def nan(self, count):
        import torch
        return torch.full((count,), np.nan, dtype=torch.float64,
                          device=self.dev)

    def shard(self, a, b):
        """The values of the nodes ``[a - (a > 0), b)``: evaluated for the
        window by ``opty_hip_eval_hess_shard`` into a buffer of their own, or
        (synthetic values) a view of the whole vector."""
        first = a - (1 if a > 0 else 0)
        if self.hessian is None:
            return self.dvalues[first*self.PH:]
        buf = self.nan(max(1, b - first)*self.PH)
        self.hessian.eval_shard(self.dfree, self.dlam, buf, first, b)
        return buf

    def window(self, y, tail_part, a, b, owner):
        """One window IN PLACE into the global vector ``y`` (row stride
        ``N``), its tail share into ``tail_part``."""
        inst = self.dvalues[self.ncn*self.PH:] if self.nnz_inst else None
        self.product.apply_shard(self.shard(a, b), inst, self.dv, y[a:],
                                 self.N, tail_part, a, b, owner)

    def partition(self, ranges, owner):
        """``(y, parts)``: every window of ``ranges`` written in place into a
        NaN-filled global vector between guard bands, the tail shares into
        the rows of a NaN-filled ``(windows, r + s)`` array between guard
        bands; the tail of ``y`` is nobody's."""
        import torch
        T = self.ntail
        buf = self.nan(GUARD + self.num_free + GUARD)
        tails = self.nan(GUARD + len(ranges)*T + GUARD)
        for g, (a, b) in enumerate(ranges):
            part = tails[GUARD + g*T:GUARD + (g + 1)*T] if T else None
            self.window(buf[GUARD:], part, a, b, g == owner)
        torch.cuda.synchronize()
        buf, tails = buf.cpu().numpy(), tails.cpu().numpy()
        for band in (buf[:GUARD], buf[-GUARD:], tails[:GUARD],
                     tails[-GUARD:]):
            assert np.isnan(band).all()
        return (buf[GUARD:-GUARD],
                tails[GUARD:len(tails) - GUARD].reshape(len(ranges), T))

    def check_partition(self, ranges, what, owner=None):
        """Contract points 1 to 3 for a partition of all the nodes."""
        owner = len(ranges) - 1 if owner is None else owner
        y, parts = self.partition(ranges, owner)
        # 1: the trajectory entries, bit for bit; 3: the tail is nobody's
        assert np.array_equal(_bits(y[:self.split]),
                              _bits(self.whole[:self.split])), what
        assert np.isnan(y[self.split:]).all(), what
        # 2: the same bits again ...
        y2, parts2 = self.partition(ranges, owner)
        assert np.array_equal(_bits(y2), _bits(y)), what
        assert np.array_equal(_bits(parts2), _bits(parts)), what
        # ... the sum of the shares in window order within the tolerance ...
        total = np.zeros(self.ntail)
        for part in parts:
            total = total + part
        got = np.concatenate((y[:self.split], total))
        mc.check(what, got, self.num_free, self.rows, self.cols, self.values,
                 self.v)
        # ... and one window has the whole product's bits
        if len(ranges) == 1:
            assert np.array_equal(_bits(total),
                                  _bits(self.whole[self.split:])), what
        return parts


def _case(label):
    if label not in _CACHE:
        col = hs.collocator(label)
        rows, cols = col.hessian_indices()
        _CACHE[label] = _Case(col, col._ensure_hessmv(),
                              col.generate_hessian_function().handle, None,
                              rows, cols, 41)
        assert _CACHE[label].ncn == cases.NCN
    return _CACHE[label]


@pytest.mark.parametrize('label', cases.PROBLEMS)
@pytest.mark.parametrize('window', cases.WINDOWS,
                         ids=['%d-%d' % w for w in cases.WINDOWS])
def test_window_edges_in_place(label, window):
    """One window through the C ABI in place into NaN-filled global vectors
    with guard bands: the whole product's bits at the owned entries, NaN
    everywhere else, the same bits from a second call."""
    c = _case(label)
    a, b = window
    lo, hi = cases.owned(c.N, a, b)
    mine = np.zeros((c.nrows, c.N), dtype=bool)
    mine[:, lo:hi] = True
    mine = np.concatenate((mine.ravel(), np.zeros(c.ntail, dtype=bool)))
    if label == 'C':
        assert c.nnz_inst > 0
    for owner in (0, -1):
        y, parts = c.partition([window], owner)
        assert np.array_equal(~np.isnan(y), mine)
        assert np.array_equal(_bits(y[mine]), _bits(c.whole[mine]))
        assert np.isfinite(parts).all()
        y2, parts2 = c.partition([window], owner)
        assert np.array_equal(_bits(y2[mine]), _bits(y[mine]))
        assert np.array_equal(_bits(parts2), _bits(parts))
        if window == (0, c.ncn) and owner == 0:
            assert np.array_equal(_bits(parts[0]),
                                  _bits(c.whole[c.split:]))
        if a == b and owner != 0:
            # an empty window's share of the sums is zero, all bits clear
            assert np.array_equal(_bits(parts), np.zeros_like(_bits(parts)))


@pytest.mark.parametrize('label', cases.PROBLEMS)
@pytest.mark.parametrize('world', cases.WORLDS)
def test_partitions_in_place(label, world):
    from opty_amd.sharded import partition_nodes
    c = _case(label)
    c.check_partition(partition_nodes(c.ncn, world),
                      '%s over %d ranks' % (label, world))


@pytest.mark.parametrize('label', ['A', 'C'])
def test_an_empty_window_may_own_the_tail(label):
    """The empty window zero-fills its share and, as the tail's owner, runs
    the finishing kernel alone (C: an instance entry)."""
    c = _case(label)
    ranges = [(0, 5), (5, 5), (5, c.ncn)]
    for owner in (1, 2):
        c.check_partition(ranges, '%s, window %d owns the tail'
                          % (label, owner), owner)


def test_three_way_partition_of_two_strips():
    from opty_amd.sharded import partition_nodes
    col = hs.collocator(cases.TWO_STRIPS)
    rows, cols = col.hessian_indices()
    c = _Case(col, col._ensure_hessmv(),
              col.generate_hessian_function().handle, None, rows, cols, 42)
    assert col._hessian_meta['strips'] == 2
    c.check_partition(partition_nodes(c.ncn, 3), 'D over 3 ranks')
    col.hip.set_stream(None)


def test_synthetic_pattern_the_owner_adds_the_tail_contributions():
    """Explicit triplets in interior trajectory rows and in tail rows, split
    three ways: every trajectory side goes to the window that owns the entry,
    the tail sides to the window that ``tail_owner`` names and to no other."""
    from opty_amd import hip_backend as hb
    from opty_amd.sharded import partition_nodes
    cname, N, nrows, ntail, desc, rows, cols = cases.synth_case()
    col = sc.carrier(cname, N)
    handle = hb.HipHessianProduct(col.hip, desc)
    tail = nrows*N
    inst_r, inst_c = desc['inst_rows'], desc['inst_cols']
    interior = (inst_r < tail) & (inst_r % N > 0) & (inst_r % N < N - 1)
    assert interior.any() and (inst_r >= tail).any() and ntail > 0
    values = np.random.default_rng(43).uniform(-1.0, 1.0, len(rows))
    c = _Case(col, handle, None, values, rows, cols, 44)
    ranges = partition_nodes(c.ncn, 3)
    # the explicit triplets in trajectory rows fall into more than one window
    assert len(set(np.searchsorted([b for _, b in ranges],
                                   inst_r[inst_r < tail] % N,
                                   side='right'))) > 1
    shares = [c.check_partition(ranges, 'synthetic, window %d owns' % g, g)
              for g in range(3)]
    _, nobody = c.partition(ranges, -1)
    for g in range(3):
        for k in range(3):
            # a window's share depends on whether it is the owner, alone
            if k != g:
                assert np.array_equal(_bits(shares[g][k]), _bits(nobody[k]))
        assert not np.array_equal(shares[g][g], nobody[g])
    handle.release()
    col.hip.set_stream(None)


def test_c_abi_rejections():
    """Every refusal of ``opty_hip_hessmv_apply_shard`` comes with the
    offending number, before anything is enqueued; the handle still works."""
    import torch
    from opty_amd import hip_backend as hb
    lib = hb.load_library()
    c = _case('A')
    h, ncn, N, PH = c.product, c.ncn, c.N, c.PH
    assert c.ntail == 2 and c.nnz_inst == 0
    y = c.nan(c.num_free)
    tail = c.nan(c.ntail)
    vals = c.dvalues

    def refused(match, values=vals, inst=None, v=c.dv, out=y, stride=N,
                part=tail, a=0, b=10, handle=h):
        with pytest.raises(hb.HipBackendError, match=match):
            handle.apply_shard(values, inst, v, out, stride, part, a, b, 1)

    refused('null', values=None)
    refused('null', v=None)
    refused('null', out=None)
    refused(r'null tail_part.* 2 tail', part=None)
    P = hb._ptr
    assert lib.opty_hip_hessmv_apply_shard(
        None, P(vals), None, P(c.dv), P(y), N, P(tail), 0, 10, 1) != 0
    assert b'null' in lib.opty_hip_last_error()
    refused(r'\[-1, 5\)', a=-1, b=5)
    refused(r'\[0, %d\)' % (ncn + 1), b=ncn + 1)
    refused(r'\[7, 6\)', a=7, b=6)
    refused('out_stride 9 < the 10 time nodes', stride=9)
    # the last window also owns time node N - 1
    refused('out_stride 10 < the 11 time nodes', stride=10, a=ncn - 10, b=ncn)
    refused('overlaps v', out=c.dv)
    refused('overlaps v', out=c.dv[c.num_free - 1:], stride=1, b=1)
    refused(r'overlaps the %d values' % (10*PH), out=vals)
    # (the halo node's values count, up to the last one)
    refused(r'overlaps the %d values' % (11*PH), out=vals[15*PH - 1:],
            values=vals[4*PH:], a=5, b=15)
    # instance entries need their values
    ci = _case('C')
    assert ci.nnz_inst > 0
    with pytest.raises(hb.HipBackendError, match='null inst_values.* %d '
                       % ci.nnz_inst):
        ci.product.apply_shard(ci.dvalues, None, ci.dv, ci.nan(ci.num_free),
                               ci.N, ci.nan(max(1, ci.ntail)), 0, 10, 1)
    # a handle with an objective section is not node-sharded
    desc = c.col._hessmv_descriptor()
    with_e = hb.HipHessianProduct(c.col.hip, dict(
        desc, obj_pattern=np.array([(0, 0, 0, 0)], dtype=np.int32)))
    ovals = torch.zeros(with_e.nnz, dtype=torch.float64, device=c.dev)
    refused(r'E 1, T 0', values=ovals, handle=with_e)
    with_e.release()
    at = np.array([c.split], dtype=np.int64)
    with_t = hb.HipHessianProduct(c.col.hip, dict(desc, tail_rows=at,
                                                  tail_cols=at))
    refused(r'E 0, T 1', values=ovals, handle=with_t)
    with_t.release()
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(tail).all()
    # the handle still works
    c.check_partition([(0, ncn)], 'after the rejections')


# -- ShardedProblem.resident_hessian_operator: processes that share the one GPU ---
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(argv, world, env=None, limit=240):
    """Starts the ranks, each under its own time limit, and checks every exit
    status; ``argv(rank)`` is a rank's command line."""
    procs = [subprocess.Popen(
        argv(r), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        env=None if env is None else env(r)) for r in range(world)]
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
    return outs


@pytest.mark.parametrize('backend,world', [('gloo', cases.RANKS),
                                           ('nccl', 1)])
def test_resident_operator_equals_the_single_gpu_operators(tmp_path, backend,
                                                           world):
    """``ShardedProblem.resident_hessian_operator`` on problem A with its
    device-backed objective Hessian, served by all ranks: the trajectory
    entries of ``matvec`` are ``fl(y_con + y_obj)`` of the single-GPU
    constraint operator and the objective-only product, bit for bit; the
    whole vector meets ``hessmv_cases.check`` on the ``[constraint |
    objective]`` triplets of ``Problem.hessian``; the operator is
    symmetric."""
    import opty_amd
    from opty_amd import hip_backend as hb
    out = str(tmp_path/'root.npz')
    port = _free_port()
    worker = os.path.join(REPO, 'tests', 'hessmv_shard_worker.py')
    outs = _run_ranks(lambda r: [sys.executable, worker, backend, str(r),
                                 str(world), str(port), out], world)
    for r, text in enumerate(outs):
        # (a serving rank gets here only when shutdown() released it)
        assert 'rank %d of %d ok' % (r, world) in text
    z = np.load(out)
    assert tuple(z['ab']) == (0, -(-cases.NCN//world))
    kw = hs.process_kwargs()
    obj_hessian = hs.process_obj_hessian(kw)
    single = opty_amd.Problem(lambda f: 0.0, lambda f: 0.0*f,
                              obj_hessian=obj_hessian, **kw)
    col = single.collocator
    n, N = single.num_free, col.num_collocation_nodes
    free, lam, v, u = z['free'], z['lam'], z['v'], z['u']
    rows, cols = single.hessianstructure()
    values = np.array(single.hessian(free, lam, 0.7))
    ncon = len(col.hessian_indices()[0])
    assert 0 < ncon < len(rows)             # both sections are there
    # the objective section alone, on this GPU
    objective = obj_hessian[2].handle
    prog = col._build_hessian_program()
    split = (prog.n + prog.q)*N
    only = hb.HipHessianProduct(col.hip, dict(
        obj_pattern=objective.pattern, obj_base=objective.desc['base'],
        tail_rows=split + objective.tail_pairs[:, 0],
        tail_cols=split + objective.tail_pairs[:, 1]))
    con_op = col.hessian_operator(free, lam)
    tols = {}
    for name, x, got in (('v', v, z['hv']), ('u', u, z['hu'])):
        y_obj = np.empty(n)
        only.apply(np.ascontiguousarray(values[ncon:]), x, y_obj, hb.HOST)
        want = con_op.matvec(x) + y_obj
        assert np.array_equal(_bits(got[:split]), _bits(want[:split])), name
        if world == 1:
            assert np.array_equal(_bits(got[split:]), _bits(want[split:]))
        mc.check('%s x %d, H %s' % (backend, world, name), got, n, rows, cols,
                 values, x)
        tols[name] = mc.reference(n, rows, cols, values, x)[1]
    only.release()
    # symmetric: each entry of H v is within its tolerance of the exact
    # product, so u.(H v) is within sum |u_r| tol_r(v) of u^T H v, the same
    # for v.(H u), and each dot product of n terms rounds within n 2**-53 of
    # the sum of its terms' magnitudes
    uhv, vhu = float(u @ z['hv']), float(v @ z['hu'])
    bound = np.abs(u) @ tols['v'] + np.abs(v) @ tols['u'] + n*2.0**-53*(
        np.abs(u) @ np.abs(z['hv']) + np.abs(v) @ np.abs(z['hu']))
    print('u.(Hv) = %.17g, v.(Hu) = %.17g, bound %.3g' % (uhv, vhu, bound))
    assert abs(uhv - vhu) <= bound
    assert np.array_equal(_bits(z['HV']),
                          _bits(np.stack([z['hv'], z['hu']], axis=1)))
    assert np.array_equal(_bits(z['again']), _bits(z['hv']))
    # twice the multipliers and twice the objective factor: exactly twice
    assert np.array_equal(z['hv2'], 2.0*z['hv'])
    np.testing.assert_array_equal(z['con0'], z['con1'])


# -- example --------------------------------------------------------------------
def test_newton_step_of_the_example(tmp_path):
    """examples/sharded_kkt_minres.py at 20 nodes over two ranks that share
    the GPU: the residual history decreases as that of examples/kkt_minres.py
    does -- MINRES' residuals do not grow, the two runs start from the same
    system, and the first residual, one product away from the right-hand
    side, agrees to the products' rounding."""
    from examples import kkt_minres
    history = str(tmp_path/'history.npy')
    port = _free_port()
    script = os.path.join(REPO, 'examples', 'sharded_kkt_minres.py')
    iterations = 30

    def env(rank):
        return dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank),
                    WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                    MASTER_PORT=str(port), OPTY_HISTORY=history)
    outs = _run_ranks(lambda r: [sys.executable, script,
                                 str(cases.EXAMPLE_NODES), str(iterations)],
                      2, env)
    assert 'minres: info' in outs[0]
    got = np.load(history)
    _, want = kkt_minres.main(cases.EXAMPLE_NODES, maxiter=iterations,
                              verbose=False)
    want = np.array(want)
    print('sharded %s\nsingle  %s' % (got, want))
    assert len(got) >= 2 and len(want) >= 2
    assert got[-1] < got[0] and want[-1] < want[0]
    np.testing.assert_allclose(got[0], want[0], rtol=1e-10)
