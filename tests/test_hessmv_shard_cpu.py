"""CPU tests of the node-sharded Hessian operator (``H v`` from shards that
stay in device memory): the header, the bindings and the library agree; the
host statement of one window (``codegen/program.py``:
``assemble_hessmv_window`` / ``hessmv_window_blocks``) tiles the whole product;
a lane-by-lane model of ``opty_hessmv`` over a window stores every owned entry
once; two gloo ranks serve ``ShardedCallbacks.hessian_load`` / ``hmv`` and
``ShardedProblem.resident_hessian_operator`` with the interpreter and the host
statement injected.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import hessian_cases as hc
import hessmv_cases as mc
import hessmv_shard_cases as cases
from test_hessian_shard_cpu import SMALL, _Interpreter, _free_port, _unused
from test_jacprod_shard_cpu import CTYPES, _declaration

from opty_amd import hip_backend as hb
from opty_amd.codegen.program import (assemble_hessmv,
                                      assemble_hessmv_window,
                                      hessmv_window_blocks,
                                      hessmv_window_owned)
from opty_amd.sharded import partition_nodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    'opty_hip_hessmv_apply_shard': (
        'int', ['*', '*', '*', '*', '*', 'int64_t', '*', 'int64_t', 'int64_t',
                'int32_t'])}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


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
    assert hasattr(hb.HipHessianProduct, 'apply_shard')
    # additive: the version is the one the existing clients were built for
    assert hb.ABI_VERSION == 12
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        header = f.read()
    assert re.search(r'#define OPTY_HIP_ABI_VERSION 12\b', header)
    comment = header[:header.index('#define OPTY_HIP_ABI_VERSION')]
    for name in DECLARED:
        assert name in comment, name


# -- the host statement ----------------------------------------------------------
def _tables(label):
    """``(N, nrows, ntail, pattern, rows, cols, at)`` of a problem at 200
    constraint nodes, or of the synthetic descriptor on its carrier; ``at``:
    where the instance entries begin."""
    if label == 'synth':
        _, N, nrows, ntail, desc, rows, cols = cases.synth_case()
        pattern = desc['pattern']
    else:
        N, nrows, ntail, pattern, rows, cols = mc.node_tables(label,
                                                              cases.NCN)
    return N, nrows, ntail, pattern, rows, cols, (N - 1)*len(pattern)


def _windows_of(tables, values, v, ranges, owner):
    N, nrows, ntail, pattern, rows, cols, at = tables
    PH = len(pattern)
    return [assemble_hessmv_window(
        N, nrows, ntail, cases.window_values(values[:at], PH, a, b),
        values[at:], v, pattern, a, b, g == owner, inst_rows=rows[at:],
        inst_cols=cols[at:]) for g, (a, b) in enumerate(ranges)]


@pytest.mark.parametrize('label', cases.PROBLEMS + ('synth',))
@pytest.mark.parametrize('world', cases.WORLDS)
def test_windows_of_a_partition_tile_the_whole_product(label, world):
    """The union of ``assemble_hessmv_window`` over a partition against
    ``assemble_hessmv`` of the whole: trajectory entries bit for bit (the
    instance triplets' terms included), the tail -- the same sum cut
    differently -- within ``hessmv_cases.check``."""
    tables = _tables(label)
    N, nrows, ntail, pattern, rows, cols, at = tables
    if label in ('C', 'synth'):
        assert len(rows) > at       # instance entries
    num_free = nrows*N + ntail
    rng = np.random.default_rng(31)
    values = rng.uniform(-1.0, 1.0, len(rows))
    v = rng.uniform(-1.0, 1.0, num_free)
    whole = assemble_hessmv(N, nrows, ntail, values, v, pattern,
                            inst_rows=rows[at:], inst_cols=cols[at:])
    ranges = partition_nodes(N - 1, world)
    # (the owner need not be the last window)
    for owner in (world - 1, 0):
        y = cases.put_together(
            N, nrows, ntail, ranges,
            _windows_of(tables, values, v, ranges, owner))
        split = nrows*N
        assert np.array_equal(_bits(y[:split]), _bits(whole[:split]))
        mc.check('%s over %d windows' % (label, world), y, num_free, rows,
                 cols, values, v)
    # without an owner the instance triplets' tail sides are nobody's
    if label == 'synth':
        none = cases.put_together(
            N, nrows, ntail, ranges,
            _windows_of(tables, values, v, ranges, -1))
        assert np.array_equal(_bits(none[:split]), _bits(whole[:split]))
        assert not np.array_equal(none[split:], y[split:])


def test_an_empty_window_owns_nothing():
    tables = _tables('C')
    N, nrows, ntail, pattern, rows, cols, at = tables
    rng = np.random.default_rng(32)
    values = rng.uniform(-1.0, 1.0, len(rows))
    v = rng.uniform(-1.0, 1.0, nrows*N + ntail)
    for a in (5, N - 1):
        (block, part), = _windows_of(tables, values, v, [(a, a)], -1)
        assert block.shape == (nrows, 0) and np.all(part == 0.0)
        assert hessmv_window_blocks(N, a, a) == 0
        assert hessmv_window_owned(N, a, a) == (a, a)


# -- the launch, lane by lane ----------------------------------------------------
def _lanes(N, wa, wb):
    """What ``opty_hessmv`` does with the window ``[wa, wb)``, lane by lane in
    the kernel's own terms: ``(stores, tail nodes, value rows)`` -- the time
    nodes stored with the column of ``y`` they go to, the nodes counted in the
    tail partials, and the rows of the shard's values that are loaded."""
    stores, tails, loads = [], [], []
    pend = wb + (1 if wb == N - 1 else 0)
    lo = wa - (1 if wa > 0 else 0)
    for B in range(hessmv_window_blocks(N, wa, wb)):
        i0 = lo + 63*B
        assert i0 < wb, 'a block with nothing to do was launched'
        nv = min(64, wb - i0)
        loads += list(range(i0 - lo, i0 - lo + nv))
        for lane in range(64):
            i = i0 + lane
            first = lane > 0 or (B == 0 and wa == 0)
            if i < wb:
                assert 0 <= i < N - 1       # v[row*N + i + slot] exists
                if first:
                    tails.append(i)
            if first and i < pend:
                # S_R1 of the lane before is a node of the window or the halo
                assert lane == 0 or lo <= i - 1 < wb
                stores.append((i, i - wa))
    return stores, tails, loads


@pytest.mark.parametrize('window', [w for w in cases.WINDOWS if w[0] < w[1]],
                         ids=lambda w: '%d-%d' % w)
def test_every_owned_entry_of_a_window_is_stored_once(window):
    a, b = window
    N = cases.NCN + 1
    stores, tails, loads = _lanes(N, a, b)
    lo, hi = cases.owned(N, a, b)
    assert (lo, hi) == hessmv_window_owned(N, a, b)
    assert sorted(p for p, _ in stores) == list(range(lo, hi))
    assert all(0 <= at == p - a < hi - lo for p, at in stores)
    assert sorted(tails) == list(range(a, b))
    # the shard holds the halo node and the window's nodes, nothing else
    assert set(loads) == set(range(b - a + (1 if a > 0 else 0)))


@pytest.mark.parametrize('world', cases.WORLDS)
def test_partitions_tile_the_vector_and_the_tail_sums(world):
    N = cases.NCN + 1
    seen, counted, blocks = np.zeros(N, dtype=int), np.zeros(N - 1, int), 0
    for a, b in partition_nodes(N - 1, world):
        stores, tails, _ = _lanes(N, a, b)
        for p, _ in stores:
            seen[p] += 1
        for i in tails:
            counted[i] += 1
        blocks = max(blocks, hessmv_window_blocks(N, a, b))
    assert (seen == 1).all() and (counted == 1).all()
    # the partials of a window fit the handle's buffer
    assert blocks <= hessmv_window_blocks(N, 0, N - 1)


def test_the_whole_problem_is_one_window():
    for ncn in (1, 2, 62, 63, 64, 65, 126, 127, 200):
        assert hessmv_window_blocks(ncn + 1, 0, ncn) == -(-ncn//63)


# -- two gloo ranks --------------------------------------------------------------
class _HostProduct(object):
    """``hessian_product_evaluator``: the host statement of one window."""

    col = None
    calls = 0

    def __call__(self, values, inst, v, out2d, tail_part, a, b, tail_owner):
        import torch
        self.calls += 1
        col = self.col
        prog = col._build_hessian_program()
        rows, cols = col.hessian_indices_closed_form()
        N = col.num_collocation_nodes
        at = (N - 1)*prog.PH
        block, part = assemble_hessmv_window(
            N, prog.n + prog.q, prog.r + prog.s, values.numpy(),
            inst.numpy(), v.numpy(), prog.index_pattern(), a, b, tail_owner,
            inst_rows=rows[at:], inst_cols=cols[at:])
        out2d.copy_(torch.from_numpy(block))
        tail_part.copy_(torch.from_numpy(part))


def _callbacks_worker(rank, world, port, label, out):
    import torch.distributed as dist
    from opty_amd.sharded import ShardedCallbacks, ShardedCollocator
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        ev, pr = _Interpreter(), _HostProduct()
        sh = ShardedCollocator(
            evaluator=_unused, instance_evaluator=_unused,
            hessian_evaluator=ev, hessian_product_evaluator=pr,
            **hc.KERNEL_PROBLEMS[label](SMALL + 1))
        ev.col = pr.col = sh.collocator
        # a collocator that is never asked holds nothing new
        assert sh.hmv_values is None and sh.hmv_local is None
        assert sh._hmv_handle is None and sh.hessian_generation == 0
        assert getattr(sh.collocator, '_hessian_program', None) is None
        cb = ShardedCallbacks(sh, name='opty_t_hm_%d' % port)
        assert cb.hy_host is None and cb.hv_host is None
        if rank != 0:
            cb.serve()
            assert (ev.calls, pr.calls) == (2, 4)
            # the values of the halo node are resident, and nothing of the
            # size of the whole Hessian
            assert sh.halo_begin == sh.a - 1
            assert sh.hmv_values.numel() == (sh.b - sh.a + 1)*sh.PH
            assert sh.hess_local is None and cb.hess_host is None
            return
        free, lam = hc.inputs(21, sh.collocator)
        v = np.random.default_rng(22).uniform(-1.0, 1.0, sh._num_free())
        with pytest.raises(RuntimeError, match='hessian_load'):
            cb.hmv(v)
        one = cb.hessian_load(free, lam)
        assert one == 1
        first = cb.hmv(v, one)
        again = cb.hmv(v)
        assert first is not again           # fresh arrays
        # one set is resident: the second load replaces the first
        two = cb.hessian_load(free, 2.0*lam)
        assert two == 2
        with pytest.raises(RuntimeError, match='replaced'):
            cb.hmv(v, one)
        second = cb.hmv(v, two)
        third = cb.hmv(2.0*v, two)
        with pytest.raises(ValueError):
            cb.hmv(v[:-1])
        with pytest.raises(ValueError):
            cb.hessian_load(free, lam[:-1])
        np.savez(out, free=free, lam=lam, v=v, first=first, again=again,
                 second=second, third=third, ab=np.array([sh.a, sh.b]))
        cb.shutdown()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('label', ['C', 'A'])
def test_two_ranks_serve_the_operator(tmp_path, label):
    """``ShardedCallbacks.hessian_load`` / ``hmv`` on the root with the
    interpreter and the host statement injected, against
    ``hessmv_cases.reference`` on the interpreter's whole-problem values,
    with (C) and without (A) instance entries."""
    import torch.multiprocessing as mp
    out = str(tmp_path/'root.npz')
    mp.spawn(_callbacks_worker, args=(2, _free_port(), label, out), nprocs=2,
             join=True)
    z = np.load(out)
    col = hc.collocator(label, SMALL)
    block, inst, _ = hc.interpreted(col, z['free'], z['lam'])
    assert (len(inst) > 0) == (label == 'C')
    values = np.concatenate((block.ravel(), inst))
    rows, cols = col.hessian_indices_closed_form()
    assert tuple(z['ab']) == partition_nodes(SMALL, 2)[0]
    mc.check('%s over 2 gloo ranks' % label, z['first'], col.num_free, rows,
             cols, values, z['v'])
    assert np.array_equal(_bits(z['again']), _bits(z['first']))
    # powers of two scale every operation exactly
    assert np.array_equal(z['second'], 2.0*z['first'])
    assert np.array_equal(z['third'], 4.0*z['first'])


def _problem_worker(rank, world, port, out):
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
        kw = hc.KERNEL_PROBLEMS['C'](SMALL + 1)

        def make(obj_hessian):
            ev, pr = _Interpreter(), _HostProduct()
            extra = {} if obj_hessian is None else dict(
                obj_hessian=obj_hessian)
            prob = opty_amd.ShardedProblem(
                lambda f: 0.0, lambda f: 0.0*f, torch_device='cpu',
                sharded_kwargs=dict(evaluator=_unused,
                                    instance_evaluator=_unused,
                                    hessian_evaluator=ev,
                                    hessian_product_evaluator=pr),
                **extra, **kw)
            ev.col = pr.col = prob.collocator
            return prob

        def no_collective(prob):
            def refuse(*args, **kwargs):
                raise AssertionError('a collective before the refusal')
            prob.callbacks._command = refuse

        free, lam = hc.inputs(22, opty_amd.ConstraintCollocator(**kw))
        # refused before any collective, on a root whose serving ranks are
        # not even listening: no obj_hessian ...
        plain = make(None)
        no_collective(plain)
        with pytest.raises(NotImplementedError, match='obj_hessian'):
            plain.resident_hessian_operator(free, lam)
        # ... and values without a device handle, as Problem.hessian_operator
        hand = make(([0], [0], lambda f: np.ones(1)))
        no_collective(hand)
        with pytest.raises(TypeError, match='device handle'):
            hand.resident_hessian_operator(free, lam)
        for prob in (plain, hand):
            with pytest.raises(NotImplementedError, match='hessian_operator'):
                prob.hessian_operator(None, None)

        # an objective Hessian without entries: the section is skipped
        prob = make((none, none, lambda f: np.zeros(0)))
        with pytest.raises(NotImplementedError, match='hessian_operator'):
            prob.hessian_operator(None, None)
        if rank != 0:
            prob.serve()
            return
        n = prob.num_free
        rng = np.random.default_rng(23)
        v, u = rng.uniform(-1.0, 1.0, (2, n))
        old = prob.resident_hessian_operator(free, lam, 0.7)
        assert old.shape == (n, n) and old.dtype == np.float64
        hv, hu = old.matvec(v), old.rmatvec(u)
        HV = old.matmat(np.stack([v, u], axis=1))
        new = prob.resident_hessian_operator(free, 2.0*lam)
        with pytest.raises(RuntimeError, match='replaced'):
            old.matvec(v)
        hv2 = new.matvec(v)
        np.savez(out, free=free, lam=lam, v=v, u=u, hv=hv, hu=hu, HV=HV,
                 hv2=hv2)
        prob.shutdown()
    finally:
        dist.destroy_process_group()


def test_sharded_problem_has_a_resident_hessian_operator(tmp_path):
    """``ShardedProblem.resident_hessian_operator``: its refusals come before
    any collective, ``hessian_operator`` keeps refusing, the operator is that
    of the constraint triplets when the objective has no entries, and an
    operator whose values were replaced says so."""
    import torch.multiprocessing as mp
    out = str(tmp_path/'root.npz')
    mp.spawn(_problem_worker, args=(2, _free_port(), out), nprocs=2,
             join=True)
    z = np.load(out)
    col = hc.collocator('C', SMALL)
    block, inst, _ = hc.interpreted(col, z['free'], z['lam'])
    values = np.concatenate((block.ravel(), inst))
    rows, cols = col.hessian_indices_closed_form()
    for what, y, x in (('matvec', z['hv'], z['v']),
                       ('rmatvec', z['hu'], z['u'])):
        mc.check('resident operator %s' % what, y, col.num_free, rows, cols,
                 values, x)
    assert np.array_equal(_bits(z['HV']),
                          _bits(np.stack([z['hv'], z['hu']], axis=1)))
    assert np.array_equal(z['hv2'], 2.0*z['hv'])
