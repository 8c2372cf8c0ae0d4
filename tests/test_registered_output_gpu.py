"""GPU tests of registered device outputs (``opty_hip_output_register``): a
Jacobian buffer whose owner keeps it between evaluations is written whole
once and by the restricted kernels (``opty_jac_var`` / ``opty_conjac_var``:
only the lines that hold an entry which can change) from then on; an
unregistered pointer is always written whole."""
import os
import subprocess
import sys

import numpy as np
import pytest

import opty_amd
from examples import problems

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: constraint nodes of the ragged launches: 2 ... 1025, multiples of 64 and
#: their neighbours among them
NODE_COUNTS = [2, 3, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 500, 511,
               512, 513, 1000, 1023, 1024, 1025]
NODES = 1026
#: the module of the flagship's 99 999-node launches: the
#: code does not depend on N, every count above is a shard of one handle
LAUNCH = 99999


def _col(deterministic=False, nodes=NODES, **kw):
    factory, fkw = problems.CONFIGS['config3_10link']
    return opty_amd.ConstraintCollocator(
        deterministic=deterministic, launch_nodes=LAUNCH, **kw,
        **factory(**dict(fkw, num_nodes=nodes)))


def _sharded(**kw):
    from opty_amd.sharded import ShardedCollocator
    factory, fkw = problems.CONFIGS['config3_10link']
    return ShardedCollocator(rank=3, world_size=8, **kw,
                             **factory(**dict(fkw, num_nodes=NODES)))


def prebuild():
    """Code objects of the tests below (``__graft_entry__.build``)."""
    # (the default build of _col() is the module of the flagship's launches
    # and delay_be_small is prebuilt under its own name: both are on
    # build()'s lists already)
    _col(True).prebuild()
    # the collocator of _sharded(): built for its largest shard
    from opty_amd.sharded import partition_nodes
    factory, fkw = problems.CONFIGS['config3_10link']
    opty_amd.ConstraintCollocator(
        specialize_parameters=True,
        launch_nodes=max(b - a for a, b in partition_nodes(NODES - 1, 8)),
        **factory(**dict(fkw, num_nodes=NODES))).prebuild()


def _static_mask(col):
    from opty_amd.codegen.program import varying_entries
    prog = col._build_program()
    mask = np.ones(prog.P, bool)
    mask[varying_entries(prog)] = False
    return mask


def _close(got, ref, P):
    """The project's rule: 1e-10 relative per entry, floored at 1e-10 of the
    largest entry of the entry's node block."""
    floor = np.abs(ref.reshape(-1, P)).max(axis=1, keepdims=True)
    tol = 1e-10*np.maximum(np.abs(ref.reshape(-1, P)), floor)
    err = np.abs(got.reshape(-1, P) - ref.reshape(-1, P))
    assert np.all(err <= tol), float((err/tol).max())


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [True, False])
def test_registered_buffer_ragged_node_counts(deterministic):
    import torch
    from opty_amd import hip_backend as hb
    dev = torch.device('cuda:0')
    col = _col(deterministic)
    hip = col.hip
    assert hip.desc['var_jac_wgs_per_block'] > 0, 'no restricted kernels'
    hip.use_torch_stream()
    P, M, ncn = hip.desc['P'], col.num_eom, NODES - 1
    static = _static_mask(col)
    # an entry no restricted wave stages: behind the 13 entries of the next
    # node that the last line of a block can reach, before the kept span
    skipped = 100
    assert static[:480].all()
    frees = []
    for seed in (11, 12):
        fh = problems.make_free(col.num_free, seed=seed)
        col._sync_known(hip, fh)
        frees.append(torch.from_numpy(fh).to(dev))
    f64 = dict(dtype=torch.float64, device=dev)
    nan = float('nan')

    def run(what, free, con, jac, n):
        hip.eval_shard(what, free, con, ncn, jac, 0, n)
        torch.cuda.synchronize()

    for n in NODE_COUNTS:
        for what in (hb.EVAL_FUSED, hb.EVAL_JAC):
            reg = torch.full((n*P,), nan, **f64)
            plain = torch.full((n*P,), nan, **f64)
            con_r = torch.full((M, ncn), nan, **f64)
            con_p = torch.full((M, ncn), nan, **f64)
            hip.output_register(reg, 0, n)
            # 1. first evaluation: everything, as into any buffer
            run(what, frees[0], con_r, reg, n)
            run(what, frees[0], con_p, plain, n)
            assert hip.routing(n)['flavour'] == 'full'
            assert not torch.isnan(reg).any()
            assert torch.equal(reg, plain), (n, what)
            first = reg.clone()
            # second evaluation, another free: the restricted kernels
            run(what, frees[1], con_r, reg, n)
            assert hip.routing(n)['flavour'] == 'restricted', (n, what)
            plain.fill_(nan)
            run(what, frees[1], con_p, plain, n)    # 4. written whole
            assert hip.routing(n)['flavour'] == 'full'
            assert not torch.isnan(plain).any()
            got, ref = reg.cpu().numpy(), plain.cpu().numpy()
            if deterministic:
                np.testing.assert_array_equal(got, ref)
            else:
                _close(got, ref, P)
            # static entries bit-identical in both modes
            np.testing.assert_array_equal(got.reshape(n, P)[:, static],
                                          ref.reshape(n, P)[:, static])
            np.testing.assert_array_equal(
                got.reshape(n, P)[:, static],
                first.cpu().numpy().reshape(n, P)[:, static])
            if what == hb.EVAL_FUSED:
                # 5. constraints of the restricted fused kernel
                c_r = con_r[:, :n].cpu().numpy()
                c_p = con_p[:, :n].cpu().numpy()
                if deterministic:
                    np.testing.assert_array_equal(c_r, c_p)
                else:
                    np.testing.assert_allclose(c_r, c_p, rtol=1e-10, atol=(
                        1e-10*np.abs(c_p).max()))
            # 2. the fast path leaves skipped entries alone
            reg.view(n, P)[:, skipped] = nan
            run(what, frees[0], con_r, reg, n)
            assert hip.routing(n)['flavour'] == 'restricted'
            assert torch.isnan(reg.view(n, P)[:, skipped]).all(), (n, what)
            assert int(torch.isnan(reg).sum()) == n
            # ... until the owner says that it wrote to the buffer
            hip.output_invalidate(reg)
            run(what, frees[0], con_r, reg, n)
            assert torch.equal(reg, first)
            # another node range into the same buffer: whole, and whole again
            if n > 2:
                reg.fill_(nan)
                run(what, frees[0], con_r, reg, n - 1)
                assert not torch.isnan(reg[:(n - 1)*P]).any()
                reg.fill_(nan)
                run(what, frees[0], con_r, reg, n)
                assert torch.equal(reg, first)
            # 4. after unregister the same address is written whole
            hip.output_unregister(reg)
            reg.fill_(nan)
            run(what, frees[1], con_r, reg, n)
            assert not torch.isnan(reg).any()
            assert hip.routing(n)['flavour'] == 'full'
    with pytest.raises(hb.HipBackendError):
        hip.output_unregister(plain)
    with pytest.raises(hb.HipBackendError):
        hip.output_register(plain, 0, ncn + 1)


@pytest.mark.gpu
def test_new_parameters_and_interval_rewrite_the_static_entries():
    import torch
    from opty_amd import hip_backend as hb
    dev = torch.device('cuda:0')
    col = _col(True)
    hip = col.hip
    hip.use_torch_stream()
    P, ncn, n = hip.desc['P'], NODES - 1, 700
    fh = problems.make_free(col.num_free, seed=5)
    col._sync_known(hip, fh)
    free = torch.from_numpy(fh).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    reg = torch.full((n*P,), float('nan'), **f64)
    plain = torch.empty(n*P, **f64)
    hip.output_register(reg, 0, n)
    static = _static_mask(col)

    def both():
        hip.eval_shard(hb.EVAL_JAC, free, None, ncn, reg, 0, n)
        flavour = hip.routing(n)['flavour']
        hip.eval_shard(hb.EVAL_JAC, free, None, ncn, plain, 0, n)
        torch.cuda.synchronize()
        assert torch.equal(reg, plain)
        return flavour

    assert both() == 'full'
    assert both() == 'restricted'
    before = reg.clone()
    pars = np.array([float(col.known_parameter_map[p])
                     for p in col.known_parameters])
    heavier = pars.copy()
    heavier[:] *= 1.25                  # masses and lengths among them
    hip.set_known_parameters(heavier)
    assert both() == 'full'
    changed = (reg != before).view(n, P).any(dim=0).cpu().numpy()
    assert changed[static].any(), 'no static entry depends on a parameter?'
    assert both() == 'restricted'
    before = reg.clone()
    hip.set_interval(col.node_time_interval*0.5)
    assert both() == 'full'
    changed = (reg != before).view(n, P).any(dim=0).cpu().numpy()
    assert changed[static].any()        # the +-1/h entries
    assert both() == 'restricted'


@pytest.mark.gpu
def test_sharded_collocator_registers_its_jacobian():
    """A 1/8 shard with halo (rank 3 of 8): ``jac_local`` is registered, the
    second evaluation is restricted and equal to an unregistered one; new
    known parameters through ``set_known`` -- a re-specialisation, i.e. a
    new handle behind the same object -- rewrite the static entries."""
    import torch
    from opty_amd import hip_backend as hb
    sh = _sharded(specialize_parameters=True)
    col = sh.collocator
    hip = col.hip
    hip.use_torch_stream()
    assert hip.desc['var_jac_wgs_per_block'] > 0
    n, P, ncn = sh.b - sh.a, sh.P, sh.N - 1
    assert sh.a > 0 and sh.b < ncn                  # halo on both sides
    dev = sh.device
    frees = [torch.from_numpy(problems.make_free(col.num_free, seed=s)).to(dev)
             for s in (1, 2)]
    plain = torch.empty(n*P, dtype=torch.float64, device=dev)
    static = _static_mask(col)

    def check(free):
        sh.evaluate(free)
        flavour = col.hip.routing(n)['flavour']
        col.hip.eval_shard(hb.EVAL_JAC, free, None, ncn, plain, sh.a, sh.b)
        torch.cuda.synchronize()
        _close(sh.jac_local.cpu().numpy(), plain.cpu().numpy(), P)
        np.testing.assert_array_equal(
            sh.jac_local.view(n, P).cpu().numpy()[:, static],
            plain.view(n, P).cpu().numpy()[:, static])
        return flavour

    sh.jac_local.fill_(float('nan'))
    assert check(frees[0]) == 'full'
    assert check(frees[1]) == 'restricted'
    before = sh.jac_local.clone()
    pars = np.array([float(col.known_parameter_map[p])
                     for p in col.known_parameters])*1.25
    sh.set_known(params=pars)
    for p, v in zip(col.known_parameters, pars):
        col.known_parameter_map[p] = float(v)
    assert check(frees[1]) == 'full'
    changed = (sh.jac_local != before).view(n, P).any(dim=0).cpu().numpy()
    assert changed[static].any()
    assert check(frees[0]) == 'restricted'
    sh.close()
    sh.jac_local.fill_(float('nan'))
    sh.evaluate(frees[0])
    torch.cuda.synchronize()
    assert col.hip.routing(n)['flavour'] == 'full'
    assert not torch.isnan(sh.jac_local).any()


@pytest.mark.gpu
def test_whole_problem_with_instance_constraints():
    """``opty_hip_eval_con_jac`` / ``opty_hip_eval_jac`` with device memory
    into a registered buffer of a problem with instance constraints: the
    tails behind the node blocks are evaluated by either flavour."""
    import torch
    from opty_amd import hip_backend as hb
    dev = torch.device('cuda:0')
    col = opty_amd.ConstraintCollocator(**problems.build('delay_be_small'))
    hip = col.hip
    hip.use_torch_stream()
    assert col.num_instance_constraints > 0
    assert hip.desc['var_jac_wgs_per_block'] > 0
    f64 = dict(dtype=torch.float64, device=dev)
    frees = []
    for seed in (3, 4):
        fh = problems.make_free(col.num_free, seed=seed)
        col._sync_known(hip, fh)
        frees.append(torch.from_numpy(fh).to(dev))
    reg = torch.full((hip.nnz,), float('nan'), **f64)
    plain = torch.full((hip.nnz,), float('nan'), **f64)
    con_r = torch.empty(col.num_constraints, **f64)
    con_p = torch.empty(col.num_constraints, **f64)
    hip.output_register(reg)
    P = hip.desc['P']
    nblk = P*(col.num_collocation_nodes - 1)
    for k, want in ((0, 'full'), (1, 'restricted'), (0, 'restricted')):
        for fused in (True, False):
            if fused:
                hip.eval_con_jac(frees[k], con_r, reg, hb.DEVICE)
            else:
                hip.eval_jac(frees[k], reg, hb.DEVICE)
            torch.cuda.synchronize()
            assert hip.routing()['flavour'] == (want if fused or k
                                                else 'restricted')
            hip.eval_con_jac(frees[k], con_p, plain, hb.DEVICE)
            torch.cuda.synchronize()
            got, ref = reg.cpu().numpy(), plain.cpu().numpy()
            _close(got[:nblk], ref[:nblk], P)
            np.testing.assert_allclose(got[nblk:], ref[nblk:], rtol=1e-10,
                                       atol=1e-10*np.abs(ref[nblk:]).max())
            if fused:
                np.testing.assert_allclose(
                    con_r.cpu().numpy(), con_p.cpu().numpy(), rtol=1e-10,
                    atol=1e-10*float(con_p.abs().max()))


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_registered_output_gpu as t
from opty_amd import hip_backend as hb
from examples import problems
col = t._col(True)
hip = col.hip
hip.use_torch_stream()
P, ncn, n = hip.desc['P'], t.NODES - 1, 300
fh = problems.make_free(col.num_free, seed=5)
col._sync_known(hip, fh)
free = torch.from_numpy(fh).cuda()
reg = torch.empty(n*P, dtype=torch.float64, device='cuda')
hip.output_register(reg, 0, n)
for k in range(3):
    reg.fill_(float('nan'))
    hip.eval_shard(hb.EVAL_FUSED, free, torch.empty(col.num_eom, ncn,
                   dtype=torch.float64, device='cuda'), ncn, reg, 0, n)
    torch.cuda.synchronize()
    assert not torch.isnan(reg).any(), k
    assert hip.routing(n)['flavour'] == 'full', k
print('dense ok')
'''


@pytest.mark.gpu
def test_dense_output_switch():
    """``OPTY_HIP_DENSE_OUTPUT=1`` (read once: a child process): registered
    buffers are written whole every time."""
    env = dict(os.environ, OPTY_HIP_DENSE_OUTPUT='1')
    out = subprocess.run(
        [sys.executable, '-c', _CHILD % (REPO, os.path.join(REPO, 'tests'))],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'dense ok' in out.stdout
