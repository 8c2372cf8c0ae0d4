"""GPU tests of the run form of the restricted Jacobian kernels
(``EmitOptions(var_order='run')``: persistent waves over contiguous runs of
(block, strip) items; the slab fill and the block's sin / cos only where the
block changes): registered outputs end as the full kernels write them, for
every way a run can start, cross a block change and end."""
import copy

import numpy as np
import pytest

import opty_amd
from examples import problems

#: 17 blocks of 64 nodes: XCD 0 holds three block slots, the others two
NODES = 1026
#: the strip geometry of the flagship's module (the code does not depend on
#: N, every node range below is a shard of one handle)
LAUNCH = 99999
#: workgroups of the restricted kernels: 8 = one wave per XCD, every run
#: crosses block changes; 16 = run boundaries inside a block, a wave starts
#: mid-block with nothing staged; 1024 = more waves than items
PERSIST = (8, 16, 1024)
#: constraint nodes per launch, from node 0 and as an inner shard [A, A + n)
COUNTS = (2, 63, 64, 65, 513, 1025)
A = 37
#: an entry no restricted wave stages (before the kept span of the block)
SKIPPED = 100


def _col(persist, deterministic):
    factory, fkw = problems.CONFIGS['config3_10link']
    kw = factory(**dict(fkw, num_nodes=NODES))
    # the flagship module's options (launch plan), the run form forced
    opts = copy.copy(opty_amd.ConstraintCollocator(
        launch_nodes=LAUNCH, **kw)._printer_options())
    opts.var_order, opts.var_persist = 'run', persist
    return opty_amd.ConstraintCollocator(
        deterministic=deterministic, launch_nodes=LAUNCH, emit_options=opts,
        **kw)


def prebuild():
    """Code objects of the tests below (``__graft_entry__.build``)."""
    for persist in PERSIST:
        for deterministic in (True, False):
            _col(persist, deterministic).prebuild()
    opty_amd.ConstraintCollocator(
        **problems.build('pend2_link_vardur_unkmass_small')).prebuild()


def _close(got, ref, P):
    """The project's rule: 1e-10 relative per entry, floored at 1e-10 of the
    largest entry of the entry's node block."""
    floor = np.abs(ref.reshape(-1, P)).max(axis=1, keepdims=True)
    tol = 1e-10*np.maximum(np.abs(ref.reshape(-1, P)), floor)
    err = np.abs(got.reshape(-1, P) - ref.reshape(-1, P))
    assert np.all(err <= tol), float((err/tol).max())


@pytest.fixture(scope='module')
def frees():
    """The two free vectors every case evaluates (host; one reference input
    for the whole module)."""
    factory, fkw = problems.CONFIGS['config3_10link']
    col = opty_amd.ConstraintCollocator(
        launch_nodes=LAUNCH, **factory(**dict(fkw, num_nodes=NODES)))
    return [problems.make_free(col.num_free, seed=s) for s in (11, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [True, False])
@pytest.mark.parametrize('persist', PERSIST)
def test_run_form_fills_registered_buffers_like_the_full_kernels(
        persist, deterministic, frees, monkeypatch):
    import torch
    from opty_amd import hip_backend as hb
    # the kernel that is asked for is the kernel that runs: EVAL_JAC ->
    # opty_jac_var, EVAL_FUSED -> opty_conjac_var
    monkeypatch.setenv('OPTY_HIP_ROUTING', 'plan')
    dev = torch.device('cuda:0')
    col = _col(persist, deterministic)
    hip = col.hip
    d = hip.desc
    assert d['var_jac_persist'] == d['var_fused_persist'] == persist
    assert d['var_run_code_object'], 'the run form was not built'
    hip.use_torch_stream()
    P, M = d['P'], col.num_eom
    dfree = []
    for fh in frees:
        col._sync_known(hip, fh)
        dfree.append(torch.from_numpy(fh).to(dev))
    f64 = dict(dtype=torch.float64, device=dev)
    nan = float('nan')
    ranges = [(0, n) for n in COUNTS] + \
        [(A, min(A + n, NODES - 1)) for n in COUNTS]
    assert A % 64 != 0
    for a, b in ranges:
        n = b - a
        for what in (hb.EVAL_JAC, hb.EVAL_FUSED):
            reg = torch.full((n*P,), nan, **f64)
            plain = torch.full((n*P,), nan, **f64)
            con_r = torch.full((M, n), nan, **f64)
            con_p = torch.full((M, n), nan, **f64)
            hip.output_register(reg, a, b)
            try:
                # pre-filled by ANOTHER free vector, written whole
                hip.eval_shard(what, dfree[0], con_r, n, reg, a, b)
                torch.cuda.synchronize()
                assert hip.routing(n)['flavour'] == 'full'
                assert not torch.isnan(reg).any()
                # a NaN in an entry the restricted kernels skip, in every node
                view = reg.view(n, P)
                view[:, SKIPPED] = nan
                # the run form
                con_r.fill_(nan)
                hip.eval_shard(what, dfree[1], con_r, n, reg, a, b)
                torch.cuda.synchronize()
                assert hip.routing(n)['flavour'] == 'restricted', (a, b, what)
                # the full kernels, same free vector, unregistered buffer
                hip.eval_shard(what, dfree[1], con_p, n, plain, a, b)
                torch.cuda.synchronize()
                assert hip.routing(n)['flavour'] == 'full'
            finally:
                hip.output_unregister(reg)
            got = reg.cpu().numpy().reshape(n, P)
            ref = plain.cpu().numpy().reshape(n, P)
            assert not np.isnan(ref).any()
            # the planted NaNs survive, nothing else is NaN
            assert np.isnan(got[:, SKIPPED]).all(), (a, b, what)
            got[:, SKIPPED] = ref[:, SKIPPED]
            assert not np.isnan(got).any(), (a, b, what)
            if deterministic:
                np.testing.assert_array_equal(got, ref)
            else:
                _close(got, ref, P)
            if what == hb.EVAL_FUSED:
                c_r, c_p = con_r.cpu().numpy(), con_p.cpu().numpy()
                assert not np.isnan(c_p).any()
                if deterministic:
                    np.testing.assert_array_equal(c_r, c_p)
                else:
                    scale = np.abs(c_p).max(axis=1, keepdims=True)
                    assert np.all(np.abs(c_r - c_p) <= 1e-10*np.maximum(
                        np.abs(c_p), scale))


@pytest.mark.gpu
def test_registration_has_no_effect_without_restricted_kernels():
    """A table that depends on ``free`` (variable duration, unknown mass):
    the module carries no restricted kernels in either form."""
    import torch
    from opty_amd import hip_backend as hb
    dev = torch.device('cuda:0')
    col = opty_amd.ConstraintCollocator(
        **problems.build('pend2_link_vardur_unkmass_small'))
    hip = col.hip
    assert hip.desc['var_jac_wgs_per_block'] == 0
    assert 'var_jac_persist' not in hip.desc
    hip.use_torch_stream()
    f64 = dict(dtype=torch.float64, device=dev)
    reg = torch.full((hip.nnz,), float('nan'), **f64)
    plain = torch.full((hip.nnz,), float('nan'), **f64)
    con = torch.empty(col.num_constraints, **f64)
    hip.output_register(reg)
    try:
        for seed in (3, 4):
            fh = problems.make_free(
                col.num_free, seed=seed,
                variable_duration=col._variable_duration)
            col._sync_known(hip, fh)
            free = torch.from_numpy(fh).to(dev)
            hip.eval_con_jac(free, con, reg, hb.DEVICE)
            torch.cuda.synchronize()
            assert hip.routing()['flavour'] == 'full'
            hip.eval_con_jac(free, con, plain, hb.DEVICE)
            torch.cuda.synchronize()
            assert torch.equal(reg, plain)
    finally:
        hip.output_unregister(reg)


@pytest.mark.gpu
def test_set_restricted_runs_refuses_what_it_cannot_launch(tmp_path):
    """``opty_hip_set_restricted_runs`` takes the place of the checks
    ``opty_hip_create`` makes for list kernels."""
    import ctypes
    from opty_amd import hip_backend as hb
    col = _col(16, False)
    hsaco, meta = col._build_code_object()
    run_hsaco = meta['run_hsaco']
    assert run_hsaco
    desc = col._descriptor(meta)
    plain = {k: v for k, v in desc.items()
             if k not in hb.HipProblem._RUN_KEYS}
    hip = hb.HipProblem(plain, hsaco)       # the dispatch form serves
    lib = hb.load_library()
    jc = (ctypes.c_float*32)(*desc['var_jac_class_cost'])
    fc = (ctypes.c_float*32)(*desc['var_fused_class_cost'])
    nj, nf = len(desc['var_jac_class_cost']), \
        len(desc['var_fused_class_cost'])
    ok = run_hsaco.encode()

    def call(path=ok, jp=16, cj=nj, costj=jc, fp=16, cf=nf, costf=fc, h=None):
        return lib.opty_hip_set_restricted_runs(
            hip._h if h is None else h, path, jp, cj, costj, fp, cf, costf)

    bogus = tmp_path/'x.hsaco'
    bogus.write_bytes(b'not a code object')
    for kw in (dict(jp=12), dict(fp=12), dict(jp=0), dict(fp=-8),
               dict(cj=0), dict(cf=33), dict(costj=None), dict(costf=None),
               dict(path=None), dict(path=str(bogus).encode()),
               dict(path=str(tmp_path/'missing.hsaco').encode()),
               # the module of the full kernels: no marker, dispatch form
               dict(path=hsaco.encode())):
        assert call(**kw) != 0, kw
        assert lib.opty_hip_last_error()
    assert b'run form' in lib.opty_hip_last_error()
    # a module without restricted kernels
    other = opty_amd.ConstraintCollocator(
        **problems.build('pend2_link_vardur_unkmass_small')).hip
    assert call(h=other._h) != 0
    assert b'no restricted kernels' in lib.opty_hip_last_error()
    # what is right is taken, once
    assert call() == 0, lib.opty_hip_last_error()
    assert call() != 0
    assert b'already' in lib.opty_hip_last_error()
    hip.close()
