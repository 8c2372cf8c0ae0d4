"""The run form of the restricted Jacobian kernels (``EmitOptions(var_order=
'run')``): the schedule the library builds for it (``opty_hip_run_schedule``:
contiguous, cost-balanced runs of (block, strip) items per XCD -- host
arithmetic) and what the printer prints."""
import ctypes
import re

import numpy as np
import pytest

from examples import problems

#: the flagship's six strips (the printer's estimate) and other shapes
COSTS = ([1348., 1524., 1536., 1528., 1509., 1668.],
         [20.5, 11.6, 4.7], [1.0], [5.0, 1.0, 1.0, 1.0, 1.0, 1.0, 9.0])


@pytest.mark.parametrize('nblk', [1, 7, 8, 9, 17, 1563])
@pytest.mark.parametrize('persist', [8, 16, 64, 1024])
@pytest.mark.parametrize('cost', COSTS)
def test_run_schedule_is_contiguous_and_balanced(persist, nblk, cost):
    from opty_amd import hip_backend as hb
    sched = hb.run_schedule(persist, nblk, cost)
    G = len(cost)
    nslot = (nblk + 7)//8
    # persist above and below the item count
    assert len(sched) == min(persist, nslot*8*G)
    bins = len(sched)//8
    for x in range(8):
        # every (slot, class) item of the XCD's blocks exactly once, on the
        # XCD of its block, and the workgroups' lists one after the other
        # ARE the XCD's (slot, class) order: every list is contiguous in it
        mine = [it for w in range(x, len(sched), 8) for it in sched[w]]
        assert all(b % 8 == x for _, b in mine)
        assert mine == [(g, b) for b in range(x, nblk, 8) for g in range(G)]
        loads = np.array([sum(cost[g] for g, _ in sched[w])
                          for w in range(x, len(sched), 8)])
        assert len(loads) == bins
        # summed cost per workgroup within one largest item of the mean
        assert np.all(np.abs(loads - loads.mean()) <= max(cost) + 1e-6), \
            (loads.min(), loads.mean(), loads.max())


def test_run_schedule_takes_unit_costs_for_missing_ones():
    from opty_amd import hip_backend as hb
    assert hb.run_schedule(8, 3, [0.0, 0.0]) == \
        hb.run_schedule(8, 3, [1.0, 1.0])


def test_run_schedule_rejects_bad_requests():
    from opty_amd import hip_backend as hb
    lib = hb.load_library()
    count = ctypes.c_int64()
    cost = (ctypes.c_float*2)(1.0, 1.0)
    for persist, nblk, classes in ((0, 4, 2), (12, 4, 2), (1024, -1, 2),
                                   (1024, 4, 0), (1024, 4, 33), (-8, 4, 2)):
        assert lib.opty_hip_run_schedule(persist, nblk, classes, cost, None,
                                         0, ctypes.byref(count)) != 0
        assert b'run-schedule' in lib.opty_hip_last_error()
    assert lib.opty_hip_run_schedule(1024, 4, 2, None, None, 0,
                                     ctypes.byref(count)) != 0
    assert lib.opty_hip_run_schedule(1024, 4, 2, cost, None, 0, None) != 0
    table = (ctypes.c_int32*4)()
    assert lib.opty_hip_run_schedule(1024, 4, 2, cost, table, 4,
                                     ctypes.byref(count)) != 0
    # a null handle is refused, not dereferenced
    assert lib.opty_hip_set_restricted_runs(None, b'x.hsaco', 8, 2, cost, 8, 2,
                                            cost) != 0


def _options(**kw):
    from opty_amd.codegen.emit_hip import EmitOptions
    return EmitOptions(groups=4, fused_groups=4, restricted=1, **kw)


#: sha of the module the parent commit prints for ``_pendulum()`` with
#: ``_options()``: the dispatch form is kept byte for byte
PARENT_SHA = 'c5ef6104c6a37b96787cdb00dd22180cd6275265dd016be5677dd7569eac7ab8'


def _pendulum():
    return problems.n_link_cart_pendulum(num_links=3, num_nodes=300)


def _kernel_text(src, name):
    start = src.index('\n%s(' % name)
    end = src.find('\nextern "C" __global__', start)
    return src[start:end if end > 0 else len(src)]


def test_run_form_prints_persistent_restricted_kernels():
    import opty_amd
    from opty_amd import hip_backend as hb
    kw = _pendulum()
    plain = opty_amd.ConstraintCollocator(emit_options=_options(), **kw)
    run = opty_amd.ConstraintCollocator(
        emit_options=_options(var_order='run', var_persist=64), **kw)
    src0, meta0 = plain.generate_source()
    main1, meta1 = run.generate_source()
    # the run form is a module of its own; the module that carries the full
    # kernels is the dispatch form's, but for the line that names the options
    assert [ln for ln in main1.split('\n') if not ln.startswith('// ')] == \
        [ln for ln in src0.split('\n') if not ln.startswith('// ')]
    assert 'run' not in meta0
    src1 = meta1['run']['source']
    assert 'opty_run_form = 1;' in src1 and 'opty_run_form' not in main1
    assert 'opty_opaque' not in main1 and 'opty_jac(' not in src1
    assert 'jac_var' in meta0['kernels'], 'no restricted kernels to test'
    # var_order=None: the parent's module
    assert meta0['sha'] == PARENT_SHA
    assert 'sched' not in src0 and 'opty_opaque' not in src0
    assert 'var_order' not in _options().key()
    assert 'var_order=run var_persist=64' in run._printer_options().key()
    # the full kernels do not change
    for key in ('con', 'jac', 'conjac', 'jac_var', 'conjac_var'):
        assert meta1['kernels'][key]['sha'] == meta0['kernels'][key]['sha']
    # one sched parameter per restricted kernel
    assert src1.count('const int *__restrict__ sched') == 2
    for key, name in (('jac_var', 'opty_jac_var'),
                      ('conjac_var', 'opty_conjac_var')):
        k, k0 = meta1['run']['kernels'][key], meta0['kernels'][key]
        assert k['order'] == 'run' and k0['order'] == 'dispatch'
        assert k['run_persist'] == 64 and k0['run_persist'] == 0
        # (``persist`` stays the mark of a LIST schedule)
        assert k['persist'] == k0['persist'] == 0
        assert k['waves_per_wg'] == 1
        # one class per strip (and constraint wave), as many as before
        assert k['wgs_per_block'] == k['groups'] == k0['groups']
        assert len(k['class_cost']) == k['wgs_per_block'] and \
            min(k['class_cost']) > 0
        text = _kernel_text(src1, name)
        assert '(const double *__restrict__ free_' in text and \
            'const int *__restrict__ sched)' in text.split('{')[0]
        # the trig stage sits under the block change, in front of the strips
        head, cases = text.split('switch (grp) {')
        assert 'if (blk != blk_prev) {' in head and \
            'blk_prev = blk;' in head
        staged = re.findall(r'^\s*double (tg\d+) = 0\.0;$', head, re.M)
        # (3 links: sin and cos of three angles)
        assert len(staged) == 6
        assert head.index('double %s = 0.0;' % staged[0]) < \
            head.index('while (item >= 0)')
        for t in staged:
            assert re.search(r'\b%s = ' % t, head.split('while (item')[1])
            assert re.search(r'\b%s\b' % t, cases)
        # no strip case evaluates sin / cos of a slab value itself
        slab = set(re.findall(r'const double (f\d+_\d+) = lds\[', cases))
        assert slab
        for fn, arg in re.findall(r'\b(sincos|sin|cos)\((\w+)', cases):
            assert arg not in slab, (fn, arg)
        # ... while the dispatch form's strips do
        text0 = _kernel_text(src0, name)
        slab0 = set(re.findall(r'const double (f\d+_\d+) = lds\[', text0))
        assert any(arg in slab0 for _, arg in re.findall(
            r'\b(sincos|sin|cos)\((\w+)', text0))
    d = run._descriptor(dict(meta1, restricted_ok=True, run_hsaco='x.hsaco'))
    assert d['var_run_code_object'] == 'x.hsaco'
    assert d['var_jac_persist'] == d['var_fused_persist'] == 64
    # one cost per class of the run form (the var_*_wgs_per_block fields
    # stay those of the module's dispatch form)
    for tag, key in (('jac', 'jac_var'), ('fused', 'conjac_var')):
        assert len(d['var_%s_class_cost' % tag]) == \
            meta1['run']['kernels'][key]['groups']
        assert d['var_%s_wgs_per_block' % tag] == \
            meta0['kernels'][key]['wgs_per_block']
    # (not fields of the descriptor: arguments of
    # opty_hip_set_restricted_runs)
    assert hb._Desc(**d).var_jac_wgs_per_block == d['var_jac_wgs_per_block']
    d0 = plain._descriptor(dict(meta0, restricted_ok=True))
    assert 'var_jac_persist' not in d0
    # builds (without MachineLICM: hb.LOOP_FLAGS), passes the static gates
    # and does not spill vector registers
    hsaco, meta = run._build_code_object()
    assert meta['restricted_ok'] is True, meta['restricted_refused']
    assert meta['run']['kernels']['jac_var']['run_persist'] == 64
    assert meta['run_hsaco'] and meta['run_hsaco'] != hsaco
    # the full kernels are built without the flags of the item loops
    assert set(hb.cached_kernel_resources(meta['run_hsaco'])) == {
        'opty_jac_var', 'opty_conjac_var'}
    assert hb.vgpr_spills(hsaco, ('opty_con', 'opty_jac', 'opty_conjac',
                                  'opty_jac_var', 'opty_conjac_var')) == {}


def test_traces_no_longer_switch_the_restricted_kernels_off():
    import opty_amd
    kw = _pendulum()
    for order in (None, 'run'):
        col = opty_amd.ConstraintCollocator(
            emit_options=_options(trace=1, var_order=order), **kw)
        src, meta = col.generate_source()
        assert 'jac_var' in meta['kernels']
        assert 'tr_w1 = wall_clock64();' in _kernel_text(
            meta['run']['source'] if order else src, 'opty_jac_var')
    # the rest of the list still does
    col = opty_amd.ConstraintCollocator(
        emit_options=_options(order='list'), **kw)
    assert 'jac_var' not in col.generate_source()[1]['kernels']


def test_a_run_form_that_fails_a_gate_falls_back_to_the_dispatch_form(
        monkeypatch):
    import opty_amd
    from opty_amd import hip_backend as hb
    kw = _pendulum()
    col = opty_amd.ConstraintCollocator(
        emit_options=_options(var_order='run', var_persist=64), **kw)
    real = hb.vgpr_spills

    def spills(hsaco, kernels=('opty_con', 'opty_jac', 'opty_conjac')):
        got = real(hsaco, kernels)
        # (only the run form's code object holds nothing but the two kernels)
        if set(hb.cached_kernel_resources(hsaco)) == {'opty_jac_var',
                                                      'opty_conjac_var'}:
            got = dict(got, opty_jac_var=3)
        return got

    monkeypatch.setattr(hb, 'vgpr_spills', spills)
    hsaco, meta = col._build_code_object()
    # the module's own restricted kernels (dispatch form) serve
    assert meta['restricted_ok'] is True and meta['run_hsaco'] is None
    assert meta['kernels']['jac_var']['order'] == 'dispatch'
    assert 'opty_jac_var=3' in col._run_form_refused.replace("': ", '=') \
        .replace("'", '')
    d = col._descriptor(meta)
    assert d['var_jac_wgs_per_block'] > 0 and 'var_run_code_object' not in d
