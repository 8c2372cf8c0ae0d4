"""The build ladder (``ConstraintCollocator._build_code_object`` and what it
calls: ``opty_amd/build_ladder.py``) with the REAL printer and a FAKE compiler:
which modules are compiled, in which batches, with which hipcc switches, and
which one is chosen, when the spill counts, the static ISA check and the
kernels' resources are scripted.  No ``hipcc`` runs.

``hb.compile_module`` records ``(second source line, extra_flags,
opt_level)`` -- the second line of a printed module holds its printer options
-- and returns a path made of their hash; ``hb.vgpr_spills``,
``hb.cached_kernel_resources``, ``isa_check.exec_copies``, ``isa_check.note``
and ``isa_check.noted`` answer from the scenario's script.

The expected values are literals (``EXPECTED``): the compile requests per
batch as SETS (the order within a batch is that of the threads), the chosen
path, the options of the chosen build and the keys of its meta that the
ladder sets.  A request is written ``(option tokens that the first request
of the scenario does not have, extra_flags, opt_level)``.

The candidate lists of rungs that no small problem reaches in seconds (the
work-aware cut, the detach phase, the parking budgets) are tested on
``build_ladder``'s pure functions at the end.
"""
import hashlib
import logging

import pytest

from opty_amd import ConstraintCollocator
from opty_amd import hip_backend as hb
from opty_amd import isa_check
from opty_amd.codegen.emit_hip import EmitOptions
from examples import problems

FULL = ('opty_con', 'opty_jac', 'opty_conjac')
VAR = ('opty_jac_var', 'opty_conjac_var')

_problems = {}


def _problem(name):
    if name not in _problems:
        _problems[name] = problems.build(name)
    return _problems[name]


class Request(object):
    """One call of the fake compiler."""

    def __init__(self, source, extra_flags, opt_level):
        lines = source.splitlines()
        self.line = lines[1]
        self.run_form = 'run form' in lines[0]
        self.flags, self.opt_level = tuple(extra_flags), opt_level
        self.path = '/nonexistent/opty_%s.hsaco' % hashlib.sha256(repr(
            (self.line, self.flags, opt_level)).encode()).hexdigest()[:12]

    def has(self, token):
        return token in self.line.split()


class Fakes(object):
    """The scripted tool chain of one scenario.  ``spills(request, kernels)``
    and ``copies(request, names)`` answer for a compile request;
    ``resources`` is what ``hb.cached_kernel_resources`` returns (None: it
    fails)."""

    def __init__(self, monkeypatch, spills=None, copies=None, resources=None):
        self.requests, self.notes = [], []
        self.by_path = {}
        self.spills = spills or (lambda req, kernels: {})
        self.copies = copies or (lambda req, names: {})
        self.resources = resources
        monkeypatch.setattr(hb, 'compile_module', self.compile_module)
        monkeypatch.setattr(hb, 'vgpr_spills', self.vgpr_spills)
        monkeypatch.setattr(hb, 'cached_kernel_resources',
                            self.cached_kernel_resources)
        monkeypatch.setattr(isa_check, 'exec_copies', self.exec_copies)
        monkeypatch.setattr(isa_check, 'noted', lambda hsaco, key: None)
        monkeypatch.setattr(isa_check, 'note', self.note)

    def compile_module(self, source, cache_dir=None,
                       show_compile_output=False, extra_flags=(),
                       opt_level=None):
        req = Request(source, extra_flags, opt_level)
        self.requests.append(req)
        self.by_path[req.path] = req
        return req.path

    def vgpr_spills(self, hsaco, kernels=FULL):
        return dict(self.spills(self.by_path[hsaco], tuple(kernels)))

    def exec_copies(self, hsaco, names=FULL):
        return dict(self.copies(self.by_path[hsaco], tuple(names)))

    def cached_kernel_resources(self, hsaco):
        if self.resources is None:
            raise hb.HipBackendError('no metadata')
        return self.resources

    def note(self, hsaco, key, value):
        self.notes.append((hsaco.rsplit('/', 1)[1], key, value))

    def batches(self, sizes):
        """The requests so far, cut into batches of ``sizes``."""
        base = set(self.requests[0].line.split())
        short = [(tuple(sorted(set(r.line.split()) - base)), r.flags,
                  r.opt_level) for r in self.requests]
        assert sum(sizes) == len(short), (sizes, short)
        out, at = [], 0
        for n in sizes:
            out.append(set(short[at:at + n]))
            assert len(out[-1]) == n, short[at:at + n]
            at += n
        return out


#: keys of ``meta`` that the ladder sets
META_KEYS = ('banned_kernels', 'vector_spills', 'auto_specialized',
             'isa_exec_copies', 'isa_replaced', 'restricted_ok',
             'restricted_refused', 'run_hsaco')


def _outcome(col, fakes, hsaco, meta, sizes, caplog):
    return dict(
        batches=fakes.batches(sizes), chosen=hsaco.rsplit('/', 1)[1],
        key=col._built_options.key(),
        meta={k: (meta[k].rsplit('/', 1)[1] if k == 'run_hsaco' and meta[k]
                  else meta[k]) for k in META_KEYS if k in meta},
        run_form_refused=col._run_form_refused, notes=fakes.notes,
        warnings=len([r for r in caplog.records
                      if r.levelno >= logging.WARNING]))


def _build(monkeypatch, caplog, name, sizes, spills=None, copies=None,
           resources=None, **kw):
    fakes = Fakes(monkeypatch, spills, copies, resources)
    col = ConstraintCollocator(**kw, **_problem(name))
    with caplog.at_level(logging.WARNING, logger='opty_amd'):
        hsaco, meta = col._build_code_object()
    return _outcome(col, fakes, hsaco, meta, sizes, caplog)


def _all_spill(req, kernels):
    return {k: 3 for k in kernels if k in FULL[1:]}


def _only(kernel):
    return lambda req, kernels: {kernel: 2} if kernel in kernels else {}


def _fails(req, names):
    raise OSError('llvm-objdump: not found')


# --- the scenarios: name -> function(monkeypatch, caplog) -> outcome -------

def clean(mp, caplog):
    return _build(mp, caplog, 'msd_be_small', [1])


def clean_with_run_form(mp, caplog):
    return _build(mp, caplog, 'config3_10link_small', [1, 1],
                  launch_nodes=99999)


def everything_spills(mp, caplog):
    # nine narrower cuts, the four ``forget`` cuts, then the least-spilling
    # source (the first: nothing spills less) with SAFE_SCHEDULER_FLAGS
    return _build(mp, caplog, 'config3_10link_small', [1, 4, 4, 1, 4, 1],
                  spills=_all_spill)


def least_spilling_cut_is_kept(mp, caplog):
    # every cut spills, the second strip step less than the rest: its source
    # is the one built with SAFE_SCHEDULER_FLAGS in the end
    def spills(req, kernels):
        return {k: 1 if req.has('fused_groups=11') else 3
                for k in kernels if k in FULL[1:]}
    return _build(mp, caplog, 'config3_10link_small', [1, 4, 4, 1, 4, 1],
                  spills=spills)


def only_jac_spills(mp, caplog):
    return _build(mp, caplog, 'config3_10link_small', [1, 4, 4, 1, 4],
                  spills=_only('opty_jac'))


def only_conjac_spills(mp, caplog):
    return _build(mp, caplog, 'config3_10link_small', [1, 4, 4, 1, 4],
                  spills=_only('opty_conjac'))


def third_step_is_clean(mp, caplog):
    # the first batch is the strip steps 1, 2, 3, 4 (9 fused strips in the
    # first build): the third is clean, the fourth too -- the third wins, all
    # four are compiled
    def spills(req, kernels):
        if req.has('fused_groups=12') or req.has('fused_groups=13'):
            return {}
        return _all_spill(req, kernels)
    return _build(mp, caplog, 'config3_10link_small', [1, 4], spills=spills)


def exec_copies_clean_sibling(mp, caplog):
    return _build(mp, caplog, 'msd_be_small', [1, 1],
                  copies=lambda req, names: {'opty_conjac': 2}
                  if 'opty_conjac' in names and not req.has('fast_trig=2')
                  else {})


def exec_copies_sibling_no_better(mp, caplog):
    return _build(mp, caplog, 'msd_be_small', [1, 1],
                  copies=lambda req, names: {'opty_conjac': 2}
                  if 'opty_conjac' in names else {})


def gate_fails_at_the_full_kernels(mp, caplog):
    return _build(mp, caplog, 'msd_be_small', [1], copies=_fails)


def gate_fails_at_the_restricted_kernels(mp, caplog):
    def copies(req, names):
        if set(names) & set(VAR):
            raise OSError('llvm-objdump: not found')
        return {}
    return _build(mp, caplog, 'config3_10link_small', [1], copies=copies,
                  launch_nodes=99999)


def gate_fails_at_the_sibling(mp, caplog):
    # NEW BEHAVIOUR (the one scenario that differs from the code before the
    # ladder had one gate, where the exception escaped): the tools fail on
    # the uniform-sincos sibling -- it counts as "no better", the first build
    # is kept and NO note is written, so that a later run tries again
    def copies(req, names):
        if req.has('fast_trig=2'):
            raise OSError('llvm-objdump: not found')
        return {'opty_conjac': 2} if 'opty_conjac' in names else {}
    return _build(mp, caplog, 'msd_be_small', [1, 1], copies=copies)


def restricted_kernels_spill(mp, caplog):
    return _build(mp, caplog, 'config3_10link_small', [1],
                  spills=lambda req, kernels: {'opty_jac_var': 2}
                  if 'opty_jac_var' in kernels else {}, launch_nodes=99999)


def run_form_spills(mp, caplog):
    return _build(mp, caplog, 'config3_10link_small', [1, 1],
                  spills=lambda req, kernels: {'opty_jac_var': 3}
                  if req.run_form else {}, launch_nodes=99999)


def automatic_specialisation(mp, caplog):
    return _build(mp, caplog, 'one_legged_small', [1, 1],
                  resources={'opty_conjac': {'.sgpr_spill_count': 250}})


def emit_options_that_spill(mp, caplog):
    return _build(mp, caplog, 'msd_be_small', [1], spills=_all_spill,
                  emit_options=EmitOptions())


SCENARIOS = [clean, clean_with_run_form, everything_spills,
             least_spilling_cut_is_kept, only_jac_spills,
             only_conjac_spills, third_step_is_clean,
             exec_copies_clean_sibling, exec_copies_sibling_no_better,
             gate_fails_at_the_full_kernels,
             gate_fails_at_the_restricted_kernels, gate_fails_at_the_sibling,
             restricted_kernels_spill, run_form_spills,
             automatic_specialisation, emit_options_that_spill]


def alternative(mp, caplog, accept):
    """``_verified_alternative`` after the referee refused the default build
    of the 10-link pendulum, with a referee that accepts the neighbour
    ``accept`` (counted over the builds it is shown)."""
    from opty_amd import launch_plan
    fakes = Fakes(mp)
    recorded = []
    mp.setattr(launch_plan, 'record',
               lambda key, entry, path=None: recorded.append(entry))
    col = ConstraintCollocator(**_problem('config3_10link_small'))
    refused, meta = col._build_code_object()
    shown = []

    def verify(hsaco, meta, force=False):
        assert force and col._built_options is not None
        # (the referee reads the candidate's own source and options)
        assert fakes.by_path[hsaco].line == col._built_source.splitlines()[1]
        shown.append(hsaco)
        if len(shown) - 1 != accept:
            raise hb.BuildRejected('no', dict(errors={'opty_jac': len(shown)}))
        return dict(ok=True)
    mp.setattr(col, '_verify_build', verify)
    err = hb.BuildRejected('refused', dict(errors={'opty_jac': 0}))
    with caplog.at_level(logging.WARNING, logger='opty_amd'):
        if accept is None:
            with pytest.raises(hb.BuildRejected, match='No neighbouring'):
                col._verified_alternative(refused, meta, err)
            return dict(batches=fakes.batches([1, 4, 4, 4, 1]),
                        shown=len(shown), pinned=col._pinned,
                        recorded=recorded)
        hsaco, m, verdict = col._verified_alternative(refused, meta, err)
    sizes = [1] + [4]*(accept//4 + 1)
    sizes[-1] = len(fakes.requests) - sum(sizes[:-1])
    out = _outcome(col, fakes, hsaco, m, sizes, caplog)
    assert verdict['replaces'] == refused.rsplit('/', 1)[1]
    assert verdict['refused'] == recorded[0]['refused']
    assert col._pinned[0] is col._built_options
    assert recorded[0]['options'] == launch_plan.options_kwargs(
        col._pinned[0])
    return dict(out, label=verdict['replacement'], how=col._pinned[1],
                refused=[tuple(r) for r in verdict['refused'][1:]],
                pinned=recorded[0]['pinned']['label'])


#: what the code before the ladder had a module of its own did, recorded by
#: running these scenarios on it
EXPECTED = {
    'clean': {'batches': [{((), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': {}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'clean_with_run_form': {'batches': [{((), (), None)},
                 {((), ('-mllvm', '-disable-machine-licm'), None)}],
     'chosen': 'opty_de3864c0aa03.hsaco',
     'key': 'chunk=32 groups=11 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=9 var_order=run var_persist=1024',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': True,
              'restricted_refused': None,
              'run_hsaco': 'opty_ae3a79bbc29b.hsaco'},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'everything_spills': {'batches': [{((), (), None)},
                 {(('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=12', 'groups=13'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)},
                 {(('fused_groups=14', 'groups=15'), (), None),
                  (('fused_groups=15', 'groups=16'), (), None),
                  (('fused_groups=17', 'groups=18'), (), None),
                  (('fused_groups=19', 'groups=20'), (), None)},
                 {(('fused_groups=21', 'groups=22'), (), None)},
                 {(('chunk=16', 'forget=1'), (), None),
                  (('chunk=16', 'forget=1', 'fused_groups=11', 'groups=12'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=13', 'groups=14'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=17', 'groups=18'),
                   (),
                   None)},
                 {((),
                   ('-mllvm',
                    '-amdgpu-disable-unclustered-high-rp-reschedule'),
                   None)}],
     'chosen': 'opty_e1f75c1216df.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': True,
              'restricted_refused': None,
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 1},
    'least_spilling_cut_is_kept': {'batches': [{((), (), None)},
                 {(('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=12', 'groups=13'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)},
                 {(('fused_groups=14', 'groups=15'), (), None),
                  (('fused_groups=15', 'groups=16'), (), None),
                  (('fused_groups=17', 'groups=18'), (), None),
                  (('fused_groups=19', 'groups=20'), (), None)},
                 {(('fused_groups=21', 'groups=22'), (), None)},
                 {(('chunk=16', 'forget=1'), (), None),
                  (('chunk=16', 'forget=1', 'fused_groups=11', 'groups=12'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=13', 'groups=14'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=17', 'groups=18'),
                   (),
                   None)},
                 {(('fused_groups=11', 'groups=12'),
                   ('-mllvm',
                    '-amdgpu-disable-unclustered-high-rp-reschedule'),
                   None)}],
     'chosen': 'opty_a971a89af9be.hsaco',
     'key': 'chunk=32 groups=12 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=11',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': True,
              'restricted_refused': None,
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 1},
    'only_jac_spills': {'batches': [{((), (), None)},
                 {(('fused_groups=9', 'groups=11'), (), None),
                  (('fused_groups=9', 'groups=12'), (), None),
                  (('fused_groups=9', 'groups=13'), (), None),
                  (('fused_groups=9', 'groups=14'), (), None)},
                 {(('fused_groups=9', 'groups=15'), (), None),
                  (('fused_groups=9', 'groups=16'), (), None),
                  (('fused_groups=9', 'groups=18'), (), None),
                  (('fused_groups=9', 'groups=20'), (), None)},
                 {(('fused_groups=9', 'groups=22'), (), None)},
                 {(('chunk=16', 'forget=1'), (), None),
                  (('chunk=16', 'forget=1', 'fused_groups=9', 'groups=12'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=9', 'groups=14'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=9', 'groups=18'),
                   (),
                   None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'banned_kernels': ['opty_jac'],
              'isa_exec_copies': {},
              'restricted_ok': False,
              'restricted_refused': "full kernels banned: ['opty_jac']",
              'run_hsaco': None,
              'vector_spills': {'opty_jac': 2}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'only_conjac_spills': {'batches': [{((), (), None)},
                 {(('fused_groups=10', 'groups=10'), (), None),
                  (('fused_groups=11', 'groups=10'), (), None),
                  (('fused_groups=12', 'groups=10'), (), None),
                  (('fused_groups=13', 'groups=10'), (), None)},
                 {(('fused_groups=14', 'groups=10'), (), None),
                  (('fused_groups=15', 'groups=10'), (), None),
                  (('fused_groups=17', 'groups=10'), (), None),
                  (('fused_groups=19', 'groups=10'), (), None)},
                 {(('fused_groups=21', 'groups=10'), (), None)},
                 {(('chunk=16', 'forget=1'), (), None),
                  (('chunk=16', 'forget=1', 'fused_groups=11', 'groups=10'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=13', 'groups=10'),
                   (),
                   None),
                  (('chunk=16', 'forget=1', 'fused_groups=17', 'groups=10'),
                   (),
                   None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'banned_kernels': ['opty_conjac'],
              'isa_exec_copies': {},
              'restricted_ok': False,
              'restricted_refused': "full kernels banned: ['opty_conjac']",
              'run_hsaco': None,
              'vector_spills': {'opty_conjac': 2}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'third_step_is_clean': {'batches': [{((), (), None)},
                 {(('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=12', 'groups=13'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)}],
     'chosen': 'opty_6d71d8598de3.hsaco',
     'key': 'chunk=32 groups=13 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=12',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': True,
              'restricted_refused': None,
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'exec_copies_clean_sibling': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None)}],
     'chosen': 'opty_190fb9a1b341.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fast_trig=2',
     'meta': {'isa_exec_copies': {}, 'isa_replaced': {'opty_conjac': 2}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'exec_copies_sibling_no_better': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': {'opty_conjac': 2}},
     'notes': [('opty_fef4983a4727.hsaco',
                'sibling_no_better',
                {'copies': {'opty_conjac': 2}, 'spills': {}})],
     'run_form_refused': None,
     'warnings': 0},
    'gate_fails_at_the_full_kernels': {'batches': [{((), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 1},
    'gate_fails_at_the_restricted_kernels': {'batches': [{((), (), None)}],
     'chosen': 'opty_de3864c0aa03.hsaco',
     'key': 'chunk=32 groups=11 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=9 var_order=run var_persist=1024',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': False,
              'restricted_refused': "static ISA check: {'isa_check': "
                                    "'llvm-objdump: not found'}",
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'gate_fails_at_the_sibling': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': {'opty_conjac': 2}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'restricted_kernels_spill': {'batches': [{((), (), None)}],
     'chosen': 'opty_de3864c0aa03.hsaco',
     'key': 'chunk=32 groups=11 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=9 var_order=run var_persist=1024',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': False,
              'restricted_refused': "vector spills: {'opty_jac_var': 2}",
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'run_form_spills': {'batches': [{((), (), None)},
                 {((), ('-mllvm', '-disable-machine-licm'), None)}],
     'chosen': 'opty_de3864c0aa03.hsaco',
     'key': 'chunk=32 groups=11 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=9 var_order=run var_persist=1024',
     'meta': {'isa_exec_copies': {},
              'restricted_ok': True,
              'restricted_refused': None,
              'run_hsaco': None},
     'notes': [],
     'run_form_refused': "vector spills: {'opty_jac_var': 3}",
     'warnings': 0},
    'automatic_specialisation': {'batches': [{((), (), None)},
                                             {((), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'auto_specialized': True, 'isa_exec_copies': {}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 0},
    'emit_options_that_spill': {'batches': [{((), (), None)}],
     'chosen': 'opty_fef4983a4727.hsaco',
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'meta': {'isa_exec_copies': {}},
     'notes': [],
     'run_form_refused': None,
     'warnings': 1},
    'alternative_0': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None),
                  (('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)}],
     'chosen': 'opty_190fb9a1b341.hsaco',
     'how': {},
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fast_trig=2',
     'label': 'uniform_trig',
     'meta': {},
     'notes': [],
     'pinned': 'uniform_trig',
     'refused': [],
     'run_form_refused': None,
     'warnings': 1},
    'alternative_2': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None),
                  (('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)}],
     'chosen': 'opty_3028fa8cab7d.hsaco',
     'how': {},
     'key': 'chunk=32 groups=14 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=13',
     'label': 'strips+4',
     'meta': {},
     'notes': [],
     'pinned': 'strips+4',
     'refused': [('uniform_trig', {'opty_jac': 1}),
                 ('strips+2', {'opty_jac': 2})],
     'run_form_refused': None,
     'warnings': 1},
    'alternative_5': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None),
                  (('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)},
                 {(('fused_groups=15', 'groups=16'), (), None),
                  (('fused_groups=17', 'groups=18'), (), None),
                  (('fused_groups=21', 'groups=22'), (), None),
                  (('fused_groups=7', 'groups=8'), (), None)}],
     'chosen': 'opty_cf67dfb182c1.hsaco',
     'how': {},
     'key': 'chunk=32 groups=18 max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0 '
            'fused_groups=17',
     'label': 'strips+8',
     'meta': {},
     'notes': [],
     'pinned': 'strips+8',
     'refused': [('uniform_trig', {'opty_jac': 1}),
                 ('strips+2', {'opty_jac': 2}),
                 ('strips+4', {'opty_jac': 3}),
                 ('strips+1', {'opty_jac': 4}),
                 ('strips+6', {'opty_jac': 5})],
     'run_form_refused': None,
     'warnings': 1},
    'alternative_11': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None),
                  (('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)},
                 {(('fused_groups=15', 'groups=16'), (), None),
                  (('fused_groups=17', 'groups=18'), (), None),
                  (('fused_groups=21', 'groups=22'), (), None),
                  (('fused_groups=7', 'groups=8'), (), None)},
                 {((), (), '-O1'),
                  (('chunk=16',), (), None),
                  (('fast_trig=1',), (), None),
                  (('fused_groups=5', 'groups=6'), (), None)}],
     'chosen': 'opty_7eb50daadea7.hsaco',
     'how': {'opt_level': '-O1'},
     'key': 'chunk=32 groups=None max_live=125 ablate=None flush_unroll=4 '
            'waves=None store_aux=18 con_rows_per_wave=0 interleave=0',
     'label': '-O1',
     'meta': {},
     'notes': [],
     'pinned': '-O1',
     'refused': [('uniform_trig', {'opty_jac': 1}),
                 ('strips+2', {'opty_jac': 2}),
                 ('strips+4', {'opty_jac': 3}),
                 ('strips+1', {'opty_jac': 4}),
                 ('strips+6', {'opty_jac': 5}),
                 ('strips+8', {'opty_jac': 6}),
                 ('strips+12', {'opty_jac': 7}),
                 ('strips-2', {'opty_jac': 8}),
                 ('strips-4', {'opty_jac': 9}),
                 ('fast_trig', {'opty_jac': 10}),
                 ('chunk16', {'opty_jac': 11})],
     'run_form_refused': None,
     'warnings': 1},
    'alternative_None': {'batches': [{((), (), None)},
                 {(('fast_trig=2',), (), None),
                  (('fused_groups=10', 'groups=11'), (), None),
                  (('fused_groups=11', 'groups=12'), (), None),
                  (('fused_groups=13', 'groups=14'), (), None)},
                 {(('fused_groups=15', 'groups=16'), (), None),
                  (('fused_groups=17', 'groups=18'), (), None),
                  (('fused_groups=21', 'groups=22'), (), None),
                  (('fused_groups=7', 'groups=8'), (), None)},
                 {((), (), '-O1'),
                  (('chunk=16',), (), None),
                  (('fast_trig=1',), (), None),
                  (('fused_groups=5', 'groups=6'), (), None)},
                 {((),
                   ('-mllvm',
                    '-amdgpu-disable-unclustered-high-rp-reschedule'),
                   None)}],
     'pinned': None,
     'recorded': [],
     'shown': 13},
}


@pytest.mark.parametrize('scenario', SCENARIOS, ids=lambda f: f.__name__)
def test_ladder(scenario, monkeypatch, caplog):
    assert scenario(monkeypatch, caplog) == EXPECTED[scenario.__name__]


@pytest.mark.parametrize('accept', [0, 2, 5, 11, None])
def test_verified_alternative(accept, monkeypatch, caplog):
    assert alternative(monkeypatch, caplog, accept) == \
        EXPECTED['alternative_%s' % accept]


# --- the rungs that no small problem reaches: build_ladder's own functions --

def _geo(**kw):
    return dict(dict(con_waves=1, line_mode=True, jac=20, fused=18), **kw)


def test_strip_steps_and_phases():
    import types
    from opty_amd import build_ladder as bl
    opts = types.SimpleNamespace(con_split='work', con_attach=None, chunk=32,
                                 forget=0)
    nine = [1, 2, 3, 4, 5, 6, 8, 10, 12]
    assert bl.strip_steps(opts, _geo(), 'coo') == nine
    assert bl.strip_steps(opts, _geo(con_waves=2), 'coo') == [0] + nine
    opts.con_split = 'count'
    assert bl.strip_steps(opts, _geo(con_waves=2), 'coo') == nine
    assert bl.strip_steps(opts, _geo(line_mode=False), 'coo') == []
    assert bl.strip_steps(opts, _geo(line_mode=False), 'csr') == nine
    # constraint rows that ride in the Jacobian waves: a phase with them
    # detached (first the same cut), and they stay detached in the last one
    meta = dict(geometry=_geo(), con_attached=True)
    assert bl.phases(opts, meta, [0] + nine) == [
        (False, False, [0] + nine), (True, False, [0] + nine),
        (True, True, [0, 2, 4, 8])]
    assert bl.phases(opts, meta, nine)[1] == (True, False, [0] + nine)
    opts.con_attach = 1                 # the plan says so: not undone
    assert bl.phases(opts, meta, nine) == [
        (False, False, nine), (False, True, [0, 2, 4, 8])]
    # no 16-entry chunks for blocks that are not written by lines, that are
    # cut into other chunks already, or that drop their temporaries already
    for change in (dict(chunk=16), dict(forget=1)):
        assert bl.phases(types.SimpleNamespace(**dict(vars(opts), **change)),
                         meta, nine) == [(False, False, nine)]
    assert bl.phases(opts, dict(geometry=_geo(line_mode=False)), nine) == [
        (False, False, nine)]


def test_narrower_cuts():
    from opty_amd import build_ladder as bl
    from opty_amd.codegen.emit_hip import WORK_CUT_MAX_LIVE
    changes = lambda *a, **k: [c[1] for c in bl.narrower_cuts(*a, **k)]
    # only the strips of the kernels that spill are made narrower
    assert changes(_geo(), {'opty_jac': 2}, [0, 1, 3]) == [
        {}, dict(groups=21, fused_groups=18), dict(groups=23, fused_groups=18)]
    assert changes(_geo(), {'opty_conjac': 1, 'opty_jac': 2}, [12]) == [
        dict(groups=32, fused_groups=30)]
    assert changes(_geo(con_waves=3), {'opty_conjac': 1}, [0, 2]) == [
        dict(con_split='count'),
        dict(con_split='count', groups=20, fused_groups=20)]
    # a work-aware cut: a smaller register budget per arithmetic strip, never
    # below 40
    work = _geo(cut='work', jac=5, fused=5)
    assert changes(work, {'opty_jac': 2}, [0, 1, 2, 12, 99]) == [
        {}, dict(work_live=WORK_CUT_MAX_LIVE - 12),
        dict(work_live=WORK_CUT_MAX_LIVE - 24),
        dict(work_live=max(40, WORK_CUT_MAX_LIVE - 144)), dict(work_live=40)]
    assert changes(work, {'opty_jac': 2}, [0, 4], detach=True,
                   forget=True) == [
        dict(forget=1, chunk=16, con_attach=0),
        dict(forget=1, chunk=16, con_attach=0,
             work_live=WORK_CUT_MAX_LIVE - 48)]
    assert all(c[2] == {} for c in bl.narrower_cuts(work, {}, [0, 1]))


def test_parking_budgets():
    import types
    from opty_amd import build_ladder as bl
    budgets = lambda live: [c[1] for c in bl.parking_budgets(
        types.SimpleNamespace(park_live=live))]
    off = dict(park=0, fused_strips=None)
    assert budgets(200) == [dict(park_live=210), dict(park_live=190),
                            dict(park_live=180), dict(park_live=170), off]
    # (kept only while above 100)
    assert budgets(125) == [dict(park_live=135), dict(park_live=115),
                            dict(park_live=105), off]
    assert budgets(90) == [off]


def test_spilling_parked_plan_and_detach_phase(monkeypatch):
    """``build_ladder.spill_free`` with a stub printer: a parked plan that
    spills is replaced by the first clean budget in list order -- one whose
    waves need more than 40 KB of LDS comes after the others --, and the
    narrowing phases go on from the replacement when none is clean."""
    import types
    from opty_amd import build_ladder as bl
    lds, spilling = {}, {}

    def emit(o):
        key = ' '.join('%s=%s' % kv for kv in sorted(vars(o).items()))
        return '// stub\n// ' + key, dict(
            geometry=_geo(line_mode=False), con_attached=bool(o.park),
            kernels=dict(jac=dict(lds_bytes=lds.get(o.park_live, 1024))))
    built = []

    def compile(source, opt_level=None, extra_flags=()):
        built.append(source.splitlines()[1])
        return source.splitlines()[1]
    monkeypatch.setattr(hb, 'vgpr_spills', lambda hsaco, kernels=FULL: dict(
        spilling.get(hsaco.split('park_live=')[1].split()[0] +
                     ('d' if 'con_attach=0' in hsaco else ''), {})))
    trials = bl.TrialBuilder(emit, compile)
    opts = types.SimpleNamespace(park=1, park_live=130, fused_strips=4,
                                 con_split='work', con_attach=None, chunk=32,
                                 forget=0)
    spilling.update({'130': {'opty_jac': 4}, '140': {}, '120': {},
                     '110': {'opty_jac': 1}})
    lds[140] = 48*1024
    best = bl.spill_free(trials, trials.build(opts), 'coo')
    # (140 is clean and first, but costs resident waves: 120 is used)
    assert best.options.park_live == 120 and best.options.park == 1
    assert len(built) == 1 + 4 and len(set(built)) == 5
    assert [b for b in built if 'park=0' in b and 'fused_strips=None' in b]
    # nothing clean: the plan stays (not the less-spilling budget), and its
    # constraint rows are detached -- the only phase such a block has
    del built[:]
    spilling.update({'140': {'opty_jac': 3}, '120': {'opty_jac': 2},
                     '130d': {}})
    first = trials.build(opts)
    best = bl.spill_free(trials, first, 'coo')
    assert best.options.park_live == 130 and best.options.con_attach == 0
    assert not best.spills and len(built) == 1 + 4 + 1


def test_static_gate_reports_tool_failures(monkeypatch):
    from opty_amd import build_ladder as bl
    asked = []
    monkeypatch.setattr(hb, 'vgpr_spills', lambda hsaco, kernels=FULL: {
        k: 2 for k in kernels if k == 'opty_jac_var' and 'spills' in hsaco})

    def copies(hsaco, names):
        asked.append(list(names))
        if 'broken' in hsaco:
            raise OSError('no llvm-objdump')
        return {k: 1 for k in names if k == 'opty_jac' and 'hit' in hsaco}
    monkeypatch.setattr(isa_check, 'exec_copies', copies)
    gate = bl.static_gate('spills.hsaco', VAR)
    assert gate.refusal() == "vector spills: {'opty_jac_var': 2}"
    assert not gate.clean and asked == []   # spills: no look at the ISA
    gate = bl.static_gate('hit.hsaco', FULL)
    assert gate.copies == {'opty_jac': 1} and not gate.clean
    assert gate.refusal() == "static ISA check: {'opty_jac': 1}"
    # a banned kernel is not looked at
    gate = bl.static_gate('hit.hsaco', FULL, ignore={'opty_jac'})
    assert asked[-1] == ['opty_con', 'opty_conjac']
    assert gate.clean and gate.refusal() is None
    gate = bl.static_gate('broken.hsaco', VAR)
    assert isinstance(gate.error, OSError) and not gate.clean
    assert gate.refusal() == \
        "static ISA check: {'isa_check': 'no llvm-objdump'}"


def test_derived_modules_halve_the_budget_then_forget(monkeypatch):
    from opty_amd import build_ladder as bl
    clean_at, copies_in = [None], []
    emit = lambda prog, budget, forget, fast_trig: (
        '%d %d %d' % (budget, forget, fast_trig), 'cut %d' % budget)
    compile = lambda source, opt_level=None, extra_flags=(): source
    monkeypatch.setattr(hb, 'vgpr_spills', lambda hsaco, kernels: (
        {} if hsaco.startswith(str(clean_at[0])) else {kernels[0]: 7}))
    monkeypatch.setattr(isa_check, 'exec_copies', lambda hsaco, names: {
        names[0]: 1} if hsaco in copies_in else {})
    names = ('opty_hess', 'opty_hess_inst')
    build = lambda: bl.spill_free_module(emit, None, compile, names, 1500)
    hsaco, cut, meta = build()
    assert hsaco is None and [t[:2] for t in meta['tried']] == [
        (1500, False), (750, False), (375, False), (187, False),
        (187, True), (187, True)]
    clean_at[0] = '187 1'
    assert build() == ('187 1 1', 'cut 187', dict(
        strip_ops=187, forget=True, isa_exec_copies={}))
    # EXEC copies: the uniform-sincos sibling when it is clean ...
    clean_at[0], copies_in = 750, ['750 0 1']
    assert build() == ('750 0 2', 'cut 750', dict(
        strip_ops=750, forget=False, isa_exec_copies={}))
    # ... the first build when it is not
    copies_in.append('750 0 2')
    assert build() == ('750 0 1', 'cut 750', dict(
        strip_ops=750, forget=False, isa_exec_copies={'opty_hess': 1}))
