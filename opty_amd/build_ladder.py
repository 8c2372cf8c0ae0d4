"""The build ladder: which code object a problem runs on.  Host only -- emit,
``hipcc``, read the spill counts, run the static ISA check, pick.  hipcc's
faults at the register limit are erratic in the cut, so a
build whose kernels spill vector registers, or carry the EXEC-copy pattern of
:mod:`opty_amd.isa_check`, is replaced by a neighbouring one.

Here is what needs no collocator: one record of a built candidate, one trial
builder, one static gate, the rungs as functions that return candidates
``(label, option changes, hipcc switches)``, and the loops over them.
``ConstraintCollocator`` decides what a verdict means (a ban, a refusal, a
warning) and holds every build to the referee.  ``hb.compile_module``,
``hb.vgpr_spills`` and ``isa_check.exec_copies`` are looked up when they are
called: tests replace them.
"""
import collections
import concurrent.futures
import copy
import logging
import subprocess
import types

from . import hip_backend as hb
from . import isa_check
from .codegen.emit_hip import WORK_CUT_MAX_LIVE

logger = logging.getLogger(__name__)

#: One built candidate: the code object, the printer's ``meta``, ``{kernel:
#: spilled vector registers}``, the printed source, the printer options and
#: the hipcc switches ``{'opt_level': ..., 'extra_flags': ...}`` (either may
#: be missing).
Build = collections.namedtuple('Build',
                               'hsaco meta spills source options how')


class TrialBuilder(object):
    """Builds candidates from ``emit(options) -> (source, meta)`` and
    ``compile(source, opt_level=, extra_flags=) -> hsaco``; the spills read
    are those of ``kernels`` (None: the three full kernels)."""

    def __init__(self, emit, compile, kernels=None):
        self.emit, self.compile, self.kernels = emit, compile, kernels

    def build(self, base, changes=None, how=None):
        """``base`` with the attributes ``changes`` set, compiled with the
        hipcc switches ``how``."""
        opts, how = copy.copy(base), dict(how or {})
        for k, v in (changes or {}).items():
            setattr(opts, k, v)
        source, meta = self.emit(opts)
        hsaco = self.compile(source, opt_level=how.get('opt_level'),
                             extra_flags=tuple(how.get('extra_flags', ())))
        spills = hb.vgpr_spills(hsaco) if self.kernels is None else \
            hb.vgpr_spills(hsaco, self.kernels)
        return Build(hsaco, meta, spills, source, opts, how)

    def build_all(self, base, candidates):
        """The builds of ``[(label, changes, how)]``, in that order; ALL are
        compiled, side by side (which files a build leaves in the cache
        depends on that)."""
        with concurrent.futures.ThreadPoolExecutor(len(candidates)) as pool:
            return list(pool.map(
                lambda cand: self.build(base, cand[1], cand[2]), candidates))


class Gate(collections.namedtuple('Gate', 'spills copies error')):
    """Verdict of :func:`static_gate`: ``{kernel: spilled vector
    registers}``, ``{kernel: EXEC copies}`` (None when the kernels spill or
    the check failed) and the tools' exception, if any."""

    @property
    def clean(self):
        return not self.spills and not self.copies and self.error is None

    def refusal(self):
        """Why an EXTRA (the restricted kernels, their run form) that fails
        the gate is left out -- a check that could not be made counts as a
        hit --, or None."""
        if self.spills:
            return 'vector spills: %s' % (self.spills,)
        if self.error is not None:
            return 'static ISA check: %s' % ({'isa_check': str(self.error)},)
        if self.copies:
            return 'static ISA check: %s' % (dict(self.copies),)
        return None


def static_gate(hsaco, names, ignore=(), spills=None):
    """The static gate of the kernels ``names`` (without those in ``ignore``:
    banned kernels are never launched) of a code object: vector spills?
    Otherwise EXEC copies (``isa_check.exec_copies``)?  ``spills``: what the
    caller has read and judged already (only the copies are looked for)."""
    names = [k for k in names if k not in ignore]
    if spills is None:
        spills = hb.vgpr_spills(hsaco, tuple(names))
        if spills:
            return Gate(spills, None, None)
    try:
        return Gate(spills, isa_check.exec_copies(hsaco, names), None)
    except (OSError, subprocess.SubprocessError) as err:
        return Gate(spills, None, err)


def _spilled(build):
    return sum(build.spills.values())


def pick(best, built):
    """The first spill-free build of a batch IN ITS ORDER; otherwise
    ``best``, or the least-spilling of the batch when it spills strictly
    less."""
    clean = [b for b in built if not b.spills]
    if clean:
        return clean[0]
    least = min(built, key=_spilled)
    return least if _spilled(least) < _spilled(best) else best


# --- the rungs ------------------------------------------------------------

def strip_steps(opts, geo, layout):
    """By how much the narrowing phases change the cut: 0 is the constraint
    rows re-cut by count alone; a step ``d`` adds ``d`` strips (work-aware
    cut: takes 12 ``d`` registers off the strips' budget)."""
    steps = []
    if geo['con_waves'] > 1 and opts.con_split == 'work':
        steps.append(0)
    if geo['line_mode'] or layout == 'csr':
        # (row-sorted blocks are cut at row starts: any count up to M)
        steps += [1, 2, 3, 4, 5, 6, 8, 10, 12]
    return steps


def phases(opts, meta, steps):
    """``[(detach, forget, steps)]``: the cuts as they are; then with the
    constraint rows back in waves of their own (the Jacobian waves they rode
    in -- arithmetic-bound blocks, ``emit_hip._attach_constraint_rows`` --
    get their registers back); then in 16-entry chunks whose temporaries are
    dropped at every chunk boundary (what the chunks share is evaluated
    again, the live values of a wave are those of 16 entries: the midpoint
    rule of the muscle-driven leg spills 24 registers at every cut
    otherwise, none this way)."""
    geo = meta['geometry']
    out = [(False, False, list(steps))]
    detachable = bool(meta.get('con_attached')) and opts.con_attach is None
    if detachable:
        out.append((True, False, [0] + [d for d in steps if d]))
    if geo['line_mode'] and opts.chunk == 32 and not opts.forget:
        out.append((detachable, True, [0, 2, 4, 8]))
    return out


def narrower_cuts(geo, spills, steps, detach=False, forget=False):
    """The candidates of the steps ``steps`` of a phase.  ``geo``: the
    geometry the steps count from; ``spills``: of the best build so far --
    only the strips of a kernel that spills are made narrower."""
    out = []
    for d in steps:
        changes = {}
        if geo['con_waves'] > 1:
            changes['con_split'] = 'count'
        if forget:
            changes.update(forget=1, chunk=16)
        if detach:
            changes['con_attach'] = 0
        if d and geo.get('cut') == 'work':
            # more strips would only split the store-only part of a
            # work-aware cut: its arithmetic strips get a smaller register
            # budget instead (the strip count follows)
            changes['work_live'] = max(40, WORK_CUT_MAX_LIVE - 12*d)
        elif d:
            changes['groups'] = geo['jac'] + (d if 'opty_jac' in spills
                                              else 0)
            changes['fused_groups'] = geo['fused'] + (
                d if 'opty_conjac' in spills else 0)
        out.append(('cut%+d' % d, changes, {}))
    return out


def parking_budgets(opts):
    """A planned wave (LDS parking) that spills: other register budgets of
    the plan -- where spills appear is erratic --, then the same options
    without the merged strips / parking."""
    return [('park_live=%d' % (opts.park_live + d),
             dict(park_live=opts.park_live + d), {})
            for d in (10, -10, -20, -30) if opts.park_live + d > 100] + \
        [('no parking', dict(park=0, fused_strips=None), {})]


def neighbours(base, geo, layout):
    """The builds tried after the referee refused one, in the order of their
    expected cost (r05): the same geometry with ``fast_trig=2``; strips +2,
    +4, +1, +6 ...; ``fast_trig=1``; 16-entry chunks; then the same source
    through ``-O1`` and without the pre-RA scheduler stage of round 3."""
    cands = []
    # (an explicit strip count is an even cut unless the work-aware one is
    # asked for: the neighbours of a work-aware cut are work-aware)
    keep = dict(cut='work') if geo.get('cut') == 'work' else {}
    if base.fast_trig != 2:
        # first the SAME geometry with sincos behind a wave-uniform test: the
        # one fault that is understood (profiles/r05_exec_fault.txt) sits in
        # the if / else of the inlined library sincos, and the plan's
        # measured geometry stays
        cands.append(('uniform_trig', dict(fast_trig=2), {}))
    if geo['line_mode'] or layout == 'csr':
        for d in (2, 4, 1, 6, 8, 12, -2, -4):
            if min(geo['jac'], geo['fused']) + d >= 1:
                cands.append(('strips%+d' % d, dict(
                    keep, groups=geo['jac'] + d,
                    fused_groups=geo['fused'] + d), {}))
    if not base.fast_trig:
        cands.append(('fast_trig', dict(fast_trig=1), {}))
    if geo['line_mode'] and base.chunk == 32:
        cands.append(('chunk16', dict(chunk=16), {}))
    return cands + [('-O1', {}, dict(opt_level='-O1')),
                    ('no-hp-reschedule', {},
                     dict(extra_flags=list(hb.SAFE_SCHEDULER_FLAGS)))]


def batches(todo, size=4):
    """``todo`` in the pieces that are compiled side by side."""
    return [todo[i:i + size] for i in range(0, len(todo), size)]


# --- the loops ------------------------------------------------------------

def spill_free(trials, best, layout):
    """The build to use in the place of ``best`` (the printer's choice,
    built): itself when it does not spill; otherwise the first spill-free one
    of the rungs above -- a few candidates at a time, where spills appear is
    erratic in the cut (24-link stand-in, fused strips 18 ... 28: only 20, 25
    and 28 are spill-free) --, or the least-spilling build met."""
    opts, meta = best.options, best.meta
    how = best.how
    steps = strip_steps(opts, meta['geometry'], layout)
    if opts.park and best.spills:
        cands = parking_budgets(opts)
        logger.info('kernels %s of a plan with LDS parking spill vector '
                    'registers: other register budgets %s', sorted(
                        best.spills), [c[0] for c in cands])
        clean = [b for b in trials.build_all(
            opts, [(c[0], c[1], how) for c in cands]) if not b.spills]
        # (a plan that needs more than a quarter of a CU's LDS per wave
        # costs resident waves: the unmerged fallback comes before it)
        clean.sort(key=lambda b: max(
            k['lds_bytes'] for k in b.meta['kernels'].values()) > 40*1024)
        if clean:
            best = clean[0]
            opts, meta = best.options, best.meta
    geo = meta['geometry']
    for detach, forget, todo in phases(opts, meta, steps):
        for batch in batches(todo):
            if not best.spills:
                break
            logger.info('kernels %s spill vector registers: rebuilding with '
                        'narrower cuts %s%s%s', sorted(best.spills), batch,
                        ', constraint rows detached' if detach else '',
                        ', temporaries dropped per chunk' if forget else '')
            best = pick(best, trials.build_all(opts, [
                (c[0], c[1], how) for c in narrower_cuts(
                    geo, best.spills, batch, detach, forget)]))
    return best


def spill_free_module(emit, prog, compile, names, budget):
    """``(hsaco, cut(s), meta)`` of a derived program's module, from
    ``emit(prog, budget, forget, fast_trig) -> (source, cut(s))``: the first
    build whose kernels ``names`` spill no vector register (the strip budget
    halved down to 200, then ``forget``; six tries), through the static ISA
    check (a hit: the uniform-sincos sibling is built in its place when it is
    clean; one that cannot be checked is no better).  ``hsaco`` is None and
    ``meta['tried']`` lists the builds when every one of them spills."""
    trials = TrialBuilder(
        lambda o: emit(prog, o.budget, o.forget, o.fast_trig), compile, names)
    opts = types.SimpleNamespace(budget=budget, forget=False, fast_trig=1)
    tried = []
    for _ in range(6):
        build = trials.build(opts)
        tried.append((opts.budget, opts.forget, build.spills))
        if not build.spills:
            break
        if opts.budget > 200:
            opts.budget //= 2
        else:
            opts.forget = True
    else:
        return None, None, dict(tried=tried)
    gate = static_gate(build.hsaco, names, spills=build.spills)
    if gate.error is not None:
        raise gate.error
    if gate.copies:
        twin = trials.build(build.options, dict(fast_trig=2))
        if not twin.spills:
            twin_gate = static_gate(twin.hsaco, names, spills=twin.spills)
            if twin_gate.clean:
                build, gate = twin, twin_gate
    return build.hsaco, build.meta, dict(
        strip_ops=build.options.budget, forget=build.options.forget,
        isa_exec_copies=gate.copies)
