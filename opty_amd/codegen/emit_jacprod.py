"""HIP source of a Jacobian-product program
(:func:`program.build_jacobian_product_program`): ``J(free) v`` and
``J(free)^T w`` without the matrix.

``opty_jvp``: lane = constraint node, one 64-node block per ``blockIdx.x``;
the M tangent roots are cut into strips (``blockIdx.y``).  Per-node inputs are
coalesced loads of the ``free`` / known-trajectory rows and of the same rows
of ``v``; the tail scalars of ``v`` are scalar loads.  Equation ``j`` of node
``i`` is stored to ``out[j*(N-1) + i]``: one 512-byte segment per wave.

``opty_jvp_inst``: one lane, ``out[M*(N-1) + k] = sum_a dinst_k/datom_a
v[idx_a]``.

``opty_vjp``: lane = constraint node, the C adjoint roots.  The entry ``p`` of
``free`` row ``R`` is ``lo_R(i = p) + hi_R(i = p - 1)`` (``lo`` / ``hi``: the
adjoint columns of the row with time offset 0 / 1), the missing term dropped
at the two ends.  Consecutive blocks OVERLAP by one constraint node (block
``b`` holds the nodes ``63 b .. 63 b + 63``): lane ``l >= 1`` writes entry
``63 b + l`` from its own ``lo`` and lane ``l - 1``'s ``hi`` (handed over
through LDS), lane 0 only hands over -- except in block 0, where it writes
entry 0.  Every entry is written exactly once, by one lane, as one sum of two
terms: no atomics, the same bits in every call.  The tail columns (unknown
parameters, a free ``h``) are sums over all constraint nodes: a fixed
butterfly over the wave (the duplicated lane 0 of a block ``b > 0`` counts as
zero), one partial per block and column.

``opty_vjp_fin``: one wave, after ``opty_vjp`` on the same stream: sums the
block partials in a fixed order into the tail of the result, then lane 0 adds
the instance constraints' ``w[M*(N-1) + k] dinst_k/datom_a`` to ``g[idx_a]``
one after the other.
"""

from . import ir
from .emit_hip import _Body, _UNIFORM_TRIG_HELPERS

#: parameter list of the four kernels; mirrored by ``struct JacprodArgs`` in
#: ``csrc/jacprod.cpp``.  ``vec``: ``v`` (jvp) or ``w`` (vjp); ``part``: the
#: block partials of the tail columns, ``part[t*gridDim.x + block]``
JACPROD_PARAMS = (
    'const double *__restrict__ free_, const double *__restrict__ known_traj, '
    'const double *__restrict__ params, const double *__restrict__ vec, '
    'const long long *__restrict__ inst_idx, double *__restrict__ out, '
    'double *__restrict__ part, double h, long long N')

#: constraint nodes a block of ``opty_vjp`` advances by (64 lanes, one shared)
VJP_STRIDE = 63

_REDUCE = '''\
// Sum over the wave in a fixed order (the same tree in every call); the
// result is in lane 0.
__device__ __forceinline__ double opty_wave_sum(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s, 64);
    return x;
}
'''


def _cut(dag, units, budget):
    """Cut of ``units`` (each a list of root nodes) into strips ``[(u0,
    u1)]``: consecutive units until the operations they add pass
    ``budget``."""
    out, start, seen, cost = [], 0, set(), 0
    for u, roots in enumerate(units):
        reach = dag.reachable(roots)
        new = [i for i in reach if i not in seen]
        add = sum(1 for i in new if dag.op[i] not in (ir.CONST, ir.INPUT))
        if u > start and cost + add > budget:
            out.append((start, u))
            start, seen, cost = u, set(), 0
            new = reach
            add = sum(1 for i in new if dag.op[i] not in (ir.CONST, ir.INPUT))
        seen.update(new)
        cost += add
    if units:
        out.append((start, len(units)))
    return out


def _scalar(prog, kind, k):
    tail = '[%dLL*N + %%d]' % (prog.n + prog.q)
    if kind == 'par':
        src, idx = prog.pars[k]
        return ('params[%d]' % idx) if src == 'known' else \
            'free_' + tail % idx
    if kind == 'h':
        return 'h' if prog.h[0] == 'fixed' else 'free_' + tail % prog.h[1]
    if kind == 'vpar':
        src, idx = prog.pars[k]
        assert src == 'tail', (kind, k)
        return 'vec' + tail % idx
    if kind == 'vh':
        assert prog.h[0] == 'tail'
        return 'vec' + tail % prog.h[1]
    if kind == 'free':
        return 'free_[inst_idx[%d]]' % k
    raise AssertionError(kind)


def _node_leaf(prog):
    dag = prog.dag

    def leaf(i):
        if dag.op[i] != ir.INPUT:
            return None
        kind, k = dag.args[i]
        if kind in ('cur', 'adj', 'vcur', 'vadj'):
            src, idx = prog.rows[k]
            off = prog.cur_offset if kind.endswith('cur') else prog.adj_offset
            if kind[0] == 'v':
                assert src == 'free', (kind, k)
                base = 'vec'
            else:
                base = 'free_' if src == 'free' else 'known_traj'
            return '%s[%dLL*N + ic + %d]' % (base, idx, off)
        if kind == 'lam':
            return 'vec[%dLL*ncn + ic]' % k
        return _scalar(prog, kind, k)
    return leaf


def _strip_switch(lines, bodies):
    lines.append('switch (blockIdx.y) {')
    for s, body in enumerate(bodies):
        lines.append('case %d: {' % s)
        lines += ['    ' + ln for ln in body]
        lines += ['    break;', '}']
    lines += ['default: break;', '}']


def _kernel(name, lines):
    return (['extern "C" __global__ void __launch_bounds__(64)',
             '%s(%s)' % (name, JACPROD_PARAMS), '{'] +
            ['    ' + ln for ln in lines] + ['}', ''])


def vjp_units(prog):
    """The units ``opty_vjp`` is cut along: ``('row', R, lo, hi)`` per
    ``free`` trajectory row (both columns of a row stay in one strip), then
    ``('tail', t, k)`` per tail column, ``t`` its position in the partials."""
    units = [('row',) + rc for rc in prog.row_columns()]
    units += [('tail', t, k) for t, (_, k) in enumerate(prog.tail_columns())]
    return units


def emit_jacprod_module(prog, budget=1500, forget=False, fast_trig=1):
    """``(source, (jvp strips, vjp strips))`` of the module.  ``budget``:
    operations per strip; ``forget``: every unit of a strip computes what it
    needs afresh; ``fast_trig`` as ``EmitOptions.fast_trig``."""
    dag = prog.dag
    leaf = _node_leaf(prog)
    M = prog.M
    src = ['// generated by opty_amd.codegen.emit_jacprod -- do not edit',
           '#include "opty_device.h"', '']
    if fast_trig == 2:
        src.append(_UNIFORM_TRIG_HELPERS)
    src.append(_REDUCE)

    # ---- opty_jvp -----------------------------------------------------
    jcut = _cut(dag, [[node] for node in prog.tan_out], budget)
    lines = ['const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long i = (long long)blockIdx.x*64 + lane;',
             'if ((long long)blockIdx.x*64 >= ncn) return;',
             'const long long ic = i < ncn ? i : ncn - 1;']
    bodies = []
    for j0, j1 in jcut:
        body = _Body(dag, set(dag.reachable(prog.tan_out[j0:j1])), leaf,
                     fast_trig)
        for j in range(j0, j1):
            if forget and j > j0:
                body.new_scope()
                body.forget()
            else:
                body.begin_entry()
            ref = body.emit(prog.tan_out[j])
            body.lines.append('if (i < ncn) out[%dLL*ncn + i] = %s;'
                              % (j, ref))
        body.end_scope()
        bodies.append(body.lines)
    _strip_switch(lines, bodies)
    src += _kernel('opty_jvp', lines)

    # ---- opty_jvp_inst --------------------------------------------------
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)),
                 lambda i: _scalar(prog, *dag.args[i])
                 if dag.op[i] == ir.INPUT else None, fast_trig)
    lines = ['if (threadIdx.x != 0 || blockIdx.x != 0) return;',
             'const long long ncn = N - 1;']
    for k in range(prog.num_inst):
        terms = [(t, a) for t, (kk, a) in enumerate(prog.inst_pairs)
                 if kk == k]
        body.lines.append('double acc%d = 0.0;' % k)
        for t, a in terms:
            ref = body.emit(prog.inst_jac_out[t])
            body.lines.append('acc%d += %s*vec[inst_idx[%d]];' % (k, ref, a))
        body.lines.append('out[%dLL*ncn + %d] = acc%d;' % (M, k, k))
        body.end_scope()
    src += _kernel('opty_jvp_inst', lines + body.lines)

    # ---- opty_vjp ---------------------------------------------------------
    units = vjp_units(prog)

    def roots_of(unit):
        if unit[0] == 'row':
            return [prog.adj_out[k] for k in unit[2:] if k is not None]
        return [prog.adj_out[unit[2]]]
    vcut = _cut(dag, [roots_of(u) for u in units], budget)
    lines = ['__shared__ double ex[2*64];',
             'const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long i0 = (long long)blockIdx.x*%d;' % VJP_STRIDE,
             'if (i0 >= ncn) return;',
             'const long long i = i0 + lane;',
             'const long long ic = i < ncn ? i : ncn - 1;',
             '// this lane evaluates a constraint node of its own',
             'const bool valid = i < ncn;',
             '// ... that no other block counts (lane 0 repeats the last '
             'lane of the previous block)',
             'const bool counted = valid && (lane > 0 || blockIdx.x == 0);',
             '// entry i of a row is this lane\'s to write',
             'const bool writer = i < N && (lane > 0 || blockIdx.x == 0);']
    bodies = []
    for u0, u1 in vcut:
        needed = set()
        for u in units[u0:u1]:
            needed |= set(dag.reachable(roots_of(u)))
        body = _Body(dag, needed, leaf, fast_trig)
        handovers = 0
        for pos, u in enumerate(units[u0:u1]):
            if forget and pos > 0:
                body.new_scope()
                body.forget()
            else:
                body.begin_entry()
            if u[0] == 'row':
                _, R, lo, hi = u
                dst = 'out[%dLL*N + i]' % R
                hi_ref = body.emit(prog.adj_out[hi]) if hi is not None \
                    else None
                if hi_ref is not None and forget:
                    # hand the upper term over first, then start afresh:
                    # the two columns of a row are not live together
                    body.lines.append('const double hi%d = %s;' % (R, hi_ref))
                    hi_ref = 'hi%d' % R
                    body.new_scope()
                    body.forget()
                lo_ref = body.emit(prog.adj_out[lo]) if lo is not None \
                    else '0.0'
                if hi_ref is None:
                    body.lines.append('if (writer) %s = valid ? %s : 0.0;'
                                      % (dst, lo_ref))
                    continue
                # two buffers in turn: one wave-level ordering point per
                # row is enough (the reads of row r precede the point of row
                # r + 1, the writes of row r + 2 follow it)
                buf = 'ex + %d' % (64*(handovers & 1))
                handovers += 1
                body.lines += [
                    '(%s)[lane] = %s;' % (buf, hi_ref),
                    'opty_wave_sync();',
                    '{',
                    '    const double up = (%s)[lane > 0 ? lane - 1 : 0];'
                    % buf,
                    '    if (writer) %s = lane == 0 ? %s : '
                    '(valid ? %s + up : up);' % (dst, lo_ref, lo_ref),
                    '}']
            else:
                _, t, k = u
                ref = body.emit(prog.adj_out[k])
                body.lines += [
                    '{',
                    '    const double sum = opty_wave_sum(counted ? %s : 0.0);'
                    % ref,
                    '    if (lane == 0) part[%dLL*gridDim.x + blockIdx.x] = '
                    'sum;' % t,
                    '}']
        body.end_scope()
        bodies.append(body.lines)
    _strip_switch(lines, bodies)
    src += _kernel('opty_vjp', lines)

    # ---- opty_vjp_fin -------------------------------------------------------
    T = len(prog.tail_columns())
    tail0 = '%dLL*N' % (prog.n + prog.q)
    lines = ['if (blockIdx.x != 0) return;',
             'const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long nblk = (ncn + %d)/%d;'
             % (VJP_STRIDE - 1, VJP_STRIDE),
             '(void)ncn; (void)nblk;']
    for t, (j, _) in enumerate(prog.tail_columns()):
        lines += ['{',
                  '    double acc = 0.0;',
                  '    for (long long b = lane; b < nblk; b += 64) '
                  'acc += part[%dLL*nblk + b];' % t,
                  '    acc = opty_wave_sum(acc);',
                  '    if (lane == 0) out[%s + %d] = acc;' % (tail0, j),
                  '}']
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)),
                 lambda i: _scalar(prog, *dag.args[i])
                 if dag.op[i] == ir.INPUT else None, fast_trig)
    for t, (k, a) in enumerate(prog.inst_pairs):
        ref = body.emit(prog.inst_jac_out[t])
        body.lines.append('out[inst_idx[%d]] += vec[%dLL*ncn + %d]*%s;'
                          % (a, M, k, ref))
    body.end_scope()
    if body.lines:
        lines += ['if (lane == 0) {'] + ['    ' + ln for ln in body.lines] + \
            ['}']
    assert T == prog.r + prog.s, (T, prog.r, prog.s)
    src += _kernel('opty_vjp_fin', lines)
    return '\n'.join(src), (jcut, vcut)
