"""HIP source of a Jacobian-product program
(:func:`program.build_jacobian_product_program`): ``J(free) v`` and
``J(free)^T w`` without the matrix.

The four kernels evaluate a WINDOW ``[wa, wb)`` of the constraint nodes of
the global problem (a rank's share of a node-sharded problem; ``[0, N-1)`` is
the whole problem): every load is from the GLOBAL ``free`` / ``v`` / ``w`` /
known rows, the results go to ``out`` with row stride ``ostride`` and origin
``wa`` (``ostride = N-1`` resp. ``N`` with ``out = global + wa`` writes in
place, a smaller stride gives a dense block).  The window is wave-uniform: it
costs scalar registers only, and a lane computes what it computes in the
whole-problem launch.

``opty_jvp``: lane = constraint node ``wa + 64 blockIdx.x + lane``; the M
tangent roots are cut into strips (``blockIdx.y``).  Per-node inputs are
coalesced loads of the ``free`` / known-trajectory rows and of the same rows
of ``v``; the tail scalars of ``v`` are scalar loads.  Equation ``j`` of node
``i`` is stored to ``out[j*ostride + (i - wa)]``: one 512-byte segment per
wave.

``opty_jvp_inst``: one lane, ``tail[k] = sum_a dinst_k/datom_a v[idx_a]``
(``tail``: the ``o`` instance rows, ``out + M*(N-1)`` of the whole vector).

``opty_vjp``: lane = constraint node, the C adjoint roots.  The entry ``p`` of
``free`` row ``R`` is ``lo_R(i = p) + hi_R(i = p - 1)`` (``lo`` / ``hi``: the
adjoint columns of the row with time offset 0 / 1), the missing term dropped
at the two ends.  A window OWNS the time nodes ``p`` in ``[wa, wb)`` and, when
``wb == N - 1``, also ``p = N - 1``; entry ``p`` goes to ``out[R*ostride + (p
- wa)]``.  Consecutive blocks OVERLAP by one constraint node (block ``b``
holds the nodes ``i0 + 63 b .. i0 + 63 b + 63``, ``i0 = wa`` for ``wa == 0``
and the halo node ``wa - 1`` otherwise): lane ``l >= 1`` writes its entry from
its own ``lo`` and lane ``l - 1``'s ``hi`` (handed over through LDS), lane 0
only hands over -- except in block 0 of a window that starts at node 0, where
it writes entry 0.  Every owned entry is written exactly once, by one lane, as
one sum of two terms -- the same two terms whatever the window: no atomics,
the same bits in every call and for every partition.  The tail columns
(unknown parameters, a free ``h``) are sums over the window's constraint
nodes: a fixed butterfly over the wave (lane 0 of a block that only hands over
counts as zero), one partial per block and column.

``opty_vjp_fin``: one wave, after ``opty_vjp`` on the same stream: sums the
window's block partials in a fixed order into the ``r + s`` doubles ``tail``
(the tail of the result for the whole problem), then lane 0 adds the instance
constraints' ``w[M*(N-1) + k] dinst_k/datom_a``, one after the other in pair
order, to the entries of the atoms whose time node the window owns.

Block products (:func:`emit_jacprod_block_module`, a module of its own):
``opty_jvp_block`` / ``opty_jvp_block_inst`` / ``opty_vjp_block`` /
``opty_vjp_block_fin`` are the four kernels above for the K columns of a
:class:`program.JacobianBlockProductProgram` in one pass -- the same geometry,
a strip unit holds all K columns of an equation / of a ``free`` row, so what
does not depend on the column is evaluated once per strip.
"""

from .emit_hip import _Body, _UNIFORM_TRIG_HELPERS
from .emit_strips import (block_preamble, column_leaf, cut, kernel, node_leaf,
                          scalar, scalar_leaf, strip_switch)


def vjp_window_blocks(wa, wb, N):
    """Blocks ``opty_vjp`` is launched with for the window ``[wa, wb)`` of an
    ``N``-node problem (``opty_vjp_fin`` and ``csrc/jacprod.cpp`` compute the
    same): the first block of a window that starts at node 0 writes 64
    entries, every other block 63."""
    pend = wb + (1 if wb == N - 1 else 0)
    span = pend - wa - (1 if wa == 0 else 0)
    return (span + VJP_STRIDE - 1)//VJP_STRIDE if span > 0 else 1

#: what the single and the block kernels share.  ``vec``: ``v`` (jvp) or ``w``
#: (vjp); ``part``: the block partials of the tail columns,
#: ``part[t*gridDim.x + block]``
_SHARED_PARAMS = (
    'const double *__restrict__ free_, const double *__restrict__ known_traj, '
    'const double *__restrict__ params, const double *__restrict__ vec, '
    'const long long *__restrict__ inst_idx, double *__restrict__ out, '
    'double *__restrict__ part, double h, long long N')

#: parameter list of the four kernels; mirrored by ``struct JacprodArgs`` in
#: ``csrc/jacprod.cpp``.  ``[wa, wb)``: the window of constraint nodes;
#: ``ostride``: row stride of ``out``, whose first column is node ``wa``;
#: ``tail``: the ``o`` instance rows (``opty_jvp_inst``) or the ``r + s`` tail
#: sums (``opty_vjp_fin``)
JACPROD_PARAMS = _SHARED_PARAMS + (
    ', long long wa, long long wb, long long ostride, '
    'double *__restrict__ tail')

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
    leaf = node_leaf(prog)
    M = prog.M
    src = ['// generated by opty_amd.codegen.emit_jacprod -- do not edit',
           '#include "opty_device.h"', '']
    if fast_trig == 2:
        src.append(_UNIFORM_TRIG_HELPERS)
    src.append(_REDUCE)

    # ---- opty_jvp -----------------------------------------------------
    jcut = cut(dag, [[node] for node in prog.tan_out], budget)
    lines = ['const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long i0 = wa + (long long)blockIdx.x*64;',
             'if (i0 >= wb) return;',
             'const long long i = i0 + lane;',
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
            body.lines.append('if (i < wb) out[%dLL*ostride + (i - wa)] = '
                              '%s;' % (j, ref))
        body.end_scope()
        bodies.append(body.lines)
    strip_switch(lines, bodies)
    src += kernel('opty_jvp', JACPROD_PARAMS, lines)

    # ---- opty_jvp_inst --------------------------------------------------
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)),
                 scalar_leaf(prog), fast_trig)
    lines = ['if (threadIdx.x != 0 || blockIdx.x != 0) return;']
    for k in range(prog.num_inst):
        terms = [(t, a) for t, (kk, a) in enumerate(prog.inst_pairs)
                 if kk == k]
        body.lines.append('double acc%d = 0.0;' % k)
        for t, a in terms:
            ref = body.emit(prog.inst_jac_out[t])
            body.lines.append('acc%d += %s*vec[inst_idx[%d]];' % (k, ref, a))
        body.lines.append('tail[%d] = acc%d;' % (k, k))
        body.end_scope()
    src += kernel('opty_jvp_inst', JACPROD_PARAMS, lines + body.lines)

    # ---- opty_vjp ---------------------------------------------------------
    units = vjp_units(prog)

    def roots_of(unit):
        if unit[0] == 'row':
            return [prog.adj_out[k] for k in unit[2:] if k is not None]
        return [prog.adj_out[unit[2]]]
    vcut = cut(dag, [roots_of(u) for u in units], budget)
    lines = ['__shared__ double ex[2*64];',
             'const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             '// a window that does not start the trajectory evaluates the '
             'node before it for its upper terms',
             'const long long i0 = wa - (wa > 0 ? 1 : 0) + '
             '(long long)blockIdx.x*%d;' % VJP_STRIDE,
             'if (i0 >= wb) return;',
             'const long long i = i0 + lane;',
             'const long long ic = i < ncn ? i : ncn - 1;',
             '// the owned time nodes end here: the last window also owns '
             'node N - 1',
             'const long long pend = wb + (wb == ncn ? 1 : 0);',
             '// lane 0 has an entry of its own only where the trajectory '
             'starts',
             'const bool first = lane > 0 || (blockIdx.x == 0 && wa == 0);',
             '// this lane evaluates a constraint node of the window',
             'const bool valid = i < wb;',
             '// ... that no other block counts and that is no halo (lane 0 '
             'repeats the last lane of the previous block)',
             'const bool counted = valid && first;',
             '// entry i of a row is this lane\'s to write',
             'const bool writer = i < pend && first;']
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
                dst = 'out[%dLL*ostride + (i - wa)]' % R
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
    strip_switch(lines, bodies)
    src += kernel('opty_vjp', JACPROD_PARAMS, lines)

    # ---- opty_vjp_fin -------------------------------------------------------
    T = len(prog.tail_columns())
    lines = ['if (blockIdx.x != 0) return;',
             'const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long pend = wb + (wb == ncn ? 1 : 0);',
             '// the blocks opty_vjp was launched with (vjp_window_blocks)',
             'const long long span = pend - wa - (wa == 0 ? 1 : 0);',
             'const long long nblk = span > 0 ? (span + %d)/%d : 1;'
             % (VJP_STRIDE - 1, VJP_STRIDE),
             '(void)ncn; (void)pend; (void)nblk;']
    for t, (j, _) in enumerate(prog.tail_columns()):
        lines += ['{',
                  '    double acc = 0.0;',
                  '    for (long long b = lane; b < nblk; b += 64) '
                  'acc += part[%dLL*nblk + b];' % t,
                  '    acc = opty_wave_sum(acc);',
                  '    if (lane == 0) tail[%d] = acc;' % j,
                  '}']
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)),
                 scalar_leaf(prog), fast_trig)
    for t, (k, a) in enumerate(prog.inst_pairs):
        ref = body.emit(prog.inst_jac_out[t])
        # the atom is entry p of row R; the window that owns p adds
        body.lines += [
            '{',
            '    const long long R = inst_idx[%d]/N, p = inst_idx[%d] - R*N;'
            % (a, a),
            '    if (p >= wa && p < pend) out[R*ostride + (p - wa)] += '
            'vec[%dLL*ncn + %d]*%s;' % (M, k, ref),
            '}']
    body.end_scope()
    if body.lines:
        lines += ['if (lane == 0) {'] + ['    ' + ln for ln in body.lines] + \
            ['}']
    assert T == prog.r + prog.s, (T, prog.r, prog.s)
    src += kernel('opty_vjp_fin', JACPROD_PARAMS, lines)
    return '\n'.join(src), (jcut, vcut)


#: parameter list of the four block kernels; mirrored by ``struct
#: JacprodBlockArgs`` in ``csrc/jacprod.cpp``.  Column ``c`` of the vector
#: argument starts at ``vec + c*ldv``, of the result at ``out + c*ldo``;
#: ``ncols``: the active columns of the pass, ``1 <= ncols <= K``; ``part``:
#: ``part[(t*K + c)*gridDim.x + block]``
JACPROD_BLOCK_PARAMS = _SHARED_PARAMS + ', long long ldv, long long ldo, ' \
    'int ncols'


def _column_pointers(K):
    """``vec<c>``: column ``c`` of the vector argument; a column past
    ``ncols`` reads column 0 (nothing outside the block is read, nothing is
    stored for it)."""
    return ['const double *__restrict__ vec%d = vec + (%d < ncols ? %dLL*ldv '
            ': 0LL);' % (c, c, c) for c in range(K)]


def emit_jacprod_block_module(prog, budget=1500, forget=False, fast_trig=1):
    """``(source, (jvp strips, vjp strips))`` of the block module of
    ``prog`` (a :class:`program.JacobianBlockProductProgram`); arguments as
    :func:`emit_jacprod_module`'s."""
    dag = prog.dag
    K, M = prog.columns, prog.M
    leaf = column_leaf(prog)
    sleaf = column_leaf(prog, scalar)
    src = ['// generated by opty_amd.codegen.emit_jacprod -- do not edit',
           '#include "opty_device.h"', '']
    if fast_trig == 2:
        src.append(_UNIFORM_TRIG_HELPERS)
    src.append(_REDUCE)

    def start(body, first):
        if forget and not first:
            body.new_scope()
            body.forget()
        else:
            body.begin_entry()

    # ---- opty_jvp_block: a unit is ONE equation, all of its K tangents ----
    # (forget: an equation whose K tangents do not fit the registers
    # together -- a unit is one tangent of one equation, computed afresh; the
    # large ones get strips of their own, where the compiler cannot share
    # what `forget` set apart)
    pairs = [[(j, c)] for j in range(M) for c in range(K)] if forget else \
        [[(j, c) for c in range(K)] for j in range(M)]
    jcut = cut(dag, [[prog.tan_out[c][j] for j, c in unit] for unit in pairs],
               budget)
    lines = ['const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long i = (long long)blockIdx.x*64 + lane;',
             'if ((long long)blockIdx.x*64 >= ncn) return;',
             'const long long ic = i < ncn ? i : ncn - 1;'] + \
        _column_pointers(K)
    bodies = []
    for u0, u1 in jcut:
        todo = [jc for unit in pairs[u0:u1] for jc in unit]
        body = _Body(dag, set(dag.reachable(
            [prog.tan_out[c][j] for j, c in todo])), leaf, fast_trig)
        # (a strip none of whose columns is active: wave-uniform)
        body.lines.append('if (%d >= ncols) break;' % min(c for _, c in todo))
        body.end_scope()
        for pos, (j, c) in enumerate(todo):
            if forget or c == 0:
                start(body, pos == 0)
            ref = body.emit(prog.tan_out[c][j])
            body.lines.append(
                'if (%d < ncols && i < ncn) out[%dLL*ldo + %dLL*ncn + i] '
                '= %s;' % (c, c, j, ref))
        body.end_scope()
        bodies.append(body.lines)
    strip_switch(lines, bodies)
    src += kernel('opty_jvp_block', JACPROD_BLOCK_PARAMS, lines)

    # ---- opty_jvp_block_inst ----------------------------------------------
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)), sleaf,
                 fast_trig)
    lines = ['if (threadIdx.x != 0 || blockIdx.x != 0) return;',
             'const long long ncn = N - 1;']
    for k in range(prog.num_inst):
        terms = [(a, body.emit(prog.inst_jac_out[t]))
                 for t, (kk, a) in enumerate(prog.inst_pairs) if kk == k]
        body.lines += ['for (int c = 0; c < ncols; ++c) {',
                       '    const double *v = vec + c*ldv;',
                       '    double acc = 0.0;']
        body.lines += ['    acc += %s*v[inst_idx[%d]];' % (ref, a)
                       for a, ref in terms]
        body.lines += ['    out[c*ldo + %dLL*ncn + %d] = acc;' % (M, k), '}']
        body.end_scope()
    src += kernel('opty_jvp_block_inst', JACPROD_BLOCK_PARAMS,
                  lines + body.lines)

    # ---- opty_vjp_block: a unit is a free row (tail column), K vectors ----
    units = vjp_units(prog)

    def roots_of(unit):
        ks = unit[2:] if unit[0] == 'row' else unit[2:3]
        return [prog.adj_out[c][k] for k in ks if k is not None
                for c in range(K)]
    vcut = cut(dag, [roots_of(u) for u in units], budget)
    lines = ['__shared__ double ex[2*64*%d];' % K] + \
        block_preamble(VJP_STRIDE) + [
            '// this lane evaluates a constraint node of its own',
            'const bool valid = i < ncn;',
            '// ... that no other block counts (lane 0 repeats the last '
            'lane of the previous block)',
            'const bool counted = valid && (lane > 0 || blockIdx.x == 0);',
            '// entry i of a row is this lane\'s to write',
            'const bool writer = i < N && (lane > 0 || blockIdx.x == 0);'] + \
        _column_pointers(K)
    bodies = []
    for u0, u1 in vcut:
        needed = set()
        for u in units[u0:u1]:
            needed |= set(dag.reachable(roots_of(u)))
        body = _Body(dag, needed, leaf, fast_trig)
        handovers = 0
        for pos, u in enumerate(units[u0:u1]):
            start(body, pos == 0)
            if u[0] == 'tail':
                _, t, k = u
                for c in range(K):
                    ref = body.emit(prog.adj_out[c][k])
                    body.lines += [
                        '{',
                        '    const double sum = opty_wave_sum(counted ? %s : '
                        '0.0);' % ref,
                        '    if (lane == 0 && %d < ncols) part[%dLL*gridDim.x '
                        '+ blockIdx.x] = sum;' % (c, t*K + c),
                        '}']
                continue
            _, R, lo, hi = u
            dst = ['out[%dLL*ldo + %dLL*N + i]' % (c, R) for c in range(K)]
            his = None
            if hi is not None:
                his = [body.emit(prog.adj_out[c][hi]) for c in range(K)]
                if forget:
                    # hand the upper terms over first, then start afresh:
                    # the two columns of a row are not live together
                    for c in range(K):
                        body.lines.append('const double hi%d_%d = %s;'
                                          % (R, c, his[c]))
                    his = ['hi%d_%d' % (R, c) for c in range(K)]
                    body.new_scope()
                    body.forget()
            los = [body.emit(prog.adj_out[c][lo]) for c in range(K)] \
                if lo is not None else ['0.0']*K
            if his is None:
                body.lines += ['if (writer && %d < ncols) %s = valid ? %s : '
                               '0.0;' % (c, dst[c], los[c]) for c in range(K)]
                continue
            # two sets of K buffers in turn, one wave-level ordering point
            # per row (as in opty_vjp)
            bufs = ['ex + %d' % (64*((handovers & 1)*K + c))
                    for c in range(K)]
            handovers += 1
            body.lines += ['(%s)[lane] = %s;' % (bufs[c], his[c])
                           for c in range(K)]
            body.lines.append('opty_wave_sync();')
            for c in range(K):
                body.lines += [
                    '{',
                    '    const double up = (%s)[lane > 0 ? lane - 1 : 0];'
                    % bufs[c],
                    '    if (writer && %d < ncols) %s = lane == 0 ? %s : '
                    '(valid ? %s + up : up);' % (c, dst[c], los[c], los[c]),
                    '}']
        body.end_scope()
        bodies.append(body.lines)
    strip_switch(lines, bodies)
    src += kernel('opty_vjp_block', JACPROD_BLOCK_PARAMS, lines)

    # ---- opty_vjp_block_fin -------------------------------------------------
    tails = prog.tail_columns()
    assert len(tails) == prog.r + prog.s, (len(tails), prog.r, prog.s)
    tail0 = '%dLL*N' % (prog.n + prog.q)
    lines = ['if (blockIdx.x != 0) return;',
             'const int lane = threadIdx.x;',
             'const long long ncn = N - 1;',
             'const long long nblk = (ncn + %d)/%d;'
             % (VJP_STRIDE - 1, VJP_STRIDE),
             '(void)ncn; (void)nblk;']
    body = _Body(dag, set(dag.reachable(prog.inst_jac_out)), sleaf,
                 fast_trig)
    refs = [body.emit(node) for node in prog.inst_jac_out]
    body.end_scope()
    lines += body.lines
    lines += ['for (int c = 0; c < ncols; ++c) {',
              '    const double *w = vec + c*ldv;',
              '    double *g = out + c*ldo;']
    for t, (j, _) in enumerate(tails):
        lines += ['    {',
                  '        double acc = 0.0;',
                  '        for (long long b = lane; b < nblk; b += 64) '
                  'acc += part[(%dLL + c)*nblk + b];' % (t*K),
                  '        acc = opty_wave_sum(acc);',
                  '        if (lane == 0) g[%s + %d] = acc;' % (tail0, j),
                  '    }']
    if refs:
        lines.append('    if (lane == 0) {')
        lines += ['        g[inst_idx[%d]] += w[%dLL*ncn + %d]*%s;'
                  % (a, M, k, refs[t])
                  for t, (k, a) in enumerate(prog.inst_pairs)]
        lines.append('    }')
    lines.append('}')
    src += kernel('opty_vjp_block_fin', JACPROD_BLOCK_PARAMS, lines)
    return '\n'.join(src), (jcut, vcut)
