"""What the emitters of the derived programs (``emit_hessian.py``,
``emit_jacprod.py``) share: kernels whose lane is a constraint node, one
64-lane block per ``blockIdx.x``, with the per-node roots cut into strips of
straight-line code (``blockIdx.y``)."""

from . import ir


def cut(dag, units, budget):
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


def scalar(prog, kind, k, vec='vec'):
    """Source of a node-invariant input; ``vec``: the kernel parameter that
    holds the direction of a product (``vpar`` / ``vh``)."""
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
        return vec + tail % idx
    if kind == 'vh':
        assert prog.h[0] == 'tail'
        return vec + tail % prog.h[1]
    if kind == 'free':
        return 'free_[inst_idx[%d]]' % k
    raise AssertionError(kind)


def scalar_leaf(prog, vec='vec'):
    """``leaf(i)`` of the single-lane kernels (instance constraints)."""
    dag = prog.dag
    return lambda i: scalar(prog, *dag.args[i], vec=vec) \
        if dag.op[i] == ir.INPUT else None


def node_input(prog, kind, k, vec='vec'):
    """Source of input ``(kind, k)`` in a kernel whose lane evaluates
    constraint node ``ic``; ``vec``: the kernel parameter that holds the
    multipliers (``lam``) or the direction (``vcur`` / ``vadj`` / ``vpar`` /
    ``vh``)."""
    if kind in ('cur', 'adj', 'vcur', 'vadj'):
        src, idx = prog.rows[k]
        off = prog.cur_offset if kind.endswith('cur') else prog.adj_offset
        if kind[0] == 'v':
            assert src == 'free', (kind, k)
            base = vec
        else:
            base = 'free_' if src == 'free' else 'known_traj'
        return '%s[%dLL*N + ic + %d]' % (base, idx, off)
    if kind == 'lam':
        return '%s[%dLL*ncn + ic]' % (vec, k)
    return scalar(prog, kind, k, vec)


def node_leaf(prog, vec='vec'):
    """``leaf(i)`` of a kernel whose lane evaluates constraint node ``ic``
    (:func:`node_input`)."""
    dag = prog.dag
    return lambda i: node_input(prog, *dag.args[i], vec=vec) \
        if dag.op[i] == ir.INPUT else None


def column_leaf(prog, source=node_input, vec='vec%d'):
    """``leaf(i)`` of a block product kernel: ``source`` (:func:`node_input`
    or :func:`scalar`) of the input within its column
    (:func:`ir.split_column`), read from the column's own pointer ``vec %
    column``."""
    dag = prog.dag

    def leaf(i):
        if dag.op[i] != ir.INPUT:
            return None
        kind, k = dag.args[i]
        c, k = ir.split_column(kind, k)
        return source(prog, kind, k, vec % c)
    return leaf


def block_preamble(stride=64, window=False):
    """First lines of a kernel whose block ``blockIdx.x`` holds the 64
    constraint nodes from ``i0 = stride*blockIdx.x`` on: ``i`` the lane's
    node, ``ic`` the same clamped to the last one.  ``window``: the kernel
    evaluates the nodes ``[wa, wb)`` of the global problem (two wave-uniform
    kernel arguments: scalar registers) -- blocks count from ``wa``, end at
    ``wb``, and ``ic`` is clamped into the window; ``i`` and ``ic`` stay
    GLOBAL node indices."""
    first, end = ('wa + ', 'wb') if window else ('', 'ncn')
    return ['const int lane = threadIdx.x;',
            'const long long ncn = N - 1;',
            'const long long i0 = %s(long long)blockIdx.x*%d;' % (first,
                                                                  stride),
            'if (i0 >= %s) return;' % end,
            'const long long i = i0 + lane;',
            'const long long ic = i < %s ? i : %s - 1;' % (end, end)]


def strip_switch(lines, bodies):
    lines.append('switch (blockIdx.y) {')
    for s, body in enumerate(bodies):
        lines.append('case %d: {' % s)
        lines += ['    ' + ln for ln in body]
        lines += ['    break;', '}']
    lines += ['default: break;', '}']


def kernel(name, params, lines):
    return (['extern "C" __global__ void __launch_bounds__(64)',
             '%s(%s)' % (name, params), '{'] +
            ['    ' + ln for ln in lines] + ['}', ''])
