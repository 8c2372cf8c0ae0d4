"""Device-resident objective and objective gradient (SURVEY.md section 8(f),
rank 1): the HIP counterpart of ``create_objective_function``
(``opty/utils.py:329-470``).

The reference lambdifies the symbolic objective and its symbolic gradient and
replaces every ``Integral(g, t)`` by a quadrature over the collocation nodes:

* backward Euler: ``h * sum_i w_i g(node i)`` with ``w = [0, 1, ..., 1]``
  (``opty/utils.py:419-425``);
* midpoint: ``h * sum_i g((node i + node i+1)/2)`` over the N-1 midpoints for
  the objective and the parameter gradient, and -- for the gradient with
  respect to a trajectory value at node i -- ``h * w'_i dg/dz(node i)`` with
  ``w' = [1/2, 1, ..., 1, 1/2]`` evaluated at the NODE values
  (``opty/utils.py:440-464``).  That second rule is reproduced as is.

Here the integrand, its partials and the quadrature run on the GPU: one
elementwise + wave-reduction kernel (``opty_objgrad``: lane == time node,
coalesced loads of ``free`` and coalesced stores of the trajectory part of the
gradient, per-wave partial sums) and one single-wave kernel (``opty_objfin``)
that adds the partial sums in a fixed order (deterministic), applies ``h`` and
the parameter-only terms and writes the value and the parameter part of the
gradient.

Supported objectives are the ones the reference evaluates correctly: linear in
their integrals, ``sum_j a_j(p) * Integral(g_j(x, u, p), t) + b(p)``.
"""

import numpy as np
import sympy as sm
import sympy.physics.mechanics as me

from .utils import sort_sympy
from .codegen import ir
from .codegen.lower import Lowerer, forward_jacobian
from .codegen.emit_hip import _Body, KERNEL_PARAMS
from . import hip_backend as hb

__all__ = ['create_objective_function',
           'create_objective_hessian_function', 'compile_objective_hessian']


def _split_objective(objective, time_symbol, time_funcs):
    """-> integrand ``G`` (a_j folded in) and parameter-only remainder ``b``."""
    objective = sm.sympify(objective)
    integrals = sorted(objective.atoms(sm.Integral), key=sm.default_sort_key)
    dummies = []
    for integral in integrals:
        if integral.function.has(sm.Integral):
            raise NotImplementedError('Nested integrals are not supported.')
        if integral.limits != ((time_symbol,),):
            raise NotImplementedError('Only indefinite integrals of time are '
                                      'supported.')
        dummies.append(sm.Dummy('I%d' % len(dummies)))
    obj_d = objective.xreplace(dict(zip(integrals, dummies)))
    G = sm.S.Zero
    for j, dj in enumerate(dummies):
        a_j = obj_d.diff(dj)
        if any(a_j.has(dk) for dk in dummies):
            raise NotImplementedError(
                'The objective must be linear in its integrals (the '
                'reference evaluates anything else incorrectly).')
        if any(a_j.has(f) for f in time_funcs):
            raise NotImplementedError(
                'Factors outside an integral may only depend on the unknown '
                'parameters.')
        G += a_j*integrals[j].function
    b = sm.sympify(obj_d.xreplace({dj: sm.S.Zero for dj in dummies}))
    if any(b.has(f) for f in time_funcs):
        raise NotImplementedError('Terms outside an integral may only depend '
                                  'on the unknown parameters.')
    return G, b


def _emit(dag, n_rows, r, N_sym_unused, method, roots):
    """HIP source of ``opty_objgrad`` / ``opty_objfin``."""
    g_quad, dp_quad, dz_node, b_val, db_val = roots
    nq = 1 + r

    def leaf(i):
        if dag.op[i] != ir.INPUT:
            return None
        kind, k = dag.args[i]
        if kind == 'cur':
            return 'zc%d' % k
        if kind == 'adj':
            return 'za%d' % k
        if kind == 'par':
            return 'free_[%dLL*N + %d]' % (n_rows, k)
        raise AssertionError(kind)

    need = set(dag.reachable([g_quad] + dp_quad + dz_node))
    rows_c = sorted({dag.args[i][1] for i in need if dag.op[i] == ir.INPUT
                     and dag.args[i][0] == 'cur'})
    rows_a = sorted({dag.args[i][1] for i in need if dag.op[i] == ir.INPUT
                     and dag.args[i][0] == 'adj'})
    body = _Body(dag, need, leaf)
    lines = ['const int lane = threadIdx.x;',
             'const long long i = (long long)blockIdx.x*64 + lane;',
             'const bool in = i < N;',
             'const long long ic = in ? i : N - 1;',
             'const long long ia = ic + 1 < N ? ic + 1 : N - 1;']
    for k in rows_c:
        lines.append('const double zc%d = free_[%dLL*N + ic];' % (k, k))
    for k in rows_a:
        lines.append('const double za%d = free_[%dLL*N + ia];' % (k, k))
    if method == 'backward euler':
        lines.append('const double wq = (in && i > 0) ? 1.0 : 0.0;')
        lines.append('const double wg = wq;')
    else:
        lines.append('const double wq = (i < N - 1) ? 1.0 : 0.0;')
        lines.append('const double wg = !in ? 0.0 : '
                     '((i == 0 || i == N - 1) ? 0.5 : 1.0);')
    # trajectory part of the gradient: elementwise, coalesced
    for k, node in enumerate(dz_node):
        body.new_scope()
        ref = body.emit(node)
        body.lines.append('if (jac && in) jac[%dLL*N + i] = h*wg*%s;'
                          % (k, ref))
    body.new_scope()
    # quadrature terms: per-wave partial sums, fixed order
    qrefs = [body.emit(g_quad)] + [body.emit(nd) for nd in dp_quad]
    body.end_scope()
    lines += body.lines
    for j, ref in enumerate(qrefs):
        lines.append('double q%d = wq*%s;' % (j, ref))
    lines.append('#pragma unroll')
    lines.append('for (int off = 32; off > 0; off >>= 1) {')
    for j in range(nq):
        lines.append('    q%d += __shfl_down(q%d, off, 64);' % (j, j))
    lines.append('}')
    lines.append('if (lane == 0) {')
    for j in range(nq):
        lines.append('    con[(long long)blockIdx.x*%d + %d] = q%d;'
                     % (nq, j, j))
    lines.append('}')
    src = ['// generated by opty_amd.objective -- do not edit',
           '#include "opty_device.h"', '',
           'extern "C" __global__ void __launch_bounds__(64)',
           'opty_objgrad(%s)' % KERNEL_PARAMS, '{']
    src += ['    ' + ln for ln in lines] + ['}', '']

    # final reduction: one wave, partials summed in a fixed order
    ubody = _Body(dag, set(dag.reachable([b_val] + db_val)), leaf)
    bref = ubody.emit(b_val)
    drefs = [ubody.emit(nd) for nd in db_val]
    ubody.end_scope()
    fin = ['const int lane = threadIdx.x;',
           'const long long nblk = con_stride;']
    for j in range(nq):
        fin.append('double s%d = 0.0;' % j)
    fin.append('for (long long b = lane; b < nblk; b += 64) {')
    for j in range(nq):
        fin.append('    s%d += con[b*%d + %d];' % (j, nq, j))
    fin.append('}')
    fin.append('#pragma unroll')
    fin.append('for (int off = 32; off > 0; off >>= 1) {')
    for j in range(nq):
        fin.append('    s%d += __shfl_down(s%d, off, 64);' % (j, j))
    fin.append('}')
    fin.append('if (lane == 0) {')
    fin += ['    ' + ln for ln in ubody.lines]
    fin.append('    uni_w[0] = h*s0 + %s;' % bref)
    for k in range(r):
        fin.append('    if (jac) jac[%dLL*N + %d] = h*s%d + %s;'
                   % (n_rows, k, 1 + k, drefs[k]))
    fin.append('}')
    src += ['extern "C" __global__ void __launch_bounds__(64)',
            'opty_objfin(%s)' % KERNEL_PARAMS, '{']
    src += ['    ' + ln for ln in fin] + ['}', '']
    return '\n'.join(src)


def _front_end(objective, state_symbols, unknown_input_trajectories,
               unknown_parameters, integration_method, time_symbol):
    """What the objective programs share: the refusals, the split into ``G``
    and ``b`` and a DAG with the INPUT nodes ``cur`` / ``adj`` / ``par``.
    -> ``(dag, table, lowerer, G, b, funcs, zc, za, params)``."""
    if time_symbol is None:
        time_symbol = me.dynamicsymbols._t
    if integration_method not in ('backward euler', 'midpoint'):
        raise NotImplementedError(
            f"Integration method '{integration_method}' is not implemented.")
    states = list(state_symbols)
    inputs = sort_sympy(unknown_input_trajectories)
    params = sort_sympy(unknown_parameters)
    funcs = states + inputs
    G, b = _split_objective(objective, time_symbol, funcs)

    dag = ir.DAG()
    zc = [sm.Dummy('zc%d' % k, real=True) for k in range(len(funcs))]
    za = [sm.Dummy('za%d' % k, real=True) for k in range(len(funcs))]
    table = {s: dag.input('cur', k) for k, s in enumerate(zc)}
    table.update({s: dag.input('adj', k) for k, s in enumerate(za)})
    table.update({p: dag.input('par', k) for k, p in enumerate(params)})
    low = Lowerer(dag, table)
    return dag, table, low, G, b, funcs, zc, za, params


def build_objective_program(objective, state_symbols,
                            unknown_input_trajectories, unknown_parameters,
                            integration_method='backward euler',
                            time_symbol=None):
    """Lowers the objective into a DAG.  Returns ``(dag, roots, n, q, r)``
    with ``roots = (g_quad, dp_quad, dz_node, b_val, db_val)``: the integrand
    at the quadrature points, its parameter partials there, its trajectory
    partials at the node values, the parameter-only remainder and its
    partials.  INPUT kinds: ``cur``/``adj`` = trajectory row at node i / i+1,
    ``par`` = unknown parameter (name-sorted, ``opty/utils.py:393-394``)."""
    dag, table, low, G, b, funcs, zc, za, params = _front_end(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, integration_method, time_symbol)
    n, q, r = len(state_symbols), len(funcs) - len(state_symbols), len(params)
    G_node = low.lower(G.xreplace(dict(zip(funcs, zc))))
    wrt_nodes = [table[s] for s in zc] + [table[p] for p in params]
    grads = forward_jacobian(dag, [G_node], wrt_nodes)[0]
    dz_node, dp_node = grads[:n + q], grads[n + q:]
    if integration_method == 'backward euler':
        g_quad, dp_quad = G_node, dp_node
    else:
        at_mid = {f: (c + a)/2 for f, c, a in zip(funcs, zc, za)}
        g_quad = low.lower(G.xreplace(at_mid))
        dp_quad = forward_jacobian(dag, [g_quad],
                                   [table[p] for p in params])[0]
    b_val = low.lower(b)
    db_val = forward_jacobian(dag, [b_val], [table[p] for p in params])[0]
    return dag, (g_quad, dp_quad, dz_node, b_val, db_val), n, q, r


def compile_objective(objective, state_symbols, unknown_input_trajectories,
                      unknown_parameters, num_collocation_nodes,
                      integration_method='backward euler', time_symbol=None,
                      tmp_dir=None):
    """Lowers, prints and builds the objective kernels (no device needed):
    ``(code object path, (n, q, r))``."""
    dag, roots, n, q, r = build_objective_program(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, integration_method, time_symbol)
    source = _emit(dag, n + q, r, int(num_collocation_nodes),
                   integration_method, roots)
    return hb.compile_module(source, tmp_dir), (n, q, r)


def create_objective_function(objective, state_symbols,
                              unknown_input_trajectories, unknown_parameters,
                              num_collocation_nodes, node_time_interval,
                              integration_method='backward euler',
                              time_symbol=None, device=0, tmp_dir=None):
    """Returns ``(obj, obj_grad)`` evaluated on the GPU; same arguments and
    return contract as the reference's ``create_objective_function``
    (``opty/utils.py:329-364``): ``obj(free) -> float``,
    ``obj_grad(free) -> ndarray (n*N + q*N + r,)``.

    Both callables also accept a ``torch`` CUDA tensor for ``free``;
    ``obj_grad`` then returns a CUDA tensor (nothing crosses PCIe).
    """
    hsaco, (n, q, r) = compile_objective(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, num_collocation_nodes, integration_method,
        time_symbol, tmp_dir)
    N = int(num_collocation_nodes)
    handle = hb.HipObjective(dict(N=N, n=n, q=q, r=r, device=int(device),
                                  h=float(node_time_interval)), hsaco)
    num_free = (n + q)*N + r

    def _as_input(free):
        if hasattr(free, 'data_ptr'):
            if tuple(free.shape) != (num_free,):
                raise ValueError('free must have shape (%d,)' % num_free)
            # ordered behind whatever produced the tensor on torch's stream
            handle.use_torch_stream()
            return free, hb.DEVICE
        free = np.ascontiguousarray(free, dtype=np.float64)
        if free.shape != (num_free,):
            raise ValueError('free must have shape (%d,)' % num_free)
        return free, hb.HOST

    def obj(free):
        free, mem = _as_input(free)
        return handle.evaluate(free, None, mem)

    def obj_grad(free):
        free, mem = _as_input(free)
        if mem == hb.DEVICE:
            import torch
            grad = torch.empty(num_free, dtype=torch.float64,
                               device=free.device)
        else:
            grad = np.empty(num_free)
        handle.evaluate(free, grad, mem)
        return grad

    obj.handle = obj_grad.handle = handle
    return obj, obj_grad


# ---------------------------------------------------------------------------
# exact Hessian of the objective
# ---------------------------------------------------------------------------
#: parameter list of ``opty_objhess`` / ``opty_objhess_fin``; must match
#: ``ObjHessArgs`` in csrc/programs.cpp
OBJHESS_PARAMS = (
    'const double *__restrict__ free_, double *__restrict__ partial, '
    'double *__restrict__ out, double h, double factor, long long N, '
    'long long nblk')
OBJHESS_KERNELS = ('opty_objhess', 'opty_objhess_fin')


def build_objective_hessian_program(objective, state_symbols,
                                    unknown_input_trajectories,
                                    unknown_parameters,
                                    integration_method='backward euler',
                                    time_symbol=None):
    """Lowers the objective (arguments, input kinds and refusals of
    :func:`build_objective_program`) and differentiates the integrand at the
    quadrature point twice with :func:`lower.forward_jacobian`.  Returns
    ``(dag, roots, n, q, r)`` with ``roots = (point_roots, pattern,
    tail_quad, tail_const, tail_pairs)``:

    * ``point_roots[e]``, ``pattern[e] = (row_var, row_off, col_var,
      col_off)``: per-point entry ``e`` has the value ``h*point_roots[e]`` at
      every quadrature point ``j`` and sits at the free indices ``var*N + j +
      base + off`` (``var = -1``: the parameter ``(n+q)*N + off``), ``base =
      1`` for backward Euler and ``0`` for midpoint.  Row >= column at every
      point: lexicographic on ``(var, off)``, parameters last.
    * tail entry ``t`` -- parameters ``tail_pairs[t] = (a, b)``, ``a >= b`` --
      has the value ``h*sum_j tail_quad[t] + tail_const[t]``.

    Midpoint: ``G((cur + adj)/2)`` depends on ``cur`` and ``adj`` through
    their sum alone, so its partials with respect to either are the same DAG
    node; it is differentiated with respect to ``cur``, which gives ``G_kl/4``
    for all four (three when ``k == l``) triplets of a pair of trajectory
    variables and ``G_pk/2`` for both offsets of a parameter-trajectory pair:
    one root, stored to each of its entries.  Entries whose second partial is
    identically zero on the DAG are dropped."""
    dag, table, low, G, b, funcs, zc, za, params = _front_end(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, integration_method, time_symbol)
    n, q, r = len(state_symbols), len(funcs) - len(state_symbols), len(params)
    nz = n + q
    mid = integration_method == 'midpoint'
    at_point = {f: (c + a)/2 for f, c, a in zip(funcs, zc, za)} if mid \
        else dict(zip(funcs, zc))
    g_quad = low.lower(G.xreplace(at_point))
    wrt = [table[s] for s in zc] + [table[p] for p in params]
    grad = forward_jacobian(dag, [g_quad], wrt)[0]
    hess = forward_jacobian(dag, grad, wrt)
    par_nodes = [table[p] for p in params]
    b_grad = forward_jacobian(dag, [low.lower(b)], par_nodes)[0]
    b_hess = forward_jacobian(dag, b_grad, par_nodes)

    point_roots, pattern = [], []
    for k in range(nz):
        for l in range(k + 1):
            node = hess[k][l]
            if node == dag.zero:
                continue
            if not mid:
                sides = [(0, 0)]
            elif k != l:
                sides = [(0, 0), (0, 1), (1, 0), (1, 1)]
            else:
                sides = [(0, 0), (1, 1), (1, 0)]
            for ro, co in sides:
                point_roots.append(node)
                pattern.append((k, ro, l, co))
    for a in range(r):
        for k in range(nz):
            node = hess[nz + a][k]
            if node == dag.zero:
                continue
            for co in ((0, 1) if mid else (0,)):
                point_roots.append(node)
                pattern.append((-1, a, k, co))
    tail_quad, tail_const, tail_pairs = [], [], []
    for a in range(r):
        for c in range(a + 1):
            gq, bc = hess[nz + a][nz + c], b_hess[a][c]
            if gq != dag.zero or bc != dag.zero:
                tail_quad.append(gq)
                tail_const.append(bc)
                tail_pairs.append((a, c))
    return dag, (point_roots, pattern, tail_quad, tail_const,
                 tail_pairs), n, q, r


def objective_hessian_indices(pattern, tail_pairs, n, q, N, method):
    """Closed-form ``(rows, cols)`` (int64) on the host of the values of an
    objective Hessian program for ``N`` nodes: entry-major ``[e*(N-1) + j]``,
    then the parameter-parameter entries."""
    N = int(N)
    base = 1 if method == 'backward euler' else 0
    pat = np.array(pattern, dtype=np.int64).reshape(-1, 4)
    j = np.arange(N - 1, dtype=np.int64)[None, :]
    tail = (n + q)*N

    def side(var, off):
        var, off = var[:, None], off[:, None]
        return np.where(var >= 0, var*N + j + base + off, tail + off)
    rows = side(pat[:, 0], pat[:, 1]).ravel()
    cols = side(pat[:, 2], pat[:, 3]).ravel()
    pairs = np.array(tail_pairs, dtype=np.int64).reshape(-1, 2)
    return (np.concatenate((rows, tail + pairs[:, 0])),
            np.concatenate((cols, tail + pairs[:, 1])))


def _emit_hessian(dag, n_rows, method, roots):
    """HIP source of ``opty_objhess`` (lane = quadrature point) and, with
    parameter-parameter entries, ``opty_objhess_fin``; it does not depend on
    the node count."""
    point_roots, pattern, tail_quad, tail_const, tail_pairs = roots
    E, T = len(point_roots), len(tail_quad)
    base = 1 if method == 'backward euler' else 0
    # tail entries with a quadrature part: a block partial each
    quad = [t for t in range(T) if tail_quad[t] != dag.zero]
    nq = len(quad)

    def leaf(i):
        if dag.op[i] != ir.INPUT:
            return None
        kind, k = dag.args[i]
        if kind == 'cur':
            return 'zc%d' % k
        if kind == 'adj':
            return 'za%d' % k
        if kind == 'par':
            return 'free_[%dLL*N + %d]' % (n_rows, k)
        raise AssertionError(kind)

    need = set(dag.reachable(list(point_roots) +
                             [tail_quad[t] for t in quad]))
    rows_c = sorted({dag.args[i][1] for i in need if dag.op[i] == ir.INPUT
                     and dag.args[i][0] == 'cur'})
    rows_a = sorted({dag.args[i][1] for i in need if dag.op[i] == ir.INPUT
                     and dag.args[i][0] == 'adj'})
    body = _Body(dag, need, leaf)
    lines = ['const int lane = threadIdx.x;',
             'const long long npts = N - 1;',
             'const long long j = (long long)blockIdx.x*64 + lane;',
             'const bool in = j < npts;',
             '// node of the point; lanes past the last point read its node',
             'const long long ic = (in ? j : npts - 1) + %d;' % base,
            ]
    for k in rows_c:
        lines.append('const double zc%d = free_[%dLL*N + ic];' % (k, k))
    for k in rows_a:
        # (the last lane's adjacent node is the next block's first)
        lines.append('const double za%d = free_[%dLL*N + ic + 1];' % (k, k))
    # per-point entries: entry-major, one coalesced segment per wave and entry
    e = 0
    while e < E:
        body.new_scope()
        ref = body.emit(point_roots[e])
        same = e
        while same < E and point_roots[same] == point_roots[e]:
            same += 1
        body.lines.append('if (in) {')
        # (factor last: obj_factor*values(free), bit for bit)
        body.lines.append('    const double val = factor*(h*%s);' % ref)
        for s in range(e, same):
            body.lines.append('    out[%dLL*npts + j] = val;' % s)
        body.lines.append('}')
        e = same
    body.new_scope()
    qrefs = [body.emit(tail_quad[t]) for t in quad]
    body.end_scope()
    lines += body.lines
    if nq:
        for s, ref in enumerate(qrefs):
            lines.append('double q%d = in ? %s : 0.0;' % (s, ref))
        lines.append('#pragma unroll')
        lines.append('for (int off = 32; off > 0; off >>= 1) {')
        for s in range(nq):
            lines.append('    q%d += __shfl_down(q%d, off, 64);' % (s, s))
        lines.append('}')
        lines.append('if (lane == 0) {')
        for s in range(nq):
            lines.append('    partial[(long long)blockIdx.x*%d + %d] = q%d;'
                         % (nq, s, s))
        lines.append('}')
    src = ['// generated by opty_amd.objective -- do not edit',
           '#include "opty_device.h"', '',
           'extern "C" __global__ void __launch_bounds__(64)',
           'opty_objhess(%s)' % OBJHESS_PARAMS, '{']
    src += ['    ' + ln for ln in lines] + ['}', '']
    if T == 0:
        return '\n'.join(src)

    # parameter-parameter entries: one wave, block partials in a fixed order
    ubody = _Body(dag, set(dag.reachable(list(tail_const))), leaf)
    crefs = [ubody.emit(nd) for nd in tail_const]
    ubody.end_scope()
    fin = ['const int lane = threadIdx.x;']
    for s in range(nq):
        fin.append('double s%d = 0.0;' % s)
    if nq:
        fin.append('for (long long b = lane; b < nblk; b += 64) {')
        for s in range(nq):
            fin.append('    s%d += partial[b*%d + %d];' % (s, nq, s))
        fin.append('}')
        fin.append('#pragma unroll')
        fin.append('for (int off = 32; off > 0; off >>= 1) {')
        for s in range(nq):
            fin.append('    s%d += __shfl_down(s%d, off, 64);' % (s, s))
        fin.append('}')
    fin.append('if (lane == 0) {')
    fin += ['    ' + ln for ln in ubody.lines]
    fin.append('    double *tail = out + %dLL*(N - 1);' % E)
    for t in range(T):
        terms = []
        if t in quad:
            terms.append('h*s%d' % quad.index(t))
        if tail_const[t] != dag.zero:
            terms.append(crefs[t])
        fin.append('    tail[%d] = factor*(%s);' % (t, ' + '.join(terms)))
    fin.append('}')
    src += ['extern "C" __global__ void __launch_bounds__(64)',
            'opty_objhess_fin(%s)' % OBJHESS_PARAMS, '{']
    src += ['    ' + ln for ln in fin] + ['}', '']
    return '\n'.join(src)


def objective_hessian_source(objective, state_symbols,
                             unknown_input_trajectories, unknown_parameters,
                             integration_method='backward euler',
                             time_symbol=None):
    """``(HIP source, program)`` of the objective Hessian kernels."""
    program = build_objective_hessian_program(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, integration_method, time_symbol)
    dag, roots, n, q, r = program
    return _emit_hessian(dag, n + q, integration_method, roots), program


def compile_objective_hessian(objective, state_symbols,
                              unknown_input_trajectories, unknown_parameters,
                              num_collocation_nodes=None,
                              integration_method='backward euler',
                              time_symbol=None, tmp_dir=None):
    """Lowers, differentiates, prints and builds the objective Hessian
    kernels (no device needed; the code does not depend on the node count):
    ``(code object path, program)``.  A build that spills vector registers is
    refused (:class:`hip_backend.BuildRejected`)."""
    source, program = objective_hessian_source(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, integration_method, time_symbol)
    hsaco = hb.compile_module(source, tmp_dir)
    spills = hb.vgpr_spills(hsaco, OBJHESS_KERNELS)
    if spills:
        raise hb.BuildRejected('the objective Hessian kernels spill vector '
                               'registers: %s' % spills, dict(spills=spills))
    return hsaco, program


#: quadrature points the build check compares one by one: the first block
#: and the last point (the tail entries are compared over all points)
_HESS_VERIFY_POINTS = 64
#: points per tape run of the tail entries' sums
_HESS_TAIL_CHUNK = 8192


def _verify_hessian(handle, program, N, h, method, device):
    """Holds an objective Hessian build to its expression DAG before first
    use: random ``free``, a device output that starts as NaN, the roots run
    as an instruction tape on the GPU (``opty_hip_tape_run``) at the first 64
    quadrature points and the last one -- the parameter-parameter entries
    over all points -- judged by ``ConstraintCollocator._tape_check``'s rule
    (64 units of each entry's rounding-error bound plus 4 units of
    magnitude).  Raises :class:`hip_backend.BuildRejected`."""
    from .codegen.tape import Tape
    from .codegen.errbound import evaluate_with_error_bound
    from .direct_collocation import ConstraintCollocator
    dag, roots, n, q, r = program
    point_roots, pattern, tail_quad, tail_const, tail_pairs = roots
    E, T = len(point_roots), len(tail_quad)
    if E == 0 and T == 0:
        return dict(ok=True, referee='tape', points=0,
                    worst_fraction_of_tolerance=0.0)
    npts, base = N - 1, 1 if method == 'backward euler' else 0
    rng = np.random.default_rng(23)
    free = rng.uniform(-1.0, 1.0, (n + q)*N + r)
    d_free = hb.DeviceVector(free, device)
    d_out = hb.DeviceVector(np.full(handle.nnz, np.nan), device)
    try:
        # the legacy stream: the blocking copy back is ordered behind it
        handle.set_stream(hb.STREAM_LEGACY)
        handle.evaluate(d_free, 1.0, d_out, hb.DEVICE)
        got = d_out.numpy()
    finally:
        handle.set_stream(None)
        d_free.close()
        d_out.close()

    def inputs_at(points):
        def inputs(kind, k):
            if kind == 'par':
                return free[(n + q)*N + k]
            off = base + (1 if kind == 'adj' else 0)
            return free[k*N + points + off]
        return inputs

    def referee(nodes, points):
        """Values and rounding-error bounds ``(len(nodes), len(points))``."""
        nodes = list(nodes)
        inputs = inputs_at(points)
        _, bound = evaluate_with_error_bound(dag, nodes, inputs)
        bnd = np.stack([np.broadcast_to(np.abs(np.asarray(
            bd, dtype=float)), (len(points),)) for bd in bound])
        # (a constant root has no instruction: the tape runs the others)
        live = [nd for nd in nodes if dag.op[nd] != ir.CONST]
        if live:
            tape = Tape(dag, live)
            vals = hb.tape_run(tape, tape.table(len(points), inputs), device)
        val = np.stack([np.full(len(points), dag.value(nd))
                        if dag.op[nd] == ir.CONST else vals[tape.slot[nd]]
                        for nd in nodes])
        return val, bnd

    check = ConstraintCollocator._tape_check
    worst = 0.0
    points = np.unique(np.r_[np.arange(min(npts, _HESS_VERIFY_POINTS)),
                             npts - 1])
    if E:
        uniq = sorted(set(point_roots))
        val, bnd = referee(uniq, points)
        at = {nd: k for k, nd in enumerate(uniq)}
        for e, nd in enumerate(point_roots):
            want, bd = h*val[at[nd]], abs(h)*bnd[at[nd]]
            worst = max(worst, check(
                'objective Hessian entry %d' % e, got[e*npts + points], want,
                bd, np.abs(want), entry=e))
    if T:
        sums, sbnd, smag = np.zeros(T), np.zeros(T), np.zeros(T)
        quad = [t for t in range(T) if tail_quad[t] != dag.zero]
        for lo in range(0, npts if quad else 0, _HESS_TAIL_CHUNK):
            pts = np.arange(lo, min(npts, lo + _HESS_TAIL_CHUNK))
            val, bnd = referee([tail_quad[t] for t in quad], pts)
            for s, t in enumerate(quad):
                sums[t] += val[s].sum()
                sbnd[t] += bnd[s].sum()
                smag[t] += np.abs(val[s]).sum()
        cval, cbnd = referee(tail_const, np.zeros(1, dtype=np.int64))
        # the additions of the sum round too, by one unit of the terms'
        # magnitude per level: 6 + 6 levels of the two shuffle trees and
        # ceil(nblk/64) serial ones in the kernels; fewer than 52 in NumPy's
        # pairwise sum of a chunk, and one per chunk
        depth = 64 + (npts + 4095)//4096 + (npts + _HESS_TAIL_CHUNK - 1) \
            // _HESS_TAIL_CHUNK
        want = h*sums + cval[:, 0]
        bd = abs(h)*(sbnd + depth*smag) + cbnd[:, 0]
        mag = np.abs(h*sums) + np.abs(cval[:, 0])
        worst = max(worst, check('objective Hessian parameter entries',
                                 got[E*npts:], want, bd, mag, tail=True))
    return dict(ok=True, referee='tape', points=len(points),
                worst_fraction_of_tolerance=worst)


def create_objective_hessian_function(objective, state_symbols,
                                      unknown_input_trajectories,
                                      unknown_parameters,
                                      num_collocation_nodes,
                                      node_time_interval,
                                      integration_method='backward euler',
                                      time_symbol=None, device=0,
                                      tmp_dir=None):
    """Returns ``(rows, cols, values)``: the exact Hessian ``H = d2 f /
    d free^2`` of the value ``f(free)`` that ``obj(free)`` of
    :func:`create_objective_function` returns (same arguments), evaluated on
    the GPU.  The result plugs into ``Problem(obj_hessian=...)`` as it is.

    Contract of the constraint Hessian (``ConstraintCollocator.
    generate_hessian_function``): only the LOWER triangle on the global free
    indices, as triplets; a ``(row, col)`` pair may repeat and the matrix is
    the SUM of its triplets; only entries whose second partial is not
    identically zero are kept.  ``rows`` and ``cols`` are the int64 indices
    from the device's closed form (``values.indices_closed_form()`` is the
    host's).  Layout: the ``E`` per-point entries entry-major, ``e*(N-1) +
    j`` for quadrature point ``j``, then the ``T`` parameter-parameter
    entries; ``nnz = E*(N-1) + T`` may be 0.

    * Backward Euler, ``f = h sum_{i=1}^{N-1} G(z_i, p) + b(p)``: ``H`` is
      also the Jacobian of what ``obj_grad`` returns.
    * Midpoint, ``f = h sum_{i=0}^{N-2} G((z_i + z_{i+1})/2, p) + b(p)``:
      ``H`` is the Hessian of the value ``obj`` returns.  The trajectory part
      of the reference-shaped midpoint gradient is evaluated at the NODE
      values with the weights ``[1/2, 1, ..., 1, 1/2]`` (module docstring);
      that gradient is not the gradient of that value, so no matrix can be
      both.

    ``values(free, obj_factor=1.0, out=None)``: a NumPy ``free`` gives a new
    ndarray; a torch CUDA tensor gives a new CUDA tensor -- or fills ``out``,
    which may be a view into a larger buffer -- on torch's current stream
    (nothing crosses PCIe).  Every value is written exactly once per call in
    a fixed order of operations: the same input gives the same bits.
    ``values.handle`` is the :class:`hip_backend.HipObjectiveHessian`.

    Before first use the kernels are held to their expression DAG on the
    device (:class:`hip_backend.BuildRejected` on disagreement)."""
    N, h = int(num_collocation_nodes), float(node_time_interval)
    hsaco, program = compile_objective_hessian(
        objective, state_symbols, unknown_input_trajectories,
        unknown_parameters, N, integration_method, time_symbol, tmp_dir)
    dag, roots, n, q, r = program
    point_roots, pattern, tail_quad, tail_const, tail_pairs = roots
    handle = hb.HipObjectiveHessian(
        dict(N=N, n=n, q=q, r=r, device=int(device), h=h,
             base=1 if integration_method == 'backward euler' else 0,
             E=len(point_roots), T=len(tail_quad)), pattern, tail_pairs,
        hsaco)
    try:
        verdict = _verify_hessian(handle, program, N, h, integration_method,
                                  int(device))
    except hb.BuildRejected:
        handle.close()
        raise
    nnz, num_free = handle.nnz, (n + q)*N + r
    rows = np.empty(nnz, dtype=np.int64)
    cols = np.empty(nnz, dtype=np.int64)
    handle.indices(rows, cols, hb.HOST)

    def values(free, obj_factor=1.0, out=None):
        if hasattr(free, 'data_ptr'):
            import torch
            if tuple(free.shape) != (num_free,):
                raise ValueError('free must have shape (%d,)' % num_free)
            free = free.to(torch.float64).contiguous()
            if out is None:
                out = torch.empty(nnz, dtype=torch.float64,
                                  device=free.device)
            elif (tuple(out.shape) != (nnz,) or out.dtype != torch.float64
                  or not out.is_contiguous() or out.device != free.device):
                raise ValueError('out must be a contiguous float64 tensor of '
                                 'shape (%d,) on the device of free' % nnz)
            # ordered behind whatever produced the tensors on torch's stream
            if nnz:     # (an empty tensor has no address to hand over)
                handle.use_torch_stream(
                    torch.cuda.current_stream(free.device))
                handle.evaluate(free, obj_factor, out, hb.DEVICE)
            return out
        free = np.ascontiguousarray(free, dtype=np.float64)
        if free.shape != (num_free,):
            raise ValueError('free must have shape (%d,)' % num_free)
        if out is None:
            out = np.empty(nnz)
        elif (not isinstance(out, np.ndarray) or out.shape != (nnz,) or
              out.dtype != np.float64 or not out.flags.c_contiguous):
            raise ValueError('out must be a contiguous float64 array of '
                             'shape (%d,)' % nnz)
        if nnz:
            handle.evaluate(free, obj_factor, out, hb.HOST)
        return out

    values.handle = handle
    values.verdict = verdict
    values.indices_closed_form = lambda: objective_hessian_indices(
        pattern, tail_pairs, n, q, N, integration_method)
    return rows, cols, values
