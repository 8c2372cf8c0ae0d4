"""Builds the per-problem *collocation program*: one DAG holding the M
discretised defect equations, their M x C analytic partials and the instance
constraints, plus the tables that say where every DAG input lives in device
memory.

This is the HIP backend's counterpart of what the reference assembles inside
``_gen_multi_arg_con_func`` / ``_gen_multi_arg_con_jac_func``
(``opty/direct_collocation.py:2304-2380``, ``:2692-2805``): the argument list
(``args``), the differentiation variables (``wrt``) and the expressions handed
to ``ufuncify_matrix``.
"""

from . import ir
import os

from .lower import Lowerer, forward_jacobian
from .simplify import collect_coefficients


def _collect(dag, con_out, jac):
    """Coefficient collection (``simplify.py``) over the defect equations and
    all their partials at once, so that sharing between them is seen.
    ``OPTY_COLLECT=0`` turns it off (A/B measurements)."""
    if os.environ.get('OPTY_COLLECT', '1') == '0':
        return con_out, jac
    width = len(jac[0]) if jac else 0
    new = collect_coefficients(dag, list(con_out) +
                               [node for row in jac for node in row])
    M = len(con_out)
    return new[:M], [new[M + j*width:M + (j + 1)*width]
                     for j in range(len(jac))]


class CollocationProgram(object):
    """Plain data; consumed by :mod:`opty_amd.codegen.emit_hip`.

    ``layout``: 'coo' or 'csr'; ``row_start[j]`` = first stored entry of
    equation j in ``jac_out`` when the entries are grouped by row (always true
    for 'csr' and for the unpruned 'coo' block).

    Attributes
    ----------
    dag : ir.DAG
    con_out : list of M node ids (defect equations)
    jac_out : list of M*C node ids, row-major ``[j*C + k]``
    inst_con_out / inst_jac_out : node ids of the instance constraints and of
        their partials (in the order of ``jacobian_indices``' tail)
    rows : list, one entry per trajectory row ``('free', k)`` (row ``k`` of
        the ``free`` vector viewed as ``(n+q, N)``) or ``('known', j)``
    cur_offset / adj_offset : time-node offset of the current / adjacent
        value relative to the constraint node (BE: 1/0, midpoint: 0/1)
    pars : list, one entry per parameter ``('known', k)`` or ``('tail', j)``
        (``free[(n+q)*N + j]``)
    h : ``('fixed',)`` or ``('tail', r)``
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def P(self):
        """Values stored per constraint node: M*C for the reference's dense
        block, fewer when structural zeros are pruned."""
        return len(self.jac_out)


def _front_end(discrete_eom, state_cur, state_adj, traj_cur, traj_adj,
               parameters, h_sym, method):
    """``(dag, symbol table, con_out)`` every builder starts from: the DAG
    inputs of the discrete symbols, in one fixed order (the node ids of an
    emitted source depend on it), and the lowered defect equations."""
    dag = ir.DAG()
    n = len(state_cur)
    table = {}
    for k, s in enumerate(state_cur):
        table[s] = dag.input('cur', k)
    for k, s in enumerate(state_adj):
        table[s] = dag.input('adj', k)
    for k, s in enumerate(traj_cur):
        table[s] = dag.input('cur', n + k)
    if method == 'midpoint':
        for k, s in enumerate(traj_adj):
            table[s] = dag.input('adj', n + k)
    for k, s in enumerate(parameters):
        table[s] = dag.input('par', k)
    table[h_sym] = dag.input('h', 0)
    low = Lowerer(dag, table)
    return dag, table, [low.lower(e) for e in discrete_eom]


def _layout(state_cur, traj_cur, num_known_traj, parameters, num_known_par,
            variable_duration, method):
    """Keyword arguments of a :class:`CollocationProgram` that say where the
    DAG inputs live in device memory (the same for every builder)."""
    n, m = len(state_cur), len(traj_cur)
    q = m - num_known_traj
    r = len(parameters) - num_known_par
    # row r of the slab: states then unknown inputs come from `free`
    # (``free`` viewed as (n+q, N), opty/utils.py:308-318); known inputs from
    # the known-trajectory buffer.  input_trajectories = known + unknown.
    rows = [('free', k) for k in range(n)]
    rows += [('known', j) for j in range(num_known_traj)]
    rows += [('free', n + j) for j in range(q)]
    pars = [('known', k) for k in range(num_known_par)]
    pars += [('tail', j) for j in range(r)]
    return dict(
        n=n, m=m, q=q, r=r, s=int(variable_duration),
        num_known_traj=num_known_traj, num_known_par=num_known_par,
        rows=rows, pars=pars, method=method,
        h=('tail', r) if variable_duration else ('fixed',),
        cur_offset=1 if method == 'backward euler' else 0,
        adj_offset=0 if method == 'backward euler' else 1)


def _lower_instance(dag, exprs, atom_syms, grads, known_pars,
                    skip_constants):
    """Lowers the instance constraints into ``dag`` over the inputs ``('free',
    a)`` of their atoms and the known parameters: yields ``(k, node of
    expression k, nodes of its atoms)``.  ``skip_constants``: an expression
    without atoms is not lowered at all."""
    itable = {s: dag.input('free', a) for a, s in enumerate(atom_syms)}
    for k, s in enumerate(known_pars):
        itable[s] = dag.input('par', k)
    ilow = Lowerer(dag, itable)
    for k, (e, atoms) in enumerate(zip(exprs, grads)):
        if atoms or not skip_constants:
            yield k, ilow.lower(e), [itable[s] for s in atoms]


def build_program(discrete_eom, state_cur, state_adj, traj_cur, traj_adj,
                  num_known_traj, parameters, num_known_par, h_sym,
                  variable_duration, wrt, method, instance=None,
                  implicit=(), prune_zeros=False, layout='coo'):
    """Lowers the discretised equations and differentiates them.

    Parameters mirror the reference's locals: ``state_cur``/``state_adj`` are
    the ``xi`` and ``xp`` (backward Euler) or ``xn`` (midpoint) symbols,
    ``traj_cur``/``traj_adj`` the ``si``/``sn`` symbols of *all* m input
    trajectories (known first), ``parameters`` known-then-unknown, ``wrt`` the
    column order of ``opty/direct_collocation.py:2719-2737``.

    ``implicit``: ``[(k, state, kd)]`` -- input trajectory ``k`` is a known
    function ``r(x_state(t))`` whose derivative ``dr/dx`` is input trajectory
    ``kd`` (``opty/direct_collocation.py:2080-2093``): its discrete symbol is an
    applied function ``r_i(x_i)``, lowered as a plain input row that carries a
    chain-rule link for the Jacobian.

    ``layout``: ``'coo'`` stores the values in the reference's order (node
    major, ``opty/direct_collocation.py:2644-2675``); ``'csr'`` stores them
    sorted by constraint row, then column -- equation-major rows
    ``j*(N-1) + i``, each row's entries in ascending free index -- the order a
    compressed-sparse-row consumer needs (opt-in: changes the index contract).

    ``instance``: optional ``(expressions, atom_symbols, known_par_syms)`` --
    instance constraints written over one placeholder Symbol per function
    atom; lowered into the same DAG with INPUT kind ``'free'``.
    """
    dag, table, con_out = _front_end(discrete_eom, state_cur, state_adj,
                                     traj_cur, traj_adj, parameters, h_sym,
                                     method)
    n, q = len(state_cur), len(traj_cur) - num_known_traj
    # (the links' inputs are all in the table already: no new node)
    chain = {}
    for k, st, kd in implicit:
        chain[dag.input('cur', n + k)] = [(dag.input('cur', st),
                                           dag.input('cur', n + kd))]
        if method == 'midpoint':
            chain[dag.input('adj', n + k)] = [(dag.input('adj', st),
                                               dag.input('adj', n + kd))]
    wrt_nodes = [table[s] for s in wrt]
    jac = forward_jacobian(dag, con_out, wrt_nodes, chain)
    con_out, jac = _collect(dag, con_out, jac)
    # (j, k) of every stored entry of the block, row-major.  The reference
    # stores all M*C of them, structural zeros included
    # (opty/direct_collocation.py:2589-2593); ``prune_zeros`` (opt-in, changes
    # the index contract) keeps only entries whose partial is not identically
    # zero.
    pattern = [(j, k) for j, row in enumerate(jac) for k, node in
               enumerate(row) if not (prune_zeros and node == dag.zero)]
    if layout == 'csr':
        # the column of wrt entry k of node i is monotone in this key for
        # every i (N >= 2): states interleave adjacent/current, then inputs,
        # then the parameter tail
        key = _column_key(n, q, method)
        pattern.sort(key=lambda jk: (jk[0], key(jk[1])))
    elif layout != 'coo':
        raise ValueError('layout must be "coo" or "csr".')
    jac_out = [jac[j][k] for j, k in pattern]
    row_start = [0]*(len(con_out) + 1)
    for j, _ in pattern:
        row_start[j + 1] += 1
    for j in range(len(con_out)):
        row_start[j + 1] += row_start[j]

    inst_con_out, inst_jac_out, num_atoms = [], [], 0
    if instance is not None:
        exprs, atom_syms, grads = instance
        num_atoms = len(atom_syms)
        for _, node, nodes in _lower_instance(
                dag, exprs, atom_syms, grads, parameters[:num_known_par],
                skip_constants=False):
            inst_con_out.append(node)
            if nodes:
                inst_jac_out += forward_jacobian(dag, [node], nodes)[0]

    return CollocationProgram(
        dag=dag, con_out=con_out, jac_out=jac_out, M=len(con_out),
        C=len(wrt), inst_con_out=inst_con_out, inst_jac_out=inst_jac_out,
        num_inst_atoms=num_atoms, pattern=pattern,
        pruned=bool(prune_zeros), layout=layout, row_start=row_start,
        **_layout(state_cur, traj_cur, num_known_traj, parameters,
                  num_known_par, variable_duration, method))


def column_side(n, q, method, k):
    """Where wrt column ``k`` of the block lives in ``free`` at constraint
    node i (the closed form of ``_column_key``): ``(row, off)`` -- free index
    ``row*N + i + off`` -- or ``(-1, j)`` -- the tail entry ``(n+q)*N + j``
    (unknown parameter / free interval)."""
    be = method == 'backward euler'
    cur, adj = (1, 0) if be else (0, 1)
    if k < n:
        return k, cur
    if k < 2*n:
        return k - n, adj
    j = k - 2*n
    if j < q:
        return n + j, cur
    if not be and j < 2*q:
        return n + j - q, adj
    return -1, j - (q if be else 2*q)


def _side_order(side):
    """Sort key equal to the order of the free index of a side at every
    node (N >= 2): trajectory rows first, by row then offset; the tail
    last."""
    row, off = side
    return (1, off, 0) if row < 0 else (0, row, off)


class HessianProgram(CollocationProgram):
    """Plain data of a Hessian program (:func:`build_hessian_program`).

    ``hess_out``: PH node ids, one per stored entry of a constraint node;
    ``hess_pairs[e] = (a, b)``: the wrt columns of entry ``e`` with ``a`` the
    row -- the larger GLOBAL free index -- and ``b`` the column;
    ``inst_hess_out``: node ids of the instance constraints' second partials
    (NOT multiplied by their multipliers), ``inst_hess_con[t]`` the
    instance constraint of entry ``t``, ``inst_hess_atoms[t] = (a, b)`` its
    atoms (indices into the atom list, free index of ``a`` >= that of
    ``b``)."""

    @property
    def PH(self):
        return len(self.hess_out)

    def index_pattern(self):
        """``[(row_a, off_a, row_b, off_b)]`` per stored entry
        (:func:`column_side` of both columns)."""
        return [column_side(self.n, self.q, self.method, a) +
                column_side(self.n, self.q, self.method, b)
                for a, b in self.hess_pairs]


def hessian_indices(prog, N, atom_free_index):
    """Closed-form ``(rows, cols)`` (int64) of every value of a Hessian
    program for ``N`` collocation nodes: node-major blocks
    ``[i*PH + e]``, then the instance entries; ``atom_free_index[a]`` = free
    index of instance atom ``a``."""
    import numpy as np
    pat = np.array(prog.index_pattern(), dtype=np.int64).reshape(-1, 4)
    i = np.arange(N - 1, dtype=np.int64)[:, None]
    tail = (prog.n + prog.q)*N

    def side(row, off):
        return np.where(row >= 0, row*N + i + off, tail + off)
    rows = side(pat[:, 0], pat[:, 1]).ravel()
    cols = side(pat[:, 2], pat[:, 3]).ravel()
    idx = np.asarray(atom_free_index, dtype=np.int64)
    irows = np.array([idx[a] for a, _ in prog.inst_hess_atoms],
                     dtype=np.int64)
    icols = np.array([idx[b] for _, b in prog.inst_hess_atoms],
                     dtype=np.int64)
    return np.concatenate((rows, irows)), np.concatenate((cols, icols))


def build_hessian_program(discrete_eom, state_cur, state_adj, traj_cur,
                          traj_adj, num_known_traj, parameters, num_known_par,
                          h_sym, variable_duration, wrt, method,
                          instance=None, implicit=()):
    """The exact Hessian of the constraint Lagrangian: arguments as
    :func:`build_program`'s (same lowering, same ``wrt`` columns, same
    implicit inputs).  At every constraint node it forms
    ``L_i = sum_j lam_j c_j`` over INPUT nodes ``('lam', j)``, differentiates
    it twice with :func:`lower.forward_jacobian` over the block's C columns
    and keeps the structurally nonzero entries of the LOWER triangle --
    lower on the global free indices: the same orientation at every node
    (:func:`column_side`), so the per-node pattern is closed form.  Instance
    constraint ``k`` contributes the second partials of its expression with
    respect to its atoms (the caller multiplies them by ``lagrange[M*(N-1) +
    k]``); ``instance`` is ``(expressions, atom symbols, atoms per
    expression, free index per atom)``.

    Implicit known trajectories are refused: only ``dr/dx`` is known, the
    second derivative is not."""
    if implicit:
        raise NotImplementedError(
            'the Hessian of a problem with implicit known trajectories (a '
            'known r(x(t)) with only dr/dx given) is not available: the '
            'second derivative of r is unknown.')
    dag, table, con_out = _front_end(discrete_eom, state_cur, state_adj,
                                     traj_cur, traj_adj, parameters, h_sym,
                                     method)
    n, q = len(state_cur), len(traj_cur) - num_known_traj
    lag = dag.sum([dag.mul(dag.input('lam', j), c)
                   for j, c in enumerate(con_out)])
    wrt_nodes = [table[s] for s in wrt]
    C = len(wrt)
    grad = forward_jacobian(dag, [lag], wrt_nodes)[0]
    hess = forward_jacobian(dag, grad, wrt_nodes)
    order = {k: _side_order(column_side(n, q, method, k)) for k in range(C)}
    pairs = sorted(((a, b) for a in range(C) for b in range(C)
                    if order[a] >= order[b] and hess[a][b] != dag.zero),
                   key=lambda ab: (order[ab[0]], order[ab[1]]))
    out = [hess[a][b] for a, b in pairs]
    if out and os.environ.get('OPTY_COLLECT', '1') != '0':
        out = collect_coefficients(dag, out)
    kept = [k for k, node in enumerate(out) if node != dag.zero]
    pairs = [pairs[k] for k in kept]
    out = [out[k] for k in kept]

    inst_out, inst_con, inst_atoms, num_atoms = [], [], [], 0
    if instance is not None:
        exprs, atom_syms, grads, free_index = instance
        num_atoms = len(atom_syms)
        pos = {s: a for a, s in enumerate(atom_syms)}
        for k, node, nodes in _lower_instance(
                dag, exprs, atom_syms, grads, parameters[:num_known_par],
                skip_constants=True):
            atoms = grads[k]
            g = forward_jacobian(dag, [node], nodes)[0]
            H = forward_jacobian(dag, g, nodes)
            fi = [free_index[pos[s]] for s in atoms]
            # every ORDERED pair on or below the diagonal of the free
            # indices: two distinct atoms at the same free index (theta(0)
            # and theta(0.001) both closest to node 0) put both of their
            # mixed partials on that diagonal entry
            for a in range(len(atoms)):
                for b in range(len(atoms)):
                    if (fi[a] > fi[b] or fi[a] == fi[b] and
                            (a >= b or atoms[a] != atoms[b])) and \
                            H[a][b] != dag.zero:
                        inst_out.append(H[a][b])
                        inst_con.append(k)
                        inst_atoms.append((pos[atoms[a]], pos[atoms[b]]))

    return HessianProgram(
        dag=dag, hess_out=out, hess_pairs=pairs, con_out=con_out, jac_out=[],
        M=len(con_out), C=C, inst_hess_out=inst_out, inst_hess_con=inst_con,
        inst_hess_atoms=inst_atoms, num_inst_atoms=num_atoms,
        **_layout(state_cur, traj_cur, num_known_traj, parameters,
                  num_known_par, variable_duration, method))


class JacobianProductProgram(CollocationProgram):
    """Plain data of a Jacobian-product program
    (:func:`build_jacobian_product_program`).

    ``tan_out``: M node ids, the directional derivative of every defect
    equation along ``v``; ``adj_out``: C node ids, ``d/d col_k sum_j lam_j
    c_j``; ``adj_sides[k]``: :func:`column_side` of column ``k``;
    ``inst_jac_out``: the instance constraints' first partials,
    ``inst_pairs[t] = (k, a)`` the constraint and the atom (index into the
    atom list) of partial ``t``."""

    def row_columns(self):
        """``[(row, lo, hi)]`` per ``free`` trajectory row: the adjoint
        columns whose free index is ``row*N + i`` (``lo``) and ``row*N + i +
        1`` (``hi``) at constraint node ``i``; None where the block has no
        such column."""
        rows = [[r, None, None] for r in range(self.n + self.q)]
        for k, (row, off) in enumerate(self.adj_sides):
            if row >= 0:
                rows[row][1 + off] = k
        return [tuple(r) for r in rows]

    def tail_columns(self):
        """``[(j, k)]``: adjoint column ``k`` is the tail entry ``(n+q)*N +
        j`` of ``free`` (unknown parameter / free interval)."""
        return sorted((off, k) for k, (row, off) in enumerate(self.adj_sides)
                      if row < 0)


def build_jacobian_product_program(discrete_eom, state_cur, state_adj,
                                   traj_cur, traj_adj, num_known_traj,
                                   parameters, num_known_par, h_sym,
                                   variable_duration, wrt, method,
                                   instance=None, implicit=()):
    """Matrix-free products with the constraint Jacobian: arguments as
    :func:`build_program`'s (same lowering, same ``wrt`` columns, same
    implicit inputs).  Two sets of roots on one DAG:

    * the TANGENT of every defect equation along a direction ``v`` shaped
      like ``free``: ONE tangent is pushed through the DAG
      (:func:`lower.forward_jacobian` with a single pseudo-column ``('dir',
      0)`` whose seeds arrive through ``chain``: column ``k``'s seed is the
      INPUT ``('vcur' | 'vadj' | 'vpar' | 'vh', index)`` with the kind and
      index of the column's own input), so the cost is a small multiple of
      the constraint evaluation's, not of the Jacobian's;
    * the ADJOINT ``d/d col_k sum_j lam_j c_j`` over the per-node inputs
      ``('lam', j)``, which carry ``w`` (the first half of
      :func:`build_hessian_program`).

    Both sweeps use the angle-difference rule of
    :func:`lower.forward_jacobian` (``angle_pairs``): the mass-matrix and
    centripetal factors of a chain of bodies are differentiated in three
    operations instead of seven.

    Implicit known trajectories stay supported (only ``dr/dx`` is needed):
    the tangent of ``r_i`` is ``dr_i v_x``, the adjoint goes through the
    same ``chain`` as :func:`build_program`'s.  The instance constraints
    contribute their first partials as in the Jacobian program."""
    tan, adj, parts = _product_parts(
        discrete_eom, state_cur, state_adj, traj_cur, traj_adj,
        num_known_traj, parameters, num_known_par, h_sym, variable_duration,
        wrt, method, instance, implicit, 1)
    return JacobianProductProgram(tan_out=tan[0], adj_out=adj[0], **parts)


def _product_parts(discrete_eom, state_cur, state_adj, traj_cur, traj_adj,
                   num_known_traj, parameters, num_known_par, h_sym,
                   variable_duration, wrt, method, instance, implicit,
                   columns):
    """What the single and the block product program share: ``(tan, adj,
    parts)`` -- the tangent roots ``tan[c][j]`` and the adjoint roots
    ``adj[c][k]`` of each of the ``columns`` columns, and the other keyword
    arguments of the program.  Column ``c``'s inputs have the indices of
    :func:`ir.split_column`; with one column the DAG is the single
    program's, node for node."""
    dag, table, con_out = _front_end(discrete_eom, state_cur, state_adj,
                                     traj_cur, traj_adj, parameters, h_sym,
                                     method)
    n, q = len(state_cur), len(traj_cur) - num_known_traj
    collect = os.environ.get('OPTY_COLLECT', '1') != '0'
    if collect:
        # the compact form FIRST: both sweeps then differentiate one
        # multiplication per collected term, not one per expanded term
        con_out = collect_coefficients(dag, con_out)
    wrt_nodes = [table[s] for s in wrt]
    C, M, K = len(wrt), len(con_out), int(columns)
    stride = ir.COLUMN_STRIDE

    chain = {}
    seeds = [dag.input('dir', stride*c) for c in range(K)]
    tchain = {}
    for node in wrt_nodes:
        kind, idx = dag.args[node]
        tchain[node] = [(seeds[c], dag.input('v' + kind, idx + stride*c))
                        for c in range(K)]
    for k, st, kd in implicit:
        sides = ['cur'] + (['adj'] if method == 'midpoint' else [])
        for side in sides:
            link = dag.input(side, n + k)
            dr = dag.input(side, n + kd)
            chain[link] = [(dag.input(side, st), dr)]
            tchain[link] = [
                (seeds[c], dag.mul(dr, dag.input('v' + side, st + stride*c)))
                for c in range(K)]
    rows = forward_jacobian(dag, con_out, seeds, tchain, angle_pairs=True)
    flat_tan = [rows[j][c] for c in range(K) for j in range(M)]
    lags = [dag.sum([dag.mul(dag.input('lam', j + stride*c), cj)
                     for j, cj in enumerate(con_out)]) for c in range(K)]
    flat_adj = [node for row in forward_jacobian(
        dag, lags, wrt_nodes, chain, angle_pairs=True) for node in row]
    if collect:
        # ... and once more over each kernel's own roots (the two sets never
        # meet in one kernel); kept where it pays: re-collecting the
        # derivative of an already collected sum can also undo sharing
        def cost(roots):
            return sum(dag.count_ops(roots).values())
        flat_tan = min(flat_tan, collect_coefficients(dag, list(flat_tan)),
                       key=cost)
        flat_adj = min(flat_adj, collect_coefficients(dag, list(flat_adj)),
                       key=cost)
    tan = [flat_tan[c*M:(c + 1)*M] for c in range(K)]
    adj = [flat_adj[c*C:(c + 1)*C] for c in range(K)]

    inst_jac_out, inst_pairs, num_atoms, num_inst = [], [], 0, 0
    if instance is not None:
        exprs, atom_syms, grads = instance
        num_atoms = len(atom_syms)
        num_inst = len(exprs)
        pos = {s: a for a, s in enumerate(atom_syms)}
        for k, node, nodes in _lower_instance(
                dag, exprs, atom_syms, grads, parameters[:num_known_par],
                skip_constants=True):
            inst_jac_out += forward_jacobian(dag, [node], nodes)[0]
            inst_pairs += [(k, pos[s]) for s in grads[k]]

    return tan, adj, dict(
        dag=dag, con_out=con_out, jac_out=[],
        adj_sides=[column_side(n, q, method, k) for k in range(C)],
        M=M, C=C, inst_jac_out=inst_jac_out,
        inst_pairs=inst_pairs, num_inst=num_inst, num_inst_atoms=num_atoms,
        **_layout(state_cur, traj_cur, num_known_traj, parameters,
                  num_known_par, variable_duration, method))


class JacobianBlockProductProgram(JacobianProductProgram):
    """Plain data of a block product program
    (:func:`build_jacobian_block_product_program`): a
    :class:`JacobianProductProgram` whose ``tan_out[c]`` / ``adj_out[c]`` are
    the M tangent / C adjoint roots of column ``c`` of ``columns``, over the
    column's own inputs (:func:`ir.split_column`).  ``adj_sides``,
    ``row_columns()``, ``tail_columns()`` and the instance partials do not
    depend on the column."""


def build_jacobian_block_product_program(discrete_eom, state_cur, state_adj,
                                         traj_cur, traj_adj, num_known_traj,
                                         parameters, num_known_par, h_sym,
                                         variable_duration, wrt, method,
                                         instance=None, implicit=(),
                                         columns=4):
    """``J V`` and ``J^T W`` for ``columns`` columns at once: arguments and
    construction as :func:`build_jacobian_product_program`'s, on ONE DAG --
    one tangent sweep with a pseudo-column ``('dir', c)`` per column of ``V``
    (seeds: the column's own ``vcur`` / ``vadj`` / ``vpar`` / ``vh``; the
    implicit-trajectory rule ``dr v_x`` per column) and one adjoint sweep
    over the ``columns`` Lagrangians ``sum_j lam_j^(c) c_j``.  What does not
    depend on the direction -- trig, the collected coefficients, the
    mass-matrix factors -- is one node for all columns."""
    if int(columns) < 1:
        raise ValueError('columns must be at least 1, got %r' % (columns,))
    tan, adj, parts = _product_parts(
        discrete_eom, state_cur, state_adj, traj_cur, traj_adj,
        num_known_traj, parameters, num_known_par, h_sym, variable_duration,
        wrt, method, instance, implicit, columns)
    return JacobianBlockProductProgram(tan_out=tan, adj_out=adj,
                                       columns=int(columns), **parts)


def assemble_jvp(prog, N, tan, inst, v, atom_free_index):
    """``J v`` from the values of a product program's roots: ``tan`` the M
    tangent roots at the N-1 constraint nodes (scalars broadcast), ``inst``
    the instance partials; in the order of ``constraints(free)``.  The host
    counterpart of ``opty_jvp`` / ``opty_jvp_inst`` (tests, verification)."""
    import numpy as np
    ncn = N - 1
    out = np.zeros(prog.M*ncn + prog.num_inst)
    for j in range(prog.M):
        out[j*ncn:(j + 1)*ncn] = tan[j]
    for t, (k, a) in enumerate(prog.inst_pairs):
        out[prog.M*ncn + k] += inst[t]*v[atom_free_index[a]]
    return out


def assemble_vjp(prog, N, adj, inst, w, atom_free_index):
    """``J^T w`` from the values of a product program's roots: ``adj`` the C
    adjoint roots at the N-1 constraint nodes; ordered like ``free``.  The
    host counterpart of ``opty_vjp`` / ``opty_vjp_fin``."""
    import numpy as np
    ncn = N - 1
    tail = (prog.n + prog.q)*N
    out = np.zeros(tail + prog.r + prog.s)
    for k, (row, off) in enumerate(prog.adj_sides):
        val = np.broadcast_to(np.asarray(adj[k], dtype=float), (ncn,))
        if row >= 0:
            out[row*N + off:row*N + off + ncn] += val
        else:
            out[tail + off] += val.sum()
    for t, (k, a) in enumerate(prog.inst_pairs):
        out[atom_free_index[a]] += inst[t]*w[prog.M*ncn + k]
    return out


def hessian_side_table(pattern, obj_pattern=(), obj_base=0):
    """The side slots of a Hessian product (``opty_hessmv``): relative to a
    node every side of an entry of the node section (``pattern``,
    :meth:`HessianProgram.index_pattern`) and of the objective section
    (``obj_pattern``, slot = ``obj_base`` + offset) is ``(row, slot)`` with
    ``slot`` in {0, 1} -- free index ``row*N + i + slot`` -- or a tail entry
    ``(-1, offset)``.  Returns ``(sides, num_trajectory, entries,
    obj_entries)``: the distinct sides, trajectory sides first in ascending
    ``(row, slot)`` order, then the tail sides by offset; ``entries[e] = (slot
    of side a, slot of side b)`` per node entry, ``obj_entries`` the same per
    objective entry."""
    def sides_of(pat, base):
        out = []
        for ra, oa, rb, ob in [tuple(int(x) for x in e) for e in pat]:
            pair = []
            for row, off in ((ra, oa), (rb, ob)):
                side = (row, base + off) if row >= 0 else (-1, off)
                if row < -1 or (row >= 0 and side[1] not in (0, 1)) or \
                        (row < 0 and off < 0):
                    raise ValueError('side (%d, %d) is neither (row, slot in '
                                     '{0, 1}) nor a tail entry' % side)
                pair.append(side)
            out.append(tuple(pair))
        return out
    node, obj = sides_of(pattern, 0), sides_of(obj_pattern, int(obj_base))
    distinct = {side for pair in node + obj for side in pair}
    sides = sorted(distinct, key=_side_order)
    slot = {side: k for k, side in enumerate(sides)}
    return (sides, sum(1 for row, _ in sides if row >= 0),
            [(slot[a], slot[b]) for a, b in node],
            [(slot[a], slot[b]) for a, b in obj])


#: bytes of the value tile of ``opty_hessmv`` (64 nodes, pitch 33 doubles) and
#: of one side's ``v`` and accumulator over the 64 lanes, per column
HESSMV_TILE_BYTES = 64*33*8
HESSMV_SIDE_BYTES = 2*64*8


def hessian_block_width(num_sides, lds_limit):
    """Columns one pass of a block product ``H V`` takes: the largest ``K``
    of 4, 3, 2 for which the LDS of ``opty_hessmv_block<K>``, ``16 896 +
    1 024*K*num_sides`` bytes, is within ``lds_limit`` (the device's LDS per
    block); 1 when not even two columns fit (every column then goes through
    ``opty_hessmv``).  The rule ``opty_hip_hessmv_create`` applies."""
    for width in (4, 3, 2):
        if HESSMV_TILE_BYTES + HESSMV_SIDE_BYTES*width*int(num_sides) <= \
                int(lds_limit):
            return width
    return 1


def assemble_hessmv(N, num_rows, num_tail, values, v, pattern, inst_rows=(),
                    inst_cols=(), obj_pattern=(), obj_base=0, tail_rows=(),
                    tail_cols=()):
    """``y = H v`` from the stored triplets, ``H`` the symmetric matrix whose
    lower triangle is the sum of the triplets; ``values`` laid out ``[node
    section (i*PH + e) | instance entries | objective section (e*(N-1) + j) |
    parameter-parameter entries]``, ``num_rows = n + q`` trajectory rows and
    ``num_tail`` tail entries of ``free``.  The host statement of
    ``opty_hessmv`` / ``opty_hessmv_fin``: per side slot ``S`` the sum over
    the entries of node ``i`` of ``value * v[other side]`` (a diagonal entry
    once), then ``y[R*N + p] = S_R0(p) + S_R1(p - 1)`` with the missing term
    dropped at both ends, a tail entry the sum over all nodes, and last the
    explicit triplets in stored order."""
    import numpy as np
    N, ncn = int(N), int(N) - 1
    sides, ntraj, entries, obj_entries = hessian_side_table(
        pattern, obj_pattern, obj_base)
    PH, E = len(entries), len(obj_entries)
    ni, nt = len(inst_rows), len(tail_rows)
    values = np.asarray(values, dtype=float)
    v = np.asarray(v, dtype=float)
    tail = num_rows*N
    assert values.shape == ((PH + E)*ncn + ni + nt,)
    assert v.shape == (tail + num_tail,)
    node = values[:PH*ncn].reshape(ncn, PH)
    inst = values[PH*ncn:PH*ncn + ni]
    obj = values[PH*ncn + ni:PH*ncn + ni + E*ncn].reshape(E, ncn)
    par = values[PH*ncn + ni + E*ncn:]
    i = np.arange(ncn)
    at = [np.broadcast_to(v[row*N + i + off] if row >= 0 else v[tail + off],
                          (ncn,)) for row, off in sides]
    S = np.zeros((len(sides), ncn))
    for val, table in ((node.T, entries), (obj, obj_entries)):
        for e, (a, b) in enumerate(table):
            S[a] += val[e]*at[b]
            if a != b:
                S[b] += val[e]*at[a]
    y = np.zeros(tail + num_tail)
    for k, (row, off) in enumerate(sides):
        if row >= 0:
            # slot 0: p = i; slot 1: p = i + 1
            y[row*N + off:row*N + off + ncn] += S[k]
        else:
            y[tail + off] += S[k].sum()
    for rows, cols, val in ((inst_rows, inst_cols, inst),
                            (tail_rows, tail_cols, par)):
        for r, c, a in zip(rows, cols, val):
            y[r] += a*v[c]
            if r != c:
                y[c] += a*v[r]
    return y


#: nodes a block of ``opty_hessmv`` advances by (64 lanes, one repeated node)
HESSMV_STRIDE = 63


def hessmv_window_owned(N, a, b):
    """``(lo, hi)``: the time nodes whose trajectory entries of ``H v`` the
    window ``[a, b)`` of the ``N - 1`` constraint nodes owns -- its nodes' and,
    for a non-empty window that ends the problem, node ``N - 1``."""
    a, b = int(a), int(b)
    return a, b + (1 if a < b == int(N) - 1 else 0)


def hessmv_window_blocks(N, a, b):
    """Blocks of ``opty_hessmv`` over the window ``[a, b)``: block 0 of a
    window that starts the problem stores 64 time nodes, every other block 63
    (its lane 0 is the halo node or repeats a node); at least one for a
    non-empty window, none for an empty one.  ``[0, N - 1)`` gives the
    whole-problem launch, ``ceil((N - 1)/63)``."""
    lo, hi = hessmv_window_owned(N, a, b)
    if int(b) <= int(a):
        return 0
    todo = hi - lo - (1 if lo == 0 else 0)
    return max(1, -(-todo//HESSMV_STRIDE))


def assemble_hessmv_window(N, num_rows, num_tail, values_shard, inst_values,
                           v, pattern, a, b, tail_owner, inst_rows=(),
                           inst_cols=()):
    """One window of :func:`assemble_hessmv` over the constraint section: the
    host statement of ``opty_hip_hessmv_apply_shard``.  ``values_shard`` holds
    the nodes ``[a - (a > 0), b)`` (one halo node in front of a window that
    does not start the problem), ``inst_values`` the instance entries, ``v``
    is the GLOBAL vector.  Returns ``(block, tail_part)``: ``block[R, p - a]``
    is entry ``R*N + p`` of ``H v`` for the owned time nodes
    (:func:`hessmv_window_owned`), with the operations of
    :func:`assemble_hessmv` in its order -- the same bits --; ``tail_part``
    (``num_tail`` doubles) the sum over the window's own nodes per tail
    entry and, for the ``tail_owner``, the instance triplets' tail sides on
    top.  An instance side at a trajectory entry goes to the window that owns
    the entry; every other side is skipped."""
    import numpy as np
    N, a, b = int(N), int(a), int(b)
    sides, ntraj, entries, _ = hessian_side_table(pattern)
    PH = len(entries)
    first = a - (1 if a > 0 else 0) if b > a else a
    nodes = np.arange(first, b)
    lo, hi = hessmv_window_owned(N, a, b)
    v = np.asarray(v, dtype=float)
    tail = num_rows*N
    assert v.shape == (tail + num_tail,)
    node = np.asarray(values_shard, dtype=float)[:len(nodes)*PH].reshape(
        len(nodes), PH)
    at = [np.broadcast_to(v[row*N + nodes + off] if row >= 0
                          else v[tail + off], nodes.shape)
          for row, off in sides]
    S = np.zeros((len(sides), len(nodes)))
    for e, (sa, sb) in enumerate(entries):
        S[sa] += node[:, e]*at[sb]
        if sa != sb:
            S[sb] += node[:, e]*at[sa]
    block = np.zeros((num_rows, hi - lo))
    tail_part = np.zeros(num_tail)
    for k, (row, off) in enumerate(sides):
        if row >= 0:
            p = nodes + off
            keep = (p >= lo) & (p < hi)
            block[row, p[keep] - lo] += S[k][keep]
        else:
            tail_part[off] += S[k][nodes >= a].sum()
    for r, c, x in zip(inst_rows, inst_cols,
                       np.asarray(inst_values, dtype=float)):
        for at_, other in ((r, c),) if r == c else ((r, c), (c, r)):
            if at_ >= tail:
                if tail_owner:
                    tail_part[at_ - tail] += x*v[other]
            else:
                R, p = divmod(int(at_), N)
                if lo <= p < hi:
                    block[R, p - lo] += x*v[other]
    return block, tail_part


#: nodes a block of ``opty_hesscsr`` advances by (64 lanes, one repeated node)
HESSCSR_STRIDE = 63


def hesscsr_lds_bytes(width):
    """LDS of one block of ``opty_hesscsr`` when the widest row class spans
    ``width`` consecutive node entries (from the first to the last entry whose
    row side is in the class): the tile of a group of classes -- ``max(64,
    width)`` entries of the block's 64 nodes at an odd pitch --, the 64 x 33
    output tile, one row start per lane.  The rule
    ``opty_hip_hesscsr_create`` applies."""
    return 8*(64*(max(64, int(width)) | 1) + 64*33 + 64)


class _HessianCsrPlan(object):
    """Where every triplet of the Hessian goes in the CSR lower triangle
    (:func:`hessian_csr_structure`).  A *source* of an output is a code ``2*e
    + back``: entry ``e`` of the combined per-node list (node section, then
    objective section) at node ``p - back``, ``p`` the time node of the
    output.

    ``runs``: ``(out, p, codes, row, off)`` -- the outputs ``out`` (an index
    array into ``data``) of the time nodes ``p`` are the sums of the sources
    ``codes``, their columns are ``row*N + p + off``; ``items``: ``(out,
    col, positions, long_codes)`` -- one output each, the sum of the values
    at ``positions`` (ascending) on top of, for a tail x tail pair with
    per-node sources, the long sum of ``long_codes`` over all nodes.

    ``with_diagonal``: every row gets its diagonal pair -- an empty source
    list for ``(R, 0)`` in every trajectory row class, in every whole row and
    in every tail row --; a pair that no triplet hits has no addends and
    evaluates to ``+0.0``.  The diagonal is the last entry of its row."""

    def __init__(self, N, num_rows, num_tail, pattern, inst_rows=(),
                 inst_cols=(), obj_pattern=(), obj_base=0, tail_rows=(),
                 tail_cols=(), with_diagonal=False):
        import numpy as np
        N = self.N = int(N)
        ncn = self.ncn = N - 1
        if ncn < 1:
            raise ValueError('N %d < 2' % N)
        num_rows, num_tail = int(num_rows), int(num_tail)
        sides, _, entries, obj_entries = hessian_side_table(
            pattern, obj_pattern, obj_base)
        PH = self.PH = len(entries)
        E = self.E = len(obj_entries)
        ni, nt = len(inst_rows), len(tail_rows)
        self.obj_at = PH*ncn + ni
        self.nnz = (PH + E)*ncn + ni + nt
        tail = num_rows*N
        self.num_free = num_free = tail + num_tail

        # per-node classes: trajectory row R -> {(R', column offset): codes},
        # tail row j -> {R': codes} (a segment of consecutive time nodes) and
        # {j': codes} (a long group)
        traj = [dict() for _ in range(num_rows)]
        segs = [dict() for _ in range(num_tail)]
        longs = [dict() for _ in range(num_tail)]
        for e, (sa, sb) in enumerate(list(entries) + list(obj_entries)):
            a, b = sides[sa], sides[sb]
            for row, off in (a, b):
                if row >= num_rows or (row < 0 and off >= num_tail):
                    raise ValueError('side (%d, %d) is outside the problem'
                                     % (row, off))
            if _side_order(a) < _side_order(b):
                raise ValueError('entry %d is above the diagonal: %s < %s'
                                 % (e, a, b))
            if a[0] >= 0:
                traj[a[0]].setdefault((b[0], b[1] - a[1]), []).append(
                    2*e + a[1])
            elif b[0] >= 0:
                segs[a[1]].setdefault(b[0], []).append(2*e + b[1])
            else:
                longs[a[1]].setdefault(b[1], []).append(2*e)
        if with_diagonal:
            for R in range(num_rows):
                traj[R].setdefault((R, 0), [])

        def in_order(codes):
            # ascending position in ``values``: node section, node p - 1
            # before node p; then the objective section, entry-major
            return sorted(codes, key=lambda c: (
                (1, c >> 1, 0) if c >> 1 >= PH else (0, 1 - (c & 1), c >> 1)))

        def valid(codes, p):
            return [c for c in codes if 0 <= p - (c & 1) < ncn]

        def traj_row(R, p):
            """{column: positions} of the regular pattern of row (R, p)."""
            out = {R*N + p: []} if with_diagonal else {}
            for (Rp, d), codes in traj[R].items():
                v = valid(codes, p)
                if v:
                    out[Rp*N + p + d] = [int(self.position(c, p)) for c in v]
            return out

        # explicit triplets: row -> {column: positions in stored order}
        explicit = {}
        for rows, cols, at in ((inst_rows, inst_cols, PH*ncn),
                               (tail_rows, tail_cols, self.obj_at + E*ncn)):
            for k, (r, c) in enumerate(zip(rows, cols)):
                r, c = int(r), int(c)
                if not 0 <= c <= r < num_free:
                    raise ValueError('explicit entry (%d, %d) is outside the '
                                     'lower triangle' % (r, c))
                explicit.setdefault(r, {}).setdefault(c, []).append(at + k)

        # whole rows that the closed form does not cover: the first and last
        # time node of every trajectory row and rows with explicit triplets
        whole = {}
        for R in range(num_rows):
            for p in (0, ncn):
                whole[R*N + p] = traj_row(R, p)
        for r, extra in explicit.items():
            if r < tail:
                row = whole.setdefault(r, traj_row(r // N, r % N))
                for c, at in extra.items():
                    row.setdefault(c, []).extend(at)

        # tail rows: segments in column order, explicit columns between them
        tail_rows_ = []
        for j in range(num_tail):
            seg = []
            for Rp in sorted(segs[j]):
                codes = in_order(segs[j][Rp])
                lo = 0 if any(c & 1 == 0 for c in codes) else 1
                hi = ncn if any(c & 1 for c in codes) else ncn - 1
                seg.append([Rp, lo, hi, codes, {}])
            extra, tcols = {}, {jp: [] for jp in longs[j]}
            if with_diagonal:
                tcols.setdefault(j, [])
            for c, at in explicit.get(tail + j, {}).items():
                if c >= tail:
                    tcols.setdefault(c - tail, []).extend(at)
                    continue
                hit = [s for s in seg
                       if s[0] == c // N and s[1] <= c % N <= s[2]]
                if hit:
                    hit[0][4][c % N] = at
                else:
                    extra[c] = at
            tail_rows_.append((seg, extra, tcols))

        lens = np.zeros(num_free, dtype=np.int64)
        for R in range(num_rows):
            lens[R*N + 1:R*N + ncn] = len(traj[R])
        for r, row in whole.items():
            lens[r] = len(row)
        for j, (seg, extra, tcols) in enumerate(tail_rows_):
            lens[tail + j] = sum(s[2] - s[1] + 1 for s in seg) + len(extra) \
                + len(tcols)
        indptr = self.indptr = np.concatenate(
            ([0], np.cumsum(lens))).astype(np.int64)
        self.nnz_unique = int(indptr[-1])

        runs, items = [], []
        for R in range(num_rows):
            p = np.arange(1, ncn, dtype=np.int64)
            p = p[~np.isin(R*N + p, list(whole))] if len(p) else p
            start = indptr[R*N + p]
            for k, key in enumerate(sorted(traj[R])):
                runs.append((start + k, p, in_order(traj[R][key])) + key)
        for r, row in whole.items():
            for k, c in enumerate(sorted(row)):
                items.append((int(indptr[r]) + k, c, sorted(row[c]), None))
        for j, (seg, extra, tcols) in enumerate(tail_rows_):
            at = int(indptr[tail + j])
            pieces = sorted([(s[0]*N + s[1], s) for s in seg] +
                            [(c, None) for c in extra], key=lambda t: t[0])
            for c, s in pieces:
                if s is None:
                    items.append((at, c, sorted(extra[c]), None))
                    at += 1
                    continue
                Rp, lo, hi, codes, on = s
                for a, b in ((0, 0), (1, ncn - 1), (ncn, ncn)):
                    a, b = max(a, lo), min(b, hi)
                    if a > b:
                        continue
                    p = np.arange(a, b + 1, dtype=np.int64)
                    p = p[~np.isin(p, list(on))] if on else p
                    runs.append((at + p - lo, p, valid(codes, a), Rp, 0))
                for q, more in on.items():
                    items.append((at + q - lo, Rp*N + q, sorted(
                        [int(self.position(c, q)) for c in valid(codes, q)]
                        + more), None))
                at += hi - lo + 1
            for jp in sorted(tcols):
                codes = in_order(longs[j].get(jp, []))
                items.append((at, tail + jp, list(tcols[jp]), codes or None))
                at += 1
            assert at == indptr[tail + j + 1]
        self.runs, self.items = runs, items

    def position(self, code, p):
        """Position in ``values`` of source ``code`` of time node(s) ``p``."""
        e, i = code >> 1, p - (code & 1)
        if e < self.PH:
            return i*self.PH + e
        return self.obj_at + (e - self.PH)*self.ncn + i

    def long_sum(self, values, codes):
        """The long sum of ``opty_hesscsr`` / ``opty_hesscsr_fin``: per node
        the sources in order from ``+0.0``; blocks of 64 lanes that advance
        by 63 nodes, lane 0 of a later block (the repeated node) and lanes
        past the last node count as ``0.0``; per block the tree ``x[l] +=
        x[l + d]`` for ``d`` = 32, 16 .. 1; the block partials in block order
        from ``+0.0``."""
        import numpy as np
        ncn = self.ncn
        node = np.zeros(ncn)
        i = np.arange(ncn, dtype=np.int64)
        for c in codes:
            node = node + values[self.position(c, i)]
        nblk = (ncn + HESSCSR_STRIDE - 1)//HESSCSR_STRIDE
        blk, lane = np.arange(nblk)[:, None], np.arange(64)[None, :]
        at = HESSCSR_STRIDE*blk + lane
        # (lane 0 of block b > 0 is node 63 b: lane 63 of block b - 1)
        counts = (at < ncn) & ~((lane == 0) & (blk > 0))
        x = np.where(counts, node[np.minimum(at, ncn - 1)], 0.0)
        for d in (32, 16, 8, 4, 2, 1):
            x[:, :d] = x[:, :d] + x[:, d:2*d]
        total = 0.0
        for b in range(nblk):
            total = total + x[b, 0]
        return total


def hessian_csr_structure(N, num_rows, num_tail, pattern, inst_rows=(),
                          inst_cols=(), obj_pattern=(), obj_base=0,
                          tail_rows=(), tail_cols=(), with_diagonal=False):
    """``(indptr, indices, slot)`` (int64) of the Hessian's lower triangle in
    compressed-sparse-row form over ``num_rows*N + num_tail`` rows: exactly
    the distinct ``(row, col)`` pairs of the triplets ``[node section (i*PH +
    e) | instance entries | objective section (e*(N-1) + j) | parameter-
    parameter entries]`` (the arguments are :func:`assemble_hessmv`'s), rows
    ascending, columns ascending within a row; ``slot[k]`` is the position in
    ``data`` of triplet ``k``.

    Closed form, nothing is sorted over the triplets: a node's entries of row
    side ``(R, 0)`` and those of ``(R, 1)`` at the node before are two runs in
    ascending column order (:func:`build_hessian_program`), so row ``R*N + p``
    is their merge -- ``len(class)`` columns at every interior time node, a
    sub-list at the first and the last --; a tail row is one segment of
    consecutive time nodes per trajectory row it couples with, then its tail
    columns.  Explicit triplets (instance, parameter-parameter) fall on a
    pair of the pattern or add a column to their row.

    ``with_diagonal=True``: every row also holds its diagonal pair, last in
    the row, whether or not a triplet lands on it."""
    import numpy as np
    plan = _HessianCsrPlan(N, num_rows, num_tail, pattern, inst_rows,
                           inst_cols, obj_pattern, obj_base, tail_rows,
                           tail_cols, with_diagonal)
    indices = np.full(plan.nnz_unique, -1, dtype=np.int64)
    slot = np.full(plan.nnz, -1, dtype=np.int64)
    every = np.arange(plan.ncn, dtype=np.int64)
    for out, p, codes, row, off in plan.runs:
        indices[out] = row*plan.N + p + off
        for c in codes:
            slot[plan.position(c, p)] = out
    for out, col, at, long_codes in plan.items:
        indices[out] = col
        if at:
            slot[at] = out
        for c in long_codes or ():
            slot[plan.position(c, every)] = out
    assert np.all(indices >= 0) and np.all(slot >= 0)
    return plan.indptr, indices, slot


def assemble_hessian_csr(N, num_rows, num_tail, values, pattern,
                         inst_rows=(), inst_cols=(), obj_pattern=(),
                         obj_base=0, tail_rows=(), tail_cols=(),
                         with_diagonal=False):
    """``data`` of the CSR lower triangle of :func:`hessian_csr_structure`
    from the triplets ``values``: element ``u`` is the sum of the triplets of
    pair ``u``.  The host statement of ``opty_hesscsr`` / ``opty_hesscsr_fin``:
    a short group adds its triplets in ascending position in ``values`` from
    ``+0.0`` (the bits of ``np.add.at``); a long group -- a tail x tail pair
    with a triplet per constraint node -- adds the block partials of
    :meth:`_HessianCsrPlan.long_sum` in block order, then its explicit
    triplets in stored order.  ``with_diagonal=True``: the structure with
    every diagonal pair; one that no triplet hits is ``+0.0``."""
    import numpy as np
    plan = _HessianCsrPlan(N, num_rows, num_tail, pattern, inst_rows,
                           inst_cols, obj_pattern, obj_base, tail_rows,
                           tail_cols, with_diagonal)
    values = np.asarray(values, dtype=float)
    assert values.shape == (plan.nnz,)
    data = np.zeros(plan.nnz_unique)
    for out, p, codes, _, _ in plan.runs:
        x = np.zeros(len(p))
        for c in codes:
            x = x + values[plan.position(c, p)]
        data[out] = x
    for out, _, at, long_codes in plan.items:
        x = plan.long_sum(values, long_codes) if long_codes else 0.0
        for k in at:
            x = x + values[k]
        data[out] = x
    return data


class _KktCsrPlan(object):
    """Where everything goes in the CSR lower triangle of the augmented
    system ``[[W + diag(sigma) + delta_w I, J^T], [J, -delta_c I]]`` over
    ``n + m`` rows (:func:`kkt_csr_structure`), in closed form: the ``W``
    part is the Hessian's plan with every diagonal; Jacobian row ``(j, i)``
    of a ``layout='csr'`` program ``prog`` has length ``L_j + 1`` and starts
    at ``nnzW + (S_j + j)*(N-1) + i*(L_j + 1)``, its diagonal is its last
    slot; the instance rows (``jac_inst_rows`` / ``jac_inst_cols``: global
    constraint rows and free columns, sorted by row then column) follow.

    ``hess``: the Hessian's plan; ``nnz_w``: its pairs; ``w_diag``: position
    of the diagonal of every free row; ``jac_slot``: position in ``data`` of
    every Jacobian value; ``con_diag``: position of the diagonal of every
    constraint row."""

    def __init__(self, prog, N, pattern, inst_rows=(), inst_cols=(),
                 obj_pattern=(), obj_base=0, tail_rows=(), tail_cols=(),
                 jac_inst_rows=(), jac_inst_cols=()):
        import numpy as np
        if getattr(prog, 'layout', None) != 'csr':
            raise ValueError("the augmented system as CSR needs a program "
                             "with jacobian_layout='csr'.")
        N = self.N = int(N)
        ncn = N - 1
        nrows, ntail = prog.n + prog.q, prog.r + prog.s
        hess = self.hess = _HessianCsrPlan(
            N, nrows, ntail, pattern, inst_rows, inst_cols, obj_pattern,
            obj_base, tail_rows, tail_cols, with_diagonal=True)
        n = self.n = hess.num_free
        nnz_w = self.nnz_w = hess.nnz_unique
        self.w_diag = hess.indptr[1:] - 1
        M, P = prog.M, len(prog.pattern)
        rs = np.asarray(prog.row_start, dtype=np.int64)
        num_inst = len(prog.inst_con_out)
        irows = np.asarray(jac_inst_rows, dtype=np.int64).reshape(-1) - M*ncn
        icols = np.asarray(jac_inst_cols, dtype=np.int64).reshape(-1)
        if len(irows) != len(prog.inst_jac_out) or len(icols) != len(irows):
            raise ValueError('%d instance rows / %d columns for %d instance '
                             'entries' % (len(irows), len(icols),
                                          len(prog.inst_jac_out)))
        if np.any((irows < 0) | (irows >= num_inst) | (icols < 0) |
                  (icols >= n)):
            raise ValueError('instance entry outside the problem')
        if np.any(np.diff(irows*n + icols) <= 0):
            raise ValueError('the instance entries are not sorted by row, '
                             'then column')
        m = self.m = M*ncn + num_inst
        counts = np.bincount(irows, minlength=num_inst).astype(np.int64)
        lens = np.concatenate((np.repeat(np.diff(rs) + 1, ncn), counts + 1))
        self.indptr = np.concatenate(
            (hess.indptr, nnz_w + np.cumsum(lens))).astype(np.int64)
        self.nnz = int(self.indptr[-1])
        self.jac_nnz = P*ncn + len(irows)

        i = np.arange(ncn, dtype=np.int64)
        tail = nrows*N
        indices = np.full(self.nnz, -1, dtype=np.int64)
        jac_slot = np.empty(self.jac_nnz, dtype=np.int64)
        for j in range(M):
            S, L = int(rs[j]), int(rs[j + 1] - rs[j])
            start = nnz_w + (S + j)*ncn + i*(L + 1)
            for c in range(L):
                jj, k = prog.pattern[S + c]
                assert jj == j
                row, off = column_side(prog.n, prog.q, prog.method, k)
                indices[start + c] = row*N + i + off if row >= 0 \
                    else tail + off
                jac_slot[S*ncn + i*L + c] = start + c
            indices[start + L] = n + j*ncn + i
        first = np.concatenate(([0], np.cumsum(counts)))[:-1]
        base = nnz_w + (P + M)*ncn
        start = base + first + np.arange(num_inst, dtype=np.int64)
        at = start[irows] + np.arange(len(irows), dtype=np.int64) \
            - first[irows]
        indices[at] = icols
        jac_slot[P*ncn:] = at
        indices[start + counts] = n + M*ncn + np.arange(num_inst)
        self.indices, self.jac_slot = indices, jac_slot
        self.con_diag = self.indptr[n + 1:] - 1


def kkt_csr_structure(prog, N, pattern, inst_rows=(), inst_cols=(),
                      obj_pattern=(), obj_base=0, tail_rows=(), tail_cols=(),
                      jac_inst_rows=(), jac_inst_cols=()):
    """``(indptr, indices)`` (int64) of the lower triangle of the augmented
    system ``K = [[W + diag(sigma) + delta_w I, J^T], [J, -delta_c I]]`` in
    compressed-sparse-row form over ``num_free + num_constraints`` rows.
    Row ``r < num_free``: the columns of row ``r`` of
    :func:`hessian_csr_structure` (its arguments are ``N, n + q, r + s`` of
    ``prog`` and ``pattern`` ...) and the diagonal ``(r, r)``, stored whether
    or not a triplet lands on it.  Row ``num_free + k``: the columns of row
    ``k`` of the CSR Jacobian of ``prog`` (``layout='csr'``; ``jac_inst_rows``
    / ``jac_inst_cols``: the indices of its instance entries), then the
    diagonal.  Every diagonal is the last entry of its row.  Closed form:
    nothing of the size of the matrix is sorted."""
    import numpy as np
    plan = _KktCsrPlan(prog, N, pattern, inst_rows, inst_cols, obj_pattern,
                       obj_base, tail_rows, tail_cols, jac_inst_rows,
                       jac_inst_cols)
    indices = plan.indices
    w = hessian_csr_structure(
        N, prog.n + prog.q, prog.r + prog.s, pattern, inst_rows, inst_cols,
        obj_pattern, obj_base, tail_rows, tail_cols, with_diagonal=True)[1]
    indices[:plan.nnz_w] = w
    assert np.all(indices >= 0)
    return plan.indptr, indices


def assemble_kkt_csr(prog, N, hess_values, jac_values, pattern, inst_rows=(),
                     inst_cols=(), obj_pattern=(), obj_base=0, tail_rows=(),
                     tail_cols=(), jac_inst_rows=(), jac_inst_cols=(),
                     sigma=None, delta_w=0.0, delta_c=0.0):
    """``data`` of :func:`kkt_csr_structure` from the Hessian's triplets
    ``hess_values`` and the values ``jac_values`` of the CSR Jacobian.  The
    host statement of ``opty_kkt_diag`` / ``opty_kkt_jrows`` /
    ``opty_kkt_inst`` behind ``opty_hesscsr``: an off-diagonal of the ``W``
    block has the bits of :func:`assemble_hessian_csr`; a diagonal of the
    ``W`` block is ``(h + sigma_r) + delta_w`` rounded in that order, ``h``
    the compressed element (``+0.0`` where no triplet lands), ``sigma_r``
    ``+0.0`` without ``sigma``; a Jacobian entry is copied; a diagonal of the
    constraint block is ``0.0 - delta_c``."""
    import numpy as np
    plan = _KktCsrPlan(prog, N, pattern, inst_rows, inst_cols, obj_pattern,
                       obj_base, tail_rows, tail_cols, jac_inst_rows,
                       jac_inst_cols)
    jac_values = np.asarray(jac_values, dtype=float)
    if jac_values.shape != (plan.jac_nnz,):
        raise ValueError('jac_values must have shape (%d,)' % plan.jac_nnz)
    sigma = np.zeros(plan.n) if sigma is None else \
        np.asarray(sigma, dtype=float)
    if sigma.shape != (plan.n,):
        raise ValueError('sigma must have shape (%d,)' % plan.n)
    data = np.empty(plan.nnz)
    data[:plan.nnz_w] = assemble_hessian_csr(
        N, prog.n + prog.q, prog.r + prog.s, hess_values, pattern, inst_rows,
        inst_cols, obj_pattern, obj_base, tail_rows, tail_cols,
        with_diagonal=True)
    data[plan.w_diag] = (data[plan.w_diag] + sigma) + float(delta_w)
    data[plan.jac_slot] = jac_values
    data[plan.con_diag] = 0.0 - float(delta_c)
    return data


def normal_columns(prog):
    """What ``opty_hip_normal_create`` derives from a program's ``pattern``:
    ``(sides, ent, coupled)`` -- ``sides``: the distinct trajectory sides
    ``(row, off)`` of the stored entries in ascending order (the tail columns
    are not part of the normal matrix); ``ent[j][c]``: the stored entry of
    equation ``j`` in sorted column ``c`` or -1; ``coupled``: ``(c0, c1,
    row)`` of every free row with an offset-0 column ``c0`` and an offset-1
    column ``c1``."""
    if getattr(prog, 'layout', None) not in ('coo', 'csr'):
        raise ValueError("the normal matrix takes jacobian_layout='coo' or "
                         "'csr'.")
    side = [column_side(prog.n, prog.q, prog.method, k)
            for _, k in prog.pattern]
    sides = sorted({s for s in side if s[0] >= 0})
    where = {s: c for c, s in enumerate(sides)}
    ent = [[-1]*len(sides) for _ in range(prog.M)]
    for e, (j, _) in enumerate(prog.pattern):
        if side[e][0] >= 0:
            assert ent[j][where[side[e]]] < 0
            ent[j][where[side[e]]] = e
    coupled = [(where[(row, 0)], where[(row, 1)], row)
               for row, off in sides if off == 0 and (row, 1) in where]
    return sides, ent, coupled


def normal_blocks(prog, N, jac_values, d=None, delta_c=0.0):
    """``(A, B)`` of the block-tridiagonal normal matrix ``S = Jc[:, :T]
    diag(1/d[:T]) Jc[:, :T]^T + delta_c I`` (``Jc``: the ``M(N-1)``
    collocation rows of the Jacobian, ``T = (n+q)N``) ordered by constraint
    node: ``A`` of shape ``(N-1, M, M)``, the diagonal blocks, ``B`` of shape
    ``(N-2, M, M)``, ``B[i] = S[i+1, i]``.  ``jac_values``: the values of
    ``jacobian(free)`` in ``prog``'s layout (``'coo'``: ``jac[i*P + e]``,
    ``'csr'``: ``jac[S_j*(N-1) + i*L_j + pos]``), pruned or not; ``d``:
    ``num_free`` (or ``T``) positive values, default ones.  The host
    statement of ``opty_normal_blocks``: with ``G_i`` the block of node ``i``
    (a pruned entry 0),

    * ``A[i][a, b] = sum_k G_i[a, k] (G_i[b, k] / d[row_k*N + i + off_k])``
      over the trajectory columns in ascending ``(row, off)`` from ``+0.0``,
      for ``a >= b``, mirrored; ``delta_c`` is added to a diagonal last;
    * ``B[i][a, b] = sum_row G_{i+1}[a, k0(row)] (G_i[b, k1(row)] /
      d[row*N + i + 1])`` over the free rows that have an offset-0 column
      ``k0`` and an offset-1 column ``k1``, ascending.

    The tail columns and the instance rows are not part of ``S`` (the kernel
    fuses each product with its addition; this statement rounds both)."""
    import numpy as np
    N = int(N)
    ncn = N - 1
    if ncn < 1:
        raise ValueError('N %d < 2' % N)
    delta_c = float(delta_c)
    if not (0.0 <= delta_c < np.inf):
        raise ValueError('delta_c must be a finite value >= 0.')
    sides, ent, coupled = normal_columns(prog)
    M, P = prog.M, len(prog.pattern)
    T = (prog.n + prog.q)*N
    jac_values = np.asarray(jac_values, dtype=float).reshape(-1)
    if len(jac_values) < P*ncn:
        raise ValueError('jac_values must hold %d block values' % (P*ncn))
    d = np.ones(T) if d is None else np.asarray(d, dtype=float).reshape(-1)
    if len(d) < T:
        raise ValueError('d must have at least %d values' % T)
    i = np.arange(ncn, dtype=np.int64)
    rs = prog.row_start

    def entry(e):
        if prog.layout == 'csr':
            j = prog.pattern[e][0]
            S, L = rs[j], rs[j + 1] - rs[j]
            return jac_values[S*ncn + i*L + (e - S)]
        return jac_values[i*P + e]
    G = np.zeros((ncn, M, len(sides)))
    for j in range(M):
        for c, e in enumerate(ent[j]):
            if e >= 0:
                G[:, j, c] = entry(e)
    A = np.zeros((ncn, M, M))
    for c, (row, off) in enumerate(sides):
        w = G[:, :, c]/d[row*N + i + off][:, None]
        A = A + G[:, :, c][:, :, None]*w[:, None, :]
    low = np.tril(A)
    A = low + np.transpose(np.tril(A, -1), (0, 2, 1))
    k = np.arange(M)
    A[:, k, k] = A[:, k, k] + delta_c
    B = np.zeros((max(ncn - 1, 0), M, M))
    for c0, c1, row in coupled:
        w = G[:-1, :, c1]/d[row*N + i[:-1] + 1][:, None]
        B = B + G[1:, :, c0][:, :, None]*w[:, None, :]
    return A, B


def _normal_cholesky(A, level, rows):
    """Batched lower Cholesky factors of the blocks ``A`` (rows ``rows`` of
    level ``level``); a pivot that is not positive and finite raises
    ``LinAlgError`` naming the level and the first such row."""
    import numpy as np
    try:
        L = np.linalg.cholesky(A)
        bad = ~np.all(np.isfinite(L), axis=(1, 2))
    except np.linalg.LinAlgError:
        L = np.zeros_like(A)
        bad = np.zeros(len(A), dtype=bool)
        for k in range(len(A)):
            try:
                L[k] = np.linalg.cholesky(A[k])
            except np.linalg.LinAlgError:
                bad[k] = True
    if bad.any():
        raise np.linalg.LinAlgError(
            'the normal matrix is not positive definite: a pivot that is '
            'not positive and finite at level %d, row %d'
            % (level, rows[int(np.flatnonzero(bad)[0])]))
    return L


def _bt(X):
    """The blocks of ``X`` transposed."""
    import numpy as np
    return np.transpose(X, (0, 2, 1))


def normal_factor(A, B):
    """Block cyclic reduction with Cholesky factors of the block-tridiagonal
    matrix with diagonal blocks ``A`` ``(n, M, M)`` and couplings ``B``
    ``(n-1, M, M)``, ``B[k] = S[k+1, k]`` -- a sparse Cholesky under an
    odd-even ordering, no pivoting; the elimination order the kernels share.
    Level ``l`` has ``n_l`` rows, ``n_0 = n``, ``n_{l+1} = ceil(n_l/2)``;
    rows 1, 3, 5, ... are eliminated, rows 0, 2, 4, ... survive as ``e =
    k/2``; a level with one row is a plain Cholesky.  Eliminated row ``k``:
    ``L_k = chol(A_k)``, ``U_k = L_k^-1 S[k, k-1]``, ``V_k = L_k^-1 S[k,
    k+1]`` (absent for a last row); survivors: ``A'_e = A_2e - U_{2e+1}^T
    U_{2e+1} - V_{2e-1}^T V_{2e-1}``, ``S'[e+1, e] = -V_{2e+1}^T U_{2e+1}``.
    Returns the list of levels ``(n_l, L, U, V)`` (``V`` zero where absent).
    Only the lower triangle of a diagonal block is read.  Raises
    ``numpy.linalg.LinAlgError`` naming level and row of the first pivot that
    is not positive and finite."""
    import numpy as np
    A = np.array(A, dtype=float)
    B = np.array(B, dtype=float)
    n, M = A.shape[0], A.shape[1]
    if A.shape != (n, M, M) or n < 1 or B.shape != (n - 1, M, M):
        raise ValueError('A must have shape (n, M, M) and B (n - 1, M, M)')
    levels = []
    level = 0
    while True:
        n = len(A)
        if n == 1:
            levels.append((1, _normal_cholesky(A, level, [0]), None, None))
            return levels
        odd = np.arange(1, n, 2)
        L = _normal_cholesky(A[odd], level, odd)
        U = np.linalg.solve(L, B[odd - 1])
        V = np.zeros_like(U)
        inner = odd + 1 < n
        V[inner] = np.linalg.solve(L[inner], _bt(B[odd[inner]]))
        levels.append((n, L, U, V))
        ne = (n + 1)//2
        An = A[0::2].copy()
        # survivor e < n//2 has the row 2e + 1 behind it, survivor e > 0 the
        # row 2e - 1 in front (whose V exists)
        An[:n//2] = An[:n//2] - _bt(U) @ U
        An[1:] = An[1:] - _bt(V[:ne - 1]) @ V[:ne - 1]
        A, B = An, -(_bt(V[:ne - 1]) @ U[:ne - 1])
        level += 1


def normal_solve(factors, r):
    """``y = S^-1 r`` from ``factors`` of :func:`normal_factor`; ``r`` of
    shape ``(M n,)`` or ``(M n, k)`` in the order of ``constraints(free)``,
    ``j*n + i``.  Forward: ``z_k = L_k^-1 r_k``, ``r'_e = r_2e - U_{2e+1}^T
    z_{2e+1} - V_{2e-1}^T z_{2e-1}``; backward: ``y_k = L_k^-T (z_k - U_k
    y_{k-1} - V_k y_{k+1})``."""
    import numpy as np
    n0 = factors[0][0]
    M = factors[0][1].shape[1]
    r = np.asarray(r, dtype=float)
    if r.ndim not in (1, 2) or r.shape[0] != M*n0:
        raise ValueError('r must have shape (%d,) or (%d, k)' % (M*n0, M*n0))
    rhs = r.reshape(M, n0, -1).transpose(1, 0, 2)       # (node, j, column)
    zs = []
    for n, L, U, V in factors:
        if n == 1:
            zs.append(np.linalg.solve(L, rhs))
            break
        z = np.linalg.solve(L, rhs[1::2])
        zs.append(z)
        ne = (n + 1)//2
        nxt = rhs[0::2].copy()
        nxt[:n//2] = nxt[:n//2] - _bt(U) @ z
        nxt[1:] = nxt[1:] - _bt(V[:ne - 1]) @ z[:ne - 1]
        rhs = nxt
    y = np.linalg.solve(_bt(factors[-1][1]), zs[-1])
    for (n, L, U, V), z in zip(factors[-2::-1], zs[-2::-1]):
        full = np.empty((n,) + y.shape[1:])
        full[0::2] = y
        w = z - U @ y[:n//2]
        inner = np.arange(1, n, 2) + 1 < n
        w[inner] = w[inner] - V[inner] @ y[1:][:inner.sum()]
        full[1::2] = np.linalg.solve(_bt(L), w)
        y = full
    return y.transpose(1, 0, 2).reshape(r.shape)


def matrix_program(dag, outputs, num_vec, num_const, shape):
    """Program of a plain matrix of expressions (the reference's
    ``ufuncify_matrix`` call shape, ``opty/utils.py:639-640``): ``outputs`` are
    the DAG nodes of the ``rows x cols`` entries, row-major, over the inputs
    ``('cur', k)`` -- vector argument ``k`` (one value per evaluation row) --
    and ``('par', k)`` -- constant argument ``k``.  The vector arguments are
    the rows of one packed ``(num_vec, n)`` buffer that the kernels see as
    their ``free`` vector with ``N = n``."""
    rows, cols = shape
    assert len(outputs) == rows*cols
    return CollocationProgram(
        dag=dag, con_out=[], jac_out=list(outputs), n=num_vec, m=0, q=0, r=0,
        s=0, M=rows, C=cols, num_known_traj=0, num_known_par=num_const,
        rows=[('free', k) for k in range(num_vec)],
        pars=[('known', k) for k in range(num_const)], h=('fixed',),
        method='matrix', cur_offset=0, adj_offset=0, inst_con_out=[],
        inst_jac_out=[], num_inst_atoms=0,
        pattern=[(j, k) for j in range(rows) for k in range(cols)],
        pruned=False, layout='coo',
        row_start=[j*cols for j in range(rows + 1)])


def _column_key(n, q, method):
    """Sort key of wrt index k equal to the order of the free-vector column
    it differentiates with respect to (the closed form of
    ``opty/direct_collocation.py:2657-2675`` at a generic node)."""
    big = 1 << 20           # stands for N; node i = 1

    def key(k):
        if method == 'backward euler':
            if k < n:
                return k*big + 2
            if k < 2*n:
                return (k - n)*big + 1
            if k < 2*n + q:
                return (n + k - 2*n)*big + 2
            return (n + q)*big + (k - 2*n - q)
        if k < n:
            return k*big + 1
        if k < 2*n:
            return (k - n)*big + 2
        if k < 2*n + q:
            return (n + k - 2*n)*big + 1
        if k < 2*n + 2*q:
            return (n + k - 2*n - q)*big + 2
        return (n + q)*big + (k - 2*n - 2*q)
    return key


def _static_tester(prog):
    """``is_static(node)``: the node's value is the same at every node and
    every call with the same known parameters and (fixed) interval."""
    dag = prog.dag
    static = {}

    def is_static(root):
        stack = [root]
        while stack:
            i = stack.pop()
            if i in static:
                if not static[i]:
                    static[root] = False
                    return False
                continue
            if dag.op[i] == ir.INPUT:
                kind, idx = dag.args[i]
                ok = ((kind == 'par' and prog.pars[idx][0] == 'known') or
                      (kind == 'h' and prog.h[0] == 'fixed'))
                static[i] = ok
                if not ok:
                    static[root] = False
                    return False
                continue
            if not dag.uni[i]:
                static[i] = False
                static[root] = False
                return False
            stack.extend(dag.operands(i))
        static[root] = True
        return True
    return is_static


def varying_entries(prog):
    """Stored block entries whose value can differ between two evaluations
    with the same known parameters and (fixed) node time interval: those that
    depend on a trajectory value, an unknown parameter or a free interval.
    The rest -- for the 10-link pendulum 660 of 990: the reference's
    structural zeros, +-1, +-1/h, products of masses and lengths
    (``opty/direct_collocation.py:2589-2593`` keeps them all in the value
    vector) -- are the same at every node and every call."""
    is_static = _static_tester(prog)
    return [e for e, node in enumerate(prog.jac_out) if not is_static(node)]


#: shortest run of node-invariant entries that the restricted Jacobian
#: kernels skip: a run of L entries holds at least (L - 15)//16 whole
#: 128-byte lines of the flat output whatever the line phase of the node's
#: row, so 32 is the shortest run that removes a whole line in every phase
SKIP_MIN_RUN = 32


def kept_spans(prog, min_run=SKIP_MIN_RUN):
    """The entry spans ``[(a, b), ...]`` of a block that an evaluation into a
    buffer which still holds the previous evaluation's values has to write
    again: the complement of the maximal runs of node-invariant entries
    (:func:`varying_entries`' complement) that are at least ``min_run`` long.
    Shorter static gaps stay inside a span (they are written as always, from
    their literal / table values: the stores stay whole lines).  Blocks
    follow each other in memory, so the run behind the last varying entry
    continues in the next node's first entries: it is skipped when the two
    parts together are long enough AND the first varying entry has 15
    static entries of its own block in front of it (the line that holds it
    then starts in the same block); otherwise the first span starts at entry
    0 and the last one ends at P.  A block without varying entries, or
    without a run worth skipping, gives ``[(0, P)]``: nothing is skipped.
    For the 10-link pendulum: ``[(496, 988)]`` of 990 entries."""
    P = prog.P
    var = varying_entries(prog)
    if not var:
        return [(0, P)]
    spans, a = [], var[0]
    for prev, e in zip(var, var[1:]):
        if e - prev - 1 >= min_run:
            spans.append((a, prev + 1))
            a = e
    spans.append((a, var[-1] + 1))
    wrap = (P - 1 - var[-1]) + var[0]
    if wrap < min_run or var[0] < 15:
        spans[0] = (0, spans[0][1])
        spans[-1] = (spans[-1][0], P)
    return spans


def line_owner_ranges(prog, spans=None):
    """What the restricted kernels make of :func:`kept_spans`: a wave owns
    the 128-byte lines whose FIRST entry lies in its range, and the line that
    holds entry ``a`` may start up to 15 entries earlier -- so the span ``(a,
    b)`` becomes the owner range ``(a - 15 rounded down to a multiple of 16,
    b)``; the entries staged are those of ``[lo, b + 15)`` (past P: the next
    node's first entries).  Empty when nothing is skipped."""
    spans = kept_spans(prog) if spans is None else spans
    if spans == [(0, prog.P)]:
        return []
    return [(max(0, (a - 15)//16*16), b) for a, b in spans]


def kept_lines_per_node(prog, spans=None):
    """``(kept, all)``: 128-byte lines of the flat output per node, averaged
    over the 16 line phases a node's row can start at, that hold at least one
    entry of a kept span / at least one entry at all (P/16)."""
    P = prog.P
    spans = kept_spans(prog) if spans is None else spans
    kept = 0
    for phase in range(16):
        lines = set()
        for a, b in spans:
            lines |= {(phase + e)//16 for e in range(a, b)}
        kept += len(lines)
    return kept/16.0, P/16.0


def varying_copies(prog):
    """Splits :func:`varying_entries` into the entries that have to be
    evaluated / moved and the ones that are *the same expression* as an
    earlier one (the same node of the hash-consed DAG: the mass matrix of a
    multibody system is symmetric, and its entries appear in the columns of
    the current and of the adjacent node's speeds).  Returns ``(unique,
    copies)``: ``unique`` ascending entry numbers, ``copies`` a list of
    ``(dst, src)`` with ``src`` in ``unique`` -- for the 10-link pendulum 275
    unique entries and 55 copies of the 330 varying ones."""
    first = {}
    unique, copies = [], []
    for e in varying_entries(prog):
        node = prog.jac_out[e]
        if node in first:
            copies.append((e, first[node]))
        else:
            first[node] = e
            unique.append(e)
    return unique, copies


def scaled_copies(prog):
    """:func:`varying_copies` taken one step further: varying entries that
    are a NODE-INVARIANT multiple of another varying entry -- ``c_1 X`` and
    ``c_2 X`` with the same per-node expression ``X`` and factors that depend
    on known parameters / the fixed interval only (a mass-matrix partial in
    the current node's column and, differently scaled, in another row) -- need
    not both cross PCIe: the host fills ``dst = (c_dst/c_src) src``.

    Returns ``(unique, copies)``: ``unique`` ascending entry numbers that are
    moved; ``copies`` a list of ``(dst, src, num, den)`` sorted by ``dst``,
    ``src`` in ``unique``, ``num`` / ``den`` the factor chains of dst / src --
    lists of ``('neg',)``, ``('mul', node)``, ``('div', node)`` over static
    DAG nodes, so that ``dst = prod(num)/prod(den) * src`` (:func:`chain_value`
    evaluates them for given known values; exact duplicates have two empty
    chains).  For the 10-link pendulum: 275 -> 269 moved entries (the
    numerical rank of the 275 as functions of the node values is 266: what
    ANY linear reconstruction could reach)."""
    dag = prog.dag
    is_static = _static_tester(prog)

    def strip(i):
        chain = []
        while True:
            op = dag.op[i]
            if op == ir.NEG:
                chain.append(('neg',))
                i = dag.args[i][0]
                continue
            if op == ir.MUL:
                a, b = dag.args[i]
                if is_static(a) and not is_static(b):
                    chain.append(('mul', a))
                    i = b
                    continue
                if is_static(b) and not is_static(a):
                    chain.append(('mul', b))
                    i = a
                    continue
            if op == ir.DIV:
                a, b = dag.args[i]
                if is_static(b) and not is_static(a):
                    chain.append(('div', b))
                    i = a
                    continue
            return chain, i

    base = {}                  # core node -> (entry, its chain)
    unique, copies = [], []
    for e in varying_entries(prog):
        chain, core = strip(prog.jac_out[e])
        if core in base:
            src, den = base[core]
            copies.append((e, src, chain, den))
        else:
            base[core] = (e, chain)
            unique.append(e)
    return unique, copies


def chain_value(chain, values):
    """Value of a factor chain of :func:`scaled_copies` given ``values``
    (static DAG node -> float)."""
    v = 1.0
    for step in chain:
        if step[0] == 'neg':
            v = -v
        elif step[0] == 'mul':
            v *= values[step[1]]
        else:
            v /= values[step[1]]
    return v

