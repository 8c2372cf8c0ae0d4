"""CPU tests of the block products of the Jacobian operator (``Y = J V`` and
``G = J^T W``, K columns per pass): the header, the bindings and the library
agree; the roots of ``build_jacobian_block_product_program``, evaluated by the
NumPy interpreter and assembled on the host, against the reference matrix and
against the single program; the operation counts; the single program is what
it was; and the block modules cross-compile for gfx950 without vector
spills.  No GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import dag_interp
import jacprod_block_cases as cases
from test_jacprod_cpu import (PROBLEMS, U, _collocator, draw,
                              product_tolerances, reference_matrix,
                              worst_ratio)

from opty_amd import hip_backend as hb
from opty_amd.codegen import ir
from opty_amd.codegen.program import assemble_jvp, assemble_vjp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4

CTYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64,
          'int': ctypes.c_int}
PRODUCT = ['*', '*', '*', 'int64_t', '*', 'int64_t', 'int32_t', 'int32_t']
DECLARED = {
    'opty_hip_jacprod_block_create': ('int', ['*', '*', '*', '*']),
    'opty_hip_jacprod_block_destroy': ('int', ['*']),
    'opty_hip_jacprod_block_width': ('int32_t', ['*']),
    'opty_hip_jacprod_block_jvp': ('int', PRODUCT),
    'opty_hip_jacprod_block_vjp': ('int', PRODUCT)}


def _declaration(name):
    """``(result type, [argument types])`` of ``name`` in the header, a
    pointer of any kind as ``'*'``."""
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        header = f.read()
    m = re.search(r'^(\w+)\s+%s\(([^)]*)\);' % name, header, re.M)
    assert m, name
    args = []
    for arg in m.group(2).split(','):
        words = arg.replace('const', ' ').split()
        args.append('*' if '*' in arg else words[0])
    return m.group(1), args


def test_header_bindings_and_library_agree():
    hb.build_runtime_library()
    lib = hb.load_library()
    for name, want in DECLARED.items():
        res, args = _declaration(name)
        assert (res, args) == want, name
        have_res, have_args = hb._SIGNATURES[name]
        assert have_res == CTYPES[res] and len(have_args) == len(args), name
        for have, a in zip(have_args, args):
            if a == '*':
                # (create: typed pointers to the descriptor and the handle)
                assert have in (hb._P, ctypes.c_char_p) or \
                    issubclass(have, ctypes._Pointer), (name, have)
            else:
                assert have == CTYPES[a], (name, have, a)
        assert hasattr(lib, name), name
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        header = f.read()
    desc = re.search(r'typedef struct opty_hip_jacprod_block_desc \{(.*?)\}',
                     header, re.S).group(1)
    fields = re.findall(r'int32_t (\w+);', desc)
    assert fields == ['width', 'jvp_strips', 'vjp_strips', 'num_tail',
                      'nnz_inst']
    assert [f[0] for f in hb._JacprodBlockDesc._fields_] == fields
    for method in ('jvp_block', 'vjp_block'):
        assert hasattr(hb.HipJacobianBlockProduct, method)
    assert isinstance(hb.HipJacobianBlockProduct.width, property)
    # additive: the version is the one the existing clients were built for
    assert hb.ABI_VERSION == 12


_CACHE = {}


def _block(name):
    """``(collocator, reference matrices, free, V, W, block products and
    their bounds per column)`` of a problem, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    col = _collocator(name)
    free, J, A, F, Kc = reference_matrix(name, col)
    rng = np.random.default_rng(41)
    V = np.stack([draw(rng, col.num_free) for _ in range(K)], axis=1)
    W = np.stack([draw(rng, col.num_constraints) for _ in range(K)], axis=1)
    prog = col._build_jacprod_block_program(K)
    N = col.num_collocation_nodes
    nodes = np.arange(N - 1)
    atoms = col._atom_free_index()
    fin = col._jacprod_block_inputs(free, V, nodes, 'jvp')
    rin = col._jacprod_block_inputs(free, W, nodes, 'vjp')
    ev = dag_interp.evaluate_with_error_bound
    inst, ib = ev(prog.dag, prog.inst_jac_out, fin)
    inst = [float(x) for x in inst]
    ib = [abs(float(x)) for x in ib]
    cols = []
    for c in range(K):
        tan, tb = ev(prog.dag, prog.tan_out[c], fin)
        adj, ab = ev(prog.dag, prog.adj_out[c], rin)
        v, w = V[:, c], W[:, c]
        cols.append((
            assemble_jvp(prog, N, tan, inst, v, atoms),
            assemble_vjp(prog, N, adj, inst, w, atoms),
            assemble_jvp(prog, N, [np.abs(x) for x in tb], ib, np.abs(v),
                         atoms),
            assemble_vjp(prog, N, [np.abs(x) for x in ab], ib, np.abs(w),
                         atoms)))
    _CACHE[name] = col, (J, A, F, Kc), free, V, W, cols
    return _CACHE[name]


@pytest.mark.parametrize('name', PROBLEMS)
def test_block_columns_against_the_reference_matrix(name):
    col, (J, A, F, Kc), free, V, W, cols = _block(name)
    assert len({V[:, c].tobytes() for c in range(K)}) == K
    for c, (jv, jtw, _, _) in enumerate(cols):
        v, w = V[:, c], W[:, c]
        tv, tw = product_tolerances(A, F, Kc, v, w)
        ev, ew = np.abs(jv - J @ v), np.abs(jtw - J.T @ w)
        print('%s column %d: worst error/tolerance jvp %.3g, vjp %.3g'
              % (name, c, worst_ratio(ev, tv), worst_ratio(ew, tw)))
        assert np.all(ev <= tv), (name, c, 'jvp', worst_ratio(ev, tv))
        assert np.all(ew <= tw), (name, c, 'vjp', worst_ratio(ew, tw))


@pytest.mark.parametrize('name', PROBLEMS)
def test_block_columns_against_the_single_program(name):
    """Column ``c`` of the block roots and the single program's roots at the
    same vector: within the sum of their two rounding-error bounds."""
    from test_jacprod_cpu import interpreted_products
    col, _, free, V, W, cols = _block(name)
    for c, (jv, jtw, jvb, jtwb) in enumerate(cols):
        sv, stw, svb, stwb = interpreted_products(col, free, V[:, c], W[:, c],
                                                  with_bounds=True)
        for what, a, b, bound in (('jvp', jv, sv, jvb + svb),
                                  ('vjp', jtw, stw, jtwb + stwb)):
            # the roots' bounds are in units of round-off; one more unit of
            # every partial sum of the host assembly on either side
            tol = U*bound + 4*U*(np.abs(a) + np.abs(b))
            err = np.abs(a - b)
            print('%s column %d %s: worst error/tolerance %.3g'
                  % (name, c, what, worst_ratio(err, tol)))
            assert np.all(err <= tol), (name, c, what)


@pytest.mark.parametrize('name', PROBLEMS)
def test_block_adjoint_identity(name):
    """``trace(W^T (J V)) == trace(V^T (J^T W))`` on the interpreter."""
    col, (J, A, F, Kc), free, V, W, cols = _block(name)
    JV = np.stack([c[0] for c in cols], axis=1)
    JTW = np.stack([c[1] for c in cols], axis=1)
    lhs, rhs = float(np.sum(W*JV)), float(np.sum(V*JTW))
    tol = 64*U*float(np.sum(np.abs(W)*(A @ np.abs(V))))
    print('%s: |tr W^T J V - tr V^T J^T W| = %.3g, tolerance %.3g'
          % (name, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol


def _ops(dag, roots):
    return sum(dag.count_ops(roots).values())


@pytest.mark.parametrize('name', PROBLEMS)
def test_block_operation_counts(name):
    col = _block(name)[0]
    single = col._build_jacprod_program()
    block = col._build_jacprod_block_program(K)
    assert block.columns == K
    t1, a1 = _ops(single.dag, single.tan_out), _ops(single.dag,
                                                   single.adj_out)
    tk = _ops(block.dag, [n for c in block.tan_out for n in c])
    ak = _ops(block.dag, [n for c in block.adj_out for n in c])
    print('%s: tangent %d -> %d (%.3f of %d singles), adjoint %d -> %d '
          '(%.3f)' % (name, t1, tk, tk/(K*t1), K, a1, ak, ak/(K*a1)))
    assert tk < K*t1 and ak < K*a1
    if name == 'config3_10link_small':
        assert tk <= 0.75*K*t1 and ak <= 0.5*K*a1
    if name == 'biped_small':
        assert ak <= 0.5*K*a1
    # what does not depend on the column is the single program's
    assert block.adj_sides == single.adj_sides
    assert block.row_columns() == single.row_columns()
    assert block.tail_columns() == single.tail_columns()
    assert len(block.inst_jac_out) == len(single.inst_jac_out)
    assert block.inst_pairs == single.inst_pairs


def test_column_inputs_are_named_and_uniform_kinds_hold():
    col = _block('pend2_link_vardur_unkmass_small')[0]
    prog = col._build_jacprod_block_program(K)
    dag = prog.dag
    for c in range(K):
        for roots, own in ((prog.tan_out[c], ('vcur', 'vadj', 'vpar', 'vh')),
                           (prog.adj_out[c], ('lam',))):
            seen = set()
            for i in dag.reachable(roots):
                if dag.op[i] != ir.INPUT:
                    continue
                kind, index = dag.args[i]
                assert kind != 'dir'
                assert dag.uni[i] == (kind in ir.UNIFORM_KINDS)
                if kind in ir.COLUMN_KINDS:
                    assert kind in own, (kind, own)
                    assert ir.split_column(kind, index)[0] == c
                    seen.add(kind)
                else:
                    assert index < ir.COLUMN_STRIDE
            assert seen, (c, own)
    assert {'vpar', 'vh'} <= set(ir.UNIFORM_KINDS)


def test_single_program_is_untouched():
    col = _block('config3_10link_small')[0]
    prog = col._build_jacprod_program()
    assert _ops(prog.dag, prog.tan_out) == 2754
    col = _collocator('implicit_traj_mid_small')
    prog = col._build_jacprod_program()
    kinds = {prog.dag.args[i] for i in prog.dag.reachable(prog.tan_out)
             if prog.dag.op[i] == ir.INPUT}
    assert {'vcur', 'vadj'} <= {k for k, _ in kinds}
    assert 'dir' not in {k for k, _ in kinds}
    assert all(index < ir.COLUMN_STRIDE for _, index in kinds)
    kinds = {prog.dag.args[i][0] for i in prog.dag.reachable(prog.adj_out)
             if prog.dag.op[i] == ir.INPUT}
    assert 'lam' in kinds and not kinds & {'vcur', 'vadj', 'vpar', 'vh'}
    # one column of the block builder is the single program, node for node
    one = col._build_jacprod_block_program(1)
    assert one.tan_out[0] == prog.tan_out and one.adj_out[0] == prog.adj_out
    assert one.dag.op == prog.dag.op and one.dag.args == prog.dag.args


@pytest.mark.parametrize('name', cases.CROSS_COMPILED)
def test_block_module_cross_compiles_without_spills(name):
    col = _collocator(name)
    hsaco, meta = col._build_jacprod_block_code_object()
    print('%s: %s' % (name, {k: meta[k] for k in (
        'width', 'strip_ops', 'forget', 'jvp_strips', 'vjp_strips',
        'tried')}))
    assert meta['width'] in (4, 2)
    res = hb.cached_kernel_resources(hsaco)
    for kernel in col._JACPROD_BLOCK_KERNELS:
        assert kernel in res, (name, kernel)
        print('%s %s: %d VGPRs, %d AGPRs, %d bytes of LDS' % (
            name, kernel, res[kernel]['.vgpr_count'],
            res[kernel].get('.agpr_count', 0),
            res[kernel]['.group_segment_fixed_size']))
        assert res[kernel]['.vgpr_spill_count'] == 0, (name, kernel)
    assert res['opty_vjp_block']['.group_segment_fixed_size'] == \
        2*64*8*meta['width']
    from opty_amd.codegen.emit_jacprod import emit_jacprod_block_module
    source, _ = emit_jacprod_block_module(
        col._build_jacprod_block_program(meta['width']))
    assert 'atomic' not in source.lower() and 'asm' not in source
    assert source.count('__launch_bounds__(64)') == 4
