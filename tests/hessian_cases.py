"""What the Hessian test files share: the CPU interpreter's values of a
Hessian program, the small problems whose modules cover every flush variant
of ``codegen/emit_hessian.py``, the flush calls of an emitted source, and the
code objects that ``__graft_entry__.build`` prebuilds for them."""
import functools
import re

import numpy as np

import dag_interp

from examples import problems

#: label -> factory(num_nodes) of the problems of tests/test_hessian_kernel_
#: gpu.py; PH does not depend on N.  At the default strip budget:
#: A  PH 52, flush16<16> x3, flush16<4>
#: B  PH 40, flush16<16> x2, flush16<8>
#: C  PH 30 and one instance entry, flush16<16>, flush16<14>
#: D  PH 190, two strips, the second starts at an odd entry (8-byte flushes
#:    inside an even PH)
#: E  PH 21, flush8<16>, flush8<5>
KERNEL_PROBLEMS = {
    'A': lambda n: problems.n_link_cart_pendulum(
        num_links=3, unknown_masses=2, num_nodes=n),
    'B': lambda n: problems.n_link_cart_pendulum(
        num_links=2, method='midpoint', num_nodes=n),
    'C': lambda n: problems.elementary_functions(
        method='midpoint', num_nodes=n),
    'D': lambda n: problems.n_link_cart_pendulum(
        num_links=5, method='midpoint', num_nodes=n),
    'E': lambda n: problems.odd_block_chain(num_nodes=n),
}

#: N - 1 of the block-edge cases: one node, one partial block, a full block
#: less one, exactly one and two blocks, one valid lane in the last block
EDGES = (1, 2, 63, 64, 65, 127, 128, 129)
BLOCK_EDGE_CASES = ([('A', m) for m in EDGES] + [('E', m) for m in EDGES] +
                    [('C', m) for m in (1, 64, 65)] +
                    [(k, m) for k in 'BD' for m in (65, 129)])

#: (label, N - 1) of tests/test_derived_handles_gpu.py: no instance constraint
#: and a full block plus one node; instance constraints, an unknown parameter
#: and a known trajectory (every kernel of both modules runs)
LIFECYCLE_CASES = (('A', 65), ('C', 65))

#: (label, N - 1) of the checks of how the Python surface takes its arguments
#: (:func:`surface_case`): five nodes, without and with instance constraints
SURFACE_CASES = (('A', 4), ('C', 4))

#: the code generator's default (``ConstraintCollocator._HESS_STRIP_OPS``)
DEFAULT_VARIANT = (1500, False, 1)
#: (label, (strip budget, forget, fast_trig)) of the emission paths that no
#: small problem reaches by itself, all at N - 1 = 65
FORCED_VARIANTS = [('A', (40, False, 1)), ('D', (40, False, 1)),
                   ('A', (200, True, 1)), ('D', (200, True, 1)),
                   ('A', (1500, False, 2))]
#: every module the GPU file launches
GPU_MODULES = [(k, DEFAULT_VARIANT) for k in 'ABCDE'] + FORCED_VARIANTS

#: the problems whose Hessian DAGs the SymPy comparison of
#: tests/test_hessian_cpu.py cannot afford
FD_PROBLEMS = ('biped_small', 'biped_mid_small', 'one_legged_small')

HESS_KERNELS = ('opty_hess', 'opty_hess_inst')

_FLUSH = re.compile(
    r'(opty_flush16|opty_flush8)<(\d+)>\(ring, hrow \+ (\d+), (\d+)LL, nv, '
    r'lane\);')
_CASE = re.compile(r'^\s*case (\d+): \{$', re.M)


def collocator(label, ncn, **extra):
    import opty_amd
    return opty_amd.ConstraintCollocator(
        **dict(KERNEL_PROBLEMS[label](ncn + 1), **extra))


def inputs(seed, col):
    rng = np.random.default_rng(seed)
    free = rng.uniform(-1.0, 1.0, col.num_free)
    if col._variable_duration:
        free[-1] = 0.02
    return free, rng.uniform(-1.0, 1.0, col.num_constraints)


@functools.lru_cache(maxsize=None)
def surface_case(label):
    """``(collocator, free, lagrange)`` of ``SURFACE_CASES`` -- in the CSR
    layout, which the augmented system needs and every other function takes
    --, one for all the test files: its handles are made once.  Nobody
    writes to the inputs."""
    col = collocator(label, dict(SURFACE_CASES)[label], jacobian_layout='csr')
    free, lam = inputs(17, col)
    free.flags.writeable = lam.flags.writeable = False
    return col, free, lam


def odd(a):
    """``(tensor, array)``: the values of ``a`` rounded to float32 as a CUDA
    tensor that is neither float64 nor contiguous (every other element of a
    float32 buffer; a two-dimensional ``a``: every other column), and as the
    float64 host array a function should make of it."""
    import torch
    a32 = np.asarray(a).astype(np.float32)
    wide = torch.from_numpy(np.repeat(a32, 2, axis=-1)).cuda()
    return wide[..., ::2], a32.astype(np.float64)


def bits(a):
    """The bit patterns of ``a`` (an array or a tensor of doubles)."""
    if hasattr(a, 'cpu'):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def interpreted(col, free, lam, nodes=None):
    """Values of the Hessian program from the CPU interpreter at the
    constraint nodes ``nodes`` (all by default): ``(block (len(nodes), PH),
    instance values, block bounds)``."""
    prog = col._build_hessian_program()
    ncn = col.num_collocation_nodes - 1
    nodes = np.arange(ncn) if nodes is None else np.asarray(nodes)
    inputs = col._hessian_inputs(free, lam, nodes)
    vals, bound = dag_interp.evaluate_with_error_bound(
        prog.dag, prog.hess_out, inputs)
    block = np.stack([np.broadcast_to(np.asarray(v, dtype=float),
                                      (len(nodes),)) for v in vals], axis=1)
    bnd = np.stack([np.broadcast_to(np.asarray(v, dtype=float),
                                    (len(nodes),)) for v in bound], axis=1)
    ivals = dag_interp.evaluate(prog.dag, prog.inst_hess_out, inputs)
    inst = np.array([float(v)*lam[prog.M*ncn + k]
                     for v, k in zip(ivals, prog.inst_hess_con)])
    return block, inst, bnd


def switch_cases(source):
    """``[(case number, text of the case)]`` of the strip switch of
    ``opty_hess`` in an emitted module, in source order."""
    end = source.index('default: break;')
    marks = [(int(m.group(1)), m.start()) for m in _CASE.finditer(source)
             if m.start() < end]
    bounds = [pos for _, pos in marks] + [end]
    return [(s, source[bounds[k]:bounds[k + 1]])
            for k, (s, _) in enumerate(marks)]


def flush_calls(text):
    """``[(kind, w, c0, P)]`` of the tile flushes in ``text``, in order:
    ``kind`` is 16 or 8 (bytes per store), ``w`` the entries flushed, ``c0``
    the first one, ``P`` the row pitch passed."""
    return [(16 if m.group(1) == 'opty_flush16' else 8, int(m.group(2)),
             int(m.group(3)), int(m.group(4))) for m in _FLUSH.finditer(text)]


def descriptor(col, cut):
    """The ``opty_hip_hessian_desc`` of ``col`` for the strip cut ``cut``, as
    ``ConstraintCollocator._ensure_hessian`` fills it."""
    prog = col._build_hessian_program()
    rows, cols = col.hessian_indices_closed_form()
    PH, ncn = prog.PH, col.num_collocation_nodes - 1
    return dict(PH=PH, nnz_inst=len(prog.inst_hess_out),
                strips=max(1, len(cut)),
                pattern=np.array(prog.index_pattern(), dtype=np.int32),
                inst_rows=rows[ncn*PH:], inst_cols=cols[ncn*PH:])


def forced_module(col, variant):
    """``(code object, strip cut, source)`` of ``col``'s Hessian module
    emitted with ``variant = (budget, forget, fast_trig)``; a build that
    spills vector registers is refused here and never launched."""
    from opty_amd import hip_backend as hb
    from opty_amd.codegen.emit_hessian import emit_hessian_module
    source, cut = emit_hessian_module(col._build_hessian_program(), *variant)
    hsaco = col._compile(source)
    assert hb.vgpr_spills(hsaco, HESS_KERNELS) == {}, (variant, hsaco)
    return hsaco, cut, source


def prebuild_jobs():
    """Thunks that build the code objects of tests/test_hessian_kernel_gpu.py
    (``__graft_entry__.build`` runs them side by side): the Hessian module of
    every problem and forced variant, the constraint / Jacobian module of
    every node count (its geometry depends on the launch size), the product
    modules of the lifecycle cases, and the Hessian and product modules of
    the finite-difference check."""
    import opty_amd

    def small():
        seen = set()
        for label, ncn in BLOCK_EDGE_CASES:
            col = collocator(label, ncn)
            col.prebuild()
            if label not in seen:
                seen.add(label)
                col._build_hessian_code_object()
        for label, variant in FORCED_VARIANTS:
            forced_module(collocator(label, 65), variant)
        for label, ncn in LIFECYCLE_CASES:
            collocator(label, ncn)._build_jacprod_code_object()
        for label, ncn in SURFACE_CASES:
            col = collocator(label, ncn, jacobian_layout='csr')
            col.prebuild()
            col._build_jacprod_code_object()
            col._build_jacprod_block_code_object()

    def named(name):
        col = opty_amd.ConstraintCollocator(**problems.build(name))
        col.prebuild()
        col._build_hessian_code_object()
        if name in FD_PROBLEMS:
            col._build_jacprod_code_object()
    return [small] + [lambda name=name: named(name)
                      for name in ('msd_be_small',) + FD_PROBLEMS]
