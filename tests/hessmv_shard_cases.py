"""What tests/test_hessmv_shard_cpu.py and tests/test_hessmv_shard_gpu.py
share with ``__graft_entry__.build``: the windows of the node-sharded Hessian
operator, how the windows of a partition are put together, the synthetic
descriptor, and the code objects no other list builds.  The problems, worlds
and the process problem are those of ``hessian_shard_cases`` (their modules are
built there), the synthetic descriptor runs on a carrier of
``hessian_synth_cases``."""
import numpy as np

import hessian_shard_cases as hs
import hessian_synth_cases as sc

NCN = hs.NCN
PROBLEMS = hs.PROBLEMS
TWO_STRIPS = hs.TWO_STRIPS
WORLDS = hs.WORLDS
RANKS = hs.RANKS
#: windows ``[a, b)`` of the 200 nodes.  A window that starts the problem
#: stores 64 time nodes in its first block, every other block 63, and a window
#: with ``a > 0`` starts one halo node early: one node short of, exactly at and
#: one past a block for both kinds of start; two blocks and a last block with
#: one node; windows that own time node N - 1; the whole problem; an empty one
WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (1, 2), (1, 64), (1, 65),
           (62, 126), (63, 127), (64, 200), (137, 200), (199, 200), (0, 200),
           (5, 5)]
#: the synthetic descriptor: carrier, N - 1 (a node count its module is built
#: for), keywords of ``hessian_synth_cases.descriptor`` -- the deliberate
#: explicit triplets in interior trajectory rows and in tail rows plus
#: scattered ones, constraint section only
SYNTH_CARRIER, SYNTH_NCN = 'c43', 127
SYNTH_KW = dict(seed=14, density=0.6, repeat=0.2, explicit=True, scattered=8,
                obj=0, pairs=0)
#: nodes of the example in the suite
EXAMPLE_NODES = 20


def owned(N, a, b):
    """``(lo, hi)``: the time nodes the window ``[a, b)`` owns (stated here on
    its own: the last non-empty window also owns node ``N - 1``)."""
    return a, b + (1 if a < b and b == N - 1 else 0)


def window_values(values, PH, a, b):
    """The values of the nodes ``[a - (a > 0), b)`` out of the whole node
    section."""
    return values[(a - (1 if a > 0 else 0))*PH:b*PH]


def synth_case():
    """``(carrier name, N, nrows, ntail, descriptor, rows, cols)``."""
    nrows, ntail = sc.CARRIERS[SYNTH_CARRIER]
    N = SYNTH_NCN + 1
    desc = sc.descriptor(nrows=nrows, ntail=ntail, N=N, **SYNTH_KW)
    assert len(desc['obj_pattern']) == 0 and len(desc['tail_rows']) == 0
    rows, cols = sc.triplets(desc, nrows, ntail, N)
    return SYNTH_CARRIER, N, nrows, ntail, desc, rows, cols


def put_together(N, nrows, ntail, ranges, shares):
    """``y`` (``nrows*N + ntail``, NaN where no window wrote) from the
    ``(block, tail_part)`` of the windows ``ranges``: the blocks at the time
    nodes their windows own, the tail the sum of the shares in window
    order."""
    y = np.full(nrows*N + ntail, np.nan)
    traj = y[:nrows*N].reshape(nrows, N)
    total = np.zeros(ntail)
    for (a, b), (block, part) in zip(ranges, shares):
        lo, hi = owned(N, a, b)
        assert block.shape == (nrows, hi - lo)
        assert np.isnan(traj[:, lo:hi]).all(), 'two windows own an entry'
        traj[:, lo:hi] = block
        total = total + part
    y[nrows*N:] = total
    return y


def prebuild_jobs():
    """Thunks that build the code objects of the sharded-operator tests which
    no other list builds (``__graft_entry__.build`` runs them side by side):
    the modules of the example at the launch sizes of its worlds."""
    def example():
        from examples import sharded_kkt_minres
        sharded_kkt_minres.prebuild(EXAMPLE_NODES)
    return [example]
