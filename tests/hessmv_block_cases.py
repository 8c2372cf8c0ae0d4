"""What tests/test_hessmv_block_gpu.py shares with ``__graft_entry__.build``:
the cases of the block products of the Hessian operator and the code objects
they load.  The answers, the tolerance and the index tables are those of
``hessmv_cases``."""
import hessian_cases as hc
import hessmv_cases as mc

#: (label, N - 1): blocks of 64 lanes advance by 63 nodes -- one node, a full
#: block less one, one node past it, one lane of a second block, two blocks
#: and a third one's first lane
EDGES = [(k, m) for k in 'AE' for m in (1, 63, 64, 65, 128)]
#: the case with an instance entry, the one of the guard bands and of the
#: Python surface
INSTANCE_CASE, GUARD_CASE, SURFACE_CASE = ('C', 65), ('A', 65), ('E', 65)
#: node count of the example's run
EXAMPLE_NODES = 20


def ncols_of(width):
    """Column counts that take every pass structure of a handle whose pass
    takes ``width`` columns: one column, two, one full pass, a full pass and
    a single column, two full passes and a single column -- and three
    columns, alone and behind a full pass, so that every instantiation of
    the kernel runs at every block edge whatever ``width`` is."""
    return sorted({1, 2, 3, width, width + 1, width + 3, 2*width + 1})


def prebuild_jobs():
    """Thunks that build the code objects the block-product tests load
    (``__graft_entry__.build`` runs them side by side).  The product kernels
    are the runtime library's; what is built here are the modules of the
    problem handles that the product handles borrow, and the example's."""
    import opty_amd
    from examples import problems

    def edges():
        for label, ncn in EDGES + [INSTANCE_CASE, GUARD_CASE, SURFACE_CASE]:
            hc.collocator(label, ncn).prebuild()

    def named():
        for name in ('vardur_pendulum_small', 'biped_small'):
            opty_amd.ConstraintCollocator(**problems.build(name)).prebuild()
        opty_amd.ConstraintCollocator(**mc.carrier_problem()).prebuild()

    def example():
        from examples import hessian_lobpcg
        hessian_lobpcg.prebuild(EXAMPLE_NODES)
    return [edges, named, example]
