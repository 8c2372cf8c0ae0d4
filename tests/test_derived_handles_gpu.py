"""GPU test of the lifecycle that the handles derived from a problem handle
share (``hip_backend.HipHessian`` / ``HipJacobianProduct``, C ABI
``opty_hip_hessian_*`` / ``opty_hip_jacprod_*``): they are released when the
problem's C handle is reloaded or closed, created again on the next call, and
follow the problem to another stream -- with the same bits every time."""
import numpy as np
import pytest

import hessian_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('label, ncn', hc.LIFECYCLE_CASES)
def test_reload_stream_change_and_close(label, ncn):
    import torch
    from opty_amd import hip_backend as hb
    col = hc.collocator(label, ncn)
    hess = col.generate_hessian_function()
    jvp, vjp = col.generate_jvp_function(), col.generate_vjp_function()
    assert jvp.handle is vjp.handle
    handles = (hess.handle, jvp.handle)
    free, lam = hc.inputs(11, col)
    v = np.random.default_rng(12).uniform(-1.0, 1.0, col.num_free)
    calls = ((hess, lam), (jvp, v), (vjp, lam))

    def values():
        # (the results are persistent buffers that the next call overwrites)
        return [f(free, x).copy() for f, x in calls]

    def same_bits(got, what):
        for (f, _), a, b in zip(calls, first, got):
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), \
                (label, what, f.__name__)

    first = values()
    assert [len(x) for x in first] == [hess.handle.nnz, col.num_constraints,
                                       col.num_free]
    assert all(np.all(np.isfinite(x)) for x in first)
    assert all(x.any() for x in first)

    # a reload of the problem's C handle releases both derived handles ...
    col._respecialize(col._hip)
    assert all(h._h is None for h in handles)
    # ... and the next call creates them again for the new one
    same_bits(values(), 'reload')
    assert all(h._h is not None for h in handles)

    # the problem moves to a fresh non-default stream: they follow it
    stream = torch.cuda.Stream()
    col._hip.use_torch_stream(stream)
    same_bits(values(), 'stream')
    same_bits(values(), 'stream, second call')

    # a closed problem handle: an error from the Python-side guard (nothing
    # reaches the device)
    col._hip.close()
    assert all(h._h is None for h in handles)
    for f, x in calls:
        with pytest.raises(hb.HipBackendError, match='closed'):
            f(free, x)
    del stream
