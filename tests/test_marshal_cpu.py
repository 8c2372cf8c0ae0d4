"""The argument marshaller (:mod:`opty_amd.marshal`) without a device: NumPy
arrays take the host path, torch CPU tensors -- they have ``data_ptr`` -- the
torch path, with the wait for torch's stream recorded and launches that
record what they are given."""
import numpy as np
import pytest
import torch

from opty_amd import marshal as ma
from opty_amd.hip_backend import HOST, DEVICE


@pytest.fixture
def events(monkeypatch):
    log = []
    monkeypatch.setattr(ma, 'wait_for_torch',
                        lambda device: log.append(('wait', device)))
    return log


# -- primitives ---------------------------------------------------------------
def test_on_device_is_the_data_ptr_test():
    assert ma.on_device(torch.zeros(2))
    assert not ma.on_device(np.zeros(2)) and not ma.on_device([0.0, 1.0])


def test_host_vector_converts_and_keeps_what_conforms():
    x = np.arange(5.0)
    assert ma.host_vector(x, 'v', 5) is x
    for given in ([0, 1, 2, 3, 4], x.astype(np.float32), np.arange(10.0)[::2],
                  np.asfortranarray(x)):
        out = ma.host_vector(given, 'v', 5)
        assert out.dtype == np.float64 and out.flags.c_contiguous
        assert out.shape == (5,)
        assert np.array_equal(out, np.asarray(given, dtype=np.float64))
    assert ma.host_vector([], 'v', 0).shape == (0,)


def test_host_vector_refusals_are_verbatim():
    with pytest.raises(ValueError) as err:
        ma.host_vector(np.zeros(4), 'free', 5)
    assert str(err.value) == 'free must have shape (5,), got (4,)'
    with pytest.raises(ValueError) as err:
        ma.host_vector(np.zeros((5, 1)), 'lagrange', 5)
    assert str(err.value) == 'lagrange must have shape (5,), got (5, 1)'


def test_host_block_converts_and_keeps_what_conforms():
    V = np.arange(12.0).reshape(4, 3)
    F = np.asfortranarray(V)
    assert ma.host_block(F, 'V', 4) is F
    assert ma.column_major(F) is F
    wide = np.arange(24.0).reshape(4, 6)
    for given in (V, V.tolist(), V.astype(np.float32), wide[:, ::2], F[:, ::2],
                  F[:, :0]):
        out = ma.host_block(given, 'V', 4)
        want = np.asarray(given, dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.f_contiguous
        assert out.shape == want.shape and np.array_equal(out, want)


def test_host_block_refusals_are_verbatim():
    with pytest.raises(ValueError) as err:
        ma.host_block(np.zeros(4), 'V', 4)
    assert str(err.value) == 'V must have shape (4, k), got (4,)'
    with pytest.raises(ValueError) as err:
        ma.host_block(np.zeros((3, 2)), 'W', 4)
    assert str(err.value) == 'W must have shape (4, k), got (3, 2)'


class _NeverCast(torch.Tensor):
    """A tensor that must be refused by its shape, before any conversion."""
    def to(self, *args, **kwargs):
        raise AssertionError('converted before the shape was checked')

    def contiguous(self, *args, **kwargs):
        raise AssertionError('converted before the shape was checked')

    t = contiguous


def test_device_shapes_are_checked_before_any_conversion():
    x = torch.zeros(4, dtype=torch.float32).as_subclass(_NeverCast)
    with pytest.raises(ValueError) as err:
        ma.device_vector(x, 'v', 5)
    assert str(err.value) == 'v must have shape (5,), got (4,)'
    with pytest.raises(ValueError) as err:
        ma.check_vector(x, 'sigma', 3)
    assert str(err.value) == 'sigma must have shape (3,), got (4,)'
    assert ma.check_vector(x, 'sigma', 4) is None
    with pytest.raises(ValueError, match=r'v must have shape \(4,\), got'):
        ma.device_vector(torch.zeros(4, 1).as_subclass(_NeverCast), 'v', 4)
    X = torch.zeros((3, 2), dtype=torch.float32).as_subclass(_NeverCast)
    with pytest.raises(ValueError) as err:
        ma.device_block(X, 'V', 4)
    assert str(err.value) == 'V must have shape (4, k), got (3, 2)'
    with pytest.raises(ValueError, match=r'V must have shape \(4, k\), got'):
        ma.device_block(torch.zeros(4).as_subclass(_NeverCast), 'V', 4)
    # ... in the vectors of one call too: the second is wrong, the first is
    # not converted
    with pytest.raises(ValueError, match=r'w must have shape \(3,\)'):
        ma.device_vectors(((torch.zeros(4).as_subclass(_NeverCast), 'v', 4),
                           (torch.zeros(2), 'w', 3)))


def test_device_vector_converts():
    x = torch.arange(5, dtype=torch.float64)
    assert ma.device_vector(x, 'v', 5).data_ptr() == x.data_ptr()
    for given in (x.to(torch.float32), torch.arange(10.0)[::2]):
        out = ma.device_vector(given, 'v', 5, torch.device('cpu'))
        assert out.dtype == torch.float64 and out.is_contiguous()
        assert torch.equal(out, given.to(torch.float64))
    assert ma.device_vector(torch.zeros(0), 'v', 0).shape == (0,)


@pytest.mark.parametrize('k', [0, 1, 3])
def test_device_block_rows_are_the_columns(k):
    n = 4
    X = torch.arange(float(n*k), dtype=torch.float32).reshape(n, k)
    for given in (X, X.to(torch.float64), X.t().contiguous().t()):
        out = ma.device_block(given, 'V', n)
        assert out.dtype == torch.float64 and out.is_contiguous()
        assert tuple(out.shape) == (k, n)
        for c in range(k):
            assert torch.equal(out[c], given[:, c].to(torch.float64))


# -- drivers ------------------------------------------------------------------
def test_call_vectors_on_the_host_returns_the_same_buffer():
    result = np.full(3, np.nan)
    calls = []

    def launch(a, b, out, kind):
        calls.append((a, b, kind))
        out[:] = a[:3] + b[:3]
    for _ in range(2):
        got = ma.call_vectors(
            launch, (([1, 2, 3, 4], 'a', 4), (np.ones(5, np.float32), 'b', 5)),
            result, lambda: calls.append('synchronize'))
        assert got is result and np.array_equal(got, [2.0, 3.0, 4.0])
    assert len(calls) == 2            # (the host launch is synchronous)
    a, b, kind = calls[0]
    assert kind == HOST and a.dtype == b.dtype == np.float64
    with pytest.raises(ValueError) as err:
        ma.call_vectors(launch, ((np.zeros(4), 'a', 4), (np.zeros(4), 'b', 5)),
                        result, None)
    assert str(err.value) == 'b must have shape (5,), got (4,)'
    assert len(calls) == 2


def test_call_vectors_torch_order_and_optional_vector(events):
    result = np.empty(3)

    def launch(a, sigma, dw, dc, out, kind):
        events.append(('launch', a, sigma, dw, dc, out, kind))

    def before(first):
        events.append(('before', first))
    a = torch.arange(8, dtype=torch.float32)[::2]
    outs = []
    for sigma in (None, torch.ones(2, dtype=torch.float32)):
        del events[:]
        out = ma.call_vectors(
            launch, ((a, 'a', 4), (sigma, 'sigma', 2)), result,
            lambda: events.append(('synchronize',)), scalars=(0.5, 0.25),
            before=before)
        outs.append(out)
        assert [e[0] for e in events] == ['before', 'wait', 'launch',
                                          'synchronize']
        # the conversions came first: what ``before`` and the launch got
        first = events[0][1]
        assert first.dtype == torch.float64 and first.is_contiguous()
        assert torch.equal(first, a.to(torch.float64))
        assert events[1][1] == a.device
        _, got_a, got_sigma, dw, dc, got_out, kind = events[2]
        assert got_a is first and (dw, dc, kind) == (0.5, 0.25, DEVICE)
        if sigma is None:
            assert got_sigma is None
        else:
            assert got_sigma.dtype == torch.float64
            assert torch.equal(got_sigma, torch.ones(2, dtype=torch.float64))
        assert got_out is out and tuple(out.shape) == (3,)
        assert out.dtype == torch.float64
    assert outs[0].data_ptr() != outs[1].data_ptr()     # new per call
    del events[:]
    with pytest.raises(ValueError, match=r'sigma must have shape \(2,\)'):
        ma.call_vectors(launch, ((a, 'a', 4), (torch.ones(3), 'sigma', 2)),
                        result, None, scalars=(0.0, 0.0), before=before)
    assert events == []


def _block_launch(log):
    def launch(x, cols, rows, out, nout, k, kind):
        log.append(('launch', x, cols, rows, nout, k, kind))
        for c in range(k):
            if kind == HOST:
                out[:, c] = x[0]*cols[:nout, c]
            else:
                out[c] = x[0]*cols[c, :nout]
    return launch


@pytest.mark.parametrize('k', [0, 1, 3])
def test_call_block_on_the_host(k):
    log = []
    V = np.arange(4.0*k).reshape(4, k)
    for given in (V, np.asfortranarray(V), V.astype(np.float32)):
        del log[:]
        out = ma.call_block(_block_launch(log), ([2.0], 'x', 1),
                            (given, 'V', 4), 3, None)
        assert out.shape == (3, k) and out.flags.f_contiguous
        assert out.dtype == np.float64
        assert np.array_equal(out, 2.0*V[:3])
        assert len(log) == (1 if k else 0)          # no column, no launch
        if k:
            assert log[0][2].flags.f_contiguous and log[0][3:] == (4, 3, k,
                                                                  HOST)
    again = ma.call_block(_block_launch(log), ([2.0], 'x', 1), (V, 'V', 4), 3,
                          None)
    assert again is not out
    with pytest.raises(ValueError) as err:
        ma.call_block(_block_launch(log), ([2.0], 'x', 1), (V[1:], 'V', 4), 3,
                      None)
    assert str(err.value) == 'V must have shape (4, k), got (3, %d)' % k


@pytest.mark.parametrize('k', [0, 1, 3])
def test_call_block_torch_order_and_layout(events, k):
    V = torch.arange(4.0*k, dtype=torch.float32).reshape(4, k)
    x = torch.tensor([2.0], dtype=torch.float32)
    out = ma.call_block(
        _block_launch(events), (x, 'x', 1), (V, 'V', 4), 3,
        lambda: events.append(('synchronize',)),
        before=lambda first: events.append(('before', first)))
    assert tuple(out.shape) == (3, k) and out.dtype == torch.float64
    assert out.t().is_contiguous()          # the view of a (k, 3) buffer
    assert torch.equal(out, 2.0*V[:3].to(torch.float64))
    if not k:
        assert events == []
        return
    assert [e[0] for e in events] == ['before', 'wait', 'launch',
                                      'synchronize']
    _, got_x, cols, rows, nout, kk, kind = events[2]
    assert got_x is events[0][1] and got_x.dtype == torch.float64
    assert cols.is_contiguous() and tuple(cols.shape) == (k, 4)
    assert (rows, nout, kk, kind) == (4, 3, k, DEVICE)


@pytest.mark.parametrize('k', [0, 1, 3])
def test_call_block_single_column_detour(events, k):
    """One column, or any number without a block launch, goes through the
    single-vector function and has its results."""
    singles = []

    def single(x, col):
        singles.append(col)
        return 3.0*col[:3]
    V = np.arange(4.0*k).reshape(4, k)
    for launch in (None, _block_launch(events)):
        for given in (V, torch.from_numpy(V)):
            del singles[:], events[:]
            x = [2.0] if given is V else torch.tensor([2.0])
            out = ma.call_block(launch, (x, 'x', 1), (given, 'V', 4), 3,
                                lambda: events.append(('synchronize',)),
                                single=single)
            assert tuple(out.shape) == (3, k)
            through_single = k == 1 or (launch is None and k > 0)
            assert len(singles) == (k if through_single else 0)
            factor = 3.0 if through_single else 2.0
            assert np.array_equal(np.asarray(out), factor*V[:3])
            if through_single or not k:
                assert not [e for e in events if e[0] == 'launch']


# -- the operators' torch hooks -----------------------------------------------
def test_tensor_operands_hands_tensors_over_as_they_are():
    from scipy.sparse.linalg import LinearOperator
    seen = []

    class Twice(ma.tensor_operands('matvec', 'matmat'), LinearOperator):
        def __init__(self):
            super().__init__(np.dtype(np.float64), (3, 3))

        def _matvec(self, x):
            seen.append(x)
            return 2*x

        def _matmat(self, X):
            seen.append(X)
            return 2*X
    op = Twice()
    x = torch.ones(3)
    assert torch.equal(op.matvec(x), 2*x) and seen[-1] is x
    X = torch.ones(3, 2)
    assert torch.equal(op.matmat(X), 2*X) and seen[-1] is X
    # an array goes SciPy's way, with its checks
    assert np.array_equal(op.matvec(np.ones(3)), 2*np.ones(3))
    assert isinstance(seen[-1], np.ndarray)
    with pytest.raises(ValueError):
        op.matvec(np.ones(4))
    assert 'rmatvec' not in vars(Twice.__mro__[1])
