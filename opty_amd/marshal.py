"""Argument handling of the functions that run a derived handle
(:mod:`opty_amd.direct_collocation`): every one of them takes NumPy arrays --
converted on the host, answered from a buffer the function owns -- or torch
tensors, converted and answered on their device.  Stateless.

The rule of the torch path is written once, in the two drivers: every torch
operation that produces an input comes BEFORE :func:`wait_for_torch`, every
launch on the collocator's stream after it.  A launch that overtook a pending
``.to()`` / ``.contiguous()`` would read what is not written yet.
"""

import numpy as np

from .hip_backend import HOST, DEVICE


def on_device(x):
    """Whether ``x`` takes the torch path (any tensor has ``data_ptr``)."""
    return hasattr(x, 'data_ptr')


def column_major(V):
    """``V`` (two-dimensional, either memory order, any real dtype) as a
    column-major float64 array: column ``c`` is the ``V.shape[0]`` contiguous
    doubles at ``c*V.shape[0]``, what ``opty_hip_hessmv_apply_block`` takes
    with ``ldv = V.shape[0]``.  A column-major float64 ``V`` is returned as
    it is; anything else is copied once."""
    return np.asfortranarray(V, dtype=np.float64)


def _refuse(name, shape, got):
    raise ValueError('{} must have shape {}, got {}'.format(name, shape,
                                                            tuple(got)))


def check_vector(x, name, count):
    """Refuses an ``x`` (an array or a tensor) whose shape is not
    ``(count,)``; nothing is converted."""
    if tuple(x.shape) != (count,):
        _refuse(name, '({},)'.format(count), x.shape)


def _check_block(X, name, rows):
    if np.ndim(X) != 2 or np.shape(X)[0] != rows:
        _refuse(name, '({}, k)'.format(rows), np.shape(X))


def host_vector(x, name, count):
    """``x`` as a contiguous float64 array of shape ``(count,)`` (``x``
    itself where it is one already)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    check_vector(x, name, count)
    return x


def host_block(X, name, rows):
    """``X`` as a column-major float64 array of shape ``(rows, k)``."""
    _check_block(X, name, rows)
    return column_major(X)


def _float64_on(torch, x, device):
    # (``torch``: the module, imported once per call by whoever converts)
    if not on_device(x):
        x = torch.as_tensor(x)
    return x.to(device=device, dtype=torch.float64)


def device_vector(x, name, count, device=None):
    """``x`` as a contiguous float64 tensor of shape ``(count,)`` on
    ``device`` (default: its own); the shape is checked before anything is
    converted."""
    import torch
    check_vector(x, name, count)
    return _float64_on(torch, x, device).contiguous()


def device_block(X, name, rows, device=None):
    """The columns of ``X`` (shape ``(rows, k)``) as the rows of a contiguous
    float64 tensor of shape ``(k, rows)`` on ``device``."""
    import torch
    _check_block(X, name, rows)
    return _float64_on(torch, X, device).t().contiguous()


def host_vectors(vectors):
    """:func:`host_vector` of every ``(x, name, count)`` of ``vectors``; an
    ``x`` that is None (an optional argument not given) stays None."""
    return [x if x is None else host_vector(x, name, count)
            for x, name, count in vectors]


def device_vectors(vectors):
    """:func:`device_vector` of every ``(x, name, count)`` of ``vectors`` on
    the first one's device, None staying None; every shape is checked before
    anything is converted."""
    import torch
    for x, name, count in vectors:
        if x is not None:
            check_vector(x, name, count)
    device = vectors[0][0].device
    return [x if x is None else _float64_on(torch, x, device).contiguous()
            for x, _, _ in vectors]


def wait_for_torch(device):
    """Waits for what torch has queued on its current stream of ``device``:
    the conversions above run there, the handles launch on a stream of their
    own."""
    import torch
    torch.cuda.current_stream(device).synchronize()


def call_vectors(launch, vectors, result, synchronize, scalars=(),
                 before=None):
    """``launch(*vectors, *scalars, out, memory kind)`` for ``vectors`` =
    ``((x, name, count), ...)``; an ``x`` that is None stays None (an optional
    argument not given).  The first ``x`` decides the path.  Host arrays: the
    launch writes ``result`` (the caller's persistent buffer), which is
    returned.  Tensors: all go to the first one's device and a new tensor
    of ``len(result)`` values there is returned; ``synchronize()`` waits for
    the launch.  ``before(first)`` runs between the conversions and the
    launch with the converted first vector."""
    if on_device(vectors[0][0]):
        args = device_vectors(vectors)
        if before is not None:
            before(args[0])
        out = args[0].new_empty(len(result))        # float64, same device
        wait_for_torch(out.device)
        launch(*args, *scalars, out, DEVICE)
        synchronize()
        return out
    args = host_vectors(vectors)
    if before is not None:
        before(args[0])
    launch(*args, *scalars, result, HOST)
    return result


def call_block(launch, vector, block, nout, synchronize, before=None,
               single=None):
    """``launch(x, columns, rows, out, nout, k, memory kind)`` for ``vector``
    = ``(x, name, count)`` and ``block`` = ``(X, name, rows)``, ``X`` of
    shape ``(rows, k)``: a new ``(nout, k)`` result, column-major on the
    host, the transpose of a ``(k, nout)`` tensor on ``x``'s device.  No
    column, no launch.  With ``single`` -- the function of one column,
    ``single(x, column)`` -- one column, or any number when ``launch`` is
    None, go through it instead."""
    x, X = vector[0], block[0]
    rows = block[2]
    if on_device(x):
        import torch
        check_vector(*vector)
        _check_block(*block)
        x = _float64_on(torch, x, None).contiguous()
        cols = _float64_on(torch, X, x.device).t().contiguous()
        k = cols.shape[0]
        if single is not None and (k == 1 or (launch is None and k)):
            return torch.stack([single(x, col) for col in cols], dim=1)
        if k and before is not None:
            before(x)
        out = x.new_empty((k, nout))                # float64, same device
        if k:
            wait_for_torch(x.device)
            launch(x, cols, rows, out, nout, k, DEVICE)
            synchronize()
        return out.t()
    x = host_vector(*vector)
    X = host_block(*block)
    k = X.shape[1]
    out = np.empty((nout, k), dtype=np.float64, order='F')
    if single is not None and (k == 1 or launch is None):
        for c in range(k):
            out[:, c] = single(x, X[:, c])
    elif k:
        if before is not None:
            before(x)
        launch(x, X, rows, out, nout, k, HOST)
    return out


def tensor_operands(*methods):
    """A mixin for a ``scipy.sparse.linalg.LinearOperator`` whose ``methods``
    (``'matvec'``, ``'matmat'``, ...) hand a tensor operand to ``_matvec``,
    ``_matmat``, ... as it is: SciPy would convert it to an array."""
    def hook(name):
        def method(self, x):
            if on_device(x):
                return getattr(self, '_' + name)(x)
            return getattr(super(TensorOperands, self), name)(x)
        method.__name__ = name
        return method
    TensorOperands = type('TensorOperands', (),
                          {name: hook(name) for name in methods})
    return TensorOperands
