"""The direct solver with the constraint normal matrix

    S = Jc[:, :T] diag(1/d[:T]) Jc[:, :T]^T + delta_c I

(``Jc``: the ``M(N-1)`` collocation rows of the constraint Jacobian, ``T =
(n+q)N`` the trajectory part of ``free``) that
:meth:`opty_amd.ConstraintCollocator.generate_normal_solver` returns:
:class:`NormalSolver` over one :class:`opty_amd.hip_backend.HipNormalSolver`
handle.  Ordered by constraint node ``S`` is
symmetric block tridiagonal; it is formed, factorised -- block cyclic
reduction with Cholesky factors -- and solved with on the GPU.

The tail columns (unknown parameters, a free interval) and the instance rows
are NOT part of ``S``: ``S`` is all of ``J D^-1 J^T`` only for a problem that
has neither; otherwise it is a preconditioner (a low-rank correction for the
tail is not done).
"""

import numpy as np

from . import hip_backend as hb
from .marshal import (device_block, device_vector, device_vectors,
                      host_block, host_vector, host_vectors, on_device,
                      wait_for_torch)


class NormalSolver(object):
    """``factor`` / ``factor_values`` form and factorise ``S``; ``solve``
    applies ``S^-1``; ``blocks`` returns the blocks of ``S`` themselves.
    NumPy arrays in give NumPy arrays out, torch CUDA tensors in give CUDA
    tensors out (nothing crosses PCIe).  ``d`` has ``num_free`` values of
    which the first ``T`` are read; they must be positive (not checked);
    default: ones.  The same inputs give the same bits."""

    def __init__(self, collocator, handle):
        self._col = collocator
        self.handle = handle
        self._hip = collocator._hip
        prog = collocator._build_program()
        self.M = prog.M
        self.num_nodes = collocator.num_collocation_nodes - 1
        #: rows of ``S``
        self.size = self.M*self.num_nodes
        self._own = {}
        #: counts the factorisations (an operator checks that it is current)
        self.generation = 0

    @property
    def workspace_bytes(self):
        """Device memory the handle owns: every level's blocks and vectors
        and the column tables."""
        return self.handle.workspace_bytes

    # -- factorisation -------------------------------------------------
    def _report(self):
        self.generation += 1
        failed = self.handle.status()
        if failed is not None:
            raise np.linalg.LinAlgError(
                'the normal matrix is not positive definite: a pivot that '
                'is not positive and finite at level %d, row %d' % failed)

    def factor_values(self, jac_values, d=None, delta_c=0.0):
        """Forms ``S`` from ``jac_values`` -- the values of
        ``jacobian(free)`` in the collocator's layout -- and factorises it.
        A pivot that is not positive and finite raises
        ``numpy.linalg.LinAlgError`` naming its level and row."""
        point = ((jac_values, 'jac_values', self._hip.nnz),
                 (d, 'd', self._col.num_free))
        if on_device(jac_values):
            jac_values, d = device_vectors(point)
            wait_for_torch(jac_values.device)
            self.handle.factor(jac_values, d, delta_c, hb.DEVICE)
        else:
            jac_values, d = host_vectors(point)
            self.handle.factor(jac_values, d, delta_c, hb.HOST)
        self._report()

    def factor(self, free, d=None, delta_c=0.0):
        """Evaluates the Jacobian at ``free`` into a device buffer of the
        solver's own, forms ``S`` and factorises it: the bits of
        ``factor_values(jacobian(free), d, delta_c)``."""
        col, hip = self._col, self._hip
        point = ((free, 'free', col.num_free), (d, 'd', col.num_free))
        if on_device(free):
            import torch
            free, d = device_vectors(point)
            col._sync_free(free)
            jac = self._own.get('torch')
            if jac is None or jac.device != free.device:
                jac = self._own['torch'] = torch.empty(
                    hip.nnz, dtype=torch.float64, device=free.device)
            wait_for_torch(free.device)
            hip.eval_jac(free, jac, hb.DEVICE)
            self.handle.factor(jac, d, delta_c, hb.DEVICE)
        else:
            free, d = host_vectors(point)
            col._sync_free(free)
            if 'host' not in self._own:
                self._own['host'] = tuple(
                    hb.DeviceVector(np.zeros(k), col._device)
                    for k in (col.num_free, hip.nnz, col.num_free))
            d_free, d_jac, d_d = self._own['host']
            d_free.assign(free)
            if d is not None:
                d_d.assign(d)
            hip.eval_jac(d_free, d_jac, hb.DEVICE)
            self.handle.factor(d_jac, None if d is None else d_d, delta_c,
                               hb.DEVICE)
        self._report()

    # -- the blocks themselves -----------------------------------------
    def blocks(self, jac_values, d=None, delta_c=0.0):
        """``(A, B)``: the diagonal blocks ``A`` of shape ``(N-1, M, M)``
        and the couplings ``B`` of shape ``(N-2, M, M)``, ``B[i] = S[i+1,
        i]``, of ``S`` ordered by constraint node.  Does not touch a
        factorisation."""
        M, n = self.M, self.num_nodes
        point = ((jac_values, 'jac_values', self._hip.nnz),
                 (d, 'd', self._col.num_free))
        if on_device(jac_values):
            jac_values, d = device_vectors(point)
            A = jac_values.new_empty((n, M, M))
            B = jac_values.new_empty((n - 1, M, M))
            wait_for_torch(jac_values.device)
            self.handle.blocks(jac_values, d, delta_c, A, B, hb.DEVICE)
            self._hip.synchronize()
            return A, B
        jac_values, d = host_vectors(point)
        A, B = np.empty((n, M, M)), np.empty((n - 1, M, M))
        self.handle.blocks(jac_values, d, delta_c, A, B, hb.HOST)
        return A, B

    # -- solve -----------------------------------------------------------
    def solve(self, r):
        """``S^-1 r`` for ``r`` of shape ``(M(N-1),)`` or ``(M(N-1), k)`` in
        the order of ``constraints(free)``; the columns are solved one after
        the other, each bit for bit as it would be alone.  A new array (or
        tensor) per call."""
        m = self.size
        if np.ndim(r) == 1:
            if on_device(r):
                r = device_vector(r, 'r', m)
                y = r.new_empty(m)
                wait_for_torch(r.device)
                self.handle.solve(r, y, 1, m, hb.DEVICE)
                self._hip.synchronize()
                return y
            r = host_vector(r, 'r', m)
            y = np.empty(m)
            self.handle.solve(r, y, 1, m, hb.HOST)
            return y
        if on_device(r):
            cols = device_block(r, 'r', m)              # (k, m)
            out = cols.new_empty(cols.shape)
            if cols.shape[0]:
                wait_for_torch(cols.device)
                self.handle.solve(cols, out, cols.shape[0], m, hb.DEVICE)
                self._hip.synchronize()
            return out.t()
        R = host_block(r, 'r', m)
        Y = np.empty(R.shape, order='F')
        if R.shape[1]:
            self.handle.solve(R, Y, R.shape[1], m, hb.HOST)
        return Y

    # -- operator --------------------------------------------------------
    def operator(self):
        """``S^-1`` of the present factorisation as a symmetric
        ``scipy.sparse.linalg.LinearOperator`` of shape ``(M(N-1),
        M(N-1))``.  The factors live in the solver: a product after a later
        factorisation raises ``RuntimeError`` instead of answering from
        another matrix."""
        from scipy.sparse.linalg import LinearOperator
        from .marshal import tensor_operands
        solver, generation = self, self.generation

        def apply(x):
            if solver.generation != generation:
                raise RuntimeError(
                    'this operator is stale: its solver has factorised '
                    'another matrix since.')
            return solver.solve(x)

        class NormalOperator(tensor_operands('matvec', 'matmat', 'rmatvec',
                                             'rmatmat'), LinearOperator):
            def __init__(op):
                super().__init__(np.dtype(np.float64),
                                 (solver.size, solver.size))

            def _matvec(op, x):
                if on_device(x):
                    return apply(x)
                return apply(np.asarray(x).reshape(-1))

            _rmatvec = _matvec

            def _matmat(op, X):
                return apply(X)

            _rmatmat = _matmat

        op = NormalOperator()
        op.solver = solver
        return op
