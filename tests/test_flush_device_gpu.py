"""Exact placement of the device flush (``opty_flush_lines``,
``opty_head_piece``, ``opty_flush_flat``, ``opty_flush16``, ``opty_flush8`` of
``opty_amd/csrc/opty_device.h``) on the GPU.

Entry ``k`` of row ``i`` of the matrices of ``flush_cases`` is the integer
``i*S + k``: exact in float64, so the device result is compared with NumPy's
by ``assert_array_equal`` -- a value that lands one node or one entry off
differs by at least 1.  The result is a view into a NaN-filled buffer with
NaN guard bands: a store that is missing leaves a NaN in the result, a stray
one takes a NaN out of a band."""
import numpy as np
import pytest

import flush_cases as fc

pytestmark = pytest.mark.gpu


def _where(P, shift, flat):
    """Node, entry and line phase of the flat result position ``flat``."""
    node, entry = divmod(int(flat), P)
    return 'node %d (lane %d of block %d) entry %d, line phase %d' % (
        node, node % 64, node//64, entry, (shift + flat) & 15)


def _check(buf, n, P, shift, want, what):
    """``buf`` (host copy of the whole buffer): the result is ``want``
    exactly, everything around it is still NaN."""
    lo, hi = fc.GUARD + shift, fc.GUARD + shift + n*P
    got = buf[lo:hi]
    bad = np.flatnonzero(got != want.ravel())
    msg = '' if not len(bad) else '%s: %d wrong, first at %s: got %r' % (
        what, len(bad), _where(P, shift, bad[0]), got[bad[0]])
    np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=msg)
    for name, band, at in (('front', buf[:lo], 0), ('back', buf[hi:], hi)):
        hit = np.flatnonzero(~np.isnan(band))
        assert not len(hit), '%s: %s guard band written at %d (%r)' % (
            what, name, at + hit[0] - lo, band[hit[0]])


class _Sweep(object):
    """One NaN-prefilled device buffer; every call evaluates into the view
    ``buf[GUARD + shift : GUARD + shift + n*width]`` of it with argument
    values ``arange(n) + offset``, the offset different in every call."""

    def __init__(self, width, nmax):
        import torch
        self.torch = torch
        self.dev = torch.device('cuda:0')
        self.width = width
        self.buf = torch.empty(2*fc.GUARD + 16 + nmax*width,
                               dtype=torch.float64, device=self.dev)
        # the line phases of the grid are counted from a 128-byte line
        assert self.buf.data_ptr() % 128 == 0
        self.offset = 0

    def values(self, n, count=1):
        """``count`` argument vectors whose values no earlier call had at
        the same node."""
        self.offset += 7
        return [np.arange(n, dtype=float) + self.offset + 1000*k
                for k in range(count)]

    def call(self, f, n, shift, vals):
        torch = self.torch
        self.buf.fill_(float('nan'))
        lo = fc.GUARD + shift
        res = self.buf[lo:lo + n*self.width].view(n, self.width)
        assert res.is_contiguous() and res.data_ptr() == \
            self.buf.data_ptr() + 8*lo
        f(res, *[torch.from_numpy(v).to(self.dev) for v in vals])
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()


@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_flush_places_every_entry(case):
    import opty_amd
    P = case.P
    f = opty_amd.ufuncify_matrix(fc.symbols(), fc.matrix(P),
                                 emit_options=fc.options(case.kw))
    assert f.source == fc.source(P, case.kw)
    sweep = _Sweep(P, max(fc.counts(case)))
    try:
        for n in fc.counts(case):
            for shift in fc.SHIFTS:
                vals = sweep.values(n)
                got = sweep.call(f, n, shift, vals)
                _check(got, n, P, shift, fc.expected(vals[0], P),
                       '%s n=%d shift=%d' % (fc.case_id(case), n, shift))
    finally:
        f.hip.set_stream(None)
        f.hip.close()


#: one case per flush kind through the host path (NumPy result: the copy
#: back from the handle's own result buffer)
HOST_CASES = [c for c in fc.CASES if (c.P, c.kw) in (
    (77, {}), (31, {}), (30, dict(small_flush='chunk', chunk=8)),
    (31, dict(small_flush='chunk', chunk=8)))]


@pytest.mark.parametrize('case', HOST_CASES, ids=fc.case_id)
def test_flush_host_path(case):
    import opty_amd
    assert len(HOST_CASES) == 4
    P = case.P
    f = opty_amd.ufuncify_matrix(fc.symbols(), fc.matrix(P),
                                 emit_options=fc.options(case.kw))
    try:
        for k, n in enumerate((129, 37, 65)):       # grows, shrinks, grows
            vals = np.arange(n, dtype=float) + 11*(k + 1)
            res = np.full((n, P), np.nan)
            out = f(res, vals)
            assert out.shape == (n, 1, P)
            np.testing.assert_array_equal(res, fc.expected(vals, P))
    finally:
        f.hip.close()


def test_flush_three_arguments_row_major():
    """3 x 30 (P = 90): row r holds argument r's values -- a row / column
    mix-up in the row-major block shows as another argument's value."""
    import opty_amd
    rows, cols = fc.MULTI_SHAPE
    P = rows*cols
    f = opty_amd.ufuncify_matrix(fc.symbols(rows), fc.multi_matrix())
    assert f.source == fc.multi_source()
    sweep = _Sweep(P, max(fc.COUNTS))

    def want(vals):
        return np.concatenate([fc.expected(v, cols) for v in vals], axis=1)
    try:
        for n in fc.COUNTS:
            for shift in fc.SHIFTS:
                vals = sweep.values(n, rows)
                got = sweep.call(f, n, shift, vals)
                _check(got, n, P, shift, want(vals),
                       '3x30 n=%d shift=%d' % (n, shift))
        f.hip.set_stream(None)
        vals = sweep.values(101, rows)
        res = np.full((101, P), np.nan)
        out = f(res, *vals)
        np.testing.assert_array_equal(res, want(vals))
        np.testing.assert_array_equal(out[:, 1, :], fc.expected(vals[1],
                                                                cols))
    finally:
        f.hip.close()
