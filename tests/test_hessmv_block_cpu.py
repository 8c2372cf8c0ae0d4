"""CPU tests of the block products of the Hessian operator (``Y = H V`` over
several columns, ``opty_hip_hessmv_apply_block``): the header, the bindings
and the ABI version agree, the pass width follows the documented LDS rule and
the column-major conversion of the Python surface is exact: no GPU is
needed."""
import ctypes
import os
import re

import numpy as np

from opty_amd import hip_backend as hb
from opty_amd.codegen.program import hessian_block_width
from opty_amd.direct_collocation import column_major

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: C argument type of the header -> ctypes type of the binding table
CTYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64,
          'int': ctypes.c_int}


def _header():
    with open(os.path.join(REPO, 'include', 'opty_hip.h')) as f:
        return f.read()


def _declaration(name):
    """``(result type, [argument types])`` of ``name`` in the header, a
    pointer of any kind as ``'*'``."""
    m = re.search(r'^(\w+)\s+%s\(([^)]*)\);' % name, _header(), re.M)
    assert m, name
    args = []
    for arg in m.group(2).split(','):
        words = arg.replace('const', ' ').split()
        args.append('*' if '*' in arg else words[0])
    return m.group(1), args


def test_header_declares_the_block_product():
    res, args = _declaration('opty_hip_hessmv_apply_block')
    assert res == 'int'
    assert args == ['*', '*', '*', 'int64_t', '*', 'int64_t', 'int32_t',
                    'int32_t']
    assert _declaration('opty_hip_hessmv_block_width') == ('int32_t', ['*'])


def test_abi_version_is_12_in_the_header_and_the_bindings():
    m = re.search(r'^#define OPTY_HIP_ABI_VERSION (\d+)$', _header(), re.M)
    assert hb.ABI_VERSION == 12 == int(m.group(1))


def test_binding_table_has_the_header_types():
    for name in ('opty_hip_hessmv_apply_block',
                 'opty_hip_hessmv_block_width'):
        res, args = _declaration(name)
        want = [hb._P if a == '*' else CTYPES[a] for a in args]
        assert hb._SIGNATURES[name] == (CTYPES[res], want), name
    assert hasattr(hb.HipHessianProduct, 'apply_block')
    assert isinstance(hb.HipHessianProduct.block_width, property)


def test_pass_width_rule():
    """The largest K of 4, 3, 2 with ``16 896 + 1 024 K sides`` bytes within
    the limit, else 1."""
    kib160, kib64 = 160*1024, 64*1024
    # config 3: 32 sides, 16 896 + 131 072 = 147 968 bytes for four columns
    assert hessian_block_width(32, kib160) == 4
    # four columns stop fitting between 35 and 36 sides (160 256 / 164 352)
    assert hessian_block_width(35, kib160) == 4
    assert hessian_block_width(36, kib160) == 3
    # the planar biped's 48 sides: three columns need 164 352 bytes, 512 more
    # than there are; two need 115 200
    assert hessian_block_width(47, kib160) == 3
    assert hessian_block_width(48, kib160) == 2
    assert hessian_block_width(71, kib160) == 2
    # not even two columns: 16 896 + 2 048*72 = 164 352
    assert hessian_block_width(72, kib160) == 1
    assert hessian_block_width(104, kib160) == 1
    # a device that gives a block 64 KiB
    assert hessian_block_width(11, kib64) == 4
    assert hessian_block_width(12, kib64) == 3
    assert hessian_block_width(23, kib64) == 2
    assert hessian_block_width(24, kib64) == 1
    assert hessian_block_width(32, kib64) == 1
    # the rule itself, over every count a device could hold
    for limit in (kib64, kib160):
        for sides in range(0, 144):
            fits = [k for k in (4, 3, 2)
                    if 64*33*8 + sides*k*2*64*8 <= limit]
            assert hessian_block_width(sides, limit) == (fits[0] if fits
                                                         else 1)


def test_column_major_conversion_is_exact():
    rng = np.random.default_rng(60)
    V = rng.uniform(-1.0, 1.0, (37, 5))
    for given in (np.ascontiguousarray(V), np.asfortranarray(V),
                  V[:, ::2], V.astype(np.float32), (100*V).astype(np.int64)):
        out = column_major(given)
        assert out.dtype == np.float64 and out.shape == given.shape
        assert out.flags.f_contiguous
        # plain NumPy: column c is the nfree doubles at c*nfree
        flat = out.ravel(order='K')
        for c in range(given.shape[1]):
            want = np.array([float(x) for x in given[:, c]])
            assert np.array_equal(flat[c*37:(c + 1)*37].view(np.int64),
                                  want.view(np.int64))
    # a column-major float64 block is taken as it is
    F = np.asfortranarray(V)
    assert column_major(F) is F
    assert column_major(np.zeros((37, 0))).shape == (37, 0)
