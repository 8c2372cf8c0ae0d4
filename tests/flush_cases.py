"""What the flush placement tests share (``tests/test_flush_device_gpu.py``,
``tests/test_flush_cases_cpu.py``, ``tests/test_flush_model.py``): matrix
programs whose entry ``k`` of row ``i`` is the integer ``i*S + k`` -- exact in
float64 whatever the compiler contracts -- over the block widths and printer
options that reach every shape of the five flush functions of
``opty_amd/csrc/opty_device.h``, the device functions each module has to name,
the ``(n, shift)`` grid the GPU tests sweep, which edge branch a grid point
meets, and the code objects ``__graft_entry__.build`` prebuilds."""
import collections
import re

import numpy as np

#: entry k of argument value a is a*S + k; a power of two >= every width
S = 1024

LINES = r'opty_flush_lines<(\d+), (\d+), (\d+)>\('
HEAD = r'opty_head_piece<\d+>\('
FLAT = r'opty_flush_flat<%d>\('
F16 = r'opty_flush16<\d+>\('
F8 = r'opty_flush8<\d+>\('
#: any call of one of the five flush functions in a printed module
ANY_FLUSH = re.compile(r'\b(opty_flush_lines|opty_head_piece|opty_flush_flat|'
                       r'opty_flush16|opty_flush8)<')

#: P: block width; kw: EmitOptions keywords; calls: regexes over the printed
#: module, one per device function it must name (and it names no other)
Case = collections.namedtuple('Case', 'P kw calls')


def _line(P, **kw):
    return Case(P, kw, (LINES, HEAD))


def _flat(P):
    return Case(P, {}, (FLAT % P,))


def _chunked(P, chunk, **kw):
    return Case(P, dict(kw, small_flush='chunk', chunk=chunk),
                (F16 if P % 2 == 0 else F8,))


#: line mode (P >= 64): every width of the list with the default options or
#: one knob, every value of chunk (NLP 1, 2, 4; R = chunk + 16), groups
#: (one strip, several strips, more than the block has lines), interleave and
#: waves with an odd and with an even width
LINE_CASES = [
    _line(64), _line(64, chunk=16, groups=2),
    _line(65, chunk=16, groups=1), _line(65, chunk=64, groups=5),
    _line(66, chunk=64, groups=3), _line(66, chunk=16, interleave=1),
    _line(71, chunk=64), _line(71, groups=2),
    _line(72, groups=1), _line(72, chunk=64, groups=2),
    _line(77), _line(77, chunk=16, groups=3),
    _line(79, groups=2), _line(79, chunk=64, groups=1),
    _line(80, groups=2), _line(80, chunk=16, groups=5),
    _line(95, groups=3), _line(95, chunk=64, groups=2, waves=2),
    _line(96, chunk=16, groups=3), _line(96, groups=5),
    _line(127, chunk=64, groups=1, interleave=1), _line(127, groups=5),
    _line(128, chunk=64, groups=5), _line(128, groups=2, interleave=1),
    _line(129, chunk=16, groups=5), _line(129, groups=3, interleave=1),
    _line(255, chunk=16, groups=3, interleave=1),
    _line(255, groups=4, waves=4),
    _line(257, chunk=64, groups=2, interleave=1), _line(257, groups=5),
    _line(990), _line(990, chunk=64, groups=8, waves=2),
]
#: P < 64, the whole block as one span
FLAT_CASES = [_flat(P) for P in (1, 2, 3, 15, 16, 17, 30, 31, 62, 63)]
#: P < 64 in K-entry pieces per node: 16-byte stores where P is even, 8-byte
#: ones where it is odd; several strips; and a wide block whose chunk is no
#: multiple of a line (which keeps it out of the line mode)
CHUNK_CASES = [
    _chunked(2, 8), _chunked(6, 8), _chunked(30, 8), _chunked(30, 16),
    _chunked(62, 8, groups=2), _chunked(62, 16),
    _chunked(3, 8), _chunked(31, 8), _chunked(31, 16, groups=2),
    _chunked(63, 8), _chunked(63, 16),
    _chunked(66, 8), _chunked(77, 8),
]
CASES = LINE_CASES + FLAT_CASES + CHUNK_CASES
#: the 3 x 30 matrix of three arguments (row r: argument r, P = 90)
MULTI_SHAPE = (3, 30)
MULTI_CALLS = (LINES, HEAD)

#: rows per call: one node, two, a block less one, one block, one node into the
#: second block, a ragged second block, one node into the third
COUNTS = (1, 2, 63, 64, 65, 101, 129)
#: ... of the widest case (129 x 990 values at the most)
COUNTS_WIDE = (1, 63, 65, 129)
#: doubles the result is shifted from a 128-byte line: even and odd phases of
#: the first block (the later blocks' follow from 64*P mod 16)
SHIFTS = (0, 1, 2, 7, 8, 15)
#: NaN doubles on each side of the result (whole lines)
GUARD = 64


def case_id(case):
    return 'P%d' % case.P + ''.join(
        '-%s%s' % (k, v) for k, v in sorted(case.kw.items()))


def counts(case):
    return COUNTS_WIDE if case.P > 512 else COUNTS


def symbols(count=1):
    import sympy as sm
    return sm.symbols('a, b, c')[:count]


def matrix(P):
    """The 1 x P matrix ``[a*S + k]`` of one vector argument ``a``."""
    import sympy as sm
    a, = symbols()
    assert P <= S
    return sm.Matrix([[a*S + k for k in range(P)]])


def multi_matrix():
    """3 x 30: row r is ``[arg_r*S + k]``."""
    import sympy as sm
    rows, cols = MULTI_SHAPE
    return sm.Matrix([[arg*S + k for k in range(cols)]
                      for arg in symbols(rows)])


def expected(values, P):
    """``(n, P)``: what :func:`matrix` evaluates to at the argument values
    ``values`` (integers as floats: every product and sum is exact)."""
    return np.asarray(values)[:, None]*float(S) + np.arange(P, dtype=float)


def options(kw):
    from opty_amd.codegen.emit_hip import EmitOptions
    return EmitOptions(**kw)


def _program(args, mat):
    from opty_amd.codegen import ir
    from opty_amd.codegen.lower import Lowerer
    from opty_amd.utils import _matrix_program
    dag = ir.DAG()
    low = Lowerer(dag, {a: dag.input('cur', k) for k, a in enumerate(args)})
    outputs = [low.lower(e) for e in mat]           # row-major
    return _matrix_program(dag, outputs, len(args), 0, mat.shape)


def program(P):
    """The matrix program of :func:`matrix`."""
    return _program(symbols(), matrix(P))


def _source(args, mat, kw):
    from opty_amd.codegen.emit_hip import emit_matrix_module
    return emit_matrix_module(_program(args, mat), options(kw))[0]


_SOURCES = {}


def source(P, kw):
    """The module text ``opty_amd.ufuncify_matrix((a,), matrix(P),
    emit_options=EmitOptions(**kw))`` compiles, by the same steps."""
    key = (P, tuple(sorted(kw.items())))
    if key not in _SOURCES:
        _SOURCES[key] = _source(symbols(), matrix(P), kw)
    return _SOURCES[key]


def multi_source():
    return _source(symbols(MULTI_SHAPE[0]), multi_matrix(), {})


def named(text):
    """The flush functions a printed module calls."""
    return set(ANY_FLUSH.findall(text))


# --- which edge branch a grid point meets (the arithmetic of opty_device.h) --

def blocks(P, n, shift):
    """``(b0, nvalid)`` of every 64-node block of a call with ``n`` rows whose
    result starts ``shift`` doubles behind a 128-byte line: the line phase of
    the block's first element and its valid nodes."""
    return [((shift + 64*blk*P) & 15, min(64, n - 64*blk))
            for blk in range((n + 63)//64)]


def straddles(P, b0, nvalid):
    """``opty_flush_lines``: the 16-byte piece that holds the block's last
    element starts at an even phase; where the block ends at an odd one that
    piece is the last element alone (``ok && !full && c0 < nvalid``)."""
    return (b0 + nvalid*P) & 1 == 1


def head_length(b0):
    """``opty_head_piece``: its ``s``, the elements of the block's first node
    that share their line with the block before."""
    return (-b0) & 15


def flat_ends(P, b0, nvalid):
    """``opty_flush_flat``: ``(odd a, odd total + a)`` -- whether the half
    piece at the front and the one at the back of the span are stored."""
    return b0 & 1 == 1, (nvalid*P + b0) & 1 == 1


def prebuild_jobs():
    """Thunks that compile the code objects of
    tests/test_flush_device_gpu.py into the default cache
    (``__graft_entry__.build`` runs them side by side; the modules are
    printed here, in the caller's thread)."""
    from opty_amd import hip_backend as hb
    sources = [source(c.P, c.kw) for c in CASES] + [multi_source()]
    return [lambda text=text: hb.compile_module(text) for text in sources]
