"""CPU side of the flush placement sweep (``tests/flush_cases.py``,
``tests/test_flush_device_gpu.py``): the printed modules call the device
functions recorded for them, the case list covers what it claims to cover,
the prebuilt code objects are the ones ``ufuncify_matrix`` loads, and the
``(n, shift)`` grid reaches the edge branches of the flush."""
import os
import re

import pytest

import flush_cases as fc

FIVE = {'opty_flush_lines', 'opty_head_piece', 'opty_flush_flat',
        'opty_flush16', 'opty_flush8'}


def _recorded(calls):
    return {re.match(r'opty_[a-z0-9_]+', rx).group(0) for rx in calls}


@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_module_names_the_recorded_device_functions(case):
    src = fc.source(case.P, case.kw)
    for rx in case.calls:
        assert re.search(rx, src), rx
    assert fc.named(src) == _recorded(case.calls)
    if fc.LINES in case.calls:
        # ring rows as the chunk width implies, line slots within them
        chunk = case.kw.get('chunk', 32)
        found = re.findall(fc.LINES, src)
        assert {int(r) for _, r, _ in found} == {chunk + 16}
        assert {int(nlp) for nlp, _, _ in found} <= {1, 2, 4}
        assert max(int(nlp) for nlp, _, _ in found) <= chunk//16


def test_three_argument_module():
    src = fc.multi_source()
    for rx in fc.MULTI_CALLS:
        assert re.search(rx, src), rx
    assert fc.named(src) == _recorded(fc.MULTI_CALLS)


def test_case_list_covers_every_flush_shape():
    assert len(fc.CASES) + 1 <= 60
    assert len({(c.P, tuple(sorted(c.kw.items()))) for c in fc.CASES}) == \
        len(fc.CASES)
    reached, nlps = set(), set()
    for c in fc.CASES:
        src = fc.source(c.P, c.kw)
        reached |= fc.named(src)
        nlps |= {int(nlp) for nlp, _, _ in re.findall(fc.LINES, src)}
    assert reached == FIVE
    assert nlps == {1, 2, 4}
    line = fc.LINE_CASES
    assert {c.P for c in line} == {64, 65, 66, 71, 72, 77, 79, 80, 95, 96,
                                   127, 128, 129, 255, 257, 990}
    # every value of every knob with an odd and with an even width
    for knob, default, values in (('chunk', 32, (16, 32, 64)),
                                  ('groups', None, (None, 1, 2, 3, 5)),
                                  ('interleave', 0, (0, 1))):
        for value in values:
            parities = {c.P % 2 for c in line
                        if c.kw.get(knob, default) == value}
            assert parities == {0, 1}, (knob, value)
    shared = [c for c in line if c.kw.get('waves', 1) > 1]
    assert len({c.P for c in shared}) >= 2
    for c in shared:        # several waves in one workgroup
        bound = re.search(r'__launch_bounds__\((\d+)\)\nopty_jac',
                          fc.source(c.P, c.kw))
        assert int(bound.group(1)) == 64*c.kw['waves']
    # several strips: another strip than the first owns lines
    for c in line:
        if c.kw.get('groups') in (2, 3, 5):
            own = set(re.findall(
                r'opty_flush_lines<[^>]*>\(ring, jrow, \d+, b0, -?\d+, \d+, '
                r'(\d+), (\d+),', fc.source(c.P, c.kw)))
            assert len(own) >= 2, fc.case_id(c)
    assert {c.P for c in fc.FLAT_CASES} == {1, 2, 3, 15, 16, 17, 30, 31,
                                            62, 63}
    for kind, parity in ((fc.F16, 0), (fc.F8, 1)):
        small = [c for c in fc.CHUNK_CASES if kind in c.calls and c.P < 64]
        assert all(c.P % 2 == parity for c in small)
        assert {c.kw['chunk'] for c in small} == {8, 16}


@pytest.mark.parametrize('P,kw', [
    (77, {}), (30, {}), (31, dict(small_flush='chunk', chunk=8))])
def test_source_is_what_ufuncify_matrix_compiles(monkeypatch, P, kw):
    """The code object :func:`flush_cases.prebuild_jobs` builds is the one
    ``ufuncify_matrix`` asks the cache for."""
    import opty_amd
    from opty_amd import hip_backend as hb
    assert any((c.P, c.kw) == (P, kw) for c in fc.CASES)
    loaded = []

    class Stub(object):
        def __init__(self, desc, hsaco):
            loaded.append((desc, hsaco))
    monkeypatch.setattr(hb, 'HipMatrix', Stub)
    f = opty_amd.ufuncify_matrix(fc.symbols(), fc.matrix(P),
                                 emit_options=fc.options(kw))
    assert f.source == fc.source(P, kw)
    (desc, hsaco), = loaded
    assert (desc['rows'], desc['cols'], desc['num_vec']) == (1, P, 1)
    assert hsaco == hb.compile_module(fc.source(P, kw)) and \
        os.path.exists(hsaco)


def _grid(case):
    for n in fc.counts(case):
        for shift in fc.SHIFTS:
            blks = fc.blocks(case.P, n, shift)
            assert sum(nv for _, nv in blks) == n
            yield n, shift, blks


def test_grid_meets_the_edge_branches():
    """From ``(P, n, shift)`` with the arithmetic of ``opty_device.h``
    (``tests/test_flush_model.py`` holds :func:`flush_cases.straddles` and
    :func:`flush_cases.head_length` to the model of ``opty_flush_lines``):
    what the sweep of ``tests/test_flush_device_gpu.py`` reaches."""
    for c in fc.LINE_CASES:
        straddle = heads = phases = 0
        ragged = set()
        for n, shift, blks in _grid(c):
            for b0, nv in blks:
                hit = fc.straddles(c.P, b0, nv)
                straddle += hit
                if hit and nv < 64:
                    ragged.add(b0 & 1)
                heads += fc.head_length(b0) > 0
                phases |= 1 << b0
        assert heads and straddle, fc.case_id(c)
        assert bin(phases).count('1') >= len(fc.SHIFTS)
        # a ragged last block that ends at an odd phase: from an odd phase of
        # its first element, and for odd widths from an even one as well
        assert ragged == ({0, 1} if c.P % 2 else {1}), fc.case_id(c)
    for c in fc.FLAT_CASES:
        ends = set()
        for n, shift, blks in _grid(c):
            ends |= {fc.flat_ends(c.P, b0, nv) for b0, nv in blks}
        # (an even width ends at the parity it starts at)
        assert ends == ({(False, False), (False, True), (True, False),
                         (True, True)} if c.P % 2 else
                        {(False, False), (True, True)}), fc.case_id(c)
    for c in fc.CHUNK_CASES:
        # 16-byte stores at both parities of the row start, valid nodes from
        # one to a full block
        seen = {(b0 & 1, nv) for n, shift, blks in _grid(c)
                for b0, nv in blks}
        assert {(0, 1), (1, 1), (0, 64), (1, 64), (0, 37), (1, 37)} <= seen
