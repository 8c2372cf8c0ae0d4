"""Synthetic index patterns for the CSR-Hessian and Hessian-product handles
(``csrc/hesscsr.cpp``, ``csrc/hessmv.cpp``): descriptors that no problem of
the zoo produces -- row classes wider than one and two column chunks, windows
wider than 64 entries, unsorted patterns, explicit triplets in interior
trajectory rows and in tail rows, long source lists, missing diagonals --,
their INDEPENDENT expansion to triplet indices, and what a descriptor
reaches.  Plain NumPy, nothing of ``codegen/program.py``.

A handle borrows only N, n, q, r, s, device and stream of its problem, so a
descriptor over ``nrows`` trajectory rows and ``ntail`` tail entries runs on
any CARRIER problem with those sizes."""
import collections
import functools

import numpy as np

#: entries of a node that row classes share a tile for (kWindow of hesscsr.cpp)
WINDOW = 64
#: columns of a row class per output tile (kChunk of hesscsr.cpp)
CHUNK = 32
#: nodes a block advances by
STRIDE = 63


def side_key(row, off):
    """The order of the free index of a side at every node: trajectory sides
    first, by row then slot; the tail last."""
    return (1, off, 0) if row < 0 else (0, row, off)


def all_entries(nrows, ntail):
    """Every valid entry ``(ra, oa, rb, ob)``: side a not before side b."""
    sides = [(R, o) for R in range(nrows) for o in (0, 1)] + \
        [(-1, j) for j in range(ntail)]
    return [a + b for a in sides for b in sides
            if side_key(*a) >= side_key(*b)]


def _entry_key(e):
    return side_key(e[0], e[1]), side_key(e[2], e[3])


def descriptor(seed, nrows, ntail, N, density=0.5, repeat=0.0, copies=1,
               shuffle=False, obj=0, obj_base=0, pairs=0, explicit=False,
               scattered=0):
    """A descriptor for ``HipHessianCsr`` / ``HipHessianProduct`` /
    ``hessian_csr_structure``.

    ``density``: share of the valid entries in the node pattern; ``repeat``:
    share of entries that occur again (twice over, so that source lists reach
    3); ``copies``: every entry occurs 1 .. ``copies`` times; ``shuffle``: the
    pattern in random order instead of sorted by row side; ``obj`` entries of
    an objective section with ``obj_base``; ``pairs`` parameter-parameter
    triplets; ``scattered`` random instance triplets; ``explicit``: the
    deliberate instance triplets of :func:`_deliberate` and the pattern they
    need (``nrows >= 3``, ``ntail >= 2``).  The patterns do not depend on
    ``N``; the explicit triplets do."""
    rng = np.random.default_rng(seed)
    ncn, tail = N - 1, nrows*N
    ents = [e for e in all_entries(nrows, ntail) if rng.random() < density]
    if explicit:
        assert nrows >= 3 and ntail >= 2
        R = nrows - 1
        # tail row 0: segments on rows 0 and 2, none on row 1; the pair
        # (tail 1, tail 0) a long group, (tail 1, tail 1) not on the pattern
        ents = [e for e in ents if e[:3] != (-1, 0, 1) and
                e != (-1, 1, -1, 1)]
        for need in ((R, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 2, 1),
                     (-1, 1, -1, 0)):
            if need not in ents:
                ents.append(need)
    for _ in range(2):
        ents += [e for e in ents if rng.random() < repeat]
    if copies > 1:
        ents = [e for e in ents
                for _ in range(int(rng.integers(1, copies + 1)))]
    ents.sort(key=_entry_key)
    if shuffle:
        ents = [ents[k] for k in rng.permutation(len(ents))]
    oents = []
    if obj:
        # trajectory offsets count from obj_base: off + base in {0, 1}; what
        # the explicit placements need absent stays absent
        ok = [e for e in all_entries(nrows, ntail)
              if (e[0] < 0 or e[1] + obj_base <= 1) and
              (e[2] < 0 or e[3] + obj_base <= 1) and
              not (explicit and (e[:3] == (-1, 0, 1) or e == (-1, 1, -1, 1)))]
        oents = [ok[k] for k in sorted(rng.choice(len(ok), min(obj, len(ok)),
                                                  replace=False))]
    par = []
    for k in range(pairs):
        a = int(rng.integers(0, ntail))
        par.append((tail + a, tail + int(rng.integers(0, a + 1))))
    if pairs and explicit:
        par[0] = (tail + 1, tail)           # on the long group
    # (a generator of their own: the patterns above are the same at every N)
    rng = np.random.default_rng([seed, N])
    inst = _deliberate(nrows, N) if explicit else []
    for _ in range(scattered):
        r = int(rng.integers(0, tail + ntail))
        inst.append((r, int(rng.integers(0, r + 1))))
    inst = [inst[k] for k in rng.permutation(len(inst))]
    return dict(
        pattern=np.array(ents, dtype=np.int32).reshape(-1, 4),
        inst_rows=np.array([r for r, _ in inst], dtype=np.int64),
        inst_cols=np.array([c for _, c in inst], dtype=np.int64),
        obj_pattern=np.array(oents, dtype=np.int32).reshape(-1, 4),
        obj_base=obj_base,
        tail_rows=np.array([r for r, _ in par], dtype=np.int64),
        tail_cols=np.array([c for _, c in par], dtype=np.int64))


def _deliberate(nrows, N):
    """The explicit triplets placed on purpose, over the pattern that
    ``descriptor(explicit=True)`` forces; ``R`` is the last row class.
    Placements that need an interior node are dropped where N is too small."""
    ncn, tail, R = N - 1, nrows*N, nrows - 1
    out = []
    # interior rows on the pair (row 0, d = 0) that the class holds: block 0,
    # node 63 (lane 63 of block 0, repeated by lane 0 of block 1), block 1
    # (the last interior node where N is too small for node 70)
    out += [(R*N + p, p) for p in sorted({5, 63, min(70, ncn - 1)})
            if 1 <= p <= ncn - 1]
    # interior rows on a pair that no pattern holds (d = -3): a column more,
    # the later rows of the class shift; blocks 0 and 1; one of them twice and
    # one in a row that also has a triplet on the pattern
    last = min(66, ncn - 1)
    out += [(R*N + p, R*N + p - 3) for p in (5, 7, last, last)
            if 3 <= p <= ncn - 1 and (p < 63 or p == last > 63)]
    # a first row and a last row
    out += [(R*N, N), (R*N + ncn, R*N + ncn - 1)]
    # tail row 0 on elements of its segments: row 0 (time nodes 0 ..) and the
    # last element of the one on row 2 (.. N - 1)
    out += [(tail, p) for p in sorted({0, min(ncn - 1, 64)})]
    out += [(tail, 2*N + ncn)]
    # tail row 0 at a column of row 1: outside every segment, between two
    out += [(tail, N + min(ncn, 3))]
    # a tail x tail pair that is a long group, and one that is not
    out += [(tail + 1, tail), (tail + 1, tail + 1)]
    return out


def window_descriptor(width, fill=8):
    """One row class (row 0) whose two entries lie ``width`` entries apart:
    its window is exactly ``width`` entries.  What lies between them are tail
    entries (segments and long groups, a few columns with long source lists),
    which are in no window.  For a carrier with ``ntail >= 2``."""
    assert width >= 2
    mid = [(-1, 0, 0, 0), (-1, 0, 0, 1), (-1, 1, 1, 0), (-1, 1, -1, 0),
           (-1, 0, -1, 0), (-1, 1, 2, 1), (-1, 1, -1, 1), (-1, 1, 3, 0)][:fill]
    ents = [(0, 0, 0, 0)] + [mid[k % len(mid)] for k in range(width - 2)] + \
        [(0, 1, 0, 0)]
    none = np.zeros(0, dtype=np.int64)
    return dict(pattern=np.array(ents, dtype=np.int32).reshape(-1, 4),
                inst_rows=none, inst_cols=none,
                obj_pattern=np.zeros((0, 4), dtype=np.int32), obj_base=0,
                tail_rows=none, tail_cols=none)


def all_sides_descriptor(nrows):
    """A few entries on every one of the ``2*nrows`` trajectory sides: the
    diagonal pair of each side and a pair with the side before."""
    ents = []
    for R in range(nrows):
        ents += [(R, 0, R, 0), (R, 1, R, 0), (R, 1, R, 1)]
        if R:
            ents += [(R, 0, R - 1, 1), (R, 1, R - 1, 0)]
    ents.sort(key=_entry_key)
    none = np.zeros(0, dtype=np.int64)
    return dict(pattern=np.array(ents, dtype=np.int32).reshape(-1, 4),
                inst_rows=none, inst_cols=none,
                obj_pattern=np.zeros((0, 4), dtype=np.int32), obj_base=0,
                tail_rows=none, tail_cols=none)


def triplets(desc, nrows, ntail, N):
    """``(rows, cols)`` of every value in the layout ``[node i*PH + e |
    instance | objective e*(N-1) + j | parameter-parameter]``."""
    ncn, tail = N - 1, nrows*N
    i = np.arange(ncn, dtype=np.int64)[:, None]

    def side(row, off, base):
        return np.where(row >= 0, row*N + i + off + base, tail + off)
    rows, cols = [], []
    p = np.asarray(desc['pattern'], dtype=np.int64).reshape(-1, 4)
    if len(p):
        rows.append(side(p[:, 0], p[:, 1], 0).ravel())
        cols.append(side(p[:, 2], p[:, 3], 0).ravel())
    rows.append(np.asarray(desc.get('inst_rows', ()), dtype=np.int64))
    cols.append(np.asarray(desc.get('inst_cols', ()), dtype=np.int64))
    o = np.asarray(desc.get('obj_pattern', ()), dtype=np.int64).reshape(-1, 4)
    if len(o):
        b = desc.get('obj_base', 0)
        rows.append(side(o[:, 0], o[:, 1], b).T.ravel())
        cols.append(side(o[:, 2], o[:, 3], b).T.ravel())
    rows.append(np.asarray(desc.get('tail_rows', ()), dtype=np.int64))
    cols.append(np.asarray(desc.get('tail_cols', ()), dtype=np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    assert np.all(cols <= rows) and np.all(cols >= 0)
    assert np.all(rows < tail + ntail)
    return rows, cols


def with_every_diagonal(rows, cols, values, num_free):
    """The triplets plus one zero triplet per diagonal: what the structure
    ``with_diagonal`` compresses."""
    d = np.arange(num_free, dtype=np.int64)
    return (np.r_[rows, d], np.r_[cols, d], np.r_[values, np.zeros(num_free)])


def lds_bytes(width):
    """Dynamic LDS of a block of ``opty_hesscsr`` whose widest tile window
    has ``width`` entries (``create_impl`` of hesscsr.cpp)."""
    return 8*(64*(width | 1) + 64*(CHUNK + 1) + 64)


def reaches(desc, nrows, N, ntail=0):
    """What a descriptor exercises, from the descriptor alone (``ntail``
    only says which tail rows there are to miss a diagonal)."""
    ncn, tail = N - 1, nrows*N
    pat = [tuple(int(x) for x in e) for e in
           np.asarray(desc['pattern']).reshape(-1, 4)]
    obj = [tuple(int(x) for x in e) for e in
           np.asarray(desc.get('obj_pattern', ())).reshape(-1, 4)]
    base, PH = desc.get('obj_base', 0), len(pat)
    traj = collections.defaultdict(lambda: collections.defaultdict(int))
    segs = collections.defaultdict(lambda: collections.defaultdict(list))
    longs = collections.defaultdict(lambda: collections.defaultdict(int))
    lo, hi = {}, {}
    for e, (ra, oa, rb, ob) in enumerate(pat + obj):
        b = 0 if e < PH else base
        oa, ob = oa + (b if ra >= 0 else 0), ob + (b if rb >= 0 else 0)
        if ra >= 0:
            traj[ra][(rb, ob - oa)] += 1
            if e < PH:
                lo[ra], hi[ra] = min(lo.get(ra, e), e), max(hi.get(ra, e), e)
        elif rb >= 0:
            segs[oa][rb].append(ob)
        else:
            longs[oa][ob] += 1
    L = {R: len(c) for R, c in traj.items()}
    widest = max([hi[R] - lo[R] + 1 for R in lo] + [0])
    # classes share a tile while their windows together stay within WINDOW
    # entries (or the widest class's)
    room, groups, tile, cur = max(widest, WINDOW), 0, 0, None
    for R in sorted(lo):
        if cur and max(cur[1], hi[R]) - min(cur[0], lo[R]) + 1 <= room:
            cur = (min(cur[0], lo[R]), max(cur[1], hi[R]))
        else:
            groups, cur = groups + 1, (lo[R], hi[R])
        tile = max(tile, cur[1] - cur[0] + 1)
    sources = max([k for c in traj.values() for k in c.values()] +
                  [len(v) for s in segs.values() for v in s.values()] +
                  [k for c in longs.values() for k in c.values()] + [0])

    # explicit triplets
    ex = collections.defaultdict(set)
    for key in ('inst', 'tail'):
        for r, c in zip(desc.get(key + '_rows', ()),
                        desc.get(key + '_cols', ())):
            ex[int(r)].add(int(c))
    # class -> (node, columns added)
    interior = collections.defaultdict(list)
    seg_nodes = between = long_explicit = 0
    tail_diag = set(j for j, c in longs.items() if j in c)
    for r, colset in ex.items():
        if r < tail:
            R, p = divmod(r, N)
            if 1 <= p <= ncn - 1:
                regular = set(Rp*N + p + d for Rp, d in traj[R])
                interior[R].append((p, len(colset - regular)))
            continue
        j = r - tail
        spans = []
        for Rp, offs in segs[j].items():
            spans.append((Rp*N + (0 if 0 in offs else 1),
                          Rp*N + (ncn if 1 in offs else ncn - 1)))
        for c in colset:
            if c >= tail:
                long_explicit += (c - tail) in longs[j]
                if c == r:
                    tail_diag.add(j)
            elif any(a <= c <= b for a, b in spans):
                seg_nodes += 1
            elif any(b < c for a, b in spans) and \
                    any(c < a for a, b in spans):
                between += 1
    return dict(
        PH=PH, L=max(list(L.values()) + [0]),
        chunks=-(-max(list(L.values()) + [0])//CHUNK),
        widest_window=widest, tile_window=tile, tile_groups=groups,
        lds_bytes=lds_bytes(tile), longest_source_list=sources,
        interior_item_rows=dict(interior),
        segment_nodes_of_items=seg_nodes, extras_between_segments=between,
        long_groups=sum(len(c) for c in longs.values()),
        long_groups_with_explicit=long_explicit,
        classes_without_diagonal=sorted(
            R for R in range(nrows) if (R, 0) not in traj[R]),
        tail_rows_without_diagonal=sorted(set(range(ntail)) - tail_diag))


# -- carriers -----------------------------------------------------------------
#: name -> (trajectory rows, tail entries)
CARRIERS = {'c43': (4, 3), 'p132': (13, 2), 'p230': (23, 0), 'p510': (51, 0),
            'p720': (72, 0)}


def chain_problem(states, parameters, num_nodes, inputs=0):
    """A carrier of any size that is derived and built in no time: a chain
    of ``states`` first-order equations with ``parameters`` unknown
    parameters and ``inputs`` unknown input trajectories.  Only its sizes
    matter."""
    import sympy as sm
    t = sm.Symbol('t')
    x = [sm.Function('x%d' % k)(t) for k in range(states)]
    u = [sm.Function('u%d' % k)(t) for k in range(inputs)]
    p = sm.symbols('p0:%d' % parameters) if parameters else ()
    eom = sm.Matrix([x[k].diff() + (p[k] if k < parameters else 1)*x[k]
                     - sm.sin(x[k - 1]) - sum(u[k::states])
                     for k in range(states)])
    return dict(equations_of_motion=eom, state_symbols=tuple(x),
                num_collocation_nodes=num_nodes, node_time_interval=0.05,
                time_symbol=t, integration_method='backward euler')


#: states of the 72-row carrier; the other rows are unknown input trajectories
#: (a node block of 72 states would be 72 x 145 entries)
WIDE_STATES = 8


def carrier_keywords(name, N):
    import hessmv_cases as mc
    if name == 'c43':
        return mc.carrier_problem(N)
    rows, tail = CARRIERS[name]
    if name == REFUSED_SIDES_CARRIER:
        return chain_problem(WIDE_STATES, tail, N, inputs=rows - WIDE_STATES)
    return chain_problem(rows, tail, N)


@functools.lru_cache(maxsize=None)
def carrier(name, N, layout=None):
    """The collocator that lends its handle (sizes checked)."""
    import opty_amd
    kw = {} if layout is None else dict(jacobian_layout=layout)
    col = opty_amd.ConstraintCollocator(**kw, **carrier_keywords(name, N))
    prog = col._build_program()
    assert (prog.n + prog.q, prog.r + prog.s) == CARRIERS[name], name
    return col


#: N - 1 of the problem with interior instance constraints and the nodes they
#: sit on: two in block 0, one in block 1 (blocks advance by 63 nodes)
INTERIOR_EDGE, INTERIOR_NODES = 65, (5, 64, 40)


def interior_instance_problem(num_nodes=INTERIOR_EDGE + 1):
    """A nonlinear oscillator -- two states, two unknown input trajectories,
    three unknown parameters; its trajectory row classes have columns -- with
    two NONLINEAR instance constraints at interior node times: ``x(t_a) v(t_b)
    - c0`` (a triplet off the pattern, in a row of block 1) and ``x(t_c)**2 +
    v(t_c)**2 - c1`` (diagonal triplets in rows of block 0)."""
    import sympy as sm
    m, c, k, t = sm.symbols('m, c, k, t')
    x, v, f1, f2 = [s(t) for s in sm.symbols('x, v, f1, f2',
                                             cls=sm.Function)]
    h = 0.3
    a, b, cc_ = INTERIOR_NODES
    eom = sm.Matrix([x.diff() - v,
                     m*v.diff() + c*v*x + k*sm.sin(x) - f1*f2])
    inst = (x.func(a*h)*v.func(b*h) - 0.3,
            x.func(cc_*h)**2 + v.func(cc_*h)**2 - 1.0)
    return dict(equations_of_motion=eom, state_symbols=(x, v),
                num_collocation_nodes=num_nodes, node_time_interval=h,
                instance_constraints=inst, time_symbol=t,
                integration_method='midpoint')


@functools.lru_cache(maxsize=None)
def interior_collocator():
    """... in the CSR layout, which the augmented system needs."""
    import opty_amd
    return opty_amd.ConstraintCollocator(jacobian_layout='csr',
                                         **interior_instance_problem())


# -- cases --------------------------------------------------------------------
#: name -> (carrier, N - 1 of the GPU file, keywords of descriptor(), tags)
CASES = collections.OrderedDict([
    # row classes of 33 .. 64 columns: two column chunks
    ('chunks2', ('p132', (1, 2, 63, 64, 65),
                 dict(seed=5, density=0.9), ('two_chunks',))),
    # ... of more than 64: three chunks, and the first windows above 64
    ('chunks3', ('p230', (64, 65),
                 dict(seed=5, density=0.95), ('three_chunks', 'wide_window'))),
    # not sorted by row side: every window spans most of the node's entries
    ('shuffled', ('p132', (2, 65, 127),
                  dict(seed=6, density=0.3, repeat=0.2, shuffle=True),
                  ('wide_window', 'tile_groups', 'sources'))),
    # a few classes, every entry several times: one class above 64 entries
    ('wide_class', ('c43', (2, 65),
                    dict(seed=7, density=1.0, copies=12),
                    ('wide_window', 'sources'))),
    # the deliberate explicit triplets, both sections, parameter pairs
    ('explicit_c43_base0', ('c43', (1, 2, 64, 65, 127),
                            dict(seed=8, density=0.6, repeat=0.2, obj=6,
                                 obj_base=0, pairs=4, explicit=True,
                                 scattered=8), ('explicit', 'sources'))),
    ('explicit_c43_base1', ('c43', (1, 2, 64, 65, 127),
                            dict(seed=9, density=0.6, repeat=0.2, obj=6,
                                 obj_base=1, pairs=4, explicit=True,
                                 scattered=8), ('explicit', 'sources'))),
    ('explicit_p132_base0', ('p132', (1, 2, 64, 65, 127),
                             dict(seed=10, density=0.5, repeat=0.2, obj=9,
                                  obj_base=0, pairs=3, explicit=True,
                                  scattered=12), ('explicit', 'sources'))),
    ('explicit_p132_base1', ('p132', (1, 2, 64, 65, 127),
                             dict(seed=11, density=0.5, repeat=0.2, obj=9,
                                  obj_base=1, pairs=3, explicit=True,
                                  scattered=12), ('explicit', 'sources'))),
    # few entries: row classes and tail rows without a diagonal triplet
    ('sparse', ('p132', (2, 65), dict(seed=12, density=0.08),
                ('diagonal',))),
])

#: the cases of the items of the issue
CHUNK_CASES = ('chunks2', 'chunks3')
WINDOW_CASES = ('shuffled', 'wide_class')
EXPLICIT_CASES = tuple(k for k in CASES if k.startswith('explicit'))
DIAGONAL_CASES = CHUNK_CASES + EXPLICIT_CASES + ('sparse',)
PRODUCT_CASES = CHUNK_CASES + EXPLICIT_CASES
#: N - 1 from which the deliberate interior placements are all there
FULL_EXPLICIT = 64

#: the carrier of the LDS limit and its N - 1
LDS_CARRIER, LDS_EDGE = 'c43', 65
#: a class window the device must refuse (about 4000 entries)
LDS_REFUSED = 4000
#: the pattern that touches all 102 sides of the 51-row carrier, its N - 1
SIDES_CARRIER, SIDES_EDGE = 'p510', 65
#: a carrier with more sides than the LDS of a block holds (144), its N - 1
REFUSED_SIDES_CARRIER, REFUSED_SIDES_EDGE = 'p720', 65
#: the carrier in the CSR layout (the augmented system) and its case
KKT_CASE, KKT_EDGE = 'explicit_c43_base0', 65


def params(names):
    """``(case, N - 1)`` of the named cases, for ``parametrize``."""
    return [(name, m) for name in names for m in CASES[name][1]]


@functools.lru_cache(maxsize=None)
def case(name, ncn):
    """``(carrier name, N, nrows, ntail, descriptor, rows, cols)``."""
    cname, _, kw, _ = CASES[name]
    nrows, ntail = CARRIERS[cname]
    N = ncn + 1
    desc = descriptor(nrows=nrows, ntail=ntail, N=N, **kw)
    rows, cols = triplets(desc, nrows, ntail, N)
    return cname, N, nrows, ntail, desc, rows, cols


def check_reaches(name, ncn):
    """The conditions a case is there for -- not measurements: a case that
    does not reach its path fails here.  Returns what it reaches."""
    cname, N, nrows, ntail, desc, _, _ = case(name, ncn)
    tags = CASES[name][3]
    got = reaches(desc, nrows, N, ntail)
    if 'two_chunks' in tags:
        assert CHUNK < got['L'] <= 2*CHUNK and got['chunks'] == 2, got
    if 'three_chunks' in tags:
        assert got['L'] > 2*CHUNK and got['chunks'] == 3, got
    if 'wide_window' in tags:
        assert got['widest_window'] > WINDOW, got
        assert got['lds_bytes'] > 8*(64*65 + 64*33 + 64), got   # pitch > 65
    if 'tile_groups' in tags:
        assert got['tile_groups'] >= 2, got
    if 'sources' in tags:
        assert got['longest_source_list'] >= 3, got
    if 'explicit' in tags:
        assert got['long_groups_with_explicit'] >= 1, got
        assert got['segment_nodes_of_items'] >= 1, got
        assert got['extras_between_segments'] >= 1, got
        if ncn >= FULL_EXPLICIT:
            best = max(got['interior_item_rows'].values(), key=len)
            assert len(best) >= 2, got
            assert any(x > 0 for _, x in best), got
        if ncn > FULL_EXPLICIT:
            # (at N - 1 = 64 the interior nodes 1 .. 63 are all in block 0)
            assert len(set((p - 1)//STRIDE for p, _ in best)) >= 2, got
            assert any(x > 0 and p > STRIDE for p, x in best), got
    if 'diagonal' in tags:
        assert got['classes_without_diagonal'], got
        assert got['tail_rows_without_diagonal'], got
    return got


def prebuild_jobs():
    """Thunks that build the code objects of tests/test_hessian_synth_gpu.py
    (``__graft_entry__.build`` runs them side by side): the carriers' base
    modules at every node count in use -- small launches are built
    differently per node count --, the carrier in the CSR layout and the
    Hessian module of the problem with interior instance constraints."""
    todo = set((CASES[name][0], m + 1, None) for name in CASES
               for m in CASES[name][1])
    todo |= {(LDS_CARRIER, LDS_EDGE + 1, None),
             (SIDES_CARRIER, SIDES_EDGE + 1, None),
             (REFUSED_SIDES_CARRIER, REFUSED_SIDES_EDGE + 1, None),
             (CASES[KKT_CASE][0], KKT_EDGE + 1, 'csr')}
    by_carrier = collections.defaultdict(list)
    for cname, N, layout in sorted(todo, key=str):
        by_carrier[cname].append((N, layout))

    def build(cname):
        for N, layout in by_carrier[cname]:
            carrier(cname, N, layout).prebuild()
    def interior():
        col = interior_collocator()
        col.prebuild()
        col._build_hessian_code_object()
    return [lambda c=c: build(c) for c in sorted(by_carrier)] + [interior]
