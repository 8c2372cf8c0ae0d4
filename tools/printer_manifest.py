#!/usr/bin/env python
"""One line per case of a fixed corpus of printed modules: what a refactor of
the printer (opty_amd/codegen/emit_hip.py) must leave byte for byte as it was.
Run it on the parent commit and on the change (``-j PROCESSES``) and compare
the outputs; keep no manifest in the repository.  Corpus: every ``*_small``
problem of ``examples.problems.CONFIGS`` x node_blocks (None, 1, 196, 1563) x
the option sets below, and every entry of opty_amd/launch_plans.json on the
small sibling of the problem it names, at the entry's own launch size.  A line:
``problem | opts.key() | node_blocks | module sha | run module sha or - |
kernel=sha ... | sha of the whole meta``, or ``ERR:<exception type>``."""
import argparse
import hashlib
import json
import multiprocessing
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)
sys.path.insert(0, REPO)
from examples import problems                                   # noqa: E402
from opty_amd import ConstraintCollocator                       # noqa: E402
from opty_amd.codegen.emit_hip import EmitOptions, emit_module  # noqa: E402

BLOCKS = (None, 1, 196, 1563)
OPTION_SETS = (
    {}, dict(order='list'), dict(order='tail', cut='work'),
    dict(var_order='run', restricted=1),
    dict(trace=1, var_order='run', restricted=1), dict(trace=1),
    dict(park=8, chunk=16), dict(publish=1),
    dict(fast_trig=2, deterministic=1), dict(chunk=16, waves=4, groups=8),
    dict(dear_first=1), dict(ablate='only_cheap'), dict(ablate='store_only'),
    dict(fold_instance=1), dict(fold_instance=0), dict(forget=1),
    dict(small_flush='chunk'))
_PROGRAMS = {}          # per worker process


def corpus():
    cases = [(name, kw, nb) for name in problems.CONFIGS
             if name.endswith('_small') for kw in OPTION_SETS for nb in BLOCKS]
    with open(os.path.join(REPO, 'opty_amd', 'launch_plans.json')) as f:
        plans = json.load(f)
    for key in sorted(plans):
        big = plans[key]['problem'].split(',')[0]
        name = [c for c in (big, big + '_small',
                            big.replace('config5_', '') + '_small')
                if c.endswith('_small') and c in problems.CONFIGS]
        if not name:
            sys.stderr.write('skipped plan %s: %s\n' % (key, big))
            continue
        cases.append((name[0], plans[key]['options'],
                      -(-int(plans[key]['nodes'])//64)))
    return sorted(cases, key=lambda c: c[0])


def line(case):
    name, kw, node_blocks = case
    if name not in _PROGRAMS:
        _PROGRAMS[name] = ConstraintCollocator(
            **problems.build(name))._build_program()
    opts = EmitOptions(**kw)
    head = '%s | %s | %s | ' % (name, opts.key(), node_blocks)
    try:
        _, meta = emit_module(_PROGRAMS[name], opts, node_blocks=node_blocks)
    except Exception as exc:
        return head + 'ERR:%s' % type(exc).__name__
    kernels = ' '.join('%s=%s' % (k, meta['kernels'][k].get('sha', '-')[:16])
                       for k in sorted(meta['kernels']))
    whole = hashlib.sha256(json.dumps(meta, sort_keys=True,
                                      default=str).encode()).hexdigest()
    return head + ' | '.join((meta['sha'], meta.get('run', {}).get('sha', '-'),
                              kernels, whole))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('.  ')[0])
    ap.add_argument('-j', type=int, default=1, help='worker processes')
    args = ap.parse_args()
    with multiprocessing.Pool(args.j) as pool:
        for text in pool.imap(line, corpus(), chunksize=1):
            print(text, flush=True)
