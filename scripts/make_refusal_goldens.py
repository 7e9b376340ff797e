#!/usr/bin/env python3
"""The pinned refusals of the evaluation front end (TEST INFRASTRUCTURE, no GPU): what each of the eight per-option
functions (evaluate.refuse_unsupported / _device_env / _opp_playouts / _grade / _grade_unroll / _true_model / _gumbel,
match.refuse_match) says alone, and what main() says before it loads a checkpoint, on the grid of tests/refusal_cases.py.
Run at the commit whose refusals are to be kept; tests/test_refusals_cpu.py compares against the file.

The file stores every distinct text once (`texts`), every distinct row of nine outcomes once (`rows`, indices into texts,
-1 where a config has no main()), and per case of the grid, in the grid's order, its row (`cases`); `names_sha256` pins the
grid itself.  --coverage also lists the `raise NotImplementedError` lines of the eight functions that no case reached.

usage: python scripts/make_refusal_goldens.py [--out FILE] [--coverage]"""
import argparse
import hashlib
import inspect
import json
import os
import sys
import traceback

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


def pack(recorded):
  texts, rows, cases = [], [], []
  index = lambda seq, x: seq.index(x) if x in seq else (seq.append(x) or len(seq) - 1)
  for _, outcomes in recorded:
    cases.append(index(rows, [-1 if o is None else index(texts, o) for o in outcomes]))
  names = hashlib.sha256('\n'.join(name for name, _ in recorded).encode()).hexdigest()
  return dict(texts=texts, rows=rows, cases=cases, names_sha256=names)


def main():
  from tests import refusal_cases as rc
  from model_based_rl_amd import evaluate, match
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'eval_refusals.json'))
  ap.add_argument('--coverage', action='store_true')
  a = ap.parse_args()
  reached = set()
  plain = rc.outcome

  def outcome(fn, *args, **kw):
    try:
      fn(*args, **kw)
    except Exception as e:
      frame = traceback.extract_tb(e.__traceback__)[-1]
      reached.add((os.path.basename(frame.filename), frame.lineno))
    return plain(fn, *args, **kw)
  if a.coverage:
    rc.outcome = outcome
  recorded = rc.recorded()
  packed = pack(recorded)
  with open(a.out, 'w') as f:
    json.dump(packed, f, separators=(',', ':'))
    f.write('\n')
  print('%d cases, %d distinct rows, %d distinct texts -> %s (%d bytes)'
        % (len(recorded), len(packed['rows']), len(packed['texts']), a.out, os.path.getsize(a.out)))
  if a.coverage:
    fns = [getattr(evaluate, 'refuse_' + k) for k in rc.OPTIONS[:-1]] + [match.refuse_match]
    lines = set()
    for fn in fns:
      src, first = inspect.getsourcelines(fn)
      lines |= {(os.path.basename(inspect.getsourcefile(fn)), first + i) for i, s in enumerate(src) if 'raise NotImplementedError' in s}
    missed = sorted(lines - reached)
    print('%d of %d raise lines reached%s' % (len(lines) - len(missed), len(lines), ''.join('\n  not reached: %s:%d' % m for m in missed)))
  return 0


if __name__ == '__main__':
  sys.exit(main())
