#!/usr/bin/env python3
"""The pinned records of the evaluation front end (TEST INFRASTRUCTURE, needs the GPU): the SHA-256 of everything
Evaluator.play_games and match.play_match return on the configurations of tests/eval_front_end_util.CASES -- every field of
every game, the summary, the grade reports without their seconds.  Run at the commit whose records are to be kept; written
to tests/golden/eval_front_end_sha256.json, which tests/test_gpu_eval_front_end.py compares against.  Records are keyed by the
counter RNG, so two runs in two processes give the same file; --check FILE compares instead of writing and exits 1 where a
digest differs.

usage: python scripts/make_eval_front_end_digests.py [--out FILE] [--check FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


def main():
  from tests.eval_front_end_util import CASES, digest
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'eval_front_end_sha256.json'))
  ap.add_argument('--check', default=None)
  a = ap.parse_args()
  got = {name: digest(name) for name in CASES}
  if a.check:
    with open(a.check) as f:
      want = json.load(f)
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    print('%d digests, %d differ%s' % (len(got), len(differ), ': ' + ', '.join(differ) if differ else ''))
    return 1 if differ else 0
  with open(a.out, 'w') as f:
    json.dump(got, f, indent=1, sort_keys=True)
    f.write('\n')
  print('%d digests -> %s' % (len(got), a.out))
  return 0


if __name__ == '__main__':
  sys.exit(main())
