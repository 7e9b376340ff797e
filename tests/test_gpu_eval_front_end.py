"""The evaluation front end returns what it returned before its side / requirement plumbing was stated once: the SHA-256 of
every field of every game, the summary and the grade reports (tests/eval_front_end_util.py) on the host path, the device
games, the true-rules and Gumbel searches, the opponents, the grading and the matches, against
tests/golden/eval_front_end_sha256.json (scripts/make_eval_front_end_digests.py wrote it at the commit before)."""
import json
import os

import pytest

from tests.eval_front_end_util import CASES, digest

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_front_end_sha256.json')) as f:
  WANT = json.load(f)


def test_the_golden_names_every_case():
  assert sorted(WANT) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_records_are_unchanged(name):
  assert digest(name) == WANT[name]
