"""The refusals of the evaluation front end are what they were before the options' requirements moved into one table
(model_based_rl_amd/sides.py): on the grid of tests/refusal_cases.py -- every single off-default value and every pair on two
options, over command lines and configs -- against tests/golden/eval_refusals.json (scripts/make_refusal_goldens.py wrote it at
the commit before):
  per option  each of the eight per-option functions, called alone, says what it said
  main        evaluate.main() refuses with the same sentence, or goes on to load a checkpoint, as it did
  combined    refuse(), the one entry the other sites call, raises exactly when some option does, with the sentence of the
              first refusing option in the table's order"""
import hashlib
import json
import os

import pytest

from tests import refusal_cases as rc

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_refusals.json')) as f:
  GOLDEN = json.load(f)


@pytest.fixture(scope='module')
def recorded():
  return rc.recorded()


@pytest.fixture(scope='module')
def wanted(recorded):
  """per case of the grid the golden's nine outcomes (None: a config has no main())"""
  names = hashlib.sha256('\n'.join(name for name, _ in recorded).encode()).hexdigest()
  assert names == GOLDEN['names_sha256'] and len(recorded) == len(GOLDEN['cases']), 'the grid is not the one the golden was written on'
  return [[None if t < 0 else GOLDEN['texts'][t] for t in GOLDEN['rows'][row]] for row in GOLDEN['cases']]


@pytest.mark.parametrize('k', range(len(rc.OPTIONS)), ids=rc.OPTIONS)
def test_each_option_alone_says_what_it_said(recorded, wanted, k):
  differ = [(name, got[k], want[k]) for (name, got), want in zip(recorded, wanted) if got[k] != want[k]]
  assert differ[:5] == [], len(differ)


def test_main_says_what_it_said(recorded, wanted):
  differ = [(name, got[-1], want[-1]) for (name, got), want in zip(recorded, wanted) if got[-1] != want[-1]]
  assert differ[:5] == [], len(differ)
  assert sum(want[-1] not in (None, 'ok') for want in wanted) > 1000      # (the grid does reach main()'s refusals)


def test_the_combined_entry_is_the_first_refusing_option(wanted):
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.sides import refuse
  differ, refused = [], 0
  for argv, want in zip(rc.cli_cases(), wanted):
    args = get_evaluation_args(list(argv))
    got, first = rc.outcome(refuse, args, match=args.match), rc.first_in_table_order(want[:8], args.match)
    assert first == want[8], argv      # (main()'s chain is this order)
    differ += [(argv, got, first)] if got != first else []
    refused += got != 'ok'
  configs = rc.config_cases()
  for (kv, match), want in zip(configs, wanted[-len(configs):]):
    got = rc.outcome(refuse, rc.default_config(**kv), match=match, other=rc.default_config() if match else None)
    first = rc.first_in_table_order(want[:8], match)
    differ += [(kv, match, got, first)] if got != first else []
    refused += got != 'ok'
  assert differ[:5] == [], len(differ)
  assert refused > 1000


def test_every_sentence_is_in_the_golden():
  """every sentence of the table is one the grid reached: as the golden has it, up to its % arguments"""
  import re
  from model_based_rl_amd.sides import OPTIONS
  texts = [t.split(': ', 1)[1] for t in GOLDEN['texts'] if t != 'ok']
  for name, option in OPTIONS.items():
    for _, sentence, *args in option.requires:
      pattern = re.sub(r'%[drsg]', '.*', re.escape(sentence).replace('\\%', '%'))
      assert any(re.fullmatch(pattern, t) for t in texts), (name, sentence)
