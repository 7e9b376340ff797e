"""Helpers of tests/test_refusals_cpu.py (no test functions here): the grid of command lines and configs whose refusals are
pinned, and what is recorded of each.  scripts/make_refusal_goldens.py writes tests/golden/eval_refusals.json from these at
the commit whose refusals are to be kept.

The grid: every single off-default value and every pair of values of two different options, on top of each base, plus the
few triples EXTRA lists (sentences that only show once two other requirements are met).  Command lines go through
get_evaluation_args on the bases none / --device_env / --match; configs are SimpleNamespaces with the scalar values a
checkpoint carries, on the bases host / device_env=True, each read with match=False and match=True.

Of a case: the outcome of each of the eight per-option functions called alone ('ok', or the exception's type and text;
refuse_match of a config gets a default TicTacToe config as `other`), and for a command line main()'s outcome up to the
point where it would load a checkpoint."""
import itertools
import types

OPTIONS = ('unsupported', 'device_env', 'opp_playouts', 'grade', 'grade_unroll', 'true_model', 'gumbel', 'match')

CLI_BASES = ((), ('--device_env',), ('--match',))
CLI_VALUES = (      # (option, its off-default values)
    ('--apply_mcts_actions', ('3', '0', '1 2')), ('--random_opp', ('1', '-1')), ('--human_opp', ('1',)),
    ('--opp_playouts', ('64', '100', '131072')), ('--grade', ('',)), ('--grade_table', ('',)), ('--grade_unroll', ('3', '0', '17')),
    ('--true_model', ('1', '0 1', '2')), ('--gumbel', ('1', '0 1', '2')), ('--only_prior', ('1', '0 1')), ('--only_value', ('1', '1 0')),
    ('--use_exploration_noise', ('1', '0 1')), ('--temperatures', ('0.5', '0 1', '1 0')), ('--gumbel_considered', ('1',)),
    ('--gumbel_c_visit', ('-1',)), ('--gumbel_c_scale', ('0',)), ('--gumbel_scale', ('-0.5',)), ('--render', ('',)),
    ('--save_gif_as', ('x.gif',)), ('--save_mcts', ('',)), ('--plot_summary', ('',)),
)
CLI_EXTRA = (      # the playout opponent's game and applied actions are read once the device path and the seat are given
    '--device_env --opp_playouts 64 --random_opp -1 --apply_mcts_actions 3',
    '--device_env --opp_playouts 64 --random_opp 1 --apply_mcts_actions 1 2',
)

CONFIG_BASES = (dict(device_env=False), dict(device_env=True))
CONFIG_VALUES = (
    ('environment', ('ConnectFour', 'CartPole-v1', 'LunarLander-v2')), ('architecture', ('MuZeroNetwork',)), ('norm_obs', (True,)),
    ('apply_mcts_actions', (3, 0)), ('only_prior', (1,)), ('only_value', (1,)), ('use_exploration_noise', (1,)), ('temperature', (0.5,)),
    ('random_opp', (1, -1)), ('human_opp', (1,)), ('render', (True,)), ('opp_playouts', (64, 100)), ('grade', (True,)),
    ('grade_table', (True,)), ('grade_unroll', (3, 17)), ('true_model', (1, 2)), ('gumbel', (1,)), ('gumbel_considered', (1,)),
    ('gumbel_scale', (-0.5,)), ('no_support', (True,)), ('value_support', ((-10, 10),)),
)
CONFIG_EXTRA = (
    dict(device_env=True, opp_playouts=64, random_opp=-1, environment='CartPole-v1'),
    dict(device_env=True, opp_playouts=64, random_opp=1, apply_mcts_actions=3),
)


def default_config(**kv):
  c = dict(environment='TicTacToe', architecture='FCNetwork', two_players=True, num_simulations=8, norm_obs=False, apply_mcts_actions=1,
           only_prior=0, only_value=0, use_exploration_noise=0, temperature=0.0, random_opp=None, human_opp=None, render=False,
           save_mcts=False, save_gif_as='', opp_playouts=0, grade=False, grade_table=False, grade_unroll=None, true_model=0, gumbel=0,
           gumbel_considered=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0, gumbel_scale=0.0, no_support=False, value_support=(-15, 15),
           reward_support=(-15, 15), device_env=False)
  c.update(kv)
  return types.SimpleNamespace(**c)


def _singles_and_pairs(values):
  flat = [(k, v) for k, vs in values for v in vs]
  yield from ([x] for x in flat)
  yield from ([x, y] for x, y in itertools.combinations(flat, 2) if x[0] != y[0])


def cli_cases():
  """the command lines, as argument lists"""
  out = []
  for base in CLI_BASES:
    out.append(list(base))
    for chosen in _singles_and_pairs(CLI_VALUES):
      out.append(list(base) + [w for k, v in chosen for w in [k] + v.split()])
  return out + [line.split() for line in CLI_EXTRA]


def config_cases():
  """the configs, as (attributes that differ from default_config(), match)"""
  out = []
  for base in CONFIG_BASES:
    for chosen in itertools.chain([[]], _singles_and_pairs(CONFIG_VALUES)):
      out += [(dict(base, **dict(chosen)), match) for match in (False, True)]
  return out + [(kv, False) for kv in CONFIG_EXTRA]


def outcome(fn, *a, **kw):
  try:
    fn(*a, **kw)
  except Exception as e:
    return '%s: %s' % (type(e).__name__, e)
  return 'ok'


def per_option(c, match, other=None):
  """the eight per-option functions, each called alone, in the order of OPTIONS"""
  from model_based_rl_amd import evaluate
  from model_based_rl_amd.match import refuse_match
  return [outcome(evaluate.refuse_unsupported, c), outcome(evaluate.refuse_device_env, c),
          outcome(evaluate.refuse_opp_playouts, c, match=match), outcome(evaluate.refuse_grade, c, match=match),
          outcome(evaluate.refuse_grade_unroll, c), outcome(evaluate.refuse_true_model, c, match=match),
          outcome(evaluate.refuse_gumbel, c, match=match), outcome(refuse_match, c, other)]


class _Loading(Exception):
  pass


def main_outcome(argv):
  """evaluate.main(argv) up to its first checkpoint: the sentence it refuses with, or 'ok' where it goes on to load"""
  from model_based_rl_amd import evaluate, match

  def loading(*a, **k):
    raise _Loading()
  saved = evaluate.state_generator, match.match_states
  evaluate.state_generator = match.match_states = loading
  try:
    evaluate.main(list(argv))
  except _Loading:
    return 'ok'
  except Exception as e:
    return '%s: %s' % (type(e).__name__, e)
  finally:
    evaluate.state_generator, match.match_states = saved
  raise AssertionError('main() returned without loading a checkpoint: %r' % (argv,))


def recorded():
  """[(case name, [the eight per-option outcomes] + [main()'s outcome, or None for a config])] over the whole grid"""
  from model_based_rl_amd.config import get_evaluation_args
  out = []
  for argv in cli_cases():
    args = get_evaluation_args(list(argv))
    out.append(('cli ' + ' '.join(argv), per_option(args, args.match) + [main_outcome(argv)]))
  for kv, match in config_cases():
    name = 'config match=%d %s' % (match, ' '.join('%s=%r' % (k, kv[k]) for k in sorted(kv)))
    out.append((name, per_option(default_config(**kv), match, default_config()) + [None]))
  return out


def first_in_table_order(outcomes, match):
  """the outcome the combined entry must give: that of the first refusing option in the table's order (main()'s), or 'ok'"""
  by = dict(zip(OPTIONS, outcomes))
  order = ('opp_playouts', 'grade', 'grade_unroll', 'true_model', 'gumbel') + (('match', 'unsupported') if match else ('unsupported', 'device_env'))
  return next((by[k] for k in order if by[k] != 'ok'), 'ok')
