"""CPU side of the matches between two networks (model_based_rl_amd/match.py, csrc/mz_match.hip.h):
  flags     --match and the per-side lists parse and reach the two sides' configs
  refusals  every refusal of refuse_match is one sentence with its word in it, and reaches the caller before any device
  score     score, Elo difference and interval on hand-computed W / D / L
  abi       the mz_match_* entry points are in the header and the ctypes table (tests/test_abi.py compares the two with the
            library's exports)
  rules     the per-game open / observe / apply bodies, compiled for the host with -fsanitize=address,undefined into a
            stand-alone program (tests/match_rules_host.cpp) that plays 3600 random games against a window scan of its
            own; the games it printed, replayed on envs.TicTacToe / envs.ConnectFour, end the same way"""
import math
import os
import subprocess
import types

import pytest

from tests.eval_device_util import eval_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_device(monkeypatch):
  """any attempt to reach a device fails the test"""
  import torch
  from model_based_rl_amd import engine, match

  def touched(*a, **k):
    raise AssertionError('a device was touched')
  monkeypatch.setattr(torch.cuda, 'is_available', touched)
  monkeypatch.setattr(engine.Engine, '__init__', touched)
  monkeypatch.setattr(match.Match, '__init__', touched)


def test_flags_reach_the_sides():
  from model_based_rl_amd import match
  from model_based_rl_amd.config import get_evaluation_args
  args = get_evaluation_args(['--match', '--saves_dir', 'd/', '--nets', 'a', 'b', '--num_games', '12', '--opening_plies', '2',
                              '--seed', '7', '--num_simulations', '8', '5', '--temperatures', '0', '0.5', '--only_prior', '0', '1',
                              '--use_exploration_noise', '1', '--out', 'o.json'])
  assert args.match and args.opening_plies == 2 and args.nets == ['a', 'b'] and args.batch == 12 and args.out == 'o.json'
  assert not get_evaluation_args(['--nets', 'a']).match and get_evaluation_args([]).opening_plies == 0
  base = eval_state('TicTacToe', sims=30)
  a, b = match.side_state(base, args, 0), match.side_state(base, args, 1)
  ca, cb = a['config'], b['config']
  assert (ca.num_simulations, cb.num_simulations) == (8, 5) and base['config'].num_simulations == 30
  assert (ca.temperature, cb.temperature) == (0.0, 0.5)
  assert (ca.only_prior, cb.only_prior) == (0, 1) and (ca.only_value, cb.only_value) == (0, 0)
  assert (ca.use_exploration_noise, cb.use_exploration_noise) == (1, 1)      # (one value: both sides)
  assert a['weights'] is base['weights']
  assert match._side(ca) == (0, 0.0, True) and match._side(cb) == (1, 0.5, True)
  with pytest.raises(ValueError, match='length one'):
    match.side_state(base, get_evaluation_args(['--match', '--temperatures', '0', '1', '2']), 0)
  # without --num_simulations a side keeps its checkpoint's
  assert match.side_state(base, get_evaluation_args(['--match']), 1)['config'].num_simulations == 30


def _cfg(**kv):
  c = types.SimpleNamespace(environment='TicTacToe', apply_mcts_actions=1, norm_obs=False, random_opp=None, human_opp=None,
                            architecture='FCNetwork', no_support=False, value_support=(-15, 15), reward_support=(-15, 15))
  for k, v in kv.items():
    setattr(c, k, v)
  return c


REFUSALS = [      # (the refused config, the second checkpoint's config or None, the word the sentence carries)
    (_cfg(environment='CartPole-v0'), None, 'CartPole-v0'),
    (_cfg(environment='LunarLander-v2'), None, 'LunarLander-v2'),
    (_cfg(apply_mcts_actions=3), None, '--apply_mcts_actions'),
    (_cfg(apply_mcts_actions=[1, 2]), None, '--apply_mcts_actions'),
    (_cfg(norm_obs=True), None, '--norm_obs'),
    (_cfg(random_opp=-1), None, '--random_opp'),
    (_cfg(human_opp=1), None, '--human_opp'),
    (_cfg(architecture='MuZeroNetwork'), None, 'MuZeroNetwork'),
    (_cfg(), _cfg(environment='ConnectFour'), 'environment'),
    (_cfg(), _cfg(value_support=(-7, 7)), 'supports'),
    (_cfg(), _cfg(reward_support=(-2, 2)), 'supports'),
    (_cfg(), _cfg(no_support=True), 'no_support'),
    (_cfg(), _cfg(norm_obs=True), '--norm_obs'),      # (the second checkpoint is held to the same rules)
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_refusals_are_one_sentence(i):
  from model_based_rl_amd.match import refuse_match
  c, other, word = REFUSALS[i]
  with pytest.raises(NotImplementedError) as err:
    refuse_match(c, other)
  msg = str(err.value)
  assert msg.startswith('--match: ') and word in msg, msg
  assert msg.endswith('.') and '\n' not in msg and '. ' not in msg[:-1], msg      # one sentence
  refuse_match(_cfg(), _cfg())      # and nothing to refuse between two TicTacToe checkpoints
  refuse_match(_cfg(environment='ConnectFour'))


def test_refusals_reach_the_caller_before_any_device(monkeypatch, tmp_path):
  from model_based_rl_amd import evaluate, match
  _no_device(monkeypatch)
  # the command line: refused before a checkpoint is read
  for flags, word in ((['--random_opp', '-1'], '--random_opp'), (['--human_opp', '1'], '--human_opp'),
                      (['--apply_mcts_actions', '2'], '--apply_mcts_actions')):
    with pytest.raises(NotImplementedError, match='^--match: .*' + word):
      evaluate.main(['--match', '--saves_dir', str(tmp_path) + os.sep, '--nets', 'a', 'b'] + flags)
  # the checkpoints' configs: refused by play_match itself
  ttt, c4, cart = eval_state('TicTacToe'), eval_state('ConnectFour'), eval_state('CartPole-v0')
  with pytest.raises(NotImplementedError, match='^--match: .*CartPole-v0'):
    match.play_match(cart, cart, 4)
  with pytest.raises(NotImplementedError, match='^--match: .*environment'):
    match.play_match(ttt, c4, 4)
  with pytest.raises(NotImplementedError, match='^--match: .*--norm_obs'):
    match.play_match(ttt, eval_state('TicTacToe', norm_obs=True), 4)
  with pytest.raises(NotImplementedError, match='^--match: .*--apply_mcts_actions'):
    match.play_match(eval_state('TicTacToe', apply_mcts_actions=2), ttt, 4)
  # ... and a match that is not refused does go on to the device
  with pytest.raises(AssertionError, match='a device was touched'):
    match.play_match(ttt, ttt, 4)


def test_score_elo_and_interval():
  from model_based_rl_amd.match import MatchGame, elo_difference, score_summary, summarize
  s = score_summary(6, 3, 1)
  # s = (6 + 1.5) / 10; per-game variance (6 * 0.25^2 + 3 * 0.25^2 + 1 * 0.75^2) / 10 = 0.1125; se = sqrt(0.1125 / 10)
  assert s['score'] == 0.75 and s['games'] == 10
  assert abs(s['score_se'] - math.sqrt(0.01125)) < 1e-15
  assert abs(s['elo'] - 400 * math.log10(3.0)) < 1e-12
  lo, hi = 0.75 - 1.96 * math.sqrt(0.01125), 0.75 + 1.96 * math.sqrt(0.01125)
  assert abs(s['elo_interval'][0] - 400 * math.log10(lo / (1 - lo))) < 1e-9
  assert abs(s['elo_interval'][1] - 400 * math.log10(hi / (1 - hi))) < 1e-9
  assert s['elo_interval'][0] < s['elo'] < s['elo_interval'][1]
  # all wins / all losses: no finite Elo, reported as None (null in the JSON)
  for w, l, score in ((5, 0, 1.0), (0, 5, 0.0)):
    e = score_summary(w, 0, l)
    assert e['score'] == score and e['elo'] is None and e['score_se'] == 0.0 and e['elo_interval'] == [None, None]
  # all draws: level, with no spread
  d = score_summary(0, 4, 0)
  assert d['score'] == 0.5 and d['elo'] == 0.0 and d['elo_interval'] == [0.0, 0.0]
  # an interval that leaves (0, 1) at one end: that end has no Elo
  e = score_summary(9, 0, 1)
  assert abs(e['score_se'] - math.sqrt(0.09 / 10)) < 1e-15 and e['elo_interval'][1] is None and e['elo_interval'][0] is not None
  assert elo_difference(0.5) == 0.0 and elo_difference(0.0) is None and elo_difference(1.0) is None
  assert abs(elo_difference(10 / 11.) - 400.0) < 1e-9
  # the summary over records: per seating and in total
  games = [MatchGame(0, 0, 1, 5), MatchGame(1, 0, 0, 9), MatchGame(0, 1, -1, 6), MatchGame(1, 1, 1, 8)]
  sm = summarize(games)
  assert (sm['wins'], sm['draws'], sm['losses'], sm['games']) == (2, 1, 1, 4) and sm['score'] == 0.625 and sm['mean_length'] == 7.0
  assert (sm['a_first']['wins'], sm['a_first']['draws'], sm['a_first']['losses']) == (1, 1, 0)
  assert (sm['b_first']['wins'], sm['b_first']['draws'], sm['b_first']['losses']) == (1, 0, 1)


def test_match_entry_points_are_declared():
  from model_based_rl_amd import _abi
  from tests.test_abi import declared_symbols
  want = {'mz_match_create', 'mz_match_destroy', 'mz_match_reset', 'mz_match_set_draws', 'mz_match_plies', 'mz_match_results',
          'mz_match_log_capacity'}
  assert want <= set(_abi.SIGNATURES) and want <= set(declared_symbols(('mz_engine.h',)))
  assert 'mz_match.hip.h' in _abi._SOURCES and 'mz_match_abi.inc' in _abi._SOURCES
  assert 'mz_match.hip.h' in _abi._ENGINE_ONLY and 'mz_match_abi.inc' in _abi._ENGINE_ONLY


def test_rule_bodies_on_the_host(tmp_path):
  """tests/match_rules_host.cpp under AddressSanitizer + UBSan, then its games on the host classes"""
  import numpy as np
  from model_based_rl_amd import envs
  exe = str(tmp_path / 'match_rules_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'include'),
         '-I', os.path.join(ROOT, 'model-based-rl_amd', 'csrc'), os.path.join(ROOT, 'tests', 'match_rules_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  lines = run.stdout.strip().splitlines()
  assert lines[-1] == 'ok 3600' and len(lines) == 3601
  seen = set()
  for line in lines[:-1]:
    kind, max_steps, path, result, length, *actions = [int(x) for x in line.split()]
    e = envs.TicTacToe() if kind == 1 else envs.ConnectFour()
    e.reset()
    assert len(actions) == length <= max_steps
    winner, done = 0, False
    for i, a in enumerate(actions):
      assert not done and a in [int(x) for x in e.legal_actions()], line
      mover = e.turn
      _, reward, done, _ = e.step(a)
      if reward:
        winner = mover
      assert (done or i + 1 >= max_steps) == (i == length - 1), line      # it ended where the host class (or the cut) ends it
    assert result == winner, line
    seen.add((kind, max_steps < 42, path, result, done))
  # both games, both bodies, all three results, the rules' end and the cut
  for kind in (1, 3):
    for path in (0, 1):
      assert {r for k, c, p, r, d in seen if (k, p) == (kind, path)} == {-1, 0, 1}, (kind, path)
      assert (kind, True, path, 0, False) in seen, (kind, path)      # a game the cut ended, not the rules
  assert np.mean([int(l.split()[4]) for l in lines[:-1]]) > 5
