"""Evaluation games on the device environments (csrc/mz_eval_env.hip.h, Evaluator.play_games(device_env=True)):
  host      the device path's games equal the host-environment path's, game by game and move by move, on the same draws
  goldens   the reference's recorded games replayed through the device path equal the host path's replay, all 167 moves
  summary   summary() of the device accumulators against SummaryTools.summary of the host games
  batches   with the device's own draws a game's record does not depend on the batch; every kept game re-steps through
            the envs.py classes, and every opponent move is the counter RNG's
  CLI       evaluate.main(... --device_env)
Shared shapes: 8 simulations, random weights with scaled heads, 37 games at batch 16 (two full batches and a tail of 5)."""
import functools
import json
import os

import numpy as np
import pytest

from tests.eval_device_util import OPP_NMIN, eval_state, make_draws, opponent_choice, record

pytestmark = pytest.mark.gpu

N, BATCH, SIMS, SEED0 = 37, 16, 8, 1000

#         name: (environment, config overrides)
CONFIGS = {
    'ttt_opp_m1': ('TicTacToe', dict(random_opp=-1)),
    'ttt_opp_p1': ('TicTacToe', dict(random_opp=1)),
    'ttt_selfplay_t05': ('TicTacToe', dict(random_opp=None, temperature=0.5)),
    'ttt_mcts_actions3': ('TicTacToe', dict(random_opp=-1, apply_mcts_actions=3)),
    'ttt_only_prior': ('TicTacToe', dict(random_opp=-1, only_prior=1)),
    'ttt_only_value': ('TicTacToe', dict(random_opp=-1, only_value=1)),
    'ttt_noise': ('TicTacToe', dict(random_opp=-1, use_exploration_noise=1)),
    'c4_opp_m1': ('ConnectFour', dict(random_opp=-1)),
    'c4_opp_p1': ('ConnectFour', dict(random_opp=1)),
    'c4_max_steps11': ('ConnectFour', dict(random_opp=-1, max_steps=11)),
    'cartpole': ('CartPole-v0', dict()),
    'cartpole_max_steps12': ('CartPole-v0', dict(max_steps=12)),
}
LONGEST = {'TicTacToe': 9, 'ConnectFour': 42, 'CartPole-v0': 200}


def _start_states(seeds):
  """the device CartPole's start states of these games (episode 0 of environment = the game's seed, engine seed 0)"""
  from model_based_rl_amd.engine import Engine
  eng = Engine(1, 4, 2, SIMS, seed=0)
  out = np.stack([eng.cartpole_reset_state(s, 0) for s in seeds])
  eng.close()
  return out


def _host_cartpoles(states):
  from model_based_rl_amd.envs import CartPole

  class StartCartPole(CartPole):
    """CartPole whose reset() sets a given start state"""

    def __init__(self, start):
      self._start = tuple(float(v) for v in start)
      CartPole.__init__(self, 200)

    def reset(self):
      self.state = self._start
      self._elapsed_steps = 0
      return self._obs()
  return [StartCartPole(s) for s in states]


@functools.lru_cache(maxsize=None)
def _pair(name):
  """(config, host games, device games) of one configuration: the same seeds and the same numpy draws on both paths"""
  from model_based_rl_amd.evaluate import Evaluator
  env, over = CONFIGS[name]
  state = eval_state(env, sims=SIMS, **over)
  cfg = state['config']
  cfg.batch = BATCH
  seeds = list(range(SEED0, SEED0 + N))
  A, M = int(cfg.action_space), int(cfg.apply_mcts_actions)
  moves = min(LONGEST[env], int(cfg.max_steps))
  draws = make_draws(np.random.RandomState(len(name) * 7 + A), N, moves, M, A, OPP_NMIN[env])
  ev = Evaluator(state)
  ev.load_network()
  envs = starts = None
  if env == 'CartPole-v0':
    starts = _start_states(seeds)
    envs = _host_cartpoles(starts)
  host = ev.play_games(N, seeds, environments=envs, draws=draws)
  # (one CartPole configuration is given the start states, the other leaves them to the device's own reset: the same ones)
  dev = ev.play_games(N, seeds, draws=draws, device_env=True, keep_history=True,
                      start_states=starts if name == 'cartpole' else None)
  return cfg, host, dev


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_device_path_equals_host_path(name):
  cfg, host, dev = _pair(name)
  assert len(host) == len(dev) == N
  lengths = set()
  for i, (h, d) in enumerate(zip(host, dev)):
    rh, rd = record(h), record(d)
    for key in rh:
      assert rh[key] == rd[key], (name, i, key, rh[key], rd[key])      # exact: the same kernels on the same inputs
    assert len(d.n_actions) == len(rd['child_visits']) and sum(d.n_actions) == d.step, (name, i)
    assert all(1 <= n <= max(1, int(cfg.apply_mcts_actions)) for n in d.n_actions), (name, i)
    assert d.step == len(rd['actions']) <= cfg.max_steps
    lengths.add(d.step)
  if 'max_steps' in name:      # the cut: no game is longer, and it -- not the environment -- ended games
    cut = [d for d in dev if d.step == int(cfg.max_steps)]
    assert max(lengths) == int(cfg.max_steps) and cut, (name, lengths)
    assert any(not any(record(d)['dones']) for d in cut), name
  else:
    assert len(lengths) > 1, (name, lengths)      # (games of different lengths: finished games sat beside live ones)
  if cfg.two_players and cfg.random_opp is not None:      # the final sign flip happened somewhere
    assert any(r < 0 for d in dev for r in d.history.rewards), name


def test_summary_of_the_device_accumulators():
  from model_based_rl_amd.evaluate import SummaryTools
  for name in ('ttt_opp_m1', 'ttt_mcts_actions3', 'c4_opp_p1', 'cartpole'):
    cfg, host, dev = _pair(name)
    sh, sd = SummaryTools().summary(host), SummaryTools().summary(dev)
    assert set(sh) == set(sd) == {'length', 'return', 'pred_return', 'pred_value', 'mcts_value', 'search_depth'}
    for key in ('length', 'return'):      # integer-valued
      assert sh[key] == sd[key], (name, key, sh[key], sd[key])
    for key in sh:
      for a, b in zip(sh[key], sd[key]):
        print(name, key, a, b)
        assert abs(a - b) <= 1e-9 * max(abs(a), abs(b)), (name, key, a, b)
    # the light objects carry the accumulators of the kept lists
    for h, d in zip(host, dev):
      assert d.ret == sum(h.history.rewards) and d.step == h.step
      assert abs(d.pred_return - sum(h.pred_rewards)) <= 1e-9 * max(1.0, abs(d.pred_return))
      assert d.search_depth == float(np.mean(max(h.search_depths)))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
G7 = sorted(f for f in os.listdir(GOLDEN) if f.startswith('g7_eval_ttt_'))


@pytest.mark.parametrize('name', G7, ids=[f[len('g7_eval_'):-4] for f in G7])
def test_reference_games_on_the_device(name):
  """the reference's recorded games, fed to both paths exactly as test_reference_games feeds the host path: the device
  path's record equals the host path's replay of the same set, field for field"""
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.envs import TicTacToe
  from model_based_rl_amd.evaluate import Evaluator
  g = np.load(os.path.join(GOLDEN, name))
  w = np.load(os.path.join(GOLDEN, str(g['weights_file'])))
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--known_bounds', '-1', '1', '--discount', '1',
                     '--num_simulations', str(int(g['num_simulations']))])
  ro = int(g['random_opp'])
  for k, v in dict(temperature=float(g['temperature']), only_prior=int(g['only_prior']), only_value=int(g['only_value']),
                   use_exploration_noise=int(g['use_exploration_noise']), apply_mcts_actions=int(g['apply_mcts_actions']),
                   random_opp=ro if ro else None, human_opp=None, render=False, save_mcts=False, save_gif_as='', label=name,
                   verbose=False).items():
    setattr(cfg, k, v)
  weights = {k[2:]: torch.from_numpy(w[k].copy()) for k in w.files if k.startswith('w.')}
  ev = Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  seeds = [int(s) for s in g['seeds']]
  all_draws, moves = [], 0
  for gi in range(len(seeds)):
    mv = np.flatnonzero(g['move_game'] == gi)
    moves += len(mv)
    pad = 12
    all_draws.append(dict(walk=[g['walk_u'][m, :g['walk_n'][m]] for m in mv] + [np.full(g['walk_u'].shape[1], 0.5)] * pad,
                          noise=[g['noise'][m] for m in mv] + [np.full(9, 1 / 9.)] * pad,
                          opp=[int(x) for m in mv for x in g['opp'][m, :g['opp_n'][m]]] + [0] * 4 * pad))
  host = [ev.play_game(TicTacToe(), seed=s, draws=d) for s, d in zip(seeds, all_draws)]
  dev = ev.play_games(len(seeds), seeds, draws=all_draws, device_env=True, keep_history=True)
  for gi, (h, d) in enumerate(zip(host, dev)):
    assert record(h) == record(d), (name, gi)
  # every recorded move's draws were fed; the two replays are equally long (where the host replay leaves the recording inside
  # the float32 allowance of test_reference_games, the device path leaves it at the same move)
  assert sum(len(d['walk']) - 12 for d in all_draws) == moves == len(g['move_game'])
  assert sum(len(d.history.child_visits) for d in dev) == sum(len(h.history.child_visits) for h in host) > 0


def test_reference_games_cover_all_moves():
  """the eight sets the test above is parametrised over hold all 167 recorded moves: none is left out"""
  assert len(G7) == 8
  assert sum(len(np.load(os.path.join(GOLDEN, f))['move_game']) for f in G7) == 167


BATCHES = {'TicTacToe': dict(random_opp=-1, temperature=0.5, use_exploration_noise=1),
           'ConnectFour': dict(random_opp=1, temperature=0.5, use_exploration_noise=1),
           'CartPole-v0': dict(temperature=0.5, use_exploration_noise=1, max_steps=40)}


@pytest.mark.parametrize('env', sorted(BATCHES))
def test_batch_invariance_and_the_device_draws(env):
  from model_based_rl_amd import envs as host_envs
  from model_based_rl_amd.evaluate import Evaluator
  seeds = list(range(100, 137))
  recs = {}
  for batch in (16, 64):
    state = eval_state(env, sims=SIMS, **BATCHES[env])
    state['config'].batch = batch
    ev = Evaluator(state)
    ev.load_network()
    recs[batch] = ev.play_games(len(seeds), seeds, device_env=True, keep_history=True)
  cfg = state['config']
  assert [record(g) for g in recs[16]] == [record(g) for g in recs[64]]
  assert len(set(str(g.history.actions) for g in recs[16])) > len(seeds) // 2      # (different seeds, different games)
  starts = _start_states(seeds) if env == 'CartPole-v0' else None
  opp_moves = 0
  for i, g in enumerate(recs[16]):
    h = g.history
    e = host_envs.get_environment(cfg)
    e.reset()
    if starts is not None:
      e.set_state(starts[i])
    at = 0
    for move, n_act in enumerate(g.n_actions):
      legal_root = [int(a) for a in e.legal_actions()]
      for j in range(n_act):
        a, mover = h.actions[at], h.to_play[at]
        assert a in [int(x) for x in e.legal_actions()], (env, i, at)
        assert mover == (e.turn if cfg.two_players else 1)
        opp = cfg.two_players and mover == cfg.random_opp
        if opp:
          assert a == opponent_choice(legal_root, 0, seeds[i], move, j), (env, i, move, j)
          opp_moves += 1
        _, reward, done, _ = e.step(a)
        last = at == g.step - 1
        assert h.dones[at] == bool(done) and (done or e._elapsed_steps >= cfg.max_steps) == last, (env, i, at)
        assert h.rewards[at] == (-reward if (last and opp) else reward), (env, i, at)
        at += 1
    assert at == g.step == len(h.actions) == len(h.rewards)
  assert opp_moves > 0 or not cfg.two_players


def _checkpoint(tmp_path):
  import torch
  state = eval_state('TicTacToe', sims=SIMS)
  saves = tmp_path / 'runs' / 'TicTacToe' / 'g' / 'r' / 'saves'
  saves.mkdir(parents=True)
  torch.save({'dirs': {}, 'config': state['config'], 'weights': state['weights'], 'optimizer': {}, 'training_step': 42},
             str(saves / '42'))
  return str(saves) + os.sep


def test_cli(tmp_path):
  from model_based_rl_amd import evaluate
  from model_based_rl_amd.config import get_evaluation_args
  saves = _checkpoint(tmp_path)
  out = tmp_path / 'summary.json'
  argv = ['--saves_dir', saves, '--nets', '42', '--num_games', '64', '--random_opp', '-1', '--seed', '0', '--batch', '16',
          '--out', str(out)]
  res = evaluate.main(argv + ['--device_env'])
  js = json.load(open(str(out)))
  assert len(js['configurations']) == 1 == len(res)
  c = js['configurations'][0]
  assert c['num_games'] == 64 and c['wins'] + c['draws'] + c['losses'] == 64
  assert set(('length', 'return', 'pred_return', 'pred_value', 'mcts_value', 'search_depth', 'games_per_s', 'host_share')) <= set(c)
  # the same invocation with and without --device_env, T = 0, the draws injected through play_games: the same three counts
  draws = make_draws(np.random.RandomState(9), 64, 9, 1, 9, OPP_NMIN['TicTacToe'])
  counts = {}
  for flag in ([], ['--device_env']):
    (state,) = list(evaluate.state_generator(get_evaluation_args(argv + flag)))
    ev = evaluate.Evaluator(state)
    ev.load_network()
    games = ev.play_games(64, list(range(64)), draws=draws)
    assert isinstance(games[0], evaluate.DeviceGame) == bool(flag)
    r = np.array([evaluate.game_return(g) for g in games])
    counts[bool(flag)] = (int((r > 0).sum()), int((r == 0).sum()), int((r < 0).sum()))
  assert counts[False] == counts[True] and sum(counts[True]) == 64, counts
