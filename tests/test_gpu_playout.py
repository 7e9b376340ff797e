"""The playout-search opponent on the device (csrc/mz_playout.hip.h, DESIGN s7d):
  host      Engine.playout_plan equals the host hook mz_playout_plan_host bit for bit in action, visits and wins.  The
            tolerance is zero and that is derived: every quantity is an integer or an exactly rounded float64 operation on
            integers, with the table of logarithms computed on the host for both
  batch     a position planned alone under its own game id gets the plan it got inside the batch
  games     evaluation games against the planner through Evaluator.play_games, replayed on the host classes: every
            opponent move is the hook's plan for that position, game seed and move, and the host stepped no game
  state     the planner's state is its own: a plan on an engine whose evaluation games have no playout opponent"""
import math

import numpy as np
import pytest
import torch

from tests.eval_device_util import eval_state
from tests.playout_util import A_OF, arrays, host_plan, random_position, shared_positions

pytestmark = pytest.mark.gpu

B, OFFSET, SEED = 128, 1000, 6
N_POSITIONS = 70      # 17 blocks of four waves and one of two: the last block of waves is partly empty


@pytest.fixture(scope='module')
def positions():
  """{kind: 70 positions}: the CPU test's and random ones of every depth"""
  rng = np.random.RandomState(77)
  out = shared_positions()
  for kind, longest in ((1, 9), (3, 42)):
    while len(out[kind]) < N_POSITIONS:
      out[kind].append(random_position(kind, int(rng.randint(0, longest - 1)), rng))
    assert len(out[kind]) == N_POSITIONS
  return out


@pytest.fixture(scope='module')
def engines():
  from model_based_rl_amd.engine import Engine
  made = {}

  def get(kind, num_envs=B, offset=OFFSET):
    key = (kind, num_envs, offset)
    if key not in made:
      made[key] = Engine(num_envs, 9 if kind == 1 else 42, A_OF[kind], 4, two_players=True, known_bounds=(-1, 1), discount=1.0,
                         seed=SEED, env_id_offset=offset, device='cuda:0')
    return made[key]
  yield get
  for e in made.values():
    e.close()


def _same(dev, host, what):
  for name, d, h in zip(('action', 'visits', 'wins'), dev, host):
    assert np.array_equal(d, h), (what, name, np.argwhere(np.asarray(d) != np.asarray(h))[:5].tolist())


@pytest.mark.parametrize('playouts', [64, 192, 1024])
@pytest.mark.parametrize('kind', [1, 3])
def test_device_equals_host(kind, playouts, positions, engines):
  bd, tn, st = arrays(positions[kind])
  dev = engines(kind).playout_plan(kind, bd, tn, st, playouts, move=4)
  _same(dev, host_plan(kind, bd, tn, st, playouts, move=4, seed=SEED, env_id_offset=OFFSET), (kind, playouts))
  assert np.all(dev[1].sum(1) == playouts)


@pytest.mark.parametrize('playouts', [16384, 32768, 65536])
@pytest.mark.parametrize('kind', [1, 3])
def test_device_equals_host_at_the_large_budgets(kind, playouts, positions, engines):
  """the budgets at which the launch takes another shape: two waves per block (16384), one (32768), and one whose tree
  needs more dynamic LDS than the default limit (65536, the largest budget).  Five positions: a block partly empty."""
  bd, tn, st = arrays(positions[kind][::15])
  assert len(bd) == 5
  dev = engines(kind).playout_plan(kind, bd, tn, st, playouts, move=1)
  _same(dev, host_plan(kind, bd, tn, st, playouts, move=1, seed=SEED, env_id_offset=OFFSET), (kind, playouts))


@pytest.mark.parametrize('kind', [1, 3])
def test_batch_independence(kind, positions, engines):
  bd, tn, st = arrays(positions[kind])
  action, visits, wins = engines(kind).playout_plan(kind, bd, tn, st, 192, move=4)
  for i in (0, 3, 41, 69):
    alone = engines(kind, 1, OFFSET + i).playout_plan(kind, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], 192, move=4)
    _same(alone, (action[i:i + 1], visits[i:i + 1], wins[i:i + 1]), (kind, i))


def _check_games(env_name, kind, n_games, playouts, seat):
  from model_based_rl_amd import envs
  from model_based_rl_amd.evaluate import MOVES_PER_SYNC, Evaluator
  state = eval_state(env_name, sims=6, random_opp=seat, opp_playouts=playouts)
  ev = Evaluator(state)
  ev.load_network()
  seeds = list(range(300, 300 + n_games))
  games = ev.play_games(n_games, seeds, device_env=True, keep_history=True)
  assert ev.device_syncs == math.ceil(max(g.step for g in games) / MOVES_PER_SYNC)      # one per chunk: the host stepped no game
  # replay on the host class; the positions the opponent moved in, by ply
  longest = max(g.step for g in games)
  start = ([0] * 42, 1, 0)
  asked = [[start] * n_games for _ in range(longest)]
  opp_moves = 0
  for i, g in enumerate(games):
    e = envs.TicTacToe() if kind == 1 else envs.ConnectFour()
    e.reset()
    ret, done = 0.0, False
    assert len(g.history.actions) == g.step
    for p, a in enumerate(g.history.actions):
      assert not done and a in [int(x) for x in e.legal_actions()], (i, p)
      mover = e.turn
      assert g.history.to_play[p] == mover
      if mover == seat:
        asked[p][i] = ([int(x) for x in e.board] + [0] * (42 - len(e.board)), mover, p)
        opp_moves += 1
      _, reward, done, _ = e.step(a)
      assert g.history.rewards[p] == (-reward if done and mover == seat else reward), (i, p)
      ret += g.history.rewards[p]
    assert done and ret == g.ret and ret in (-1.0, 0.0, 1.0), i
  assert opp_moves >= n_games
  for p in range(longest):
    bd, tn, st = arrays(asked[p])
    plan = host_plan(kind, bd, tn, st, playouts, move=p, seed=0, env_id_offset=seeds[0])[0]
    for i, g in enumerate(games):
      if asked[p][i] is not start:
        assert g.history.actions[p] == plan[i], (i, p)
  return games


@pytest.mark.parametrize('seat', [-1, 1])
def test_tictactoe_games_against_the_planner(seat):
  _check_games('TicTacToe', 1, 64, 256, seat)


@pytest.mark.parametrize('seat', [-1, 1])
def test_connect_four_games_against_the_planner(seat):
  _check_games('ConnectFour', 3, 16, 128, seat)


def test_plan_without_prior_planning(positions):
  """after a reset with an opponent's seat, mz_eval_env_set_opponent(e, 0) and no planner launch, playout_plan works on the
  same engine: the planner's state is its own"""
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.evaluate import flatten_weights
  state = eval_state('TicTacToe', sims=6)
  eng = Engine.from_config(state['config'], 8, device='cuda:0', seed=SEED, env_id_offset=OFFSET)
  try:
    eng.set_weights(flatten_weights(state['weights']))
    eng.eval_env_reset('TicTacToe', 9, 0, -1, False)
    eng.eval_env_set_opponent(0)
    bd, tn, st = arrays(positions[1][:8])
    _same(eng.playout_plan(1, bd, tn, st, 192, move=2), host_plan(1, bd, tn, st, 192, move=2, seed=SEED, env_id_offset=OFFSET), 'own state')
    # ... and the games go on against the random mover, to their end
    live, chunks = 8, 0
    while live > 0 and chunks < 3:
      live = eng.eval_env_moves(8, 0, 1, 0.0, False)
      chunks += 1
    assert live == 0
    # the refusals of mz_eval_env_set_opponent: games already started; a reset without a seat; a bad budget; CartPole
    with pytest.raises(RuntimeError, match='started'):
      eng.eval_env_set_opponent(64)
    eng.eval_env_reset('TicTacToe', 9, 0, None, False)
    with pytest.raises(RuntimeError, match='seat'):
      eng.eval_env_set_opponent(64)
    eng.eval_env_reset('TicTacToe', 9, 0, 1, False)
    with pytest.raises(RuntimeError, match='multiple of 64'):
      eng.eval_env_set_opponent(100)
    eng.eval_env_set_opponent(64)
    with pytest.raises(RuntimeError, match='max_actions'):
      eng.eval_env_moves(1, 0, 2, 0.0, False)
    with pytest.raises(RuntimeError, match='kind'):
      eng.playout_plan(2, bd, tn, st, 64)
    with pytest.raises(RuntimeError, match='Connect Four needs'):
      eng.playout_plan(3, bd, tn, st, 64)
    with pytest.raises(RuntimeError, match='num_envs'):
      eng.playout_plan(1, np.concatenate([bd, bd]), np.concatenate([tn, tn]), np.concatenate([st, st]), 64)
  finally:
    eng.close()
