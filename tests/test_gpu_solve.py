"""The exact game solver on the device (csrc/mz_solve.hip.h, DESIGN s7f):
  host      Engine.solve equals the host hook mz_solve_host in values and node counts.  The tolerance is zero and that is
            derived: the same integer bodies search the same units in the same order with the same budget; only the
            distribution of the units over the lanes differs
  budget    at a small budget the pattern of unsolved units and the node counts are the host's too
  batch     a position solved alone gets the values it got inside the batch
  grade     evaluate --grade through Evaluator.play_games: the report equals the one recomputed from the kept histories with
            the Python minimax of tests/solve_util.py
  state     the solver's state is its own: an engine that solved positions plays the evaluation games it played without"""
import numpy as np
import pytest

from tests import playout_py as pp
from tests import solve_util as su
from tests.eval_device_util import eval_state
from tests.playout_util import A_OF, arrays

pytestmark = pytest.mark.gpu

B = 128
SMALL = 256      # a budget at which some units are cut and some are not


@pytest.fixture(scope='module')
def engines():
  from model_based_rl_amd.engine import Engine
  made = {}

  def get(kind, num_envs=B):
    if (kind, num_envs) not in made:
      made[(kind, num_envs)] = Engine(num_envs, 9 if kind == 1 else 42, A_OF[kind], 4, two_players=True, known_bounds=(-1, 1),
                                      discount=1.0, seed=0, device='cuda:0')
    return made[(kind, num_envs)]
  yield get
  for e in made.values():
    e.close()


def _positions(kind):
  """TicTacToe: all 4520; Connect Four: the CPU test's 206 and 70 at mixed depths up to 14 empty cells"""
  return su.ttt_positions() if kind == 1 else su.c4_endgames() + su.c4_mixed()


def _host(kind, max_nodes):
  if kind == 1:
    return su.host_reference('ttt', max_nodes)
  a, b = su.host_reference('c4_endgames', max_nodes), su.host_reference('c4_mixed', max_nodes)
  return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def _same(dev, host, what):
  for name, d, h in zip(('values', 'nodes'), dev, host):
    assert d.dtype == h.dtype and np.array_equal(d, h), (what, name, np.argwhere(d != h)[:5].tolist())


@pytest.mark.parametrize('kind', [1, 3])
def test_device_equals_host(kind, engines):
  """n above num_envs (the chunks: 4520 and 276 positions through a staging of 128), n = 70 (units that do not fill the
  last wave) and n = 1"""
  bd, tn, st = arrays(_positions(kind))
  host = _host(kind, su.BUDGET)
  assert len(bd) > B and not np.any(host[0] == -3)
  _same(engines(kind).solve(kind, bd, tn, st, max_nodes=su.BUDGET), host, (kind, 'all'))
  lo = len(bd) - 70
  _same(engines(kind).solve(kind, bd[lo:], tn[lo:], st[lo:], max_nodes=su.BUDGET), (host[0][lo:], host[1][lo:]), (kind, 70))
  _same(engines(kind).solve(kind, bd[lo:lo + 1], tn[lo:lo + 1], st[lo:lo + 1], max_nodes=su.BUDGET),
        (host[0][lo:lo + 1], host[1][lo:lo + 1]), (kind, 1))
  if kind == 1:
    assert np.array_equal(host[0][0], np.zeros(9, np.int8))      # the start position first, all draws


@pytest.mark.parametrize('kind', [1, 3])
def test_small_budget(kind, engines):
  bd, tn, st = arrays(_positions(kind))
  host = _host(kind, SMALL)
  assert np.any(host[0] == -3) and np.any(host[0] >= -1)      # both kinds of unit occur
  assert np.all(host[1][host[0] == -3] == SMALL) and host[1].max() == SMALL
  _same(engines(kind).solve(kind, bd, tn, st, max_nodes=SMALL), host, (kind, SMALL))


@pytest.mark.parametrize('kind', [1, 3])
def test_batch_independence(kind, engines):
  bd, tn, st = arrays(_positions(kind))
  host = _host(kind, su.BUDGET)
  for i in (0, 3, 41, len(bd) - 1):
    alone = engines(kind, 1).solve(kind, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], max_nodes=su.BUDGET)
    _same(alone, (host[0][i:i + 1], host[1][i:i + 1]), (kind, i))


def test_refusals(engines):
  bd, tn, st = arrays(su.ttt_positions()[:4])
  with pytest.raises(RuntimeError, match='Connect Four needs'):
    engines(1).solve(3, bd, tn, st)
  with pytest.raises(RuntimeError, match='kind must be 1'):
    engines(1).solve(2, bd, tn, st)
  over = bd.copy()
  over[1, :3] = 1
  with pytest.raises(RuntimeError, match='position 1'):
    engines(1).solve(1, over, tn, st)


def _regrade(games, kind, max_empties, seat):
  """the report of solver.grade_games for the moves of `seat` (None: both), from the kept histories: positions replayed on
  playout_py's rules, values by the Python minimax"""
  cells = 9 if kind == 1 else 42
  best, chosen, root, pred = [], [], [], []
  for g in games:
    bd, mover = [0] * 42, 1
    for p, a in enumerate(g.history.actions):
      assert g.history.to_play[p] == mover
      if (max_empties is None or cells - p <= max_empties) and seat in (None, mover):
        v = su.action_values(kind, bd, mover)
        best.append(max(v)); chosen.append(v[a]); root.append(g.history.root_values[p]); pred.append(g.pred_values[p])
      end = pp.play(kind, bd, mover, a)
      assert (end != 0) == (p == g.step - 1)
      mover = -mover
  best, chosen = np.array(best), np.array(chosen)
  root, pred = np.array(root, np.float64), np.array(pred, np.float64)
  dec = best != 0
  return dict(graded=len(best), unsolved=0, optimal=int((best == chosen).sum()),
              blunders=dict(win_to_draw=int(((best == 1) & (chosen == 0)).sum()), win_to_loss=int(((best == 1) & (chosen == -1)).sum()),
                            draw_to_loss=int(((best == 0) & (chosen == -1)).sum())),
              decisive=int(dec.sum()), root_value_mae=float(np.abs(root - best).mean()), pred_value_mae=float(np.abs(pred - best).mean()),
              root_value_sign=float((np.sign(root[dec]) == best[dec]).mean()), pred_value_sign=float((np.sign(pred[dec]) == best[dec]).mean()))


@pytest.mark.parametrize('env_name,kind,n_games,empties,over', [
    ('TicTacToe', 1, 64, None, dict(random_opp=-1)),      # the network moves first against the random mover: its moves are graded
    ('ConnectFour', 3, 32, 10, dict(temperature=1.0)),    # both sides the network, sampling: both sides' moves are graded
])
def test_graded_games(env_name, kind, n_games, empties, over):
  """untrained weights, 10 simulations; without an opponent or a temperature every game of a run would be the same game"""
  from model_based_rl_amd.evaluate import Evaluator
  state = eval_state(env_name, sims=10, grade=True, grade_empties=empties if empties is not None else 14, grade_nodes=1 << 20, **over)
  ev = Evaluator(state)
  ev.load_network()
  games = ev.play_games(n_games, list(range(500, 500 + n_games)), device_env=True)
  assert all(g.history is not None for g in games)      # --grade keeps the histories itself
  assert len({tuple(g.history.actions) for g in games}) > n_games // 2
  seat = -over['random_opp'] if 'random_opp' in over else None
  got, want = ev.grade_report, _regrade(games, kind, empties, seat)
  print(got)
  assert want['graded'] > 0 and got['max_empties'] == empties
  for key in ('graded', 'unsolved', 'optimal', 'blunders', 'decisive'):
    assert got[key] == want[key], key
  assert got['optimal_rate'] == want['optimal'] / want['graded']
  for key in ('root_value_mae', 'pred_value_mae', 'root_value_sign', 'pred_value_sign'):
    assert abs(got[key] - want[key]) <= 1e-12, key


def test_solver_state_is_its_own():
  """two engines play the same evaluation games; one of them solves positions before the reset and between the chunks of
  moves.  Their records are equal"""
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.evaluate import flatten_weights
  state = eval_state('ConnectFour', sims=6)
  bd, tn, st = arrays(su.c4_mixed())
  host = su.host_reference('c4_mixed')
  results = []
  for solving in (False, True):
    eng = Engine.from_config(state['config'], 16, device='cuda:0', seed=0, env_id_offset=40)
    try:
      eng.set_weights(flatten_weights(state['weights']))
      if solving:
        _same(eng.solve(3, bd, tn, st, max_nodes=su.BUDGET), host, 'before the reset')
      eng.eval_env_reset('ConnectFour', 42, 0, None, True)
      live, chunks = 16, 0
      while live > 0 and chunks < 6:
        live = eng.eval_env_moves(8, 0, 1, 0.0, False)
        chunks += 1
        if solving:
          _same(eng.solve(3, bd, tn, st, max_nodes=su.BUDGET), host, 'between chunks')
      assert live == 0
      results.append(eng.eval_env_results())
    finally:
      eng.close()
  plain, solved = results
  assert set(plain) == set(solved)
  for key in plain:
    assert np.array_equal(np.asarray(plain[key]), np.asarray(solved[key])), key
