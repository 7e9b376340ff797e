"""The table search of the exact solver on the device (k_solve_tt, csrc/mz_solve.hip.h; DESIGN s7f, "The table search"):
  host      Engine.solve(table=True) equals the host hook mz_solve_tt_host in values and node counts.  The tolerance is zero
            and that is derived: the same integer bodies search the same units with the same budget, and a unit sees no
            table entry but its own, so neither the lane a unit lands on nor what that lane searched before matters
  budget    at a small budget the pattern of unsolved units and the node counts are the host's too
  batch     a position solved alone gets the values and counts it got inside the batch
  wrap      every lane's generation counter crosses its wrap within a run over tables earlier runs filled
  plain     Engine.solve(table=False) on the same engine is the plain solver it was, and the evaluation games do not see
            the tables
  grade     evaluate --grade --grade_table through Evaluator.play_games: the report equals the one recomputed from the kept
            histories with the PLAIN host hook's values"""
import numpy as np
import pytest

from tests import playout_py as pp
from tests import solve_tt_util as tu
from tests import solve_util as su
from tests.eval_device_util import eval_state
from tests.playout_util import A_OF, arrays

pytestmark = pytest.mark.gpu

B = 128
SMALL = 256      # a budget at which some units are cut and some are not
BUDGET = {1: su.BUDGET, 3: tu.DEEP_BUDGET}
LISTS = {1: ('ttt',), 3: ('c4_endgames', 'c4_mixed', 'c4_deep')}


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
  """TicTacToe: all 4520; Connect Four: the 206 endgames, the 70 at mixed depths and the 64 at 16 to 20 empty cells"""
  return [p for name in LISTS[kind] for p in tu.POSITIONS[name][1]()]


def _host(kind, max_nodes):
  parts = [tu.host_reference_tt(name, max_nodes) for name in LISTS[kind]]
  return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _same(dev, host, what):
  for name, d, h in zip(('values', 'nodes'), dev, host):
    assert d.dtype == h.dtype and np.array_equal(d, h), (what, name, np.argwhere(d != h)[:5].tolist())


@pytest.mark.parametrize('kind', [1, 3])
def test_device_equals_host(kind, engines):
  """n above num_envs (the chunks: 4520 and 340 positions through a staging of 128), n = 70 (units that do not fill the
  last wave) and n = 1"""
  bd, tn, st = arrays(_positions(kind))
  host = _host(kind, BUDGET[kind])
  assert len(bd) > B and not np.any(host[0] == -3)
  eng = engines(kind)
  _same(eng.solve(kind, bd, tn, st, max_nodes=BUDGET[kind], table=True), host, (kind, 'all'))
  lo = len(bd) - 70
  _same(eng.solve(kind, bd[lo:], tn[lo:], st[lo:], max_nodes=BUDGET[kind], table=True), (host[0][lo:], host[1][lo:]), (kind, 70))
  _same(eng.solve(kind, bd[lo:lo + 1], tn[lo:lo + 1], st[lo:lo + 1], max_nodes=BUDGET[kind], table=True),
        (host[0][lo:lo + 1], host[1][lo:lo + 1]), (kind, 1))


@pytest.mark.parametrize('kind', [1, 3])
def test_small_budget(kind, engines):
  bd, tn, st = arrays(_positions(kind))
  budget = SMALL      # (TicTacToe: the largest unit of the table search is 265 nodes, so one unit is cut)
  host = _host(kind, budget)
  assert np.any(host[0] == -3) and np.any(host[0] >= -1)      # both kinds of unit occur
  assert np.all(host[1][host[0] == -3] == budget) and host[1].max() == budget
  _same(engines(kind).solve(kind, bd, tn, st, max_nodes=budget, table=True), host, (kind, budget))


@pytest.mark.parametrize('kind', [1, 3])
def test_batch_independence(kind, engines):
  bd, tn, st = arrays(_positions(kind))
  host = _host(kind, BUDGET[kind])
  for i in (0, 3, 41, len(bd) - 1):
    alone = engines(kind, 1).solve(kind, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], max_nodes=BUDGET[kind], table=True)
    _same(alone, (host[0][i:i + 1], host[1][i:i + 1]), (kind, i))


def test_generation_wrap(engines):
  """the tables hold the entries of a run from generation 1 on; the counters are then set three units before the wrap, and
  the TicTacToe list gives every lane of its 18 waves at least 35 units: each crosses the wrap, clears its table, and goes
  through the generations the first run left entries of.  A lane that did not clear would meet them"""
  from model_based_rl_amd import _abi
  eng = engines(1)
  bd, tn, st = arrays(su.ttt_positions())
  host = _host(1, su.BUDGET)
  assert len(bd) * 9 // (B * 9) >= 35
  _same(eng.solve(1, bd, tn, st, max_nodes=su.BUDGET, table=True), host, 'before the wrap')
  _abi.check(eng.lib.mz_solve_tt_set_generation(eng._h, tu.GEN_WRAP - 3), 'mz_solve_tt_set_generation')
  _same(eng.solve(1, bd, tn, st, max_nodes=su.BUDGET, table=True), host, 'across the wrap')
  _same(eng.solve(1, bd, tn, st, max_nodes=su.BUDGET, table=True), host, 'after the wrap')
  with pytest.raises(RuntimeError, match='generation must be in 0 .. 2047'):
    _abi.check(eng.lib.mz_solve_tt_set_generation(eng._h, tu.GEN_WRAP), 'mz_solve_tt_set_generation')


@pytest.mark.parametrize('kind', [1, 3])
def test_plain_untouched(kind, engines):
  """after table solves the plain entry gives the plain search's values and node counts, and the other way round"""
  names = ('ttt',) if kind == 1 else ('c4_endgames', 'c4_mixed')
  positions = [p for name in names for p in tu.POSITIONS[name][1]()]
  bd, tn, st = arrays(positions)
  plain = [su.host_reference(name) for name in names]
  plain = (np.concatenate([p[0] for p in plain]), np.concatenate([p[1] for p in plain]))
  table = [tu.host_reference_tt(name) for name in names]
  table = (np.concatenate([p[0] for p in table]), np.concatenate([p[1] for p in table]))
  eng = engines(kind)
  _same(eng.solve(kind, bd, tn, st, max_nodes=su.BUDGET, table=True), table, (kind, 'table'))
  _same(eng.solve(kind, bd, tn, st, max_nodes=su.BUDGET), plain, (kind, 'plain after table'))
  _same(eng.solve(kind, bd, tn, st, max_nodes=su.BUDGET, table=False), plain, (kind, 'plain, table=False'))
  _same(eng.solve(kind, bd, tn, st, max_nodes=su.BUDGET, table=True), table, (kind, 'table after plain'))


def test_table_state_is_its_own():
  """two engines play the same evaluation games; one of them runs table solves before the reset and between the chunks of
  moves.  Their records are equal"""
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.evaluate import flatten_weights
  state = eval_state('ConnectFour', sims=6)
  bd, tn, st = arrays(su.c4_mixed())
  host = tu.host_reference_tt('c4_mixed')
  results = []
  for solving in (False, True):
    eng = Engine.from_config(state['config'], 16, device='cuda:0', seed=0, env_id_offset=40)
    try:
      eng.set_weights(flatten_weights(state['weights']))
      if solving:
        _same(eng.solve(3, bd, tn, st, max_nodes=su.BUDGET, table=True), host, 'before the reset')
      eng.eval_env_reset('ConnectFour', 42, 0, None, True)
      live, chunks = 16, 0
      while live > 0 and chunks < 6:
        live = eng.eval_env_moves(8, 0, 1, 0.0, False)
        chunks += 1
        if solving:
          _same(eng.solve(3, bd, tn, st, max_nodes=su.BUDGET, table=True), host, 'between chunks')
      assert live == 0
      results.append(eng.eval_env_results())
    finally:
      eng.close()
  plain, solved = results
  assert set(plain) == set(solved)
  for key in plain:
    assert np.array_equal(np.asarray(plain[key]), np.asarray(solved[key])), key


def _regrade(games, max_empties):
  """the report of solver.grade_games for both sides' moves of Connect Four games, from the kept histories: positions
  replayed on playout_py's rules, values by the plain host hook at 2^24 nodes a unit (test_gpu_solve.py's method with another
  source of the truth: the Python minimax is too slow at 16 empty cells)"""
  positions, actions, root, pred = [], [], [], []
  for g in games:
    bd, mover = [0] * 42, 1
    for p, a in enumerate(g.history.actions):
      assert g.history.to_play[p] == mover
      if 42 - p <= max_empties:
        positions.append((list(bd), mover, p)); actions.append(a)
        root.append(g.history.root_values[p]); pred.append(g.pred_values[p])
      end = pp.play(3, bd, mover, a)
      assert (end != 0) == (p == g.step - 1)
      mover = -mover
  values = su.host_solve(3, *arrays(positions), max_nodes=tu.DEEP_PLAIN_BUDGET)[0].astype(np.int64)
  assert not np.any(values == -3)
  best, chosen = values.max(1), values[np.arange(len(actions)), actions]
  root, pred = np.array(root, np.float64), np.array(pred, np.float64)
  dec = best != 0
  return dict(graded=len(best), unsolved=0, optimal=int((best == chosen).sum()),
              blunders=dict(win_to_draw=int(((best == 1) & (chosen == 0)).sum()), win_to_loss=int(((best == 1) & (chosen == -1)).sum()),
                            draw_to_loss=int(((best == 0) & (chosen == -1)).sum())),
              decisive=int(dec.sum()), root_value_mae=float(np.abs(root - best).mean()), pred_value_mae=float(np.abs(pred - best).mean()),
              root_value_sign=float((np.sign(root[dec]) == best[dec]).mean()), pred_value_sign=float((np.sign(pred[dec]) == best[dec]).mean()))


def test_graded_games():
  """untrained weights, 10 simulations, both sides the network, sampling: 32 different games graded from 16 empty cells on"""
  from model_based_rl_amd.evaluate import Evaluator
  n_games, empties = 32, 16
  state = eval_state('ConnectFour', sims=10, grade=True, grade_table=True, grade_empties=empties, grade_nodes=1 << 20, temperature=1.0)
  ev = Evaluator(state)
  ev.load_network()
  games = ev.play_games(n_games, list(range(500, 500 + n_games)), device_env=True)
  assert all(g.history is not None for g in games)
  assert len({tuple(g.history.actions) for g in games}) > n_games // 2
  got, want = ev.grade_report, _regrade(games, empties)
  print(got)
  assert want['graded'] > 0 and got['max_empties'] == empties and got['solver'] == 'table'
  assert got['unsolved'] == 0
  for key in ('graded', 'unsolved', 'optimal', 'blunders', 'decisive'):
    assert got[key] == want[key], key
  assert got['optimal_rate'] == want['optimal'] / want['graded']
  for key in ('root_value_mae', 'pred_value_mae', 'root_value_sign', 'pred_value_sign'):
    assert abs(got[key] - want[key]) <= 1e-12, key
