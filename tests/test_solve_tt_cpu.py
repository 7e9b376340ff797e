"""The table search of the exact solver on the host (mz_solve_tt_host, the __host__ side of sv_unit_tt in
csrc/mz_solve.hip.h; DESIGN s7f, "The table search").  No GPU.
  truth     the values equal the Python minimax on the first form of the rules: every TicTacToe position, the Connect Four
            endgames and the mixed depths, every action
  deep      at 16 to 20 empty cells the values equal the PLAIN host hook's at 2^24 nodes a unit
  fewer     the point of the search: far fewer nodes than the plain one
  budget    a small budget cuts some units, counts saturate there, and what is solved is true
  alone     a unit sees only its own table entries: reordering the list or solving a position alone changes nothing
  flags     --grade_table without --grade is refused; grade_games(table=True) asks the engine for the table search"""
import types

import numpy as np
import pytest

from tests import playout_util as pu
from tests import solve_tt_util as tu
from tests import solve_util as su
from tests.test_solve_cpu import PERFECT, THROWN, UNSOLVED, MinimaxEngine

SMALL = 256


@pytest.mark.parametrize('name,n', [('ttt', 4520), ('c4_endgames', 206), ('c4_mixed', 70)])
def test_truth(name, n):
  values, nodes = tu.host_reference_tt(name)
  ref = su.reference(name)
  assert values.shape == ref.shape == (n, su.A_OF[tu.POSITIONS[name][0]]) and values.dtype == np.int8 and nodes.dtype == np.uint32
  assert not np.any(values == -3)
  assert np.array_equal(values, ref)
  assert np.all((nodes > 0) == (values != -2)) and nodes.max() < su.BUDGET


def test_deep():
  positions = tu.c4_deep()
  assert len(positions) == 64 and {42 - p[2] for p in positions} == {16, 17, 18, 19, 20}
  truth, plain_nodes = tu.deep_truth()
  assert not np.any(truth == -3) and plain_nodes.max() < tu.DEEP_PLAIN_BUDGET      # the seed's choice: the plain search solves them all
  values, nodes = tu.host_reference_tt('c4_deep', tu.DEEP_BUDGET)
  assert not np.any(values == -3)
  assert np.array_equal(values, truth)
  assert set(np.unique(values)) == {-2, -1, 0, 1}
  assert np.all((nodes > 0) == (values != -2)) and nodes.max() < tu.DEEP_BUDGET


def test_fewer_nodes():
  total = lambda nodes: int(np.asarray(nodes, np.uint64).sum())
  plain = total(su.host_reference('c4_endgames')[1]) + total(su.host_reference('c4_mixed')[1])
  table = total(tu.host_reference_tt('c4_endgames')[1]) + total(tu.host_reference_tt('c4_mixed')[1])
  deep_plain, deep_table = total(tu.deep_truth()[1]), total(tu.host_reference_tt('c4_deep', tu.DEEP_BUDGET)[1])
  print('nodes, plain / table: endgames + mixed %d / %d, deep %d / %d' % (plain, table, deep_plain, deep_table))
  assert table < plain
  assert 4 * deep_table < deep_plain


def test_small_budget():
  values, nodes = tu.host_reference_tt('c4_deep', SMALL)
  cut = values == -3
  assert np.any(cut) and np.any(values >= -1)      # both kinds of unit occur
  assert np.all(nodes[cut] == SMALL) and nodes.max() == SMALL
  truth = tu.deep_truth()[0]
  assert np.array_equal(values[~cut], truth[~cut])
  # what is solved costs what it cost at the large budget: the budget cuts a search, it does not change one
  assert np.array_equal(nodes[~cut], tu.host_reference_tt('c4_deep', tu.DEEP_BUDGET)[1][~cut])


@pytest.mark.parametrize('name,budget', [('c4_deep', tu.DEEP_BUDGET), ('c4_deep', SMALL), ('c4_mixed', su.BUDGET)])
def test_unit_alone(name, budget):
  kind, positions = tu.POSITIONS[name]
  bd, tn, st = pu.arrays(positions())
  values, nodes = tu.host_reference_tt(name, budget)
  rv, rn = tu.host_solve_tt(kind, bd[::-1], tn[::-1], st[::-1], max_nodes=budget)
  assert np.array_equal(rv[::-1], values) and np.array_equal(rn[::-1], nodes)
  for i in range(len(bd)):
    v, n = tu.host_solve_tt(kind, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], max_nodes=budget)
    assert np.array_equal(v[0], values[i]) and np.array_equal(n[0], nodes[i]), i


def test_generation_wrap_on_the_host():
  """the TicTacToe list is 40680 units on the hook's one table: its counter wraps 19 times, and test_truth holds the values.
  Here: the list twice in one call (the second half meets a table the first half filled) equals the list once"""
  bd, tn, st = pu.arrays(su.ttt_positions())
  values, nodes = tu.host_reference_tt('ttt')
  assert values.size > 19 * tu.GEN_WRAP
  v2, n2 = tu.host_solve_tt(1, np.concatenate([bd, bd]), np.concatenate([tn, tn]), np.concatenate([st, st]))
  assert np.array_equal(v2, np.concatenate([values, values])) and np.array_equal(n2, np.concatenate([nodes, nodes]))


def test_refusals():
  ok = pu.ttt('XO. ... ...')
  with pytest.raises(RuntimeError, match='mz_solve_tt_host: position 1 already holds a finished line'):
    tu.host_solve_tt(1, *pu.arrays([ok, pu.ttt('XXX OO. ...', turn=-1)]))
  with pytest.raises(RuntimeError, match='max_nodes'):
    tu.host_solve_tt(1, *pu.arrays([ok]), max_nodes=0)


def test_refuse_grade_table():
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import refuse_grade
  ok = dict(grade=True, grade_table=True, device_env=True, environment='ConnectFour', apply_mcts_actions=1)
  refuse_grade(types.SimpleNamespace(**ok))
  refuse_grade(types.SimpleNamespace(**dict(ok, grade=False, grade_table=False)))
  with pytest.raises(NotImplementedError) as err:
    refuse_grade(types.SimpleNamespace(**dict(ok, grade=False)))
  msg = str(err.value)
  assert msg.startswith('--grade_table: ') and msg.count('.') == 1 and msg.endswith('.')
  # with --grade the sentences are --grade's own
  with pytest.raises(NotImplementedError, match='^--grade: '):
    refuse_grade(types.SimpleNamespace(**dict(ok, device_env=False)))
  # the flag changes no default
  args = get_evaluation_args(['--saves_dir', 'x', '--device_env', '--grade', '--grade_table'])
  assert args.grade_table and args.grade_empties == 12 and args.grade_nodes == 4096
  assert not get_evaluation_args(['--saves_dir', 'x']).grade_table


class TableEngine(MinimaxEngine):
  """the stub of test_solve_cpu.py, recording what solve() was asked for"""

  def __init__(self):
    MinimaxEngine.__init__(self)
    self.asked = []

  def solve(self, kind, boards, turn, step, max_nodes=0, **kw):
    self.asked.append(kw)
    return MinimaxEngine.solve(self, kind, boards, turn, step, max_nodes=max_nodes)


def test_grade_games_table():
  from model_based_rl_amd import solver
  games = [THROWN, PERFECT, UNSOLVED]
  eng = TableEngine()
  plain = solver.grade_games(games, 'TicTacToe', eng)
  table = solver.grade_games(games, 'TicTacToe', eng, table=True)
  assert eng.asked == [{}, dict(table=True)]      # the plain call is the call it was
  assert 'solver' not in plain and table['solver'] == 'table'
  assert {k: v for k, v in table.items() if k != 'solver'} == plain
  assert table['graded'] == 6 + 9 + 5 and table['unsolved'] == 0
  r = solver.grade_games([THROWN], 'TicTacToe', eng, graded_seat=1, table=True)
  assert (r['graded'], r['unsolved'], r['optimal'], r['optimal_rate']) == (3, 0, 2, 2 / 3)
  assert r['blunders'] == dict(win_to_draw=0, win_to_loss=1, draw_to_loss=0)
  assert solver.grade_games([], 'TicTacToe', eng, table=True)['solver'] == 'table'
  # the printed block names the solver, and only then
  assert 'exact solver (table search)' in solver.format_report(table, 'net:0')
  assert 'table' not in solver.format_report(plain, 'net:0')
