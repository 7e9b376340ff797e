"""The exact game solver on the host (mz_solve_host, the __host__ side of csrc/mz_solve.hip.h) against a Python minimax
written on the rules of tests/playout_py.py, and solver.grade_games on hand-written game records.  No GPU.

The solver's rules are bitboards, a second form beside mz_ttt_step / mz_c4_step: test_ttt_every_position and
test_c4_endgames are what pins them against the first form."""
import types

import numpy as np
import pytest

from tests import playout_util as pu
from tests import solve_util as su


def test_ttt_every_position():
  positions = su.ttt_positions()
  assert len(positions) == 4520
  bd, turn, step = positions[0]
  assert not any(bd) and turn == 1 and step == 0
  values, nodes = su.host_reference('ttt')
  ref = su.reference('ttt')
  assert values.shape == ref.shape == (4520, 9)
  assert np.array_equal(values, ref)
  assert np.array_equal(values[0], np.zeros(9, np.int8))      # the start: every first move draws
  assert np.all((nodes > 0) == (values != -2)) and nodes.max() < su.BUDGET


def test_c4_endgames():
  positions = su.c4_endgames()
  assert len(positions) == 206 and all(6 <= 42 - p[2] <= 12 for p in positions[:200])
  values, nodes = su.host_reference('c4_endgames')
  assert not np.any(values == -3)      # the budget leaves nothing unsolved
  assert np.array_equal(values, su.reference('c4_endgames'))
  assert set(np.unique(values)) == {-2, -1, 0, 1}
  assert np.all((nodes > 0) == (values != -2)) and nodes.max() < su.BUDGET


def test_budget():
  bd, turn, step = pu.ttt('... ... ...')
  values, nodes = su.host_solve(1, *pu.arrays([(bd, turn, step)]), max_nodes=8)
  assert np.array_equal(values, np.full((1, 9), -3, np.int8))
  assert np.array_equal(nodes, np.full((1, 9), 8, np.uint32))
  bd, turn, step = pu.ttt('XO. ... ...')
  values, nodes = su.host_solve(1, *pu.arrays([(bd, turn, step)]), max_nodes=8)
  assert np.array_equal(values[0, :2], [-2, -2]) and np.array_equal(nodes[0, :2], [0, 0])
  assert np.all(values[0, 2:] == -3) and np.all(nodes[0, 2:] == 8)
  # a win at once costs one node whatever the budget, and one refuted action is settled beside the cut ones
  bd, turn, step = pu.ttt('XX. OO. ...')
  values, nodes = su.host_solve(1, *pu.arrays([(bd, turn, step)]), max_nodes=1)
  assert values[0, 2] == 1 and nodes[0, 2] == 1
  assert values[0, 6] == -1 and nodes[0, 6] == 1      # O answers with its own line at once
  full = su.host_solve(1, *pu.arrays([(bd, turn, step)]))[0]
  assert np.array_equal(full[0], [-2, -2, 1, -2, -2, 0, -1, -1, -1])      # 2 wins, 5 blocks and draws, the rest lose to 5
  assert np.array_equal(full[0], su.action_values(1, bd, turn))


def test_refusals():
  ok = pu.ttt('XO. ... ...')
  with pytest.raises(RuntimeError, match='finished line'):
    su.host_solve(1, *pu.arrays([ok, pu.ttt('XXX OO. ...', turn=-1)]))
  bd, turn, step = pu.c4('XXXX', 'OOO', '', '', '', '', '')
  with pytest.raises(RuntimeError, match='position 0 already holds a finished line'):
    su.host_solve(3, *pu.arrays([(bd, turn, step)]))
  with pytest.raises(RuntimeError, match='step 3 but 2 stones'):
    su.host_solve(1, *pu.arrays([(ok[0], ok[1], 3)]))
  with pytest.raises(RuntimeError, match='kind must be 1'):
    su.host_solve(2, *pu.arrays([ok]), A=9)
  with pytest.raises(RuntimeError, match='max_nodes'):
    su.host_solve(1, *pu.arrays([ok]), max_nodes=0)


# ---- solver.grade_games on hand-written records

class MinimaxEngine(object):
  """solve() by the Python minimax; `cut`: (board tuple, action) pairs reported as not solved"""

  def __init__(self, cut=()):
    self.cut = set(cut)

  def solve(self, kind, boards, turn, step, max_nodes=0):
    values = np.array([su.action_values(kind, [int(x) for x in bd], int(t)) for bd, t in zip(boards, turn)], np.int8)
    for i, bd in enumerate(boards):
      for a in range(values.shape[1]):
        if (tuple(int(x) for x in bd[:9]), a) in self.cut:
          values[i, a] = -3
    return values, np.ones(values.shape, np.uint32)


def _game(actions, root_values, pred_values):
  h = types.SimpleNamespace(actions=list(actions), root_values=list(root_values))
  return types.SimpleNamespace(history=h, pred_values=list(pred_values), step=len(actions))


# X: 0 (draws), O: 3 (against a corner only the centre draws: a loss), X: 1 (keeps the win: O must block at 2), O: 4 (lost
# either way), X: 8 -- X had two in the top row with cell 2 empty, one move from a win, and throws it: O completes 3-4-5 by 5.
# The stored values are the mover's view: before X's third move (ply 4) the true value is +1, before O's last (ply 5) +1 too.
THROWN = _game([0, 3, 1, 4, 8, 5], [0.0, 0.0, 0.5, -0.5, 0.75, 0.25], [0.0, 0.0, 0.25, -0.25, -0.5, 1.0])
# every move keeps the draw
PERFECT = _game([4, 0, 2, 6, 3, 5, 1, 7, 8], [0.0] * 9, [0.125] * 9)
# X: 4, O: 1 (an edge against the centre loses), X: 0 (keeps the win), O: 8 (the forced block), X: 2 (3 or 6 made two
# threats and won; 2 makes one, which O blocks: win to draw)
UNSOLVED = _game([4, 1, 0, 8, 2], [0.0, 0.0, 1.0, -1.0, 1.0], [0.0] * 5)


def test_grade_games_by_hand():
  from model_based_rl_amd import solver
  eng = MinimaxEngine()
  # the positions are rebuilt on envs.py and carry the mover
  pos = solver.positions_of([THROWN], 'TicTacToe')
  assert list(pos['turn']) == [1, -1, 1, -1, 1, -1] and list(pos['step']) == list(range(6)) and list(pos['action']) == THROWN.history.actions
  assert list(pos['boards'][4][:9]) == [1, 1, 0, -1, -1, 0, 0, 0, 0]
  # the values by the minimax agree with the story above
  vals = [su.action_values(1, [int(x) for x in pos['boards'][k]], int(pos['turn'][k])) for k in range(6)]
  assert max(vals[4]) == 1 and vals[4][2] == 1 and vals[4][8] == -1      # one move from a win, thrown to a loss
  best = [max(v) for v in vals]
  chosen = [vals[k][THROWN.history.actions[k]] for k in range(6)]
  assert best == [0, 0, 1, -1, 1, 1] and chosen == [0, -1, 1, -1, -1, 1]
  # X's moves (seat +1): plies 0, 2 and 4; the win thrown at ply 4
  r = solver.grade_games([THROWN], 'TicTacToe', eng, graded_seat=1)
  assert (r['graded'], r['unsolved'], r['optimal'], r['optimal_rate']) == (3, 0, 2, 2 / 3)
  assert r['blunders'] == dict(win_to_draw=0, win_to_loss=1, draw_to_loss=0)
  # the perspective: the stored values are the mover's view, as v* is.  Ply 4, one move from a win: v* = +1, root 0.75, pred -0.5
  assert r['root_value_mae'] == pytest.approx((0.0 + 0.5 + 0.25) / 3, abs=1e-15)
  assert r['pred_value_mae'] == pytest.approx((0.0 + 0.75 + 1.5) / 3, abs=1e-15)
  assert (r['decisive'], r['root_value_sign'], r['pred_value_sign']) == (2, 1.0, 0.5)
  # O's moves (seat -1): plies 1, 3, 5.  At ply 5 O is one move from a win: +1 in O's view (the first player's view would
  # be -1), against which the stored 0.25 errs by 0.75 and has the right sign; at ply 3 O is lost, -1, and -0.5 has it too
  r = solver.grade_games([THROWN], 'TicTacToe', eng, graded_seat=-1)
  assert (r['graded'], r['optimal']) == (3, 2) and r['blunders'] == dict(win_to_draw=0, win_to_loss=0, draw_to_loss=1)
  assert r['root_value_mae'] == pytest.approx((0.0 + 0.5 + 0.75) / 3, abs=1e-15)
  assert r['pred_value_mae'] == pytest.approx((0.0 + 0.75 + 0.0) / 3, abs=1e-15)
  assert (r['decisive'], r['root_value_sign'], r['pred_value_sign']) == (2, 1.0, 1.0)

  r = solver.grade_games([PERFECT], 'TicTacToe', eng)
  assert (r['graded'], r['unsolved'], r['optimal'], r['optimal_rate']) == (9, 0, 9, 1.0)
  assert r['blunders'] == dict(win_to_draw=0, win_to_loss=0, draw_to_loss=0)
  assert r['root_value_mae'] == 0.0 and r['pred_value_mae'] == 0.125 and r['decisive'] == 0 and r['root_value_sign'] is None

  # an unsolved decision is counted, not dropped: at UNSOLVED's ply 2 the chosen action is cut; at ply 4 another action
  # is cut but a winning one is solved, so v* = +1 stands and the decision is graded
  p = solver.positions_of([UNSOLVED], 'TicTacToe')
  cut = [(tuple(int(x) for x in p['boards'][2][:9]), 0), (tuple(int(x) for x in p['boards'][4][:9]), 3)]
  full = solver.grade_games([UNSOLVED], 'TicTacToe', MinimaxEngine(), graded_seat=1)
  r = solver.grade_games([UNSOLVED], 'TicTacToe', MinimaxEngine(cut), graded_seat=1)
  assert (full['graded'], full['unsolved'], full['optimal']) == (3, 0, 2)
  assert full['blunders'] == dict(win_to_draw=1, win_to_loss=0, draw_to_loss=0)
  assert (r['graded'], r['unsolved'], r['optimal']) == (2, 1, 1)
  assert r['blunders'] == dict(win_to_draw=1, win_to_loss=0, draw_to_loss=0)
  # an action other than the chosen one cut where no solved action wins: v* is not known, the decision is left out
  r = solver.grade_games([UNSOLVED], 'TicTacToe', MinimaxEngine([((0,) * 9, 8)]), graded_seat=1)
  assert (r['graded'], r['unsolved'], r['optimal']) == (2, 1, 1)
  # all three together, both seats; max_empties keeps the late positions only
  r = solver.grade_games([THROWN, PERFECT, UNSOLVED], 'TicTacToe', eng)
  assert r['graded'] == 6 + 9 + 5 and r['unsolved'] == 0
  r = solver.grade_games([THROWN, PERFECT, UNSOLVED], 'TicTacToe', eng, max_empties=5)
  assert r['graded'] == 2 + 5 + 1 and r['max_empties'] == 5
  # the block the CLI prints: the counts as they are, 'n/a' where a rate has nothing under it
  text = solver.format_report(r, 'net:0')
  assert 'label: (net:0)' in text and '8 decisions (positions with at most 5 empty cells), 0 left out as unsolved' in text
  assert 'n/a' in solver.format_report(solver.grade_games([], 'TicTacToe', eng))


def test_refuse_grade():
  from model_based_rl_amd.evaluate import refuse_grade
  ok = dict(grade=True, device_env=True, environment='ConnectFour', apply_mcts_actions=1)
  refuse_grade(types.SimpleNamespace(**ok))
  refuse_grade(types.SimpleNamespace(**dict(ok, grade=False, device_env=False, environment='CartPole-v0')))
  for change, match in ((dict(device_env=False), False), (dict(environment='CartPole-v0'), False),
                        (dict(apply_mcts_actions=[1, 2]), False), ({}, True)):
    with pytest.raises(NotImplementedError) as err:
      refuse_grade(types.SimpleNamespace(**dict(ok, **change)), match=match)
    msg = str(err.value)
    assert msg.startswith('--grade: ') and msg.count('.') == 1 and msg.endswith('.')
