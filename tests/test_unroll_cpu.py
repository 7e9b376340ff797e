"""The unroll diagnostic without a GPU (DESIGN s7f, "Grading by unroll depth"):
  lines      mz_unroll_lines_host -- the __host__ __device__ body the device runs -- equals the Python restatement on the rules
             of tests/playout_py.py.  The tolerance is zero: lines are integers and float casts of -1 / 0 / +1
  terms      mz_unroll_terms_host equals the restatement: counts, top1_agree and sign outcomes exactly, masses and means within
             1e-12 -- derived: the sides differ in exp() only, a few ulp a term, over at most A + 1 terms of a quantity in [0, 1]
  report     solver.grade_unroll on a stub engine (the restatement through tests/fc64.FC64, the host solver) equals a
             plain-Python recomputation field by field
  refusals   one test per sentence, and the formatted block"""
import types

import numpy as np
import pytest

from tests import playout_py as pp
from tests import solve_util as su
from tests import unroll_util as uu
from tests.c4_positions import POSITIONS as C4_FORCED, WINS
from tests.playout_util import arrays, random_position


def _same_lines(kind, boards, turn, step, actions, what):
  got, want = uu.host_lines(kind, boards, turn, step, actions), uu.py_lines(kind, boards, turn, step, actions)
  for key in ('obs', 'legal', 'terminal', 'reward_true', 'depth', 'flags'):
    assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:5].tolist())
  return got


def _prefix_rows(kind, games, K):
  """every prefix of the games as a row with the next K actions (-1 past the game's end)"""
  return uu.rows_of(games, kind, K)[:4]


@pytest.mark.parametrize('kind,n_games,K', [(1, 300, 5), (1, 40, 16), (3, 24, 5), (3, 6, 16)])
def test_lines_of_random_games(kind, n_games, K):
  """every prefix of random games: lines that run their K plies, lines the game's end cuts short (a line that ends inside K:
  terminal p_k, padding behind it) and, at K = 16, TicTacToe lines that always end inside K"""
  bd, tn, st, ac = _prefix_rows(kind, uu.random_games(kind, n_games, 20241101 + K), K)
  got = _same_lines(kind, bd, tn, st, ac, (kind, K))
  assert got['flags'].max() == 0 and got['depth'].max() == min(K, 9 if kind == 1 else K) and got['depth'].min() == 1
  ended = got['terminal'].max(1) == 1
  assert ended.all() if (kind, K) == (1, 16) else ended.any() and (~ended).any()
  assert np.all(got['reward_true'][got['terminal'] == 0] == 0)      # only the move that ends a game can win it
  wins = got['reward_true'] == 1
  assert wins.any() and np.all(got['terminal'][wins] == 1)
  # past the line's end everything is zero
  past = np.arange(K + 1)[None, :] > got['depth'][:, None]
  assert past.any() and not got['obs'][past].any() and not got['legal'][past].any() and not got['terminal'][past].any()


def test_forced_connect_four_positions():
  """the six one-legal-column boards: the four winning moves give true reward 1 and a terminal p_1, 'draw' reward 0 and a
  terminal p_1, 'plain' goes on"""
  for name, turn, col, board in C4_FORCED:
    bd, tn, st = arrays([([int(x) for x in board], int(turn), int(np.count_nonzero(board)))])
    got = _same_lines(3, bd, tn, st, np.array([[col, -1, -1]], np.int32), name)
    assert got['depth'][0] == 1 and got['flags'][0] == 0
    assert got['legal'][0, 0].tolist() == [int(c == col) for c in range(7)]
    assert np.array_equal(got['obs'][0, 0], (turn * board).astype(np.float32))
    assert got['reward_true'][0].tolist() == [0.0, 1.0 if name in WINS else 0.0, 0.0, 0.0], name
    assert got['terminal'][0].tolist() == [0, 0 if name == 'plain' else 1, 0, 0], name
    after = board.copy()
    after[7 * int(np.flatnonzero(board.reshape(6, 7)[:, col] == 0)[0]) + col] = turn
    assert np.array_equal(got['obs'][0, 1], (-turn * after).astype(np.float32))


@pytest.mark.parametrize('kind', [1, 3])
def test_padding_at_every_index_and_k0(kind):
  """-1 at index j ends the line with depth j whatever follows it; K = 0 is the start position alone"""
  rng = np.random.RandomState(5)
  K = 4
  pos = random_position(kind, 2, rng)
  line = []
  bd, mover = list(pos[0]), pos[1]
  for _ in range(K):
    a = next(a for a in pp.legal_actions(kind, bd) if pp.play(kind, list(bd), mover, a) == 0)
    line.append(a)
    pp.play(kind, bd, mover, a)
    mover = -mover
  rows = [line[:j] + [-1] + line[j + 1:] for j in range(K)] + [line]
  bd, tn, st = arrays([pos] * len(rows))
  got = _same_lines(kind, bd, tn, st, np.array(rows, np.int32), (kind, 'padding'))
  assert got['depth'].tolist() == list(range(K)) + [K]
  got0 = _same_lines(kind, bd[:1], tn[:1], st[:1], np.zeros((1, 0), np.int32), (kind, 'K = 0'))
  assert got0['obs'].shape[1] == 1 and got0['depth'].tolist() == [0]
  assert np.array_equal(got0['obs'][0, 0], got['obs'][0, 0])


@pytest.mark.parametrize('kind', [1, 3])
def test_illegal_action_sets_the_flag(kind):
  """an occupied cell / a full column / an action past the action count stops the line where it stands and flags the row;
  the rows beside it are untouched"""
  if kind == 1:
    pos, bad = ([1, -1, 0, 0, 0, 0, 0, 0, 0] + [0] * 33, 1, 2), 0
  else:
    name, turn, col, board = C4_FORCED[5]      # 'plain': one legal column
    pos, bad = ([int(x) for x in board], int(turn), int(np.count_nonzero(board))), (col + 1) % 7
  good = pp.legal_actions(kind, pos[0])[0]
  A = uu.A_OF[kind]
  bd, tn, st = arrays([pos] * 4)
  got = _same_lines(kind, bd, tn, st, np.array([[bad, good], [good, -1], [A, good], [good, bad if kind == 1 else -1]], np.int32), kind)
  assert got['flags'].tolist() == [1, 0, 1, 1 if kind == 1 else 0]
  assert got['depth'].tolist() == [0, 1, 0, 1]


# ---------------------------------------------------------------- terms
def _random_items(A, n, rng, one_legal):
  lu, lf = rng.normal(0, 2.0, (n, A)).astype(np.float32), rng.normal(0, 2.0, (n, A)).astype(np.float32)
  tie = rng.rand(n) < 0.2
  lu[tie, 0] = lu[tie, A - 1] = lu[tie].max(1) + 1                      # a tied arg-max: the largest action on both sides
  same = rng.rand(n) < 0.2
  lf[same] = lu[same]                                                  # k = 0's case: one computation
  legal = np.ones((n, A), np.uint8)
  if one_legal:
    legal[:] = 0
    legal[np.arange(n), rng.randint(0, A, n)] = 1
  truth = rng.choice(np.array([-3, -1, 0, 1], np.int8), (n, A))
  truth[legal == 0] = -2
  return dict(logits_u=lu, logits_f=lf, legal=legal, terminal=(rng.rand(n) < 0.15).astype(np.uint8), live=(rng.rand(n) < 0.9).astype(np.uint8),
              k=rng.randint(0, 6, n).astype(np.int32), reward_true=(rng.rand(n) < 0.3).astype(np.float32),
              reward_u=rng.normal(0, 1, n).astype(np.float32), value_u=rng.normal(0, 1, n).astype(np.float32),
              value_f=np.where(same, 0, rng.normal(0, 1, n)).astype(np.float32), truth=truth, same=same)


@pytest.mark.parametrize('A', [7, 9])
@pytest.mark.parametrize('one_legal', [True, False], ids=['one_legal', 'all_legal'])
@pytest.mark.parametrize('with_truth', [True, False], ids=['truth', 'no_truth'])
def test_terms_equal_the_restatement(A, one_legal, with_truth):
  rng = np.random.RandomState(100 * A + 2 * one_legal + with_truth)
  it = _random_items(A, 400, rng, one_legal)
  it['value_f'][it['same']] = it['value_u'][it['same']]
  same = it.pop('same')
  truth = it.pop('truth')
  if not with_truth:
    truth = None
  got = uu.host_terms(A, truth=truth, **it)
  want = uu.terms_array([uu.py_terms(it['logits_u'][i], it['logits_f'][i], it['legal'][i], it['terminal'][i], it['live'][i], it['k'][i],
                                     it['reward_true'][i], it['reward_u'][i], it['value_u'][i], it['value_f'][i],
                                     None if truth is None else truth[i]) for i in range(400)])
  uu.assert_terms(got, want, (A, one_legal, with_truth))
  T = {name: i for i, name in enumerate(uu.TERMS)}
  pos = got[:, T['position']] == 1
  assert pos.any() and (~pos).any() and not got[~pos][:, T['value']:].any()      # a terminal or dead p_k carries reward terms at the most
  # one computation on both sides: no drift, no distance, the same arg-max -- exactly
  one = pos & same
  assert one.any() and np.all(got[one, T['value_drift']] == 0) and np.all(got[one, T['policy_tv']] == 0) and np.all(got[one, T['top1_agree']] == 1)
  if with_truth:
    assert (got[:, T['solved']] == 1).any() and (pos & (got[:, T['solved']] == 0)).any()
    assert np.all(got[:, T['optimal_mass']] <= 1 + 1e-12)
  else:
    assert not got[:, T['solved']:].any()
  if one_legal:      # the mass off the one legal action is the illegal mass
    assert np.all(got[pos, T['illegal_mass']] > 0)
  else:
    assert np.all(got[:, T['illegal_mass']] == 0)


# ---------------------------------------------------------------- the report
@pytest.fixture(scope='module')
def ttt_report():
  from model_based_rl_amd import solver
  net = fc64_net(1)
  games = uu.random_games(1, 32, 77)
  K = 3
  out = {}
  for seat in (None, 1):
    stub = uu.StubEngine(net, 1)
    got = solver.grade_unroll(games, 'TicTacToe', stub, K, graded_seat=seat, max_nodes=su.BUDGET)
    bd, tn, st, ac, where = uu.rows_of(games, 1, K, seat)
    truth = uu.minimax_truth(games, 1, K, where)
    ref = uu.fc_unroll(net, 1, bd, tn, st, ac, truth)
    out[seat] = (got, uu.py_report(ref['terms'], K), stub, ref)
  return out


def fc64_net(kind, seed=5):
  from tests.eval_device_util import weights
  return uu.FC32Scalars(weights(uu.O_OF[kind], uu.A_OF[kind], seed), uu.O_OF[kind], uu.A_OF[kind])


@pytest.mark.parametrize('seat', [None, 1], ids=['both_seats', 'first_seat'])
def test_report_equals_a_plain_recomputation(ttt_report, seat):
  got, want, stub, ref = ttt_report[seat]
  assert stub.solve_calls == 1      # one solve over every position of the games
  T = {name: i for i, name in enumerate(uu.TERMS)}
  # TicTacToe is fully solvable at this budget: the reference leaves nothing out ...
  for d in want['depth']:
    assert d['solved'] == d['positions'] and d['n'] >= d['positions'] > 0
  # ... and then neither does the report
  uu.assert_report(got, want, 1e-12, seat)
  for d in got['depth']:
    assert d['solved'] == d['positions']
  assert got['rows'] == (sum(g.step for g in uu.random_games(1, 32, 77)) if seat is None else sum((g.step + 1) // 2 for g in uu.random_games(1, 32, 77)))
  d0 = got['depth'][0]
  assert d0['n'] == d0['positions'] == got['rows'] and d0['transitions'] == 0 and d0['reward_mae'] is None and d0['reward_at_wins'] is None
  assert d0['value_drift'] == 0.0 and d0['policy_tv'] == 0.0 and d0['top1_agree'] == 1.0      # one computation at k = 0
  assert d0['value_mae'] == d0['value_mae_fresh'] and d0['optimal_mass'] == d0['optimal_mass_fresh']
  assert got['depth'][1]['value_drift'] > 0 and got['depth'][1]['wins'] > 0
  assert [d['n'] for d in got['depth']] == sorted([d['n'] for d in got['depth']], reverse=True)


def test_report_does_not_depend_on_the_chunking(ttt_report):
  """the per-depth means are sums in row order over per-(row, k) scalars: an engine that hands the rows on in pieces gives the
  same report, bit for bit"""
  from model_based_rl_amd import solver
  got, _, stub, _ = ttt_report[None]

  class Pieces(uu.StubEngine):
    def unroll(self, kind, boards, turn, step, actions, truth=None, raw=False):
      parts = [uu.StubEngine.unroll(self, kind, boards[lo:lo + 7], turn[lo:lo + 7], step[lo:lo + 7], actions[lo:lo + 7], truth[lo:lo + 7])
               for lo in range(0, len(boards), 7)]
      return dict(depth=np.concatenate([p['depth'] for p in parts]), terms=np.concatenate([p['terms'] for p in parts]))
  again = solver.grade_unroll(uu.random_games(1, 32, 77), 1, Pieces(stub.net, 1), 3, max_nodes=su.BUDGET)
  assert again == got


def test_report_scope_and_empty_sets():
  """Connect Four with a scope: truth only where at most max_empties cells are empty, so solved < positions at small k; a
  seat nobody holds gives an empty report with None means"""
  from model_based_rl_amd import solver
  net = fc64_net(3)
  games = uu.random_games(3, 4, 9, min_len=37)      # long games: their last plies have at most E empty cells
  K, E = 2, 8
  got = solver.grade_unroll(games, 3, uu.StubEngine(net, 3), K, max_empties=E, max_nodes=su.BUDGET)
  bd, tn, st, ac, where = uu.rows_of(games, 3, K)
  ref = uu.fc_unroll(net, 3, bd, tn, st, ac, uu.minimax_truth(games, 3, K, where, E))
  uu.assert_report(got, uu.py_report(ref['terms'], K), 1e-12, 'scope')
  assert 0 < got['depth'][0]['solved'] < got['depth'][0]['positions']
  # in scope nothing is dropped: every non-terminal p_k with at most E empty cells is solved at this budget
  in_scope = sum(1 for (gi, p) in where if 42 - p <= E)
  assert got['depth'][0]['solved'] == in_scope
  empty = solver.grade_unroll(games, 3, uu.StubEngine(net, 3), K, max_empties=E, graded_seat=0)
  assert empty['rows'] == 0 and all(d['n'] == 0 and d['value_mae'] is None and d['policy_tv'] is None for d in empty['depth'])


def test_grade_unroll_raises_on_an_illegal_record():
  from model_based_rl_amd import solver
  games = uu.random_games(1, 2, 3)
  games[1].history.actions[1] = games[1].history.actions[0]      # the occupied cell
  with pytest.raises(ValueError, match='illegal'):
    solver.grade_unroll(games[1:], 1, uu.StubEngine(fc64_net(1), 1), 2)


# ---------------------------------------------------------------- refusals and formatting
def _ttt_row():
  return arrays([([0] * 42, 1, 0)])


@pytest.mark.parametrize('kind', [0, 2])
def test_lines_refuse_a_kind_that_is_no_board_game(kind):
  bd, tn, st = _ttt_row()
  with pytest.raises(RuntimeError, match='kind must be 1'):
    uu.host_lines(kind, bd, tn, st, np.zeros((1, 2), np.int32))


def test_lines_refuse_k_outside_0_to_16():
  bd, tn, st = _ttt_row()
  with pytest.raises(RuntimeError, match='K must be in 0 .. 16, got 17'):
    uu.host_lines(1, bd, tn, st, np.full((1, 17), -1, np.int32))


def test_lines_refuse_no_rows():
  with pytest.raises(RuntimeError, match='n must be >= 1, got 0'):
    uu.host_lines(1, np.zeros((0, 42), np.int8), np.zeros(0, np.int8), np.zeros(0, np.int32), np.zeros((0, 2), np.int32))


def test_lines_refuse_null_arguments():
  from model_based_rl_amd import _abi
  lib = _abi.load()
  assert lib.mz_unroll_lines_host(1, None, None, None, None, 1, 2, None, None, None, None, None, None) != 0
  assert b'mz_unroll_lines_host: null argument' in lib.mz_last_error()
  assert lib.mz_unroll_terms_host(9, 1, None, None, None, None, None, None, None, None, None, None, None, None) != 0
  assert b'mz_unroll_terms_host: null argument' in lib.mz_last_error()
  assert lib.mz_unroll(None, 1, None, None, None, None, 1, 2, None, None, None, None, None, None, None) != 0
  assert b'mz_unroll: null argument' in lib.mz_last_error()


def test_lines_refuse_a_start_that_is_no_position():
  bd, tn, st = _ttt_row()
  over = bd.copy()
  over[0, :3] = 1
  with pytest.raises(RuntimeError, match='position 0'):
    uu.host_lines(1, over, tn, np.array([3], np.int32), np.zeros((1, 2), np.int32))


def _args(**kv):
  base = dict(grade=True, device_env=True, environment='TicTacToe', apply_mcts_actions=1, grade_unroll=3, grade_table=False)
  base.update(kv)
  return types.SimpleNamespace(**base)


def test_cli_refuses_unroll_without_grade():
  from model_based_rl_amd.evaluate import refuse_grade_unroll
  with pytest.raises(NotImplementedError, match=r'^--grade_unroll: .*without --grade\.$'):
    refuse_grade_unroll(_args(grade=False))


@pytest.mark.parametrize('K', [0, 17, -1])
def test_cli_refuses_a_depth_outside_1_to_16(K):
  from model_based_rl_amd.evaluate import refuse_grade_unroll
  with pytest.raises(NotImplementedError, match=r'^--grade_unroll: the depth is 1 to 16'):
    refuse_grade_unroll(_args(grade_unroll=K))


def test_cli_accepts_and_parses_the_flag():
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import refuse_grade, refuse_grade_unroll
  a = get_evaluation_args(['--device_env', '--grade', '--grade_unroll', '5'])
  assert a.grade_unroll == 5
  refuse_grade(a); refuse_grade_unroll(a)
  assert get_evaluation_args(['--device_env', '--grade']).grade_unroll is None
  refuse_grade_unroll(get_evaluation_args([]))      # nothing to refuse without the flag
  refuse_grade_unroll(_args(no_support=True))      # --no_support checkpoints are served by the same inference path
  # what --grade refuses stays refused by --grade's own sentence
  with pytest.raises(NotImplementedError, match=r'^--grade: '):
    refuse_grade(_args(device_env=False))
  with pytest.raises(NotImplementedError, match=r'^--grade: '):
    refuse_grade(_args(environment='CartPole-v0'))


def test_main_refuses_before_loading_anything():
  from model_based_rl_amd import evaluate
  with pytest.raises(NotImplementedError, match=r'^--grade_unroll: '):
    evaluate.main(['--device_env', '--grade_unroll', '3', '--nets', 'missing'])
  with pytest.raises(NotImplementedError, match=r'^--grade_unroll: '):
    evaluate.main(['--device_env', '--grade', '--grade_unroll', '40', '--nets', 'missing'])


def test_grade_unroll_refuses_a_depth_outside_0_to_16():
  from model_based_rl_amd import solver
  with pytest.raises(ValueError, match='K must be in 0 .. 16'):
    solver.grade_unroll([], 1, None, 17)


def test_format_unroll(ttt_report):
  from model_based_rl_amd import solver
  got = ttt_report[None][0]
  text = solver.format_unroll(got, 'net:0')
  lines = text.split('\n')
  assert lines[0].startswith('The model by unroll depth against the true game - label: (net:0): %d rows, K = 3' % got['rows'])
  assert len(lines) == 1 + 4 + 1 and lines[-1] == ''
  assert [ln[:4] for ln in lines[1:5]] == ['k=0 ', 'k=1 ', 'k=2 ', 'k=3 ']
  assert 'reward mae n/a' in lines[1] and 'drift 0.000 tv 0.000 top1 100.0%' in lines[1]      # k = 0: no transition, one computation
  assert 'n/a' not in lines[2]
  empty = solver.format_unroll(dict(K=0, rows=0, depth=[dict(got['depth'][0], n=0, value_mae=None, value_sign=None)]))
  assert 'label' not in empty and 'value mae u n/a' in empty and 'sign u n/a' in empty
