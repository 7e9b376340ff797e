"""CPU side of the playout-search opponent (csrc/mz_playout.hip.h, DESIGN s7d):
  restatement  the host hook mz_playout_plan_host -- the device's own bodies with the lanes looped on the host -- equals the
               pure-Python restatement of tests/playout_py.py in action, visits and wins, exactly
  asan         the bodies compiled into a stand-alone program (tests/playout_host.cpp) under AddressSanitizer + UBSan; the
               plans it prints are the hook's
  tactics      win-in-one and must-block positions of both games through the hook
  abi, cli     the entry points are declared; --opp_playouts parses, and every refusal is one sentence that reaches the
               caller before any device is touched"""
import os
import subprocess

import numpy as np
import pytest

from tests import playout_py as pp
from tests.eval_device_util import eval_state
from tests.playout_util import A_OF, arrays, c4, host_plan, shared_positions, ttt, winning_moves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', [1, 3])
def test_hook_equals_the_restatement(kind):
  positions = shared_positions()[kind]
  assert len(positions) == (9 if kind == 1 else 37)
  bd, tn, st = arrays(positions)
  for playouts in (64, 192, 1024):
    action, visits, wins = host_plan(kind, bd, tn, st, playouts, move=5, seed=3, env_id_offset=1000)
    for i, (board, turn, _) in enumerate(positions):
      want = pp.plan(kind, board, turn, playouts, 3, 1000 + i, 5)
      got = (int(action[i]), [int(x) for x in visits[i]], [int(x) for x in wins[i]])
      assert got == want, (kind, playouts, i)
      assert sum(got[1]) == playouts and got[0] in pp.legal_actions(kind, board)


def test_one_legal_action_is_exact():
  """k = 1: all 64 lanes of the root's evaluation take the one action and its result is exact, draws included; every
  later iteration meets the root's ended edge and adds the exact value again"""
  from tests.c4_positions import POSITIONS, WINS
  from tests.playout_util import TTT_ONE_EMPTY
  bd, tn, st = arrays([TTT_ONE_EMPTY])
  action, visits, wins = host_plan(1, bd, tn, st, 192)
  assert action[0] == 8 and visits[0, 8] == 192 and wins[0, 8] == 192 and visits[0].sum() == 192      # a draw: 1 per playout
  for name, turn, col, board in POSITIONS:
    action, visits, wins = host_plan(3, np.array([board], np.int8), [turn], [int(np.count_nonzero(board))], 192)
    assert action[0] == col and visits[0, col] == 192 and visits[0].sum() == 192
    if name in WINS:
      assert wins[0, col] == 2 * 192, name
    elif name == 'draw':
      assert wins[0, col] == 192, name


def test_plan_depends_on_its_own_game_only():
  """(seed, game id, move, position, N) and nothing else of its batch: a position planned alone under its own id"""
  positions = shared_positions()[3][:8]
  bd, tn, st = arrays(positions)
  action, visits, wins = host_plan(3, bd, tn, st, 192, move=2, seed=9, env_id_offset=40)
  for i in range(len(positions)):
    a, v, w = host_plan(3, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], 192, move=2, seed=9, env_id_offset=40 + i)
    assert a[0] == action[i] and np.array_equal(v[0], visits[i]) and np.array_equal(w[0], wins[i])
  # ... and the key matters: another move, another seed, another game id give other statistics
  for kw in (dict(move=3, seed=9, env_id_offset=40), dict(move=2, seed=10, env_id_offset=40), dict(move=2, seed=9, env_id_offset=41)):
    assert not np.array_equal(host_plan(3, bd, tn, st, 192, **kw)[2], wins), kw


def test_hook_refusals():
  bd, tn, st = arrays(shared_positions()[1][:1])
  for kw, word in ((dict(kind=2), 'kind'), (dict(playouts=100), 'multiple of 64'), (dict(playouts=0), 'multiple of 64'),
                   (dict(playouts=65536 + 64), 'multiple of 64')):
    args = dict(kind=1, playouts=64)
    args.update(kw)
    with pytest.raises(RuntimeError, match=word):
      host_plan(args['kind'], bd, tn, st, args['playouts'])
  with pytest.raises(RuntimeError, match='stones'):
    host_plan(1, bd, tn, [3], 64)
  with pytest.raises(RuntimeError, match='turn'):
    host_plan(1, bd, [0], st, 64)
  full = np.array([[1, -1, 1, 1, -1, -1, -1, 1, 1] + [0] * 33], np.int8)
  with pytest.raises(RuntimeError, match='no legal action'):
    host_plan(1, full, [-1], [9], 64)
  c4_on_ttt = np.zeros((1, 42), np.int8)
  c4_on_ttt[0, 20] = 1
  with pytest.raises(RuntimeError, match='not a board'):
    host_plan(1, c4_on_ttt, [-1], [1], 64)


def test_bodies_under_the_sanitizers(tmp_path):
  """tests/playout_host.cpp under AddressSanitizer + UBSan; its plans are the hook's"""
  exe = str(tmp_path / 'playout_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'include'),
         '-I', os.path.join(ROOT, 'model-based-rl_amd', 'csrc'), os.path.join(ROOT, 'tests', 'playout_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  lines = run.stdout.strip().splitlines()
  assert lines[-1] == 'ok 300' and len(lines) == 301
  rows = [[int(x) for x in line.split()] for line in lines[:-1]]
  at = 0
  for kind in (1, 3):
    A = A_OF[kind]
    mine = [r for r in rows if r[0] == kind]
    assert len(mine) == 150 and all(len(r) == 4 + 2 * A + 42 for r in mine)
    boards = np.array([r[4 + 2 * A:] for r in mine], np.int8)
    action, visits, wins = host_plan(kind, boards, [r[1] for r in mine], [r[2] for r in mine], 1024, move=3, seed=11,
                                     env_id_offset=5000 + at)
    assert np.array_equal(action, [r[3] for r in mine])
    assert np.array_equal(visits, [r[4:4 + A] for r in mine]) and np.array_equal(wins, [r[4 + A:4 + 2 * A] for r in mine])
    assert len({r[2] for r in mine}) >= 7      # positions of many depths
    at += len(mine)


# ---- tactics.  The lists were written out before the first run; test_tactic_lists_are_what_they_say holds them to the rules of playout_py.
TTT_WIN = [ttt('XX. OO. ...'), ttt('X.. OX. .O.'), ttt('XO. .X. O..'), ttt('XX. .OO X..'), ttt('X.X OO. .X.'), ttt('..X .XO ..O'),
           ttt('O.X .OX X..')]
TTT_BLOCK = [(ttt('OO. X.. ..X'), 2), (ttt('O.X XO. ...'), 8), (ttt('XX. .O. ...'), 2), (ttt('X.. OX. ...'), 8),
             (ttt('X.. X.O ...'), 6), (ttt('XO. .O. ..X'), 7), (ttt('X.O ... .XO'), 5)]
C4_WIN = [c4('', '', '', 'XXX', 'OOO', '', ''), c4('O', 'X', 'X', 'X', '', '', 'OO'), c4('X', 'OX', 'XOX', 'OXO', '', '', 'O'),
          c4('X', '', 'OOO', '', '', 'XXX', ''), c4('OO', 'O', 'X', 'X', '', 'X', ''), c4('O', '', '', 'OXO', 'XOX', 'OX', 'X'),
          c4('X', '', '', 'XOOO', '', '', 'XX')]
C4_BLOCK = [(c4('X', 'X', '', '', 'OOO', '', 'X'), 4), (c4('', '', 'XXX', '', '', 'O', 'O'), 2),
            (c4('X', 'O', 'O', 'O', '', '', 'XX'), 4), (c4('O', '', '', 'X', 'X', 'X', 'O'), 2),
            (c4('O', 'XO', 'OXO', 'XOX', '', '', 'X'), 3), (c4('O', '', '', 'OXXX', '', '', ''), 3),
            (c4('O', 'O', '', 'O', 'X', '', 'XX'), 2)]
BLOCK_PLAYOUTS = 4096


def test_tactic_lists_are_what_they_say():
  for kind, wins, blocks in ((1, TTT_WIN, TTT_BLOCK), (3, C4_WIN, C4_BLOCK)):
    assert len(wins) >= 6 and len(blocks) >= 6
    for board, turn, _ in wins:
      assert winning_moves(kind, board, turn), (kind, board)
    for (board, turn, _), block in blocks:
      assert not winning_moves(kind, board, turn), (kind, board)      # the mover has no win of their own
      assert winning_moves(kind, board, -turn) == [block], (kind, board)      # the other side wins next move by exactly this one


@pytest.mark.parametrize('kind', [1, 3])
def test_takes_a_win_in_one(kind):
  positions = TTT_WIN if kind == 1 else C4_WIN
  bd, tn, st = arrays(positions)
  action, visits, wins = host_plan(kind, bd, tn, st, 1024, move=1, seed=0, env_id_offset=0)
  missed = [(i, int(action[i]), visits[i].tolist()) for i, (board, turn, _) in enumerate(positions)
            if int(action[i]) not in winning_moves(kind, board, turn)]
  assert not missed, missed


@pytest.mark.parametrize('kind', [1, 3])
def test_blocks_a_win_in_one(kind):
  blocks = TTT_BLOCK if kind == 1 else C4_BLOCK
  bd, tn, st = arrays([p for p, _ in blocks])
  action, visits, wins = host_plan(kind, bd, tn, st, BLOCK_PLAYOUTS, move=1, seed=0, env_id_offset=0)
  missed = [(i, int(action[i]), visits[i].tolist()) for i, (_, block) in enumerate(blocks) if int(action[i]) != block]
  assert not missed, missed


# ---- ABI and command line
def test_entry_points_are_declared():
  from model_based_rl_amd import _abi
  from tests.test_abi import declared_symbols
  assert {'mz_playout_plan', 'mz_eval_env_set_opponent'} <= set(_abi.SIGNATURES) & set(declared_symbols(('mz_engine.h',)))
  assert 'mz_playout_plan_host' in _abi.SIGNATURES and 'mz_playout_plan_host' in declared_symbols(('mz_engine_debug.h',))
  for f in ('mz_playout.hip.h', 'mz_playout_abi.inc'):
    assert f in _abi._SOURCES and f in _abi._ENGINE_ONLY
  assert _abi.load().mz_version() == 1


def test_flags_parse():
  from model_based_rl_amd.config import get_evaluation_args
  args = get_evaluation_args(['--device_env', '--random_opp', '-1', '--opp_playouts', '1024', '--nets', 'a'])
  assert args.opp_playouts == 1024 and args.random_opp == -1 and args.device_env
  assert get_evaluation_args(['--nets', 'a']).opp_playouts == 0


def _no_device(monkeypatch):
  """any attempt to reach a device fails the test"""
  import torch
  from model_based_rl_amd import engine, match

  def touched(*a, **k):
    raise AssertionError('a device was touched')
  monkeypatch.setattr(torch.cuda, 'is_available', touched)
  monkeypatch.setattr(engine.Engine, '__init__', touched)
  monkeypatch.setattr(match.Match, '__init__', touched)


def _one_sentence(msg, word):
  assert msg.startswith('--opp_playouts: ') and word in msg, msg
  assert msg.endswith('.') and '\n' not in msg and '. ' not in msg[:-1], msg


CLI_REFUSALS = [      # (flags after --saves_dir DIR --nets a b, the word the sentence carries)
    (['--random_opp', '-1', '--opp_playouts', '1024'], '--device_env'),
    (['--device_env', '--opp_playouts', '1024'], '--random_opp'),
    (['--device_env', '--random_opp', '-1', '--opp_playouts', '1024', '--apply_mcts_actions', '2'], '--apply_mcts_actions'),
    (['--device_env', '--random_opp', '-1', '--opp_playouts', '1024', '--apply_mcts_actions', '1', '3'], '--apply_mcts_actions'),
    (['--device_env', '--random_opp', '1', '--opp_playouts', '100'], 'multiple of 64'),
    (['--device_env', '--random_opp', '1', '--opp_playouts', '32'], 'multiple of 64'),
    (['--device_env', '--random_opp', '1', '--opp_playouts', '131072'], 'multiple of 64'),
    (['--match', '--opp_playouts', '1024'], '--match'),
]


@pytest.mark.parametrize('i', range(len(CLI_REFUSALS)))
def test_cli_refusals_reach_the_caller_before_any_device(i, monkeypatch, tmp_path):
  from model_based_rl_amd import evaluate
  _no_device(monkeypatch)
  flags, word = CLI_REFUSALS[i]
  with pytest.raises(NotImplementedError) as err:      # refused before a checkpoint is read (there is none)
    evaluate.main(['--saves_dir', str(tmp_path) + os.sep, '--nets', 'a', 'b'] + flags)
  _one_sentence(str(err.value), word)


def test_config_refusals_reach_the_caller_before_any_device(monkeypatch):
  from model_based_rl_amd import evaluate
  _no_device(monkeypatch)
  # the checkpoint's own configuration: refused by the Evaluator and again by the batch itself
  cart = eval_state('CartPole-v0', device_env=True, random_opp=-1, opp_playouts=1024)
  with pytest.raises(NotImplementedError) as err:
    evaluate.Evaluator(cart)
  _one_sentence(str(err.value), 'CartPole-v0')
  for over, word in ((dict(opp_playouts=1024), '--random_opp'), (dict(opp_playouts=1024, random_opp=1, apply_mcts_actions=3), '--apply_mcts_actions'),
                     (dict(opp_playouts=96, random_opp=1), 'multiple of 64')):
    with pytest.raises(NotImplementedError) as err:
      evaluate.Evaluator(eval_state('TicTacToe', device_env=True, **over))
    _one_sentence(str(err.value), word)
  ev = evaluate.Evaluator.__new__(evaluate.Evaluator)      # the host path asked for the playout opponent
  ev.config = eval_state('ConnectFour', random_opp=1, opp_playouts=1024)['config']
  with pytest.raises(NotImplementedError) as err:
    ev.play_games(2, [0, 1])
  _one_sentence(str(err.value), '--device_env')
  ev = evaluate.Evaluator.__new__(evaluate.Evaluator)      # (a batch of an evaluator whose configuration changed after its creation)
  ev.config = eval_state('TicTacToe', opp_playouts=1024)['config']
  with pytest.raises(NotImplementedError) as err:
    ev._play_batch_device([0, 1], None, None, False)
  _one_sentence(str(err.value), '--random_opp')
  # ... and nothing to refuse at 0, or for the two games with a seat named
  evaluate.refuse_opp_playouts(eval_state('CartPole-v0')['config'])
  for env in ('TicTacToe', 'ConnectFour'):
    evaluate.refuse_opp_playouts(eval_state(env, device_env=True, random_opp=-1, opp_playouts=65536)['config'])
  # a configuration that is not refused does go on to the device
  ok = eval_state('TicTacToe', device_env=True, random_opp=-1, opp_playouts=64)
  with pytest.raises(AssertionError, match='a device was touched'):
    evaluate.Evaluator(ok)
