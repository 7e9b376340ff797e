"""Helpers of the playout-opponent tests (no test functions here): the ctypes host hook mz_playout_plan_host, positions as
(board42, turn, step) built on the rules of tests/playout_py.py, and the positions test_playout_cpu.py and
test_gpu_playout.py share."""
import ctypes as C

import numpy as np

from tests import playout_py as pp
from tests.c4_positions import POSITIONS as C4_FORCED

A_OF = {1: 9, 3: 7}


def host_plan(kind, boards, turn, step, playouts, move=0, seed=0, env_id_offset=0):
  """mz_playout_plan_host -> action [n], visits [n, A], wins [n, A] (int32)"""
  from model_based_rl_amd import _abi
  lib = _abi.load()
  A = A_OF.get(kind, 9)
  bd = np.ascontiguousarray(boards, np.int8).reshape(-1, 42)
  tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
  n = bd.shape[0]
  action, visits, wins = np.zeros(n, np.int32), np.zeros((n, A), np.int32), np.zeros((n, A), np.int32)
  p = lambda a: a.ctypes.data_as(C.c_void_p)
  _abi.check(lib.mz_playout_plan_host(kind, A, int(seed), int(env_id_offset), p(bd), p(tn), p(st), n, int(playouts), int(move),
                                      p(action), p(visits), p(wins)), 'mz_playout_plan_host')
  return action, visits, wins


def random_position(kind, plies, rng):
  """a position after `plies` uniformly random legal plies from the start in which the game has not ended"""
  while True:
    bd, turn = [0] * 42, 1
    for _ in range(plies):
      acts = pp.legal_actions(kind, bd)
      if pp.play(kind, bd, turn, acts[rng.randint(len(acts))]):
        break
      turn = -turn
    else:
      return bd, turn, plies


def ttt(cells, turn=None):
  """a TicTacToe position from nine characters, rows top to bottom: X = +1 (moves first), O = -1, . empty"""
  cells = cells.replace(' ', '')
  assert len(cells) == 9
  bd = [{'X': 1, 'O': -1, '.': 0}[c] for c in cells] + [0] * 33
  x, o = cells.count('X'), cells.count('O')
  assert x - o in (0, 1)
  return bd, (1 if x == o else -1) if turn is None else turn, x + o


def c4(*columns):
  """a Connect Four position from its seven columns, each a string of stones from the bottom up (X = +1 moves first)"""
  assert len(columns) == 7 and all(len(c) <= 6 for c in columns)
  bd = [0] * 42
  for c, col in enumerate(columns):
    for r, s in enumerate(col):
      bd[7 * r + c] = {'X': 1, 'O': -1}[s]
  x, o = sum(c.count('X') for c in columns), sum(c.count('O') for c in columns)
  assert x - o in (0, 1)
  return bd, 1 if x == o else -1, x + o


def winning_moves(kind, board, mover):
  """the legal actions by which `mover` wins at once"""
  return [a for a in pp.legal_actions(kind, board) if pp.play(kind, list(board), mover, a) == 1]


TTT_ONE_EMPTY = ttt('XOX XOO OX.')      # one legal cell; the ninth move draws


def shared_positions():
  """{kind: [(board42, turn, step)]}: the TicTacToe start, positions after 1-7 random plies and one with a single empty
  cell; the Connect Four start, positions after 1-30 random plies and the six one-legal-column boards of c4_positions"""
  rng = np.random.RandomState(20240607)
  out = {1: [random_position(1, p, rng) for p in range(8)] + [TTT_ONE_EMPTY],
         3: [random_position(3, p, rng) for p in range(31)]}
  for _, turn, _, board in C4_FORCED:
    out[3].append(([int(x) for x in board], int(turn), int(np.count_nonzero(board))))
  return out


def arrays(positions):
  """(boards [n, 42] int8, turn [n] int8, step [n] int32) of a list of positions"""
  return (np.array([p[0] for p in positions], np.int8), np.array([p[1] for p in positions], np.int8),
          np.array([p[2] for p in positions], np.int32))
