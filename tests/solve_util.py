"""Helpers of the exact-solver tests (no test functions here): the ctypes host hook mz_solve_host, a Python minimax on the
rules of tests/playout_py.py (the first form of the rules, restated), and the positions test_solve_cpu.py and
test_gpu_solve.py share.  Every reference is computed once and cached."""
import ctypes as C
import functools

import numpy as np

from tests import playout_py as pp
from tests import playout_util as pu
from tests.c4_positions import POSITIONS as C4_FORCED

A_OF = {1: 9, 3: 7}
BUDGET = 65536      # per (position, action): at 12 empty cells a whole position was measured at 13.5 k nodes at the most


def host_solve(kind, boards, turn, step, max_nodes=BUDGET, A=None):
  """mz_solve_host -> values [n, A] int8, nodes [n, A] uint32"""
  from model_based_rl_amd import _abi
  lib = _abi.load()
  A = A_OF.get(kind, 9) if A is None else A
  bd = np.ascontiguousarray(boards, np.int8).reshape(-1, 42)
  tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
  n = bd.shape[0]
  values, nodes = np.zeros((n, A), np.int8), np.zeros((n, A), np.uint32)
  p = lambda a: a.ctypes.data_as(C.c_void_p)
  _abi.check(lib.mz_solve_host(kind, A, p(bd), p(tn), p(st), n, int(max_nodes), p(values), p(nodes)), 'mz_solve_host')
  return values, nodes


# ---- the reference: minimax on playout_py's rules, the outcome for `mover` to move on `board`; memoised on the position
_memo = {}


def negamax(kind, board, mover):
  key = (kind, tuple(board), mover)
  if key not in _memo:
    best = -1
    for a in pp.legal_actions(kind, board):
      bd = list(board)
      end = pp.play(kind, bd, mover, a)
      best = max(best, 1 if end == 1 else 0 if end == 2 else -negamax(kind, bd, -mover))
      if best == 1:
        break
    _memo[key] = best
  return _memo[key]


def action_values(kind, board, mover):
  """[A]: +1 / 0 / -1 for the mover after each action, -2 where it is illegal"""
  out = [-2] * A_OF[kind]
  for a in pp.legal_actions(kind, board):
    bd = list(board)
    end = pp.play(kind, bd, mover, a)
    out[a] = 1 if end == 1 else 0 if end == 2 else -negamax(kind, bd, -mover)
  return out


@functools.lru_cache(None)
def ttt_positions():
  """every non-terminal position of TicTacToe reachable from the start (X = +1 moves first), the start first"""
  seen, order, todo = set(), [], [((0,) * 42, 1, 0)]
  while todo:
    bd, turn, step = todo.pop()
    if bd in seen:
      continue
    seen.add(bd)
    order.append((list(bd), turn, step))
    for a in pp.legal_actions(1, list(bd)):
      nb = list(bd)
      if pp.play(1, nb, turn, a) == 0:
        todo.append((tuple(nb), -turn, step + 1))
  order.sort(key=lambda p: (p[2], p[0]))
  return order


@functools.lru_cache(None)
def c4_endgames():
  """200 Connect Four positions after 30 to 36 random plies (6 to 12 empty cells) and the six one-legal-column boards"""
  rng = np.random.RandomState(20241019)
  out = [pu.random_position(3, 30 + (i % 7), rng) for i in range(200)]
  for _, turn, _, board in C4_FORCED:
    out.append(([int(x) for x in board], int(turn), int(np.count_nonzero(board))))
  return out


@functools.lru_cache(None)
def c4_mixed():
  """70 Connect Four positions at mixed depths, 28 to 36 random plies (6 to 14 empty cells)"""
  rng = np.random.RandomState(20241020)
  return [pu.random_position(3, 28 + (i % 9), rng) for i in range(70)]


@functools.lru_cache(None)
def reference(name):
  """values [n, A] int8 of a named position list by the Python minimax"""
  kind, positions = {'ttt': (1, ttt_positions), 'c4_endgames': (3, c4_endgames), 'c4_mixed': (3, c4_mixed)}[name]
  return np.array([action_values(kind, bd, turn) for bd, turn, _ in positions()], np.int8)


@functools.lru_cache(None)
def host_reference(name, max_nodes=BUDGET):
  """(values, nodes) of a named position list by the host hook"""
  kind, positions = {'ttt': (1, ttt_positions), 'c4_endgames': (3, c4_endgames), 'c4_mixed': (3, c4_mixed)}[name]
  return host_solve(kind, *pu.arrays(positions()), max_nodes=max_nodes)
