"""Helpers of the table-search tests (no test functions here): the ctypes host hook mz_solve_tt_host, the deep Connect Four
positions test_solve_tt_cpu.py and test_gpu_solve_tt.py share, and the references on them.  Every reference is computed
once and cached; the truth on the deep positions is the PLAIN host hook's (mz_solve_host), never the code under test."""
import ctypes as C
import functools

import numpy as np

from tests import playout_util as pu
from tests import solve_util as su

GEN_WRAP = 1 << 11      # MZ_SVT_GEN_WRAP: a lane's generation counter runs 1 .. GEN_WRAP - 1, then the lane clears its table
DEEP_SEED = 20241021
DEEP_PLAIN_BUDGET = 1 << 24      # the plain search solves every unit of c4_deep() within this (the seed is chosen so)
DEEP_BUDGET = 1 << 20


def host_solve_tt(kind, boards, turn, step, max_nodes=su.BUDGET, A=None):
  """mz_solve_tt_host -> values [n, A] int8, nodes [n, A] uint32"""
  from model_based_rl_amd import _abi
  lib = _abi.load()
  A = su.A_OF.get(kind, 9) if A is None else A
  bd = np.ascontiguousarray(boards, np.int8).reshape(-1, 42)
  tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
  n = bd.shape[0]
  values, nodes = np.zeros((n, A), np.int8), np.zeros((n, A), np.uint32)
  p = lambda a: a.ctypes.data_as(C.c_void_p)
  _abi.check(lib.mz_solve_tt_host(kind, A, p(bd), p(tn), p(st), n, int(max_nodes), p(values), p(nodes)), 'mz_solve_tt_host')
  return values, nodes


@functools.lru_cache(None)
def c4_deep():
  """64 Connect Four positions after 22 to 26 random plies (16 to 20 empty cells)"""
  rng = np.random.RandomState(DEEP_SEED)
  return [pu.random_position(3, 22 + (i % 5), rng) for i in range(64)]


POSITIONS = {'ttt': (1, su.ttt_positions), 'c4_endgames': (3, su.c4_endgames), 'c4_mixed': (3, su.c4_mixed), 'c4_deep': (3, c4_deep)}


@functools.lru_cache(None)
def deep_truth():
  """(values, nodes) of c4_deep() by the plain host hook at 2^24 nodes a unit"""
  return su.host_solve(3, *pu.arrays(c4_deep()), max_nodes=DEEP_PLAIN_BUDGET)


@functools.lru_cache(None)
def host_reference_tt(name, max_nodes=su.BUDGET):
  """(values, nodes) of a named position list by the table search's host hook"""
  kind, positions = POSITIONS[name]
  return host_solve_tt(kind, *pu.arrays(positions()), max_nodes=max_nodes)
