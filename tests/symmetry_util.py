"""shared by tests/test_symmetry_cpu.py and tests/test_gpu_symmetry.py: batches of the two games' shapes, the host hook
(mz_fcl_symmetry_host) as a function of a host batch, and the draw's seed"""
import ctypes as C

import numpy as np

from model_based_rl_amd import symmetry as sy

# chosen on the CPU (symmetry.draw): with this seed and update 3 the first 16 samples draw all 8 TicTacToe elements and both
# Connect Four ones, the identity among them -- test_symmetry_cpu.test_the_seed_draws_every_element holds it to that
SEED, UPDATE = 6, 3
KINDS = (sy.TICTACTOE, sy.CONNECT_FOUR)
ENV_OF = {sy.TICTACTOE: 'TicTacToe', sy.CONNECT_FOUR: 'ConnectFour'}


def ptr(a):
  return C.c_void_p(a.__array_interface__['data'][0])


def batch(kind, bs, K, act_dtype=np.int64, seed=0):
  """a batch shaped as replay_buffer.sample_batch_arrays returns it: boards of -1 / 0 / +1, actions of the game, policy
  targets with absorbing (all-zero) positions, targets inside the default supports"""
  O, A = sy.CELLS[kind], sy.ACTIONS[kind]
  rng = np.random.default_rng(1000 * kind + 10 * bs + K + 7919 * seed)
  t_pol = rng.dirichlet([0.5] * A, size=(bs, K + 1)).astype(np.float32)
  t_val = rng.uniform(-1, 1, size=(bs, K + 1)).astype(np.float32)
  t_rew = rng.integers(0, 2, size=(bs, K + 1)).astype(np.float32)
  for b in range(0, bs, 5):      # past the end of the episode
    cut = int(rng.integers(1, K + 1))
    t_pol[b, cut:] = 0.0; t_val[b, cut:] = 0.0; t_rew[b, cut:] = 0.0
  return {'obs': rng.integers(-1, 2, size=(bs, O)).astype(np.float32), 'act': rng.integers(0, A, size=(bs, K)).astype(act_dtype),
          't_rew': t_rew, 't_val': t_val, 't_pol': t_pol, 'w': rng.uniform(0.2, 1.0, size=bs)}


def host_apply(host, kind, seed, update):
  """mz_fcl_symmetry_host on the batch -> (obs', act', t_pol', elements)"""
  from model_based_rl_amd import _abi
  lib = _abi.load()
  obs, act, pol = (np.ascontiguousarray(host[k]) for k in ('obs', 'act', 't_pol'))
  out = [np.full_like(obs, np.nan), np.full_like(act, -7), np.full_like(pol, np.nan), np.full(obs.shape[0], -1, np.int32)]
  _abi.check(lib.mz_fcl_symmetry_host(kind, seed, update, obs.shape[0], act.shape[1], ptr(obs), ptr(act), int(act.dtype == np.int32), ptr(pol),
                                      ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])), 'mz_fcl_symmetry_host')
  return out


def same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
