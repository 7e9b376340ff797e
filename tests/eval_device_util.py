"""Helpers of the device-environment evaluation tests (no test functions here): the counter RNG restated in Python for any
purpose tag (csrc/mz_rng.h; parity_util.philox_action_uniform is the MZ_RNG_ACTION case), and the configurations / draws
the tests share."""
import types

import numpy as np

MZ_RNG_ACTION, MZ_RNG_EVAL, MZ_RNG_OPP = 4, 5, 7


def philox4x32(seed, c0, c1, c2, c3):
  """Philox4x32-10 (csrc/mz_rng.h:mz_philox) on Python integers -> the four output words"""
  k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
  for _ in range(10):
    p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
    c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
    k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
  return c0, c1, c2, c3


def philox_uniform(seed, env, move, tag, step=0):
  """mz_u01 of the first two words for the counter (env, move lo, move hi, tag << 24 | step): the uniform of
  select_action (tag MZ_RNG_ACTION, step 0), of the evaluation walk (MZ_RNG_EVAL) and of the random opponent (MZ_RNG_OPP)"""
  x, y, _, _ = philox4x32(int(seed), int(env) & 0xFFFFFFFF, int(move) & 0xFFFFFFFF, (int(move) >> 32) & 0xFFFFFFFF,
                          (int(tag) << 24) | (int(step) & 0xFFFFFF))
  return float(((x << 32) | y) >> 11) * (1.0 / 9007199254740992.0)


def opponent_choice(legal_root, seed, game_seed, move, step):
  """the device opponent's move: legal_root[min(floor(u * n), n - 1)]"""
  n = len(legal_root)
  u = philox_uniform(seed, game_seed, move, MZ_RNG_OPP, step)
  return int(legal_root[min(int(np.floor(u * n)), n - 1)])


def weights(O, A, seed, scale_heads=3.0):
  """random FCNetwork weights with the value / reward heads scaled (test_gpu_evaluate._weights)"""
  import torch
  from model_based_rl_amd.networks import FCNetwork
  torch.manual_seed(seed)
  cfg = types.SimpleNamespace(value_support=(-15, 15), reward_support=(-15, 15), no_support=False, no_target_transform=False)
  w = {k: v.numpy().copy() for k, v in FCNetwork(O, A, torch.device('cpu'), cfg).state_dict().items()}
  for k in w:
    if k.endswith('value.weight') or k.endswith('reward.weight'):
      w[k] = (w[k] * scale_heads).astype(np.float32)
  return {k: torch.from_numpy(v) for k, v in w.items()}


ENV_FLAGS = {
    'TicTacToe': ['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'],
    'ConnectFour': ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'],
    'CartPole-v0': ['--environment', 'CartPole-v0'],
}


def eval_state(env, sims=8, wseed=5, **over):
  """a state dict as evaluate.state_generator yields one, with random weights"""
  from model_based_rl_amd.config import make_config
  cfg = make_config(ENV_FLAGS[env] + ['--num_simulations', str(sims)])
  for k, v in dict(temperature=0.0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, render=False,
                   save_mcts=False, save_gif_as='', random_opp=None, human_opp=None, label='t', verbose=False).items():
    setattr(cfg, k, v)
  for k, v in over.items():
    setattr(cfg, k, v)
  O, A = int(np.prod(cfg.obs_space)), int(cfg.action_space)
  return {'config': cfg, 'weights': weights(O, A, wseed), 'training_step': 0}


def make_draws(rng, n_games, moves, M, A, opp_nmin):
  """every draw of n_games games, generated once with numpy: walk uniforms [moves][M], Dirichlet draws [moves][A] (positive
  everywhere: both paths read them at the legal positions only) and the opponent's choices -- indices into the legal list
  of the move's root position, the k-th below opp_nmin[k], a lower bound of that list's length at the opponent's k-th move"""
  return [dict(walk=[rng.uniform(size=M) for _ in range(moves)],
               noise=[rng.dirichlet([0.25] * A) for _ in range(moves)],
               opp=[int(rng.randint(0, max(1, n))) for n in opp_nmin]) for _ in range(n_games)]


# fewest legal actions the root position can have at the random opponent's k-th move (it moves at step 2k or 2k + 1):
# nine cells less the stones; seven columns less the ones (2k + 1) stones can fill
OPP_NMIN = {'TicTacToe': [8 - 2 * k for k in range(6)], 'ConnectFour': [7 - (2 * k + 1) // 6 for k in range(22)], 'CartPole-v0': []}


def record(g):
  """a game's record as test_gpu_evaluate._record takes it, plus movers and dones"""
  h = g.history
  return dict(step=g.step, actions=[int(a) for a in h.actions], rewards=[float(r) for r in h.rewards],
              to_play=[int(t) for t in h.to_play], dones=[bool(d) for d in h.dones],
              child_visits=[[float(x) for x in c] for c in h.child_visits], root_values=[float(v) for v in h.root_values],
              pred_values=[float(v) for v in g.pred_values], pred_rewards=[float(v) for v in g.pred_rewards],
              search_depths=[[int(x) for x in d] for d in g.search_depths])
