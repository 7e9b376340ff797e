"""The device-environment evaluation path without a GPU: its two flags, its refusals and the Python restatement of the
counter RNG the GPU tests check the device's opponent against."""
import os
import types

import numpy as np
import pytest

from tests.eval_device_util import MZ_RNG_ACTION, philox4x32, philox_uniform
from tests.parity_util import philox_action_uniform


def _checkpoint(tmp_path):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--num_simulations', '5'])
  saves = tmp_path / 'saves'
  saves.mkdir()
  torch.save({'dirs': {}, 'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'optimizer': {},
              'training_step': 3}, str(saves / '3'))
  return str(saves) + os.sep, '3'


def test_flags_parse_and_reach_the_config(tmp_path):
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import state_generator
  saves, net = _checkpoint(tmp_path)
  base = ['--saves_dir', saves, '--nets', net]
  args = get_evaluation_args(base)
  assert args.device_env is False and args.keep_history is False      # the host-environment path stays the default
  (state,) = list(state_generator(args))
  assert state['config'].device_env is False and state['config'].keep_history is False
  args = get_evaluation_args(base + ['--device_env', '--keep_history', '--batch', '32'])
  assert args.device_env is True and args.keep_history is True
  (state,) = list(state_generator(args))
  assert state['config'].device_env is True and state['config'].keep_history is True and state['config'].batch == 32


def _cfg(**kv):
  c = types.SimpleNamespace(environment='TicTacToe', device_env=True, norm_obs=False, apply_mcts_actions=1)
  for k, v in kv.items():
    setattr(c, k, v)
  return c


@pytest.mark.parametrize('kv,word', [
    (dict(environment='LunarLander-v2'), 'LunarLander-v2'),
    (dict(norm_obs=True), '--norm_obs'),
    (dict(environment='ConnectFour', apply_mcts_actions=3), 'ConnectFour'),
    (dict(environment='ConnectFour', apply_mcts_actions=[1, 2]), 'ConnectFour'),
], ids=['no_device_form', 'norm_obs', 'c4_mcts_actions', 'c4_mcts_actions_list'])
def test_refusals(kv, word):
  from model_based_rl_amd.evaluate import refuse_device_env
  with pytest.raises(NotImplementedError) as ei:
    refuse_device_env(_cfg(**kv))
  msg = str(ei.value)
  assert msg.startswith('--device_env: ') and word in msg and msg.endswith('.'), msg
  assert msg.count('. ') == 0, msg      # one sentence


def test_nothing_refused_without_the_flag_or_for_the_device_environments():
  from model_based_rl_amd.evaluate import DEVICE_ENVS, refuse_device_env
  assert set(DEVICE_ENVS) == {'TicTacToe', 'ConnectFour', 'CartPole-v0', 'CartPole-v1'}
  refuse_device_env(_cfg(device_env=False, environment='LunarLander-v2', norm_obs=True))
  for env in DEVICE_ENVS:
    refuse_device_env(_cfg(environment=env))
  refuse_device_env(_cfg(environment='TicTacToe', apply_mcts_actions=3))


def test_refusal_reaches_the_evaluator_before_any_device(tmp_path):
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  cfg = make_config(['--environment', 'LunarLander-v2'])
  cfg.device_env = True
  with pytest.raises(NotImplementedError, match='no device form'):
    Evaluator({'config': cfg, 'weights': {}, 'training_step': 0})


def test_python_philox():
  # Philox4x32-10's published known answers (Random123 kat_vectors): all-zero and all-ones counter and key
  assert philox4x32(0, 0, 0, 0, 0) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
  assert philox4x32(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
  # the existing MZ_RNG_ACTION stream, as parity_util restates it (vectorised over the environments)
  for seed in (0, 11, (7 << 32) | 5):
    for move in (0, 3, (1 << 32) + 9):
      envs = np.array([0, 1, 17, 4095, 2 ** 31 + 3])
      want = philox_action_uniform(seed, envs, move)
      got = [philox_uniform(seed, int(e), move, MZ_RNG_ACTION) for e in envs]
      assert got == [float(x) for x in want], (seed, move)
  assert 0.0 <= philox_uniform(0, 100, 2, 7, 1) < 1.0 and philox_uniform(0, 100, 2, 7, 1) != philox_uniform(0, 100, 2, 7, 0)
