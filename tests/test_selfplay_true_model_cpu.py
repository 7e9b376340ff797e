"""--selfplay_true_model without a GPU (DESIGN s7k): the flags and their defaults, every refusal of train's preflight, that a
config saved by such a run does not turn its checkpoint's evaluation into the true-rules search, and that
scripts/tictactoe_learning.py passes the flags on to the training run and to nothing else."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '30', '--selfplay_true_model']


def _config(argv):
  from model_based_rl_amd.config import make_config
  return make_config(argv)


def test_flags_reach_the_config_with_their_defaults():
  off = _config(BASE[:-1])
  assert off.selfplay_true_model is False and off.selfplay_true_model_loop is False
  cfg = _config(BASE)
  assert cfg.selfplay_true_model is True and cfg.selfplay_true_model_loop is False
  cfg = _config(BASE + ['--selfplay_true_model_loop'])
  assert cfg.selfplay_true_model is True and cfg.selfplay_true_model_loop is True
  assert not any(k == 'true_model' for k in vars(cfg))      # (the evaluation's flag is another one)


def test_preflight_refusals():
  from model_based_rl_amd.train import refuse_selfplay_true_model
  for env in ('TicTacToe', 'ConnectFour'):
    refuse_selfplay_true_model(_config(['--environment', env] + BASE[2:]))
    refuse_selfplay_true_model(_config(['--environment', env] + BASE[2:] + ['--symmetry']))      # --symmetry goes with it
    refuse_selfplay_true_model(_config(['--environment', env] + BASE[2:] + ['--selfplay_true_model_loop']), ranks=1)
  refuse_selfplay_true_model(_config(['--environment', 'LunarLander-v2', '--split_f16', '--reanalyse_rows', '8']), ranks=4)   # off: nothing is asked
  cases = [(['--environment', 'LunarLander-v2', '--num_envs', '64', '--selfplay_true_model'], {}, 'board games'),
           (['--environment', 'CartPole-v1', '--num_envs', '64', '--selfplay_true_model'], {}, 'CartPole-v1 has none'),
           (BASE + ['--architecture', 'MuZeroNetwork'], {}, 'FCNetwork'),
           (BASE[:3] + ['--num_envs', '1', '--selfplay_true_model'], {}, 'host-environment'),
           (BASE + ['--parity_rng'], {}, 'host-environment'),
           (BASE + ['--split_f16'], {}, 'split_f16'),
           (BASE, dict(ranks=2), 'ranks'),
           (BASE + ['--selfplay_gumbel'], {}, 'selfplay_gumbel'),
           (BASE + ['--reanalyse_rows', '512'], {}, 'reanalyse_rows')]
  seen = set()
  for argv, kw, word in cases:
    with pytest.raises(SystemExit) as exc:
      refuse_selfplay_true_model(_config(argv), **kw)
    msg = str(exc.value)
    assert msg.startswith('--selfplay_true_model: ') and word in msg and msg.count('. ') == 0 and msg.endswith('.'), msg
    seen.add(msg)
  assert len(seen) == len(cases) - 1      # (the two host-environment cases share their sentence)
  with pytest.raises(SystemExit) as exc:      # the option without the flag
    refuse_selfplay_true_model(_config(BASE[:-1] + ['--selfplay_true_model_loop']))
  assert str(exc.value).startswith('--selfplay_true_model_loop: ')


def test_train_main_asks_before_any_device(monkeypatch):
  from model_based_rl_amd import train
  called = []
  monkeypatch.setattr(train, 'launch', lambda *a, **k: called.append(a))
  with pytest.raises(SystemExit) as exc:
    train.main(BASE + ['--reanalyse_rows', '512'])
  assert str(exc.value).startswith('--selfplay_true_model: ') and not called
  with pytest.raises(SystemExit) as exc:
    train.main(BASE + ['--ranks', '2'])
  assert str(exc.value).startswith('--selfplay_true_model: ') and 'ranks' in str(exc.value) and not called
  train.main(BASE)
  assert len(called) == 1 and called[0][0].selfplay_true_model is True


def test_a_saved_config_does_not_make_the_evaluation_side_true_rules():
  from model_based_rl_amd.sides import Side
  cfg = _config(BASE + ['--selfplay_true_model_loop'])
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1).items():
    setattr(cfg, k, v)      # (what evaluate / match set on a checkpoint's config)
  side = Side.of(cfg)
  assert side.true_model is False and side.gumbel is None and side.search == 'puct' and side.num_simulations == 30
  assert Side.of(cfg, true_model=1).search == 'true_rules'      # evaluate --true_model 1 on such a checkpoint still asks for it


def _script():
  spec = importlib.util.spec_from_file_location('tictactoe_learning', os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_learning_script_passes_the_flags_on():
  from model_based_rl_amd.train import refuse_selfplay_true_model
  mod = _script()
  ap = mod.build_parser()
  base, extra = mod.recipe(ap.parse_args([]))
  assert 'selfplay_true_model' not in ' '.join(base + extra) and extra == []      # as before
  for env in ('TicTacToe', 'ConnectFour'):
    for loop in (False, True):
      a = ap.parse_args(['--environment', env, '--selfplay_true_model', '--symmetry'] + (['--selfplay_true_model_loop'] if loop else []))
      base, extra = mod.recipe(a)
      run = _config(base + extra)      # the training run's config
      assert run.environment == env and run.selfplay_true_model is True and run.selfplay_true_model_loop is loop
      assert run.num_simulations == 30 and run.symmetry is True
      refuse_selfplay_true_model(run)
      evaluated = _config(base)          # what the evaluation blocks build their configs from: the plain search
      assert evaluated.selfplay_true_model is False and not getattr(evaluated, 'true_model', 0)
