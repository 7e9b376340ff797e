"""--selfplay_gumbel without a GPU (DESIGN s7i): the flags and their defaults, every refusal of train's preflight, that a config
saved by such a run does not turn its checkpoint's evaluation into the Gumbel search, and that scripts/tictactoe_learning.py
passes the flags on to the training run and to nothing else."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '8', '--selfplay_gumbel']


def _config(argv):
  from model_based_rl_amd.config import make_config
  return make_config(argv)


def test_flags_reach_the_config_with_their_defaults():
  from model_based_rl_amd.selfplay_search import selfplay_gumbel_params
  off = _config(BASE[:-1])
  assert off.selfplay_gumbel is False
  cfg = _config(BASE)
  assert cfg.selfplay_gumbel is True
  assert (cfg.selfplay_gumbel_considered, cfg.selfplay_gumbel_c_visit, cfg.selfplay_gumbel_c_scale, cfg.selfplay_gumbel_scale) == (16, 50.0, 1.0, 1.0)
  assert cfg.selfplay_gumbel_value == 'mean'
  assert selfplay_gumbel_params(cfg) == (16, 50.0, 1.0, 1.0)
  cfg = _config(BASE + ['--selfplay_gumbel_considered', '4', '--selfplay_gumbel_c_visit', '25', '--selfplay_gumbel_c_scale', '0.5',
                        '--selfplay_gumbel_scale', '0.25', '--selfplay_gumbel_value', 'vmix'])
  assert selfplay_gumbel_params(cfg) == (4, 25.0, 0.5, 0.25) and cfg.selfplay_gumbel_value == 'vmix'
  with pytest.raises(SystemExit):
    _config(BASE + ['--selfplay_gumbel_value', 'median'])


def test_train_refusals_are_one_sentence_each():
  from model_based_rl_amd.train import refuse_selfplay_gumbel
  for env in ('TicTacToe', 'ConnectFour'):
    refuse_selfplay_gumbel(_config(['--environment', env] + BASE[2:]))
    refuse_selfplay_gumbel(_config(['--environment', env] + BASE[2:] + ['--symmetry']))      # pi' moves with the policy targets
  for env in ('CartPole-v0', 'CartPole-v1'):
    refuse_selfplay_gumbel(_config(['--environment', env, '--num_envs', '64', '--selfplay_gumbel']), ranks=1)
  refuse_selfplay_gumbel(_config(['--environment', 'LunarLander-v2', '--split_f16', '--reanalyse_rows', '8']), ranks=4)   # off: nothing is asked
  cases = [(['--environment', 'LunarLander-v2', '--num_envs', '64', '--selfplay_gumbel'], {}, 'device games'),
           (BASE + ['--architecture', 'TinyNetwork'], {}, 'FCNetwork'),
           (BASE + ['--parity_rng'], {}, 'host-environment'),
           (BASE[:3] + ['--num_envs', '1', '--selfplay_gumbel'], {}, 'host-environment'),
           (BASE + ['--split_f16'], {}, 'split_f16'),
           (BASE, dict(ranks=2), 'ranks'),
           (BASE + ['--reanalyse_rows', '512'], {}, 'reanalyse_rows'),
           (BASE + ['--selfplay_gumbel_considered', '1'], {}, 'selfplay_gumbel_considered'),
           (BASE + ['--selfplay_gumbel_c_visit', '-1'], {}, 'selfplay_gumbel_c_visit'),
           (BASE + ['--selfplay_gumbel_c_scale', '0'], {}, 'selfplay_gumbel_c_scale'),
           (BASE + ['--selfplay_gumbel_scale', '-0.5'], {}, 'selfplay_gumbel_scale'),
           (BASE + ['--selfplay_gumbel_scale', 'nan'], {}, 'selfplay_gumbel_scale')]
  seen = set()
  for argv, kw, word in cases:
    with pytest.raises(SystemExit) as exc:
      refuse_selfplay_gumbel(_config(argv), **kw)
    msg = str(exc.value)
    assert msg.startswith('--selfplay_gumbel: ') and word in msg and msg.count('. ') == 0 and msg.endswith('.'), msg
    seen.add(msg.split(',')[0])
  assert len(seen) >= len(cases) - 2      # (the two host-environment and the two scale cases share their sentences)


def test_train_main_asks_before_any_device(monkeypatch):
  from model_based_rl_amd import train
  called = []
  monkeypatch.setattr(train, 'launch', lambda *a, **k: called.append(a))
  with pytest.raises(SystemExit) as exc:
    train.main(BASE + ['--reanalyse_rows', '512'])
  assert str(exc.value).startswith('--selfplay_gumbel: ') and not called
  with pytest.raises(SystemExit) as exc:
    train.main(BASE + ['--ranks', '2'])
  assert str(exc.value).startswith('--selfplay_gumbel: ') and 'ranks' in str(exc.value) and not called
  train.main(BASE)
  assert len(called) == 1 and called[0][0].selfplay_gumbel is True


def test_a_saved_config_does_not_make_the_evaluation_side_gumbel():
  from model_based_rl_amd.sides import Side
  cfg = _config(BASE + ['--selfplay_gumbel_value', 'vmix'])
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1).items():
    setattr(cfg, k, v)      # (what evaluate / match set on a checkpoint's config)
  side = Side.of(cfg)
  assert side.gumbel is None and side.search == 'puct' and side.num_simulations == 8
  assert not any(k.startswith('gumbel') for k in vars(cfg))
  asked = Side.of(cfg, gumbel=True)      # evaluate --gumbel 1 on such a checkpoint: the evaluation defaults, scale 0 -- not the training scale
  assert asked.gumbel['gumbel_scale'] == 0.0 and asked.gumbel['max_considered'] == 16


def _script():
  spec = importlib.util.spec_from_file_location('tictactoe_learning', os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_learning_script_passes_the_flags_on():
  mod = _script()
  ap = mod.build_parser()
  base, extra = mod.recipe(ap.parse_args([]))
  assert 'selfplay_gumbel' not in ' '.join(base + extra) and extra == []      # as before
  for env in ('TicTacToe', 'ConnectFour'):
    a = ap.parse_args(['--environment', env, '--selfplay_gumbel', '--num_simulations', '8', '--selfplay_gumbel_value', 'vmix',
                       '--selfplay_gumbel_considered', '4', '--selfplay_gumbel_scale', '0.5', '--symmetry'])
    base, extra = mod.recipe(a)
    run = _config(base + extra)      # the training run's config
    assert run.environment == env and run.selfplay_gumbel is True and run.num_simulations == 8 and run.symmetry is True
    assert run.selfplay_gumbel_value == 'vmix' and run.selfplay_gumbel_considered == 4 and run.selfplay_gumbel_scale == 0.5
    assert run.selfplay_gumbel_c_visit == 50.0 and run.selfplay_gumbel_c_scale == 1.0
    from model_based_rl_amd.train import refuse_selfplay_gumbel
    refuse_selfplay_gumbel(run)
    evaluated = _config(base)          # what the evaluation blocks build their configs from: PUCT at 30 simulations
    assert evaluated.selfplay_gumbel is False and evaluated.num_simulations == 30 and not getattr(evaluated, 'gumbel', 0)
