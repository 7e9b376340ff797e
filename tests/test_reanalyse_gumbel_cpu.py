"""--reanalyse_gumbel without a GPU (DESIGN s7j): the two flags and their defaults, every sentence of train's preflight, that the
old --selfplay_gumbel --reanalyse_rows refusal stands without the new flag and is gone with it, that a config saved by such a run
still gives a PUCT evaluation side, that the entry point is declared, and that scripts/tictactoe_learning.py passes the flags on."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '8']
BASE = PLAIN + ['--selfplay_gumbel', '--reanalyse_rows', '512', '--reanalyse_gumbel']


def _config(argv):
  from model_based_rl_amd.config import make_config
  return make_config(argv)


def test_flags_reach_the_config_with_their_defaults():
  off = _config(PLAIN)
  assert off.reanalyse_gumbel is False and off.reanalyse_gumbel_scale == 0.0
  cfg = _config(BASE)
  assert cfg.reanalyse_gumbel is True and cfg.reanalyse_gumbel_scale == 0.0 and cfg.reanalyse_rows == 512
  assert cfg.selfplay_gumbel_scale == 1.0      # (self-play keeps its own scale)
  cfg = _config(BASE + ['--reanalyse_gumbel_scale', '0.5'])
  assert cfg.reanalyse_gumbel_scale == 0.5 and cfg.selfplay_gumbel_scale == 1.0


def test_preflight_sentences():
  from model_based_rl_amd.reanalyse import refuse_reanalyse, refuse_reanalyse_gumbel
  from model_based_rl_amd.selfplay_search import refuse_selfplay_gumbel
  for argv in (BASE, BASE + ['--reanalyse_gumbel_scale', '1'], BASE + ['--selfplay_gumbel_value', 'vmix'],
               ['--environment', 'ConnectFour'] + BASE[2:], PLAIN, PLAIN + ['--reanalyse_rows', '512'],
               PLAIN + ['--reanalyse_gumbel_scale', '-1']):      # (the scale alone, the flag off: nothing is asked)
    cfg = _config(argv)
    refuse_reanalyse(cfg)
    refuse_reanalyse_gumbel(cfg)
    refuse_selfplay_gumbel(cfg)
  cases = [(PLAIN + ['--selfplay_gumbel', '--reanalyse_gumbel'], 'reanalyse_rows'),
           (PLAIN + ['--selfplay_gumbel', '--reanalyse_gumbel', '--reanalyse_rows', '0'], 'reanalyse_rows'),
           (PLAIN + ['--reanalyse_rows', '512', '--reanalyse_gumbel'], 'selfplay_gumbel'),
           (BASE + ['--reanalyse_gumbel_scale', '-0.5'], 'reanalyse_gumbel_scale'),
           (BASE + ['--reanalyse_gumbel_scale', 'nan'], 'reanalyse_gumbel_scale')]
  seen = set()
  for argv, word in cases:
    with pytest.raises(SystemExit) as exc:
      refuse_reanalyse_gumbel(_config(argv))
    msg = str(exc.value)
    assert msg.startswith('--reanalyse_gumbel: ') and word in msg and msg.count('. ') == 0 and msg.endswith('.'), msg
    seen.add(msg.split(',')[0])
  assert len(seen) == 3      # (the two row cases and the two scale cases share their sentences)


def test_reanalyse_rows_own_refusals_apply_as_before():
  from model_based_rl_amd.reanalyse import refuse_reanalyse
  with pytest.raises(SystemExit) as exc:
    refuse_reanalyse(_config(BASE), ranks=2)
  assert str(exc.value).startswith('--reanalyse_rows: ') and 'ranks' in str(exc.value)
  with pytest.raises(SystemExit) as exc:
    refuse_reanalyse(_config(BASE + ['--norm_obs']))
  assert str(exc.value).startswith('--reanalyse_rows: ') and 'norm_obs' in str(exc.value)


def test_the_old_refusal_stands_without_the_flag_and_is_gone_with_it():
  from model_based_rl_amd.selfplay_search import refuse_selfplay_gumbel
  with pytest.raises(SystemExit) as exc:
    refuse_selfplay_gumbel(_config(PLAIN + ['--selfplay_gumbel', '--reanalyse_rows', '512']))
  msg = str(exc.value)
  assert msg.startswith('--selfplay_gumbel: --reanalyse_rows would mix visit-share and pi\' policy targets in one replay'), msg
  assert 'reanalyse_gumbel' in msg and msg.count('. ') == 0 and msg.endswith('.')      # (and it points to the new flag)
  refuse_selfplay_gumbel(_config(BASE))
  with pytest.raises(SystemExit) as exc:      # the mode's other refusals are untouched by the new flag
    refuse_selfplay_gumbel(_config(BASE), ranks=2)
  assert 'ranks' in str(exc.value)


def test_train_main_asks_before_any_device(monkeypatch):
  from model_based_rl_amd import train
  called = []
  monkeypatch.setattr(train, 'launch', lambda *a, **k: called.append(a))
  for argv, start in ((PLAIN + ['--selfplay_gumbel', '--reanalyse_gumbel'], '--reanalyse_gumbel: '),
                      (PLAIN + ['--reanalyse_rows', '512', '--reanalyse_gumbel'], '--reanalyse_gumbel: '),
                      (BASE + ['--reanalyse_gumbel_scale', '-1'], '--reanalyse_gumbel: '),
                      (PLAIN + ['--selfplay_gumbel', '--reanalyse_rows', '512'], '--selfplay_gumbel: '),
                      (BASE + ['--num_envs', '1'], '--reanalyse_rows: ')):
    with pytest.raises(SystemExit) as exc:
      train.main(argv)
    assert str(exc.value).startswith(start) and not called, (argv, str(exc.value))
  train.main(BASE)
  assert len(called) == 1
  cfg = called[0][0]
  assert cfg.selfplay_gumbel is True and cfg.reanalyse_gumbel is True and cfg.reanalyse_rows == 512 and cfg.reanalyse_gumbel_scale == 0.0


def test_a_saved_config_still_gives_a_puct_evaluation_side():
  from model_based_rl_amd.sides import Side
  cfg = _config(BASE + ['--reanalyse_gumbel_scale', '1'])
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1).items():
    setattr(cfg, k, v)      # (what evaluate / match set on a checkpoint's config)
  side = Side.of(cfg)
  assert side.gumbel is None and side.search == 'puct' and side.num_simulations == 8
  assert not any(k.startswith('gumbel') for k in vars(cfg))
  asked = Side.of(cfg, gumbel=True)      # evaluate --gumbel 1 on such a checkpoint: the evaluation defaults, not the training scales
  assert asked.gumbel['gumbel_scale'] == 0.0 and asked.gumbel['max_considered'] == 16


def test_entry_point_is_declared():
  import ctypes as C
  from model_based_rl_amd import _abi
  from model_based_rl_amd.engine import Engine
  from tests.test_abi import declared_symbols
  assert 'mz_reanalyse_gumbel' in declared_symbols(('mz_engine.h',))
  res, args = _abi.SIGNATURES['mz_reanalyse_gumbel']
  plain = _abi.SIGNATURES['mz_reanalyse'][1]
  assert res is C.c_int and args == plain[:-1] + [C.c_int, C.c_uint64] + plain[-1:]      # value_kind and draw_key before the stream
  assert callable(Engine.reanalyse_gumbel)


def _script():
  spec = importlib.util.spec_from_file_location('tictactoe_learning', os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_learning_script_passes_the_flags_on():
  from model_based_rl_amd.reanalyse import refuse_reanalyse, refuse_reanalyse_gumbel
  from model_based_rl_amd.selfplay_search import refuse_selfplay_gumbel
  mod = _script()
  ap = mod.build_parser()
  base, extra = mod.recipe(ap.parse_args(['--reanalyse_rows', '4096']))
  assert extra == ['--reanalyse_rows', '4096']      # as before
  a = ap.parse_args(['--selfplay_gumbel', '--num_simulations', '8', '--reanalyse_rows', '4096', '--reanalyse_gumbel'])
  base, extra = mod.recipe(a)
  run = _config(base + extra)      # the training run's config
  assert run.selfplay_gumbel and run.num_simulations == 8 and run.reanalyse_rows == 4096
  assert run.reanalyse_gumbel is True and run.reanalyse_gumbel_scale == 0.0
  for refuse in (refuse_reanalyse, refuse_reanalyse_gumbel, refuse_selfplay_gumbel):
    refuse(run)
  a = ap.parse_args(['--selfplay_gumbel', '--num_simulations', '8', '--reanalyse_rows', '4096', '--reanalyse_every', '64',
                     '--reanalyse_gumbel', '--reanalyse_gumbel_scale', '0.25'])
  base, extra = mod.recipe(a)
  run = _config(base + extra)
  assert run.reanalyse_gumbel is True and run.reanalyse_gumbel_scale == 0.25 and run.reanalyse_every == 64
  evaluated = _config(base)          # what the evaluation blocks build their configs from: no Reanalyse, PUCT at 30 simulations
  assert evaluated.reanalyse_gumbel is False and evaluated.reanalyse_rows == 0 and evaluated.num_simulations == 30
