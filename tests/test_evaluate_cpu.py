"""CPU-side checks of the evaluator (model_based_rl_amd.evaluate, the reference's evaluate.py): its flags and defaults, the
configurations and labels state_generator expands, the summary numbers, the refused interactive flags, and the resource
usage of the new kernels (csrc/mz_eval.hip.h, gfx950 cross-compile)."""
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evaluation_args_defaults():
  from model_based_rl_amd.config import get_evaluation_args
  a = get_evaluation_args([])
  # the reference's defaults (config.py:233-262)
  assert a.seed is None and a.num_games == 1 and a.saves_dir == [''] and a.nets == ['']
  assert a.num_simulations == [None] and a.temperatures == [0] and a.only_prior == [0] and a.only_value == [0]
  assert a.use_exploration_noise == [0] and a.apply_mcts_actions == [1]
  assert not a.render and a.sleep == 0 and a.human_opp is None and a.random_opp is None and not a.plot_summary
  assert a.save_gif_as == '' and not a.save_mcts and a.save_mcts_after_step == 0 and not a.parallel and not a.verbose
  # the additions
  assert a.batch == 1 and a.out is None
  assert get_evaluation_args(['--num_games', '10000']).batch == 4096
  assert get_evaluation_args(['--num_games', '100']).batch == 100
  assert get_evaluation_args(['--num_games', '100', '--batch', '7']).batch == 7
  with pytest.raises(SystemExit):
    get_evaluation_args(['--random_opp', '0'])


def _checkpoint(tmp_path, step=123):
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'])
  torch.manual_seed(0)
  net = get_network(cfg, torch.device('cpu'))
  saves = tmp_path / 'saves'
  saves.mkdir(parents=True, exist_ok=True)
  torch.save({'config': cfg, 'weights': net.state_dict(), 'training_step': step}, str(saves / str(step)))
  return str(saves) + os.sep, str(step)


def test_state_generator_configurations_and_labels(tmp_path):
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import state_generator
  saves, net = _checkpoint(tmp_path)
  argv = ['--saves_dir', saves, saves, '--nets', net, '--temperatures', '0', '0.5', '--num_simulations', '10', '30',
          '--only_prior', '0', '1', '--only_value', '0', '1', '--use_exploration_noise', '0', '1', '--apply_mcts_actions', '1', '3',
          '--detailed_label', '--random_opp', '-1']
  states = list(state_generator(get_evaluation_args(argv)))
  # 2 dirs x 1 net x 2 temperatures x 2 sims x (2 x 2 - 1: only_prior with only_value excluded) x 2 noise x 2 mcts actions
  assert len(states) == 2 * 2 * 2 * 3 * 2 * 2
  labels = [s['config'].label for s in states]
  assert 'net:123, path:0, sims:10' in labels
  assert 'net:123, path:1, sims:30, mcts-actions:3, temp:0.5, with noise' in labels
  assert 'net:123, path:0, only value' in labels and 'net:123, path:1, only prior' in labels
  assert not any(s['config'].only_prior and s['config'].only_value for s in states)
  c = states[0]['config']
  assert c.random_opp == -1 and c.num_simulations == 10 and c.batch == 1 and c.saves_dir == saves
  # without --detailed_label every configuration is labelled by its network alone (evaluate.py:387-404)
  plain = list(state_generator(get_evaluation_args(['--saves_dir', saves, '--nets', net])))
  assert len(plain) == 1 and plain[0]['config'].label == 'net:123'
  assert plain[0]['config'].num_simulations == 30        # --num_simulations None keeps the checkpoint's


def _game(step, rewards, pred_rewards, pred_values, root_values, search_depths):
  g = types.SimpleNamespace(step=step, pred_rewards=pred_rewards, pred_values=pred_values, search_depths=search_depths)
  g.history = types.SimpleNamespace(rewards=rewards, root_values=root_values)
  return g


def test_print_summary_numbers(capsys):
  from model_based_rl_amd.evaluate import SummaryTools
  st = SummaryTools()
  st.config = types.SimpleNamespace(label='net:7')
  games = [_game(3, [0, 0, 1], [0.5, 0.25, 1.0], [0.1, 0.2, 0.3], [0.0, 0.5, 1.0], [[2, 9], [3, 2], [3, 1, 1]]),
           _game(5, [0, 0, 0, 0, -1], [0, 0, 0, 0, 0], [1.0], [2.0], [[1], [1]])]
  s = st.print_summary(games)
  assert s['length'] == [4.0, 1.0]
  assert s['return'] == [0.0, 1.0]
  assert s['pred_return'] == [pytest.approx(0.875), pytest.approx(0.875)]
  assert s['pred_value'][0] == pytest.approx((0.2 + 1.0) / 2)
  assert s['mcts_value'][0] == pytest.approx((0.5 + 2.0) / 2)
  # max() of lists is lexicographic: [3, 2] beats [3, 1, 1] and [2, 9] -> mean 2.5 (the deepest simulation, 9, is not it)
  assert s['search_depth'] == [pytest.approx((2.5 + 1.0) / 2), pytest.approx(0.75)]
  out = capsys.readouterr().out
  assert 'Evaluation finished! - label: (net:7)' in out
  for line in ('Average length: 4.0(1.0)', 'Average return: 0.0(1.0)', 'Average predicted return: 0.9(0.9)',
               'Average predicted value: 0.6(0.4)', 'Average mcts value: 1.2(0.8)', 'Average search depth: 1.8(0.8)'):
    assert line in out, (line, out)


@pytest.mark.parametrize('flag', [['--render'], ['--save_gif_as', 'x'], ['--save_mcts'], ['--human_opp', '1'],
                                  ['--plot_summary']])
def test_interactive_flags_refused(flag, tmp_path):
  from model_based_rl_amd import evaluate
  saves, net = _checkpoint(tmp_path)
  with pytest.raises(NotImplementedError) as ei:
    evaluate.main(['--saves_dir', saves, '--nets', net] + flag)
  msg = str(ei.value)
  assert msg.startswith(flag[0]) and msg.count('.') == 1 and msg.endswith('.'), msg     # one sentence


def test_conv_networks_refused():
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  cfg = make_config(['--environment', 'BreakoutNoFrameskip-v4', '--architecture', 'MuZeroNetwork'])
  with pytest.raises(NotImplementedError, match='FCNetwork'):
    Evaluator({'config': cfg, 'weights': {}, 'training_step': 0})


def test_eval_kernels_resource_usage():
  """the new kernels compile for gfx950 without scratch (private arrays spilled to memory would put every select_action
  step of the walk behind a scratch round trip)"""
  from model_based_rl_amd import _abi
  if shutil.which('hipcc') is None:
    pytest.skip('hipcc not on PATH')
  csrc = os.path.join(os.path.dirname(_abi.__file__), 'csrc')
  unit = ('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "mz_engine.h"\n#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS\n'
          '#include "mz_eval.hip.h"\n'
          'template __global__ void k_eval_rows<1>(NetView, TreeView, int, const int32_t *, int, float *, float *, float *, float *);\n'
          'template __global__ void k_eval_rows<2>(NetView, TreeView, int, const int32_t *, int, float *, float *, float *, float *);\n')
  with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, 'eval_unit.hip')
    with open(src, 'w') as f:
      f.write(unit)
    r = subprocess.run(['hipcc'] + list(_abi.HIPCC_FLAGS) + ['-I', csrc, '-I', os.path.join(ROOT, 'include'),
                        '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.path.join(tmp, 'eval_unit.o')],
                       capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-2000:]
  usage, cur = {}, None
  for line in r.stderr.splitlines():
    m = re.search(r'remark: +Function Name: (\S+)', line)
    if m:
      cur = usage.setdefault(m.group(1), {})
    m = re.search(r'remark: +(VGPRs|ScratchSize \[bytes/lane\]): (\d+)', line)
    if m and cur is not None:
      cur[m.group(1).split(' [')[0]] = int(m.group(2))
  ours = {k: v for k, v in usage.items() if 'k_eval_' in k}
  assert len(ours) == 5, sorted(usage)          # walk, rows<1>, rows<2>, choose_value, choose_prior
  for k, v in ours.items():
    assert v['ScratchSize'] == 0, (k, v)
    assert v['VGPRs'] <= 128, (k, v)            # (a 64-lane walk wave and the 256-thread row tiles keep >= 4 / 3 waves per SIMD)
