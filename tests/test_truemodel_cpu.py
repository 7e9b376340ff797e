"""The true-rules search without a GPU (DESIGN s7g):
  twin       mz_tm_search_host -- sequential C++, the rules of csrc/mz_games.h -- equals the Python restatement of
             tests/truemodel_py.py (dict Nodes after the reference's mcts.py, the rules of tests/playout_py.py) in every field.
             The tolerance is zero: both sides use glibc's exp / log / sqrt on the same float32 network outputs, in the same
             IEEE double operation order
  reach      the shared positions reach the cases that can go wrong
  invariants of the exported trees, checked in plain Python
  refusals   one test per sentence of evaluate.refuse_true_model, the label and the --out key on a stub engine"""
import json
import types

import numpy as np
import pytest

from tests import playout_py as pp
from tests import truemodel_py as tp

SIMS = tp.SIMS


def _cfg(kind, n, sims=SIMS):
  from model_based_rl_amd.engine import mz_config
  A, O = (9, 9) if kind == 1 else (7, 42)
  return mz_config(n, O, A, sims, two_players=True)


@pytest.fixture(scope='module')
def searched():
  """per (kind, with noise): (the host twin's trees, the restatement's, the positions)"""
  from model_based_rl_amd.engine import tm_search_host
  out = {}
  for kind in (1, 3):
    A = 9 if kind == 1 else 7
    bd, tn, st, lg, noise = tp.case_positions(kind)
    for with_noise in (False, True):
      nz = noise if with_noise else None
      host = tm_search_host(_cfg(kind, len(bd)), kind, bd, tn, st, lg, lambda obs: tp.fake_network(obs, A), noise=nz)
      want = tp.search_batch(kind, bd, tn, st, lg, SIMS, noise=nz)
      out[kind, with_noise] = (host, want, (bd, tn, st))
  return out


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
@pytest.mark.parametrize('with_noise', [False, True], ids=['plain', 'noise'])
def test_host_twin_equals_the_restatement(searched, kind, with_noise):
  host, want, _ = searched[kind, with_noise]
  assert np.array_equal(host['EX'], want['EX'])
  ex = want['EX'] == 1
  for key in tp.TREE_FIELDS:
    diff = np.argwhere((host[key] != want[key]) & ex)
    assert len(diff) == 0, (key, diff[:5].tolist())
  for key in ('nexp', 'legal', 'minmax', 'leaf_depth') + tp.SLOT_FIELDS:
    assert np.array_equal(host[key], np.asarray(want[key]).astype(host[key].dtype)), key
  # an illegal child of a taken slot is marked as at the root: to_play 0, prior 0, never visited, never expanded
  A = 9 if kind == 1 else 7
  for b in range(len(host['nexp'])):
    taken = np.zeros(host['EX'].shape[1], bool)
    taken[1:1 + int(host['nexp'][b]) * A] = True
    gone = taken & (host['EX'][b] == 0)
    assert not host['TP'][b][gone].any() and not host['P'][b][gone].any() and not host['N'][b][gone].any()
    assert (host['E'][b][gone] == -1).all()


def array_digests(d):
  """SHA-256 of every array a host twin returns (C order, its own dtype)"""
  import hashlib
  return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in d.items()}


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
@pytest.mark.parametrize('with_noise', [False, True], ids=['plain', 'noise'])
def test_host_twin_reproduces_the_pinned_outputs(searched, kind, with_noise):
  """Every output array of mz_tm_search_host on the committed positions, bit for bit, as the twin gave it before its tree
  code moved into csrc/mz_tree_host.h -- leaf_depth and the slot records included, which the restatement does not all
  cover.  tests/golden/search_twins_sha256.json holds the digests of both twins (keys tm/<kind>/<plain|noise> and
  gz/<set>/<scale>); from a checkout of the commit to pin, built, in the repository root:

    import json
    from tests import gumbel_py as gp, truemodel_py as tp
    from tests.test_gumbel_cpu import host_search
    from tests.test_truemodel_cpu import _cfg, array_digests
    from model_based_rl_amd.engine import tm_search_host
    out = {}
    for kind in (1, 3):
      A = 9 if kind == 1 else 7
      bd, tn, st, lg, noise = tp.case_positions(kind)
      for name, nz in (('plain', None), ('noise', noise)):
        host = tm_search_host(_cfg(kind, len(bd)), kind, bd, tn, st, lg, lambda obs: tp.fake_network(obs, A), noise=nz)
        out['tm/%d/%s' % (kind, name)] = array_digests(host)
    for name in gp.SETS:
      for scale in (1.0, 0.0):
        out['gz/%s/%g' % (name, scale)] = array_digests(host_search(gp.case(name), scale))
    json.dump(out, open('tests/golden/search_twins_sha256.json', 'w'), indent=1, sort_keys=True)"""
  import os
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'search_twins_sha256.json')) as f:
    want = json.load(f)['tm/%d/%s' % (kind, 'noise' if with_noise else 'plain')]
  got = array_digests(searched[kind, with_noise][0])
  assert sorted(got) == sorted(want)
  assert [k for k in sorted(got) if got[k] != want[k]] == []


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
def test_the_positions_reach_the_cases_that_can_go_wrong(searched, kind):
  host, _, (bd, tn, st) = searched[kind, False]
  A = 9 if kind == 1 else 7
  full = (1 << A) - 1
  n = len(bd)
  fin_slot = [(b, e) for b in range(n) for e in range(1, int(host['nexp'][b])) if host['finished'][b, e]]
  assert fin_slot, 'no finished node has its slot'
  E, N = host['E'], host['N']
  twice = [(b, e) for b, e in fin_slot if N[b][np.flatnonzero((E[b] == e) & (host['EX'][b] == 1))[0]] >= 2]
  assert twice, 'no finished node was visited twice'
  assert (SIMS + 1 - host['nexp']).sum() >= len(twice)      # revisits take no slot
  live = host['finished'] == 0
  taken = np.arange(SIMS + 1)[None, :] < host['nexp'][:, None]
  assert ((host['mask'] != full) & live & taken & (np.arange(SIMS + 1)[None, :] > 0)).any(), 'no node below a root has an illegal child'
  assert host['leaf_depth'].max() >= 3
  if kind == 3:
    assert any(bin(int(m)).count('1') == 1 for m in host['legal']), 'no root with a single legal action'


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
@pytest.mark.parametrize('with_noise', [False, True], ids=['plain', 'noise'])
def test_invariants_of_the_exported_trees(searched, kind, with_noise):
  host, _, (bd, tn, st) = searched[kind, with_noise]
  A = 9 if kind == 1 else 7
  cells = 9 if kind == 1 else 42
  for b in range(len(bd)):
    nexp = int(host['nexp'][b])
    assert host['N'][b, 0] == SIMS      # N[root] = the simulations run
    parent_of = {}
    for k in np.flatnonzero(host['EX'][b]):
      e = int(host['E'][b, k])
      if k > 0 and e >= 0:
        assert e not in parent_of and 1 <= e < nexp
        parent_of[e] = ((k - 1) // A, (k - 1) % A)
    assert sorted(parent_of) == list(range(1, nexp))
    for e in range(nexp):
      board = host['boards'][b, e, :cells].tolist()
      legal = pp.legal_actions(kind, board)
      mask = int(host['mask'][b, e])
      if host['finished'][b, e]:
        assert mask == 0      # no node exists below a finished one
        assert not host['EX'][b, 1 + e * A:1 + (e + 1) * A].any()
      else:
        assert [a for a in range(A) if (mask >> a) & 1] == legal      # every existing child is legal in its parent's position
      if e > 0:
        pe, a = parent_of[e]
        pb = host['boards'][b, pe, :cells].tolist()
        assert not host['finished'][b, pe] and a in pp.legal_actions(kind, pb)
        end = pp.play(kind, pb, int(host['mover'][b, pe]), a)
        assert pb == board and host['mover'][b, e] == -host['mover'][b, pe] and host['step'][b, e] == host['step'][b, pe] + 1
        assert bool(host['finished'][b, e]) == (end != 0)
        node = 1 + pe * A + a
        assert host['R'][b, node] == (1.0 if end == 1 else 0.0)      # R is 1 exactly when the move into it won
        assert host['TP'][b, node] == host['mover'][b, e]
    visited = (host['N'][b] > 0) & (host['EX'][b] == 1)
    assert set(host['R'][b][visited].tolist()) <= {0.0, 1.0}


def test_a_partial_search_and_its_continuation_are_prefixes():
  """fewer simulations than the trees are sized for: the first k simulations of the full search"""
  from model_based_rl_amd.engine import tm_search_host
  bd, tn, st, lg, _ = tp.case_positions(1)
  bd, tn, st, lg = bd[:32], tn[:32], st[:32], lg[:32]
  net = lambda obs: tp.fake_network(obs, 9)
  part = tm_search_host(_cfg(1, 32), 1, bd, tn, st, lg, net, num_simulations=7)
  want = tp.search_batch(1, bd, tn, st, lg, SIMS, num_simulations=7)
  assert np.array_equal(part['EX'], want['EX']) and np.array_equal(part['N'][:, 0], np.full(32, 7))
  for key in tp.TREE_FIELDS:
    assert np.array_equal(part[key][want['EX'] == 1], want[key][want['EX'] == 1]), key


def test_host_twin_refusals():
  from model_based_rl_amd.engine import mz_config, tm_search_host
  bd, tn, st, lg, _ = tp.case_positions(1)
  net = lambda obs: tp.fake_network(obs, 9)
  with pytest.raises(RuntimeError, match='mz_tm_search_host: kind must be 1'):
    tm_search_host(_cfg(1, 4), 2, bd[:4], tn[:4], st[:4], lg[:4], net)
  with pytest.raises(RuntimeError, match='mz_tm_search_host: Connect Four needs obs_dim 42'):
    tm_search_host(_cfg(1, 4), 3, bd[:4], tn[:4], st[:4], lg[:4], net)
  with pytest.raises(RuntimeError, match='simulations exceed'):
    tm_search_host(_cfg(1, 4), 1, bd[:4], tn[:4], st[:4], lg[:4], net, num_simulations=SIMS + 1)
  with pytest.raises(RuntimeError, match='TicTacToe needs .* two_players'):
    tm_search_host(mz_config(4, 9, 9, SIMS), 1, bd[:4], tn[:4], st[:4], lg[:4], net)


# ---- the command line
def _args(**kv):
  base = dict(true_model=1, device_env=True, environment='TicTacToe', apply_mcts_actions=1, only_prior=0, only_value=0,
              architecture='FCNetwork')
  base.update(kv)
  return types.SimpleNamespace(**base)


def test_cli_refuses_the_host_path():
  from model_based_rl_amd.evaluate import refuse_true_model
  with pytest.raises(NotImplementedError, match=r'^--true_model: .*needs --device_env \(or --match\)\.$'):
    refuse_true_model(_args(device_env=False))
  refuse_true_model(_args(device_env=False), match=True)


@pytest.mark.parametrize('env', ['CartPole-v1', 'LunarLander-v2'])
def test_cli_refuses_an_environment_without_rules(env):
  from model_based_rl_amd.evaluate import refuse_true_model
  with pytest.raises(NotImplementedError, match=r'^--true_model: %s has no true-rules search; it searches TicTacToe and ConnectFour\.$' % env):
    refuse_true_model(_args(environment=env))


@pytest.mark.parametrize('m', [2, 0, [1, 3]])
def test_cli_refuses_more_than_one_applied_action(m):
  from model_based_rl_amd.evaluate import refuse_true_model
  with pytest.raises(NotImplementedError, match=r'^--true_model: .*--apply_mcts_actions 1 only\.$'):
    refuse_true_model(_args(apply_mcts_actions=m))


def test_cli_refuses_a_lookahead_on_the_same_side():
  from model_based_rl_amd.evaluate import refuse_true_model
  for kv in (dict(only_prior=1), dict(only_value=1), dict(only_prior=[0, 1], true_model=[1])):
    with pytest.raises(NotImplementedError, match=r'^--true_model: --only_prior / --only_value run no search'):
      refuse_true_model(_args(**kv))
  with pytest.raises(NotImplementedError, match=r'^--true_model: --only_prior / --only_value run no search'):
    refuse_true_model(_args(true_model=[0, 1], only_value=[0, 1]), match=True)
  refuse_true_model(_args(true_model=[0, 1], only_value=[1, 0]), match=True)      # the other side's lookahead is its own business


def test_cli_refuses_another_architecture():
  from model_based_rl_amd.evaluate import refuse_true_model
  with pytest.raises(NotImplementedError, match=r'^--true_model: the architecture MuZeroNetwork has no engine path'):
    refuse_true_model(_args(architecture='MuZeroNetwork'))


def test_cli_refuses_a_value_that_is_no_switch():
  from model_based_rl_amd.evaluate import refuse_true_model
  with pytest.raises(NotImplementedError, match=r'^--true_model: the values are 0 .* and 1'):
    refuse_true_model(_args(true_model=3))


def test_cli_parses_the_flag_and_the_default_refuses_nothing():
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import refuse_true_model
  assert get_evaluation_args([]).true_model == [0]
  assert get_evaluation_args(['--match', '--true_model', '0', '1']).true_model == [0, 1]
  refuse_true_model(get_evaluation_args([]))
  refuse_true_model(_args(true_model=0, device_env=False, environment='CartPole-v1', apply_mcts_actions=5))


def test_main_refuses_before_loading_anything():
  from model_based_rl_amd import evaluate
  with pytest.raises(NotImplementedError, match=r'^--true_model: '):
    evaluate.main(['--true_model', '1', '--nets', 'missing'])
  with pytest.raises(NotImplementedError, match=r'^--true_model: '):
    evaluate.main(['--match', '--true_model', '1', '--only_prior', '1', '--nets', 'missing', 'missing'])


class StubEngine(object):
  """what Evaluator._play_batch_device calls, recording the calls; every game is over after the first chunk"""
  made = []

  def __init__(self, B, A, sims):
    self.B, self.A, self.sims, self.calls = B, A, sims, []
    StubEngine.made.append(self)

  @classmethod
  def from_config(cls, config, num_envs, device=None, seed=None, env_id_offset=0):
    return cls(num_envs, config.action_space, config.num_simulations)

  def set_weights(self, w):
    self.calls.append('set_weights')

  def set_true_model(self, kind):
    self.calls.append(('set_true_model', kind))

  def eval_env_reset(self, kind, max_steps, time_limit, random_opp, keep_history):
    self.calls.append('eval_env_reset')
    self.eval_log_cap = 9

  def eval_env_moves(self, n, mode, M, T, noise_on):
    self.calls.append('eval_env_moves')
    return 0

  def eval_env_results(self):
    z = lambda *s: np.zeros(s)
    return dict(step=np.full(self.B, 5, np.int32), n_moves=np.full(self.B, 5, np.int32), sum_reward=z(self.B), sum_pred_reward=z(self.B),
                sum_pred_value=z(self.B), sum_root_value=z(self.B), depth_mean=z(self.B), depth_max=z(self.B, self.sims))

  def close(self):
    pass


def test_label_and_out_key_on_a_stub_engine(tmp_path, monkeypatch):
  """evaluate --device_env --true_model 0 1: two configurations, the second labelled and run with the engine's true-rules
  search set before the games start; --out carries true_model per configuration"""
  import torch
  from model_based_rl_amd import evaluate
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--architecture', 'FCNetwork', '--num_simulations', '4'])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 7}
  torch.save(state, str(tmp_path / 'net'))
  monkeypatch.setattr(evaluate, 'Engine', StubEngine)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  StubEngine.made = []
  out = tmp_path / 'out.json'
  res = evaluate.main(['--saves_dir', str(tmp_path) + '/', '--nets', 'net', '--num_games', '3', '--seed', '0', '--device_env',
                       '--detailed_label', '--true_model', '0', '1', '--out', str(out)])
  assert [r['true_model'] for r in res] == [0, 1]
  assert 'true rules' not in res[0]['label'] and res[1]['label'].endswith('true rules')
  assert [c['true_model'] for c in json.load(open(str(out)))['configurations']] == [0, 1]
  plain, true = StubEngine.made
  assert not [c for c in plain.calls if c[0] == 'set_true_model']
  assert true.calls.index(('set_true_model', 'TicTacToe')) < true.calls.index('eval_env_reset') < true.calls.index('eval_env_moves')
  # play_games(true_model=True) on a config without the flag takes the same path
  ev = evaluate.Evaluator(dict(state, config=evaluate._with(cfg, temperature=0, only_prior=0, only_value=0, use_exploration_noise=0,
                                                            apply_mcts_actions=1, random_opp=None, label='x', batch=4)))
  ev.load_network()
  StubEngine.made = []
  ev.play_games(2, [0, 1], device_env=True, true_model=True)
  assert ('set_true_model', 'TicTacToe') in StubEngine.made[0].calls
  with pytest.raises(NotImplementedError, match=r'^--true_model: .*needs --device_env'):
    ev.play_games(2, [0, 1], true_model=True)


def test_host_twin_under_the_sanitizers(tmp_path):
  """tests/truemodel_host.cpp -- the twin's own file in a stand-alone program -- under AddressSanitizer + UBSan"""
  import os
  import subprocess
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  exe = str(tmp_path / 'truemodel_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(root, 'include'),
         '-I', os.path.join(root, 'model-based-rl_amd', 'csrc'), os.path.join(root, 'tests', 'truemodel_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.strip().splitlines()[-1] == 'ok 600'
