"""CPU side of the board-symmetry augmentation (--symmetry; csrc/mz_symmetry.hip.h, model_based_rl_amd/symmetry.py, DESIGN s7e).
Every comparison is exact: a permutation has no rounding.
  tables       the eight TicTacToe permutations are a group, a_g = p_g; Connect Four's mirror is an involution
  rules        200 random legal games per kind replayed under every element on envs.TicTacToe / envs.ConnectFour
  restatement  the host hook mz_fcl_symmetry_host -- the kernel's own bodies looped on the host -- equals symmetry.apply_batch
  own data     a sample's image depends on (seed, update, b) and its own data only
  refusals     every --symmetry refusal is one sentence that reaches the caller before any device is touched
  plumbing     a CPU Learner update with --symmetry on batch X leaves the weights of an update without it on apply_batch(X)
  asan         the bodies as a stand-alone program (tests/symmetry_host.cpp) under AddressSanitizer + UBSan"""
import os
import subprocess

import numpy as np
import pytest

from model_based_rl_amd import symmetry as sy
from tests.symmetry_util import ENV_OF, KINDS, SEED, UPDATE, batch, host_apply, ptr, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables
def test_tictactoe_tables_are_a_group():
  p, a = sy.cell_perm(1), sy.action_perm(1)
  assert p.shape == (8, 9) and np.array_equal(p, a)      # a_g = p_g on cells
  rows = [tuple(r) for r in p]
  assert len(set(rows)) == 8 and all(sorted(r) == list(range(9)) for r in rows) and rows[0] == tuple(range(9))
  for g in range(8):
    for h in range(8):
      assert tuple(p[h][p[g]]) in rows, (g, h)      # closed under composition
  assert all(r[4] == 4 for r in rows)                    # the centre stays
  # g = 4 f + q by the definition's words: q quarter turns (r, c) -> (c, 2 - r), then the mirror (r, c) -> (r, 2 - c)
  assert tuple(p[1]) == tuple(3 * c + (2 - r) for r in range(3) for c in range(3))
  assert tuple(p[4]) == tuple(3 * r + (2 - c) for r in range(3) for c in range(3))
  assert np.array_equal(p[5], p[4][p[1]]) and np.array_equal(p[2], p[1][p[1]])


def test_connect_four_mirror_is_an_involution():
  p, a = sy.cell_perm(3), sy.action_perm(3)
  assert p.shape == (2, 42) and a.shape == (2, 7)
  assert np.array_equal(p[0], np.arange(42)) and np.array_equal(a[0], np.arange(7))
  assert np.array_equal(p[1][p[1]], np.arange(42)) and np.array_equal(a[1][a[1]], np.arange(7)) and not np.array_equal(p[1], p[0])
  assert all(p[1][7 * r + c] == 7 * r + 6 - c for r in range(6) for c in range(7)) and all(a[1][c] == 6 - c for c in range(7))


# ---- the tables are symmetries of the rules
@pytest.mark.parametrize('kind', KINDS)
def test_replayed_games_agree_with_the_rules(kind):
  from model_based_rl_amd import envs
  make = envs.TicTacToe if kind == 1 else envs.ConnectFour
  p, a = sy.cell_perm(kind), sy.action_perm(kind)
  rng = np.random.RandomState(kind)
  lengths = set()
  for game in range(200):
    env = make()
    env.reset()
    trace, done = [], False      # (legal before the move, action, obs, reward, done)
    while not done:
      legal = np.array(env.legal_actions())
      action = int(rng.choice(legal))
      obs, reward, done, _ = env.step(action)
      trace.append((legal, action, np.array(obs), reward, done))
    lengths.add(len(trace))
    for g in range(sy.ELEMENTS[kind]):
      twin = make()
      twin.reset()
      for legal, action, obs, reward, done in trace:
        assert sorted(a[g][legal]) == sorted(int(x) for x in twin.legal_actions()), (game, g)      # the image of the legal list
        obs2, reward2, done2, _ = twin.step(int(a[g][action]))
        want = np.empty_like(obs)
        want[p[g]] = obs                                    # obs'[p_g(c)] = obs[c]
        assert np.array_equal(np.array(obs2), want) and reward2 == reward and done2 == done, (game, g)
  assert len(lengths) >= 4      # games of many lengths, wins and draws


# ---- the host hook equals the numpy restatement
def test_the_seed_draws_every_element():
  for kind in KINDS:
    g = sy.draw(kind, SEED, UPDATE, 16)
    assert set(g.tolist()) == set(range(sy.ELEMENTS[kind])) and 0 in g      # every element, the identity among them
    assert np.array_equal(sy.draw(kind, SEED, UPDATE, 48)[:16], g)          # (b's element does not depend on the batch size)
    assert not np.array_equal(sy.draw(kind, SEED, UPDATE + 1, 16), g) and not np.array_equal(sy.draw(kind, SEED + 1, UPDATE, 16), g)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('bs', [16, 48])
def test_hook_equals_the_restatement(kind, K, dtype, bs):
  host = batch(kind, bs, K, dtype)
  host['act'][0, 0], host['act'][1, -1] = -1, sy.ACTIONS[kind]      # no actions of the game: they stay what they are
  keep = {k: v.copy() for k, v in host.items()}
  want, g = sy.apply_batch(host, kind, SEED, UPDATE)
  obs, act, pol, el = host_apply(host, kind, SEED, UPDATE)
  assert all(same_bits(host[k], keep[k]) for k in keep)               # the sources are not written
  assert same_bits(obs, want['obs']) and same_bits(act, want['act']) and same_bits(pol, want['t_pol'])
  assert act.dtype == dtype and el.dtype == np.int32 and np.array_equal(el, g)
  assert set(el.tolist()) == set(range(sy.ELEMENTS[kind])) and 0 in el
  assert act[0, 0] == -1 and act[1, -1] == sy.ACTIONS[kind]
  for k in ('t_rew', 't_val', 'w'):                                    # untouched, the same objects
    assert want[k] is host[k]
  # the identity's samples are what they were, the others' contents are permuted, not changed
  same = el == 0
  assert same_bits(obs[same], host['obs'][same]) and same_bits(pol[same], host['t_pol'][same]) and same_bits(act[same], host['act'][same])
  assert np.array_equal(np.sort(obs, axis=1), np.sort(host['obs'], axis=1)) and np.array_equal(np.sort(pol, axis=2), np.sort(host['t_pol'], axis=2))
  assert not same_bits(obs, host['obs']) and not same_bits(pol, host['t_pol'])
  # the definition, element by element
  p, a = sy.cell_perm(kind), sy.action_perm(kind)
  for b in range(bs):
    assert np.array_equal(obs[b][p[el[b]]], host['obs'][b]) and np.array_equal(pol[b][:, a[el[b]]], host['t_pol'][b])


def test_a_sample_depends_on_its_own_data_only():
  for kind in KINDS:
    host = batch(kind, 48, 5)
    base = host_apply(host, kind, SEED, UPDATE)
    other = batch(kind, 48, 5, seed=1)
    for b in (0, 17, 47):
      mixed = {k: other[k].copy() for k in other}
      for k in ('obs', 'act', 't_pol'):
        mixed[k][b] = host[k][b]      # every other sample's contents replaced
      for got in (host_apply(mixed, kind, SEED, UPDATE), list(sy.apply_batch(mixed, kind, SEED, UPDATE)[0][k] for k in ('obs', 'act', 't_pol'))):
        assert all(same_bits(got[i][b], base[i][b]) for i in range(3)), (kind, b)
    # a batch of 16 is the first 16 samples of the batch of 48
    small = host_apply({k: v[:16] for k, v in host.items()}, kind, SEED, UPDATE)
    assert all(same_bits(small[i], base[i][:16]) for i in range(4))
    # ... and the key matters
    assert not np.array_equal(host_apply(host, kind, SEED, UPDATE + 1)[3], base[3]) and not np.array_equal(host_apply(host, kind, SEED + 1, UPDATE)[3], base[3])


# ---- refusals, the flag
def _one_sentence(msg, word, start='--symmetry: '):
  assert msg.startswith(start) and word in msg, msg
  assert msg.endswith('.') and '\n' not in msg and '. ' not in msg[:-1], msg


def _no_device(monkeypatch):
  """HIP initialisation fails: whoever reaches for a device fails the test"""
  import torch

  def touched(*a, **k):
    raise AssertionError('a device was touched')
  for name in ('is_available', 'init', '_lazy_init', 'device_count', 'current_device'):
    monkeypatch.setattr(torch.cuda, name, touched)


def _config(env, flags=(), **over):
  from model_based_rl_amd.config import make_config
  return make_config(['--environment', env, '--two_players', '--batch_size', '16', '--seed', '0', '--use_gpu_for', 'actors', 'learner',
                      '--symmetry'] + list(flags), **over)


REFUSALS = [      # (configuration, the word its sentence carries)
    (lambda: _config('LunarLander-v2'), 'LunarLander-v2'),
    (lambda: _config('CartPole-v1'), 'CartPole-v1'),
    (lambda: _config('TicTacToe', ['--norm_obs', '--obs_range', '-1', '1']), '--norm_obs'),
    (lambda: _config('ConnectFour', obs_u8=True), 'byte observations'),
    (lambda: _config('TicTacToe', ['--stack_obs', '4']), '--stack_obs 4'),
    (lambda: _config('ConnectFour', action_space=7, obs_space=(84,)), '84 values'),
    (lambda: _config('TicTacToe', action_space=9, obs_space=(1, 3, 3), obs_u8=False), '(1, 3, 3)'),
    (lambda: _config('TicTacToe', ['--architecture', 'MuZeroNetwork']), 'MuZeroNetwork'),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_refusals_reach_the_caller_before_any_device(i, monkeypatch, tmp_path):
  from model_based_rl_amd.learners import Learner
  _no_device(monkeypatch)
  make, word = REFUSALS[i]
  cfg = make()
  cfg.runs_dir = str(tmp_path)
  with pytest.raises(NotImplementedError) as err:
    sy.refuse_symmetry(cfg)
  _one_sentence(str(err.value), word)
  with pytest.raises(NotImplementedError) as err2:      # the learner asks before it reaches for its device
    Learner(cfg, None, None)
  assert str(err2.value) == str(err.value)


def test_train_refuses_before_any_device(monkeypatch, tmp_path):
  from model_based_rl_amd import train
  _no_device(monkeypatch)
  for flags, word in ((['--environment', 'LunarLander-v2'], 'LunarLander-v2'),
                      (['--environment', 'TicTacToe', '--two_players', '--norm_obs', '--obs_range', '-1', '1'], '--norm_obs'),
                      (['--environment', 'Pong-ramNoFrameskip-v4'], 'Pong-ramNoFrameskip-v4'),
                      (['--environment', 'ConnectFour', '--two_players', '--stack_obs', '2'], '--stack_obs 2')):
    with pytest.raises(NotImplementedError) as err:
      train.main(flags + ['--symmetry', '--use_gpu_for', 'actors', 'learner', '--runs_dir', str(tmp_path)])
    _one_sentence(str(err.value), word)


def test_nothing_to_refuse():
  from model_based_rl_amd.config import make_config
  _config('TicTacToe'), _config('ConnectFour')
  for env in ('TicTacToe', 'ConnectFour'):
    cfg = _config(env)
    sy.refuse_symmetry(cfg)
    assert sy.kind_of(cfg) == (1 if env == 'TicTacToe' else 3) and sy.seed_of(cfg) == 0
  off = make_config(['--environment', 'LunarLander-v2', '--norm_obs', '--obs_range', '0', '1'])      # without the flag nothing is asked
  sy.refuse_symmetry(off)
  assert sy.kind_of(off) == 0 and sy.seed_of(off) == 0 and sy.seed_of(make_config(['--seed', '11'])) == 11


def test_flag_parses():
  from model_based_rl_amd.config import make_config
  assert make_config(['--environment', 'TicTacToe', '--symmetry']).symmetry is True
  assert make_config(['--environment', 'TicTacToe']).symmetry is False


def test_library_refusals_without_a_handle():
  from model_based_rl_amd import _abi
  from tests.test_abi import declared_symbols
  lib = _abi.load()
  assert 'mz_fcl_set_symmetry' in _abi.SIGNATURES and 'mz_fcl_set_symmetry' in declared_symbols(('mz_engine.h',))
  for hook in ('mz_fcl_symmetry_apply', 'mz_fcl_symmetry_host'):
    assert hook in _abi.SIGNATURES and hook in declared_symbols(('mz_engine_debug.h',))
  assert 'mz_symmetry.hip.h' in _abi._SOURCES and 'mz_symmetry.hip.h' in _abi._ENGINE_ONLY
  assert lib.mz_version() == 1
  assert lib.mz_fcl_set_symmetry(None, 1, 0, 0) != 0 and b'mz_fcl_set_symmetry: null argument' in lib.mz_last_error()
  host = batch(1, 16, 5)
  for kind in (0, 2, 4):
    with pytest.raises(RuntimeError, match='unknown kind %d' % kind):
      host_apply(host, kind, SEED, UPDATE)
  obs = host['obs']
  assert lib.mz_fcl_symmetry_host(1, 0, 0, 16, 5, ptr(obs), ptr(host['act']), 0, ptr(host['t_pol']), ptr(obs), ptr(host['act'].copy()),
                                  ptr(host['t_pol'].copy()), None) != 0
  assert b'written over their sources' in lib.mz_last_error()


# ---- the flag through the learner
@pytest.mark.parametrize('kind', KINDS)
def test_cpu_learner_update_trains_on_the_images(kind, tmp_path):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  from tests.test_learner import Sink
  host = batch(kind, 16, 5)
  idxs = list(range(16))

  def run(tag, flags, feed, step):
    cfg = make_config(['--environment', ENV_OF[kind], '--two_players', '--known_bounds', '-1', '1', '--discount', '1', '--batch_size', '16',
                       '--seed', str(SEED), '--runs_dir', str(tmp_path / tag), '--run_tag', 'x'] + flags)
    sink = Sink()
    learner = Learner(cfg, sink, sink)
    assert learner.device.type == 'cpu'
    learner.training_step = step
    learner.update_weights(({k: v.copy() for k, v in feed.items()}, idxs))
    return {k: v.detach().clone() for k, v in learner.network.state_dict().items()}, sink.updates[-1][1]
  for step in (0, UPDATE):
    image, g = sy.apply_batch(host, kind, SEED, step)
    assert len(set(g.tolist())) > 1
    on, err_on = run('on%d' % step, ['--symmetry'], host, step)
    want, err_want = run('want%d' % step, [], image, step)
    plain, _ = run('plain%d' % step, [], host, step)
    assert all(torch.equal(on[k], want[k]) for k in want) and np.array_equal(err_on, err_want)
    assert any(not torch.equal(on[k], plain[k]) for k in plain)      # (and the flag did something)


# ---- the bodies under the sanitizers
def test_bodies_under_the_sanitizers(tmp_path):
  """tests/symmetry_host.cpp under AddressSanitizer + UBSan; its digests are the hook's on batches made again here"""
  exe = str(tmp_path / 'symmetry_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'include'),
         '-I', os.path.join(ROOT, 'model-based-rl_amd', 'csrc'), os.path.join(ROOT, 'tests', 'symmetry_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  lines = run.stdout.strip().splitlines()
  assert lines[-1] == 'ok 600' and len(lines) == 601
  rows = [[int(x) for x in line.split()] for line in lines[:-1]]
  assert [r[0] for r in rows] == list(range(600)) and [r[1] for r in rows] == [1] * 300 + [3] * 300
  M = (1 << 64) - 1

  def again(n, kind, bs, K, i32):      # the program's batch n, from its generator
    state = [(0x9E3779B97F4A7C15 + n * 0xD1B54A32D192ED03) & M]

    def rnd():
      s = state[0]
      s ^= s >> 12; s = (s ^ (s << 25)) & M; s ^= s >> 27
      state[0] = s
      return ((s * 0x2545F4914F6CDD1D) & M) >> 32
    O, A = sy.CELLS[kind], sy.ACTIONS[kind]
    obs = np.array([float(rnd() % 3) - 1.0 for _ in range(bs * O)], np.float32).reshape(bs, O)
    act = []
    for _ in range(bs * K):
      r = rnd()
      act.append(-1 if r >> 28 == 0 else (A if r >> 28 == 1 else r % A))
    pol = np.array([(rnd() >> 8) / 16777216.0 for _ in range(bs * (K + 1) * A)], np.float32).reshape(bs, K + 1, A)
    return {'obs': obs, 'act': np.array(act, np.int32 if i32 else np.int64).reshape(bs, K), 't_pol': pol}
  checked = 0
  for n, kind, bs, K, i32, digest in rows:
    assert (bs, K, i32) == (1 + (7 * n) % 48, 1 + n % 7, n & 1)
    if n % 25 not in (0, 8):      # 24 batches per kind made again here; the program itself holds all 600 to the definition
      continue
    out = host_apply(again(n, kind, bs, K, i32), kind, 6, n)
    words = np.concatenate([np.ascontiguousarray(x).view(np.uint32).reshape(-1) for x in out]).astype(np.uint64)
    with np.errstate(over='ignore'):
      h = int((words * np.arange(1, words.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    assert h == digest, n
    checked += 1
  assert checked == 48
