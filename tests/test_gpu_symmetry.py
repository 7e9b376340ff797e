"""GPU side of the board-symmetry augmentation (mz_fcl_set_symmetry, k_fcl_symmetry of csrc/mz_symmetry.hip.h; DESIGN s7e).
Every comparison is bit for bit: a permutation has no rounding, and the step kernels are the same with and without it.
  kernel     mz_fcl_symmetry_apply (the kernel alone) equals mz_fcl_symmetry_host, from device memory and from pinned host memory
  update     three mz_fcl_update calls with symmetry on and raw batches == three with symmetry off on the host-transformed batches
  run        2 * slots + 1 updates of mz_fcl_run (several in flight over the handle's one image buffer) == the per-update path
  off        after mz_fcl_set_symmetry(c, 0, ..) a further update is the plain one
  resume     a handle set with first_update = 3 makes the fourth update of a handle that started at 0
  learner    --symmetry through Learner.update_weights on the native step, a resumed training step included"""
import ctypes as C

import numpy as np
import pytest
import torch

from model_based_rl_amd import symmetry as sy
from tests.eval_device_util import ENV_FLAGS
from tests.symmetry_util import ENV_OF, KINDS, SEED, UPDATE, batch, host_apply, same_bits

pytestmark = pytest.mark.gpu


def transformed(host, kind, update, seed=SEED):
  """the batch with its three arrays replaced by the host hook's images"""
  obs, act, pol, _ = host_apply(host, kind, seed, update)
  return dict(host, obs=obs, act=act, t_pol=pol)


# ---- the kernel alone
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('bs', [16, 48])
@pytest.mark.parametrize('K', [1, 5])
def test_kernel_equals_the_host_hook(kind, bs, K):
  from model_based_rl_amd import _abi
  lib = _abi.load()
  dev = torch.device('cuda', torch.cuda.current_device())
  O, A = sy.CELLS[kind], sy.ACTIONS[kind]
  h = C.c_void_p()
  with torch.cuda.device(dev):
    _abi.check(lib.mz_fcl_create(bs, K, O, A, -15, 15, -15, 15, 0, C.byref(h)), 'mz_fcl_create')
  try:
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    obs_out = torch.empty(bs, O, dtype=torch.float32, device=dev)
    pol_out = torch.empty(bs, K + 1, A, dtype=torch.float32, device=dev)
    el = torch.empty(bs, dtype=torch.int32, device=dev)
    host = batch(kind, bs, K)
    src = [torch.from_numpy(host[k]) for k in ('obs', 'act', 't_pol')]
    # without a kind the hook has nothing to run
    args = lambda o, a, q, act_out: (h, p(o), p(a), int(a.dtype == torch.int32), p(q), UPDATE, p(obs_out), p(act_out), p(pol_out), p(el), stream)
    act_out = torch.empty(bs, K, dtype=torch.int64, device=dev)
    on_dev = [t.to(dev) for t in src]
    assert lib.mz_fcl_symmetry_apply(*args(*on_dev, act_out)) != 0 and b'no symmetry set' in lib.mz_last_error()
    _abi.check(lib.mz_fcl_set_symmetry(h, kind, SEED, 0), 'mz_fcl_set_symmetry')
    for dtype in (np.int32, np.int64):
      host = batch(kind, bs, K, dtype)
      host['act'][0, 0], host['act'][1, -1] = -1, A      # no actions of the game: they stay what they are
      want = host_apply(host, kind, SEED, UPDATE)
      assert set(want[3].tolist()) == set(range(sy.ELEMENTS[kind]))
      src = [torch.from_numpy(host[k]) for k in ('obs', 'act', 't_pol')]
      act_out = torch.empty(bs, K, dtype=src[1].dtype, device=dev)
      for where in ('device', 'pinned'):      # (pinned: what mz_fcl_run's kernels read, the staging slot itself)
        ins = [t.to(dev) for t in src] if where == 'device' else [t.pin_memory() for t in src]
        for t in (obs_out, pol_out):
          t.fill_(float('nan'))
        act_out.fill_(-7); el.fill_(-1)
        _abi.check(lib.mz_fcl_symmetry_apply(*args(*ins, act_out)), 'mz_fcl_symmetry_apply')
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in (obs_out, act_out, pol_out, el)]
        assert all(same_bits(g, w) for g, w in zip(got, want)), (where, dtype)
        assert all(same_bits(t.cpu().numpy(), host[k]) for t, k in zip(ins, ('obs', 'act', 't_pol')))      # the sources are not written
    # the images cannot be written over their sources
    assert lib.mz_fcl_symmetry_apply(h, p(obs_out), p(act_out), 0, p(pol_out), UPDATE, p(obs_out), p(act_out), p(pol_out), None, stream) != 0
    assert b'written over their sources' in lib.mz_last_error()
  finally:
    lib.mz_fcl_destroy(h)


def test_set_symmetry_refusals():
  from model_based_rl_amd import _abi
  lib = _abi.load()
  h = C.c_void_p()
  _abi.check(lib.mz_fcl_create(16, 5, 9, 9, -15, 15, -15, 15, 0, C.byref(h)), 'mz_fcl_create')
  try:
    for kind in (2, 4, -1):
      assert lib.mz_fcl_set_symmetry(h, kind, 0, 0) != 0
      msg = lib.mz_last_error().decode()
      assert msg.startswith('mz_fcl_set_symmetry: unknown kind %d' % kind) and '. ' not in msg and '\n' not in msg, msg
    assert lib.mz_fcl_set_symmetry(h, 3, 0, 0) != 0      # a TicTacToe handle asked for Connect Four's tables
    msg = lib.mz_last_error().decode()
    assert msg.startswith('mz_fcl_set_symmetry: Connect Four has obs_dim 42 and action_space 7') and '. ' not in msg and '\n' not in msg, msg
    assert lib.mz_fcl_set_symmetry(h, 1, 0, 0) == 0 and lib.mz_fcl_set_symmetry(h, 0, 0, 0) == 0
  finally:
    lib.mz_fcl_destroy(h)
  _abi.check(lib.mz_fcl_create(16, 5, 8, 4, -15, 15, -15, 15, 0, C.byref(h)), 'mz_fcl_create')      # LunarLander's shapes
  try:
    assert lib.mz_fcl_set_symmetry(h, 1, 0, 0) != 0 and b'TicTacToe has obs_dim 9 and action_space 9' in lib.mz_last_error()
    assert lib.mz_fcl_set_symmetry(h, 0, 0, 0) == 0      # switching off is always possible
  finally:
    lib.mz_fcl_destroy(h)


# ---- through the step
def make_learner(tmp_path, tag, kind, flags=(), first_step=0):
  """a learner of the game's shapes at batch 16, K = 5; every one starts from the same weights"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  from tests.test_learner import Sink
  cfg = make_config(ENV_FLAGS[ENV_OF[kind]] + ['--seed', str(SEED), '--batch_size', '16', '--use_gpu_for', 'actors', 'learner',
                                               '--runs_dir', str(tmp_path / tag), '--run_tag', 'x', '--no_tune_gemms'] + list(flags))
  sink = Sink()
  learner = Learner(cfg, sink, sink)
  learner.training_step = first_step
  return learner


def native(tmp_path, tag, kind):
  """... and its native step, driven by the test itself"""
  from model_based_rl_amd.learners import _NativeFC
  learner = make_learner(tmp_path, tag, kind)
  host = batch(kind, 16, 5)
  assert _NativeFC.eligible(learner, host)
  return learner, _NativeFC(learner, host)


def update(nat, host):
  return nat.errors(nat.launch(host)).copy()


def state(nat):
  torch.cuda.synchronize()
  return [t.detach().cpu().numpy().copy() for t in (nat.flat, nat.m, nat.v, nat.steps)]


def equal_states(a, b):
  return all(same_bits(x, y) for x, y in zip(state(a), state(b)))


def set_symmetry(nat, kind, first_update, seed=SEED):
  from model_based_rl_amd import _abi
  _abi.check(nat.lib.mz_fcl_set_symmetry(nat.h, kind, seed, first_update), 'mz_fcl_set_symmetry')


@pytest.mark.parametrize('kind', KINDS)
def test_updates_on_raw_batches_equal_updates_on_the_images(tmp_path, kind):
  batches = [batch(kind, 16, 5, seed=i) for i in range(3)]
  _, on = native(tmp_path, 'on', kind)
  _, off = native(tmp_path, 'off', kind)
  _, plain = native(tmp_path, 'plain', kind)
  assert equal_states(on, off)
  set_symmetry(on, kind, 0)
  for i, host in enumerate(batches):
    keep = {k: v.copy() for k, v in host.items()}
    e_on = update(on, host)
    e_off = update(off, transformed(host, kind, i))
    update(plain, host)
    assert same_bits(e_on, e_off), i
    assert all(same_bits(host[k], keep[k]) for k in keep)      # the caller's arrays are not written
    assert equal_states(on, off), i
  assert not equal_states(on, plain)                            # (the images are other batches than the raw ones)
  assert state(on)[3].max() == 3.0
  for nat in (on, off, plain):
    nat.close()


@pytest.mark.parametrize('kind', KINDS)
def test_switching_off_and_resuming(tmp_path, kind):
  batches = [batch(kind, 16, 5, seed=10 + i) for i in range(5)]
  _, a = native(tmp_path, 'a', kind)
  _, b = native(tmp_path, 'b', kind)
  set_symmetry(a, kind, 0)
  for i in range(3):
    update(a, batches[i])
    update(b, transformed(batches[i], kind, i))
  # resume: b joins at update 3 with the counter a has reached by itself
  set_symmetry(b, kind, 3)
  assert same_bits(update(a, batches[3]), update(b, batches[3])) and equal_states(a, b)
  assert not same_bits(transformed(batches[3], kind, 3)['obs'], transformed(batches[3], kind, 0)['obs'])      # (update 3's draw is not update 0's)
  # off: a further update is the plain one
  set_symmetry(a, 0, 0)
  e_a, e_b = update(a, batches[4]), update(b, batches[4])      # (b, still on, trains on the images)
  assert not same_bits(e_a, e_b)
  _, c = native(tmp_path, 'c', kind)
  for i in range(4):
    update(c, transformed(batches[i], kind, i))
  assert same_bits(update(c, batches[4]), e_a) and equal_states(a, c)
  # a step with no_update set is neither transformed nor counted
  set_symmetry(a, kind, 7)
  dev = lambda nat: [torch.from_numpy(batches[0][k]).to(nat.dev) for k in ('obs', 'act', 't_rew', 't_val', 't_pol', 'w')]
  before = state(a)
  probe = a.step(*dev(a), no_update=True).cpu().numpy()
  assert same_bits(probe, c.step(*dev(c), no_update=True).cpu().numpy())      # (c, with symmetry off, sees the raw batch)
  assert all(same_bits(x, y) for x, y in zip(before, state(a)))
  set_symmetry(c, kind, 7)                                                     # a's counter is still 7
  assert same_bits(update(a, batches[1]), update(c, batches[1])) and equal_states(a, c)
  for nat in (a, b, c):
    nat.close()


def test_native_loop_with_symmetry_equals_the_per_update_path(tmp_path):
  """mz_fcl_run with symmetry on -- several updates in flight, every one's images in the handle's single buffer -- against the same
  updates driven one call at a time in mz_fcl_run's order, on twin replays from the same generator states (as
  test_learner.test_native_loop_equals_the_per_update_path does without symmetry): weights, moments and priorities bit for bit"""
  import random
  from collections import deque
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine, flatten_weights
  from model_based_rl_amd.learners import Learner
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  kind, B = 1, 48
  flags = ENV_FLAGS['TicTacToe'] + ['--seed', str(SEED), '--batch_size', '16', '--num_envs', str(B), '--num_simulations', '8', '--window_size', '4096',
                                    '--use_gpu_for', 'actors', 'learner', '--send_weights_frequency', '1000', '--learner_log_frequency', '1000',
                                    '--save_state_frequency', '1000000', '--beta', '0.6', '--runs_dir', str(tmp_path), '--run_tag', 'x']
  cfg_on, cfg_off = make_config(flags + ['--symmetry']), make_config(flags)
  torch.manual_seed(0)
  eng = Engine.from_config(cfg_off, B)
  eng.set_weights(flatten_weights(get_network(cfg_off, torch.device('cpu')).state_dict()))
  eng.selfplay_set_env('tictactoe')
  eng.selfplay_reset(9, 1.0)
  eng.selfplay_steps(16)
  buf, nmv = eng.selfplay_drain()
  torch.cuda.synchronize()
  records = buf[:nmv].numpy().copy()
  eng.close()

  def world(cfg):
    replay = PrioritizedReplay(cfg)
    replay.ingest_records(records, nmv, B)
    learner = Learner(cfg, SharedStorage(cfg), replay)
    random.seed(7); np.random.seed(8)
    learner.update_weights(replay.sample_batch_arrays())      # builds the native step (update 0 of the handle's counter)
    learner.training_step += 1
    assert learner._native is not None and learner._native.sym_kind == (kind if cfg.symmetry else 0)
    return learner, replay

  def per_update(cfg, n):
    a, ra = world(cfg)
    slots = a._native.lib.mz_fcl_slots(a._native.h)
    owed = deque()
    for i in range(n):
      if len(owed) == slots:
        ix, slot = owed.popleft()
        ra.update(ix, a._native.errors(slot))
      host, ix = a._host_batch(ra.sample_batch_arrays())
      owed.append((ix, a._native.launch(host)))
    while owed:
      ix, slot = owed.popleft()
      ra.update(ix, a._native.errors(slot))
    return a, ra
  probe, _ = world(cfg_on)
  slots = probe._native.lib.mz_fcl_slots(probe._native.h)
  assert 2 <= slots <= 8
  n = 2 * slots + 1
  a, ra = per_update(cfg_on, n)
  b, rb = world(cfg_on)
  b._native.run(rb, n)
  assert b._native.in_flight
  b._native.flush()
  assert equal_states(a._native, b._native)
  assert np.array_equal(ra.tree.leaves(), rb.tree.leaves()) and ra.tree.total_priority == rb.tree.total_priority
  c, _ = per_update(cfg_off, n)                                 # (and the flag did something)
  assert not equal_states(a._native, c._native) and state(a._native)[3].max() == 1.0 + n


# ---- the flag through the learner
@pytest.mark.parametrize('kind', KINDS)
def test_learner_flag_on_the_native_step(tmp_path, kind):
  """Learner.update_weights with --symmetry (the handle set from the configuration: the run's seed, the learner's training step --
  here a resumed one) == update_weights without it on symmetry.apply_batch's images"""
  idxs = list(range(16))
  for first in (0, UPDATE):
    on = make_learner(tmp_path, 'on%d' % first, kind, ['--symmetry'], first_step=first)
    off = make_learner(tmp_path, 'off%d' % first, kind, first_step=first)
    for i in range(2):
      host = batch(kind, 16, 5, seed=20 + i)
      on.update_weights((host, idxs))
      off.update_weights((sy.apply_batch(host, kind, SEED, first + i)[0], idxs))
      on.training_step += 1; off.training_step += 1
    assert on._native is not None and off._native is not None and on._native.sym_kind == kind and off._native.sym_kind == 0
    assert equal_states(on._native, off._native)
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(on.storage.updates, off.storage.updates)) and len(on.storage.updates) == 2
