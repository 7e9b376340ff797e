"""SGD and RMSprop (utils.py:73-83: torch.optim.SGD(lr, momentum, weight_decay), torch.optim.RMSprop(lr, momentum, eps=0.01,
weight_decay)) in the learner: a float64 restatement of both optimisers against torch's own, the PyTorch learner against two steps of
the unmodified reference (goldens g8, scripts/make_optimizer_goldens.py), and on the MI355X the native step (mz_fcl_set_optimizer,
csrc/mz_fcl.hip.h) against the reference, against the eager PyTorch learner in lock-step, across its launch structures, in the native
loop and across checkpoints."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from .test_learner import G, Sink, _random_batch

LOCKSTEP_FLAGS = [['--optimizer', 'SGD'], ['--optimizer', 'SGD', '--momentum', '0'], ['--optimizer', 'SGD', '--clip_grad', '1', '--weight_decay', '0'],
                  ['--optimizer', 'SGD', '--lr_scheduler', 'WarmUpLR'], ['--optimizer', 'RMSprop'],
                  ['--optimizer', 'RMSprop', '--momentum', '0', '--lr_scheduler', 'MuZeroLR']]


def restate(kind, w, g, buf, sq, lr, mom, wd, alpha=0.99, eps=0.01):
  """one step of torch.optim.SGD (dampening 0, no Nesterov) / RMSprop (not centred) on float64 tensors -> (w, buf, sq); a zero
  buffer stands for torch's missing one (its first step sets buf = g)"""
  g = g + wd * w if wd else g
  d = g
  if kind == 'RMSprop':
    sq = alpha * sq + (1 - alpha) * g * g
    d = g / (sq.sqrt() + eps)
  if mom:
    buf = mom * buf + d
    d = buf
  return w - lr * d, buf, sq


def clip_coef(grads, clip):
  """torch.nn.utils.clip_grad_norm_'s factor (learners.py:220-221)"""
  norm = float(torch.cat([g.reshape(-1) for g in grads]).norm())
  return min(1.0, clip / (norm + 1e-6))


@pytest.mark.parametrize('kind', ['SGD', 'RMSprop'])
@pytest.mark.parametrize('mom', [0.0, 0.9])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('clip', [0.0, 0.5])
def test_restatement_equals_torch_optimizers_in_float64(kind, mom, wd, clip):
  """five steps of the float64 restatement against torch.optim.SGD / RMSprop (as utils.py:73-83 builds them) in float64"""
  rng = np.random.default_rng(3)
  shapes = [(7, 5), (5,), (3, 7)]
  params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
  opt = (torch.optim.SGD(params, lr=0.01, momentum=mom, weight_decay=wd) if kind == 'SGD' else
         torch.optim.RMSprop(params, lr=0.01, momentum=mom, eps=0.01, weight_decay=wd))
  w = [p.detach().clone() for p in params]
  buf, sq = [torch.zeros_like(x) for x in w], [torch.zeros_like(x) for x in w]
  for step in range(5):
    grads = [torch.from_numpy(rng.standard_normal(s)) for s in shapes]
    for p, g in zip(params, grads):
      p.grad = g.clone()
    if clip:
      torch.nn.utils.clip_grad_norm_(params, clip)
      c = clip_coef(grads, clip)
      grads = [g * c for g in grads]
    opt.step()
    for i, g in enumerate(grads):
      w[i], buf[i], sq[i] = restate(kind, w[i], g, buf[i], sq[i], 0.01, mom, wd)
    for i, p in enumerate(params):
      assert torch.allclose(p.detach(), w[i], rtol=1e-14, atol=1e-15), (step, i)
      st = opt.state[p]
      if mom:
        assert torch.allclose(st['momentum_buffer'], buf[i], rtol=1e-14, atol=1e-15)
      else:
        assert 'momentum_buffer' not in st or st['momentum_buffer'] is None
      if kind == 'RMSprop':
        assert torch.allclose(st['square_avg'], sq[i], rtol=1e-14, atol=1e-18) and float(st['step']) == step + 1


def test_native_kind_of_torch_optimisers():
  """which torch optimisers the native step runs: Adam / AdamW with a device-tensor rate (the capturable form), SGD without
  Nesterov or dampening, RMSprop not centred; one parameter group, not maximising"""
  from model_based_rl_amd.learners import _NativeFC
  p = [torch.nn.Parameter(torch.zeros(3))]
  assert _NativeFC.kind_of(torch.optim.SGD(p, lr=0.1, momentum=0.9)) == _NativeFC.SGD
  assert _NativeFC.kind_of(torch.optim.SGD(p, lr=0.1)) == _NativeFC.SGD
  assert _NativeFC.kind_of(torch.optim.RMSprop(p, lr=0.1, momentum=0.9, eps=0.01)) == _NativeFC.RMSPROP
  assert _NativeFC.kind_of(torch.optim.AdamW(p, lr=torch.tensor(0.1))) == _NativeFC.ADAM
  for opt in (torch.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True), torch.optim.SGD(p, lr=0.1, momentum=0.9, dampening=0.1),
              torch.optim.SGD(p, lr=0.1, maximize=True), torch.optim.RMSprop(p, lr=0.1, centered=True),
              torch.optim.RMSprop(p, lr=0.1, maximize=True), torch.optim.AdamW(p, lr=0.1), torch.optim.Adam(p, lr=torch.tensor(0.1), amsgrad=True),
              torch.optim.SGD([{'params': p}, {'params': [torch.nn.Parameter(torch.zeros(1))]}], lr=0.1), torch.optim.Adagrad(p)):
    assert _NativeFC.kind_of(opt) is None, opt


def g8_run(tmp_path, device_flag, opt, w_tol, far_tol, far_frac, loss_tol, err_tol=2e-4):
  """two Learner.update_weights steps on g5_learner_lunar's weights and batch against g8_learner_<opt>_lunar (the reference's
  SGD / RMSprop steps): every weight within w_tol, at most far_frac of them further than far_tol; loss sums; priority refreshes"""
  import sys
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
  from make_optimizer_goldens import decode_weights
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  g5 = np.load(os.path.join(G, 'g5_learner_lunar.npz'))
  g8 = np.load(os.path.join(G, 'g8_learner_%s_lunar.npz' % opt.lower()))
  w0 = {k[3:]: g5[k] for k in g5.files if k.startswith('w0.')}
  want = decode_weights(g8, w0)
  cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '256', '--optimizer', opt, '--seed', '0', '--use_gpu_for'] + device_flag +
                    ['--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'g8'])
  sink = Sink()
  learner = Learner(cfg, sink, sink)
  learner.network.load_state_dict({k: torch.from_numpy(v) for k, v in w0.items()})
  batch = ((g5['sample_obs'].copy(), g5['sample_actions'].tolist(),
            (g5['sample_target_rewards'].copy(), g5['sample_target_values'].copy(), g5['sample_target_policies'].copy())),
           g5['sample_idxs'].tolist(), g5['sample_is_weights'].copy())
  worst, far, total = 0.0, 0, 0
  for step in (1, 2):
    learner.update_weights(batch)
    for k, v in learner.network.state_dict().items():
      dd = np.abs(v.cpu().numpy() - want['w%d.%s' % (step, k)])
      worst = max(worst, float(dd.max()))
      far += int((dd > far_tol).sum()); total += dd.size
      assert dd.max() <= w_tol, (step, k, float(dd.max()))
  assert far <= far_frac * total, (far, total)
  losses = np.array([learner.losses_to_log[k] for k in ('reward', 'value', 'policy')])
  print('%s learner on %s: max |dw| %.3g after two steps, %.4f %% of the weights further than %g, max |dloss| %.3g' %
        (opt, learner.device, worst, 100.0 * far / total, far_tol, np.abs(losses - g8['losses']).max()))
  assert np.abs(losses - g8['losses']).max() <= loss_tol
  assert len(sink.updates) == 2
  for (idxs, err), ref in zip(sink.updates, g8['new_errors']):
    assert idxs == [int(i) for i in g5['sample_idxs']]
    assert np.abs(err - ref).max() <= err_tol
  return learner


@pytest.mark.parametrize('opt', ['SGD', 'RMSprop'])
def test_pytorch_learner_matches_reference_sgd_rmsprop(tmp_path, opt):
  """the PyTorch learner on the CPU against the reference's two SGD / RMSprop steps (g8).  SGD's step lr * buf is linear in the
  gradient: a host-to-host difference of a few 1e-6 in a 256-row float32 sum moves a weight by lr times that, ~1e-9 -- every weight
  within 2e-6 (a float32 ulp of the largest weights is 1.2e-7).  RMSprop divides by sqrt(square_avg) + 0.01: the first step's
  amplification of a gradient difference is up to lr / eps = 0.08, still far below Adam's 5.3 -- every weight within 2e-5, 99.9 %
  within 2e-6."""
  if opt == 'SGD':
    g8_run(tmp_path, ['actors'], opt, 2e-6, 2e-6, 0.0, 1e-5)
  else:
    g8_run(tmp_path, ['actors'], opt, 2e-5, 2e-6, 1e-3, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['SGD', 'RMSprop'])
def test_native_sgd_rmsprop_step_matches_reference(tmp_path, opt):
  """... and through the native step on the MI355X (mz_fcl_update with mz_fcl_set_optimizer), under the CPU test's bounds, loss sums
  and priority refreshes alike (measured: max |dw| 3.0e-8 for SGD, 5.1e-7 for RMSprop, no weight further than 2e-6)"""
  if opt == 'SGD':
    learner = g8_run(tmp_path, ['actors', 'learner'], opt, 2e-6, 2e-6, 0.0, 5e-5)
  else:
    learner = g8_run(tmp_path, ['actors', 'learner'], opt, 2e-5, 2e-6, 1e-3, 5e-5)
  assert learner.device.type == 'cuda' and learner._native is not None


@pytest.mark.gpu
@pytest.mark.parametrize('flags', LOCKSTEP_FLAGS, ids=['-'.join(f[1::2]) for f in LOCKSTEP_FLAGS])
def test_native_sgd_rmsprop_learner_equals_the_eager_learner(tmp_path, flags):
  """six updates on changing random batches, LunarLander shapes, batch 64: the native step against the eager PyTorch learner
  (--no_native_learner), in lock-step -- after every update the weights, buffers, RMSprop's step, the rate, the priority
  refreshes and the loss sums are compared, then the eager learner's state is copied into the native one.  The native step's own
  gradient through the float64 restatement reproduces its new weights (2e-7) and buffers (1e-6 of their largest).  A ReLU unit
  within float32 rounding of zero may fall on different sides in the two evaluations: 98 % of the weights within 1e-6, every
  weight within 2.5 times the largest move of the update.  Finally the optimiser's state_dict has the eager learner's keys and
  shapes, and the native learner's checkpoint resumes under the PyTorch learner."""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import WEIGHT_ORDER
  from model_based_rl_amd.learners import Learner
  L = {}
  for name, extra in (('native', []), ('torch', ['--no_native_learner'])):
    cfg = make_config(['--environment', 'LunarLander-v2', '--seed', '1', '--batch_size', '64', '--use_gpu_for', 'actors', 'learner',
                       '--runs_dir', str(tmp_path / name), '--run_tag', 'x'] + flags + extra)
    cfg.obs_space, cfg.action_space = (8,), 4
    sink = Sink()
    L[name] = (Learner(cfg, sink, sink), sink, cfg)
  a, b = L['native'][0], L['torch'][0]
  kind = a.config.optimizer
  grp = b.optimizer.param_groups[0]
  mom, wd, clip = float(grp['momentum']), float(grp['weight_decay']), float(getattr(a.config, 'clip_grad', 0) or 0)
  keys = (['momentum_buffer'] if mom else []) + (['square_avg'] if kind == 'RMSprop' else [])
  rng = np.random.default_rng(11)
  for step in range(6):
    h = _random_batch(rng, 64, 5, 8, 4)
    batch = ((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(64)), h['w'])
    lr_used = float(np.float32(float(a.optimizer.param_groups[0]['lr'])))
    snap = [t.clone() for t in (a._native.flat, a._native.m, a._native.v)] if a._native is not None else None
    before = [p.detach().clone() for p in b.network.parameters()]
    for ln in (a, b):
      ln.update_weights(batch)
      ln.training_step += 1
    assert a._native is not None and b._native is None and b._graph is None
    assert not torch.is_tensor(a.optimizer.param_groups[0]['lr'])
    lr = float(b.optimizer.param_groups[0]['lr'])
    assert float(a.optimizer.param_groups[0]['lr']) == lr
    if snap is not None:
      gd = a._native.grad()
      g = torch.cat([gd[k].reshape(-1) for k in WEIGHT_ORDER]).double().to(a.device)
      if clip:
        g = g * clip_coef([g], clip)
      w0, m0, v0 = [t.double() for t in snap]
      w1, m1, v1 = restate(kind, w0, g, m0, v0, lr_used, mom, wd)
      assert (a._native.flat.double() - w1).abs().max().item() <= 2e-7, (a._native.flat.double() - w1).abs().max().item()
      if mom:
        assert (a._native.m.double() - m1).abs().max().item() <= 1e-6 * m1.abs().max().item()
      else:
        assert torch.equal(a._native.m, snap[1])          # (no buffer: never written)
      if kind == 'RMSprop':
        assert (a._native.v.double() - v1).abs().max().item() <= 1e-6 * v1.abs().max().item()
      else:
        assert torch.equal(a._native.v, snap[2])
    moved = max((pb.detach() - q).abs().max().item() for pb, q in zip(b.network.parameters(), before))
    dws = []
    for (k, pa), pb in zip(a.network.named_parameters(), b.network.parameters()):
      sa, sb = a.optimizer.state.get(pa, {}), b.optimizer.state.get(pb, {})
      assert set(sa) == set(sb), (k, set(sa), set(sb))
      if kind == 'RMSprop':
        assert float(sa['step']) == float(sb['step']) == step + 1
      d = (pa - pb).abs().reshape(-1)
      dws.append(d)
      assert d.max().item() <= 2.5 * moved + 1e-6, (step, k, d.max().item(), moved)
      for key in keys:
        dm = (sa[key] - sb[key]).abs().max().item() / (sb[key].abs().max().item() + 1e-30)
        assert dm <= 3e-2, (step, k, key, dm)
    frac = (torch.cat(dws) > 1e-6).float().mean().item()
    assert frac <= 0.02, (step, frac)
    ea, eb = L['native'][1].updates[-1][1], L['torch'][1].updates[-1][1]
    assert np.abs(ea - eb).max() <= 5e-4
    la, lb = dict(a.losses_to_log), dict(b.losses_to_log)
    assert all(abs(la[k] - lb[k]) <= 1e-4 * max(1.0, abs(lb[k])) for k in lb), (la, lb)
    with torch.no_grad():                       # lock-step: the eager learner's state into the native learner's flat vectors
      for pa, pb in zip(a.network.parameters(), b.network.parameters()):
        pa.copy_(pb)
        for key in keys:
          a.optimizer.state[pa][key].copy_(b.optimizer.state[pb][key])
  sa, sb = a.optimizer.state_dict(), b.optimizer.state_dict()
  assert set(sa['state']) == set(sb['state'])
  for i in sb['state']:
    assert {k: tuple(v.shape) for k, v in sa['state'][i].items()} == {k: tuple(v.shape) for k, v in sb['state'][i].items()}
  assert sa['param_groups'][0].keys() == sb['param_groups'][0].keys()
  path_n = a.save_state()
  state = torch.load(path_n, map_location='cpu', weights_only=False)
  again = Learner(L['torch'][2], Sink(), Sink(), state=state)
  for (k, v), pa in zip(again.network.state_dict().items(), a.network.state_dict().values()):
    assert torch.equal(v.cpu(), pa.cpu()), k
  for pa, pg in zip(a.network.parameters(), again.network.parameters()):
    for key in keys:
      assert torch.equal(again.optimizer.state[pg][key].cpu(), a.optimizer.state[pa][key].cpu()), key


def _g5_batch():
  g5 = np.load(os.path.join(G, 'g5_learner_lunar.npz'))
  w0 = {k[3:]: torch.from_numpy(g5[k]) for k in g5.files if k.startswith('w0.')}
  batch = ((g5['sample_obs'].copy(), g5['sample_actions'].tolist(),
            (g5['sample_target_rewards'].copy(), g5['sample_target_values'].copy(), g5['sample_target_policies'].copy())),
           g5['sample_idxs'].tolist(), g5['sample_is_weights'].copy())
  return w0, batch


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['SGD', 'RMSprop'])
def test_sgd_rmsprop_launch_structures_give_the_same_bits(tmp_path, monkeypatch, opt):
  """batch 256: the two-launch step (k_fcl_fb + k_fcl_dwa), the three-launch one (MZ_FCL_FUSE_FB=0) and the four-launch one
  (MZ_FCL_FUSE_FWD=0) give the same weights, buffers, refreshes and loss sums bit for bit after two updates"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  w0, batch = _g5_batch()

  def run(tag):
    cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '256', '--optimizer', opt, '--seed', '0', '--use_gpu_for', 'actors',
                       'learner', '--runs_dir', str(tmp_path / tag), '--run_tag', 'x'])
    sink = Sink()
    ln = Learner(cfg, sink, sink)
    ln.network.load_state_dict(w0)
    for _ in range(2):
      ln.update_weights(batch)
    assert ln._native is not None
    out = (ln._native.flat.cpu().numpy().copy(), ln._native.m.cpu().numpy().copy(), ln._native.v.cpu().numpy().copy(),
           [np.asarray(e).copy() for _, e in sink.updates], [ln.losses_to_log[k] for k in ('reward', 'value', 'policy')])
    ln._native.close()
    return out
  base = run('fb')
  assert base[1].any() and (opt == 'SGD') == (not base[2].any())
  for knobs in ({'MZ_FCL_FUSE_FB': '0'}, {'MZ_FCL_FUSE_FWD': '0'}):
    with monkeypatch.context() as m:
      for k, val in knobs.items():
        m.setenv(k, val)
      other = run('k' + ''.join(knobs))
    for x, y in zip(base[:3], other[:3]):
      assert np.array_equal(x, y), knobs
    assert all(np.array_equal(x, y) for x, y in zip(base[3], other[3])) and base[4] == other[4], knobs


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['SGD', 'RMSprop'])
@pytest.mark.parametrize('bs,extra', [(512, []), (1024, []), (2048, []), (256, ['--clip_grad', '1']), (64, ['--clip_grad', '1', '--momentum', '0'])])
def test_sgd_rmsprop_unfused_paths_against_the_restatement(tmp_path, opt, bs, extra):
  """the other structures of the update: batch 512 (four launches, the update fused into the weight-gradient jobs), 1024 and 2048
  (row slabs: the update in k_fcl_adam) and gradient clipping (k_fcl_grad + k_fcl_adam): the third update's new weights and buffers
  are the float64 restatement applied to the native step's own gradient"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import WEIGHT_ORDER
  from model_based_rl_amd.learners import Learner
  cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', str(bs), '--optimizer', opt, '--seed', '5', '--use_gpu_for', 'actors',
                     'learner', '--runs_dir', str(tmp_path), '--run_tag', 'x'] + extra)
  cfg.obs_space, cfg.action_space = (8,), 4
  ln = Learner(cfg, Sink(), Sink())
  rng = np.random.default_rng(bs)
  grp = ln.optimizer.param_groups[0]
  mom, wd, clip = float(grp['momentum']), float(grp['weight_decay']), float(getattr(cfg, 'clip_grad', 0) or 0)
  for i in range(3):
    h = _random_batch(rng, bs, 5, 8, 4)
    batch = ((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(bs)), h['w'])
    if i == 2:
      snap = [t.double() for t in (ln._native.flat, ln._native.m, ln._native.v)]
      lr = float(np.float32(grp['lr']))
    ln.update_weights(batch)
  assert ln._native is not None
  gd = ln._native.grad()
  g = torch.cat([gd[k].reshape(-1) for k in WEIGHT_ORDER]).double().to(ln.device)
  if clip:
    g = g * clip_coef([g], clip)
  w1, m1, v1 = restate(opt, snap[0], g, snap[1], snap[2], lr, mom, wd)
  assert (ln._native.flat.double() - w1).abs().max().item() <= 2e-7
  if mom:
    assert (ln._native.m.double() - m1).abs().max().item() <= 1e-6 * m1.abs().max().item()
  if opt == 'RMSprop':
    assert (ln._native.v.double() - v1).abs().max().item() <= 1e-6 * v1.abs().max().item()
    assert float(ln.optimizer.state[ln._native.params[0]]['step']) == 3


@pytest.mark.gpu
@pytest.mark.parametrize('flags', [['--optimizer', 'SGD', '--lr_scheduler', 'MuZeroLR', '--lr_decay_steps', '50'], ['--optimizer', 'RMSprop']])
def test_native_loop_with_sgd_rmsprop_equals_the_per_update_path(tmp_path, flags):
  """Learner.learn through mz_fcl_run (the loop body in native code) against the per-update path driven from Python in the same
  order on twin replays: the same weights, buffers and priorities bit for bit after 37 updates"""
  import random
  from collections import deque
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine, flatten_weights
  from model_based_rl_amd.learners import Learner
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = make_config(['--environment', 'LunarLander-v2', '--seed', '2', '--batch_size', '64', '--num_envs', '256', '--num_simulations', '8',
                     '--window_size', '16384', '--stored_before_train', '1000', '--use_gpu_for', 'actors', 'learner', '--send_weights_frequency', '16',
                     '--learner_log_frequency', '10', '--save_state_frequency', '1000000', '--beta', '0.6', '--runs_dir', str(tmp_path), '--run_tag', 'x'] + flags)
  torch.manual_seed(0)
  eng = Engine.from_config(cfg, 256)
  eng.set_weights(flatten_weights(get_network(cfg, torch.device('cpu')).state_dict()))
  eng.selfplay_reset(12, 1.0, stagger=True)
  eng.selfplay_steps(40)
  buf, nmv = eng.selfplay_drain()
  torch.cuda.synchronize()
  records = buf[:nmv].numpy().copy()
  eng.close()

  def world():
    replay = PrioritizedReplay(cfg)
    replay.ingest_records(records, nmv, 256)
    learner = Learner(cfg, SharedStorage(cfg), replay)
    random.seed(7); np.random.seed(8)
    learner.update_weights(replay.sample_batch_arrays())
    learner.training_step += 1
    assert learner._native is not None
    return learner, replay

  n = 37
  a, ra = world()
  slots = a._native.lib.mz_fcl_slots(a._native.h)
  owed = deque()
  lrs = a._scheduled_lrs(n)
  for i in range(n):
    if len(owed) == slots:
      ix, slot = owed.popleft()
      ra.update(ix, a._native.errors(slot))
    host, ix = a._host_batch(ra.sample_batch_arrays())
    if lrs is not None:
      a.optimizer.param_groups[0]['lr'] = float(lrs[i])
    owed.append((ix, a._native.launch(host)))
  while owed:
    ix, slot = owed.popleft()
    ra.update(ix, a._native.errors(slot))
  c, rc = world()
  c.learn(max_steps=n)
  assert c.training_step == 1 + n and c.native_loop_updates == n > 0
  for name, t_a, t_c in (('weights', a._native.flat, c._native.flat), ('buffer', a._native.m, c._native.m), ('square_avg', a._native.v, c._native.v),
                         ('steps', a._native.steps, c._native.steps)):
    assert torch.equal(t_a, t_c), (name, (t_a - t_c).abs().max().item())
  assert np.array_equal(ra.tree.leaves(), rc.tree.leaves())
  if lrs is not None:
    assert float(c.optimizer.param_groups[0]['lr']) == float(c.lr_scheduler.lr) < cfg.lr_init


@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['SGD', 'RMSprop'])
@pytest.mark.parametrize('before', [0, 2])
def test_eager_sgd_rmsprop_checkpoint_resumes_under_the_native_step(tmp_path, opt, before):
  """a checkpoint of the eager learner (--no_native_learner) -- saved before its first update (torch's SGD has no momentum_buffer
  yet, RMSprop no state) or after two -- resumes under the native step, whose next update matches the eager learner's under the
  lock-step bound"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  rng = np.random.default_rng(17)
  batches = []
  for _ in range(before + 1):
    h = _random_batch(rng, 64, 5, 8, 4)
    batches.append(((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(64)), h['w']))

  def cfg_of(extra, tag):
    c = make_config(['--environment', 'LunarLander-v2', '--seed', '3', '--batch_size', '64', '--optimizer', opt, '--use_gpu_for', 'actors',
                     'learner', '--runs_dir', str(tmp_path / tag), '--run_tag', 'x'] + extra)
    c.obs_space, c.action_space = (8,), 4
    return c
  eager = Learner(cfg_of(['--no_native_learner'], 'e'), Sink(), Sink())
  for bt in batches[:before]:
    eager.update_weights(bt)
    eager.training_step += 1
  path = eager.save_state()
  state = torch.load(path, map_location='cpu', weights_only=False)
  assert bool(state['optimizer']['state']) == (before > 0)
  w_before = [p.detach().clone() for p in eager.network.parameters()]
  eager.update_weights(batches[before])
  moved = max((p.detach() - q).abs().max().item() for p, q in zip(eager.network.parameters(), w_before))
  native = Learner(cfg_of([], 'n'), Sink(), Sink(), state=state)
  native.update_weights(batches[before])
  assert native._native is not None and eager._native is None
  d = torch.cat([(pa - pb).abs().reshape(-1) for pa, pb in zip(native.network.parameters(), eager.network.parameters())])
  assert d.max().item() <= 2.5 * moved + 1e-6 and (d > 1e-6).float().mean().item() <= 0.02, (d.max().item(), moved)
  for pa, pb in zip(native.network.parameters(), eager.network.parameters()):
    sa, sb = native.optimizer.state[pa], eager.optimizer.state[pb]
    assert set(sa) == set(sb)
    if opt == 'RMSprop':
      assert float(sa['step']) == float(sb['step']) == before + 1


@pytest.mark.gpu
def test_sgd_switches_and_set_optimizer_refusals(tmp_path):
  """--no_graph_learner and --no_native_learner keep SGD on the eager PyTorch step; mz_fcl_set_optimizer refuses an unknown kind,
  a negative or NaN momentum and alpha outside [0, 1), naming the problem"""
  from model_based_rl_amd import _abi
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  rng = np.random.default_rng(5)
  h = _random_batch(rng, 64, 5, 8, 4)
  batch = ((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(64)), h['w'])
  nat = None
  for extra, native in (([], True), (['--no_graph_learner'], False), (['--no_native_learner'], False)):
    cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '64', '--optimizer', 'SGD', '--use_gpu_for', 'actors', 'learner',
                       '--runs_dir', str(tmp_path / ('r%d' % len(extra))), '--run_tag', 'x'] + extra)
    cfg.obs_space, cfg.action_space = (8,), 4
    ln = Learner(cfg, Sink(), Sink())
    ln.update_weights(batch)
    assert (ln._native is not None) == native and ln._graph is None and not ln.use_graph, extra
    nat = nat or ln._native
  lib, hnd = _abi.load(), nat.h
  for args, word in (((3, 0.9, 0.99), 'kind'), ((-1, 0.9, 0.99), 'kind'), ((1, -0.1, 0.99), 'momentum'), ((2, float('nan'), 0.99), 'momentum'),
                     ((2, 0.9, 1.0), 'alpha'), ((2, 0.9, -0.5), 'alpha')):
    assert lib.mz_fcl_set_optimizer(hnd, *args) != 0, args
    with pytest.raises(Exception, match=word):
      _abi.check(lib.mz_fcl_set_optimizer(hnd, *args), 'mz_fcl_set_optimizer')
  assert lib.mz_fcl_set_optimizer(hnd, 1, 0.9, 0.0) == 0
  assert lib.mz_fcl_set_optimizer(C.c_void_p(), 1, 0.9, 0.0) != 0
