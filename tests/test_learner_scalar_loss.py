"""--no_support in the learner (utils.py:61-70, learners.py:182-206): the value and reward heads end in one output each, trained with
torch.nn.MSELoss or SmoothL1Loss (--scalar_loss Huber) against the transformed scalar targets.  A float64 restatement of both losses
against torch's own, the PyTorch learner against two steps of the unmodified reference (goldens g9,
scripts/make_scalar_loss_goldens.py), and on the MI355X the native step in scalar mode (mz_fcl_set_scalar_loss, csrc/mz_fcl.hip.h)
against the reference, against autograd entry by entry, across its launch structures, against the PyTorch learner in lock-step, in the
native loop, at the C ABI and on the way to the actor."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from .test_learner import G, Sink, _random_batch, grads_close, native_tape

LOSSES = {'MSE': [], 'Huber': ['--scalar_loss', 'Huber']}


# ------------------------------------------------------------------------------------------------ the two losses, restated
def restate_loss(kind, y, t):
  """(l, dl / dy) of torch.nn.MSELoss / SmoothL1Loss (beta 1), reduction 'none', on float64 tensors -- what csrc/mz_fcl.hip.h's
  scalar heads compute per (sample, position)"""
  d = y - t
  if kind == 'MSE':
    return d * d, 2.0 * d
  quad = d.abs() < 1.0
  return torch.where(quad, 0.5 * d * d, d.abs() - 0.5), torch.where(quad, d, torch.sign(d))


@pytest.mark.parametrize('kind', ['MSE', 'Huber'])
def test_restated_scalar_losses_equal_torch_in_float64(kind):
  """the restatement against torch.nn.MSELoss / SmoothL1Loss and autograd in float64: residuals of exactly 0 and +-1, one ulp (and a
  little more) on either side of +-1, and a random spread"""
  one = 1.0
  below, above = np.nextafter(one, 0.0), np.nextafter(one, 2.0)
  edge = [0.0, one, -one, below, -below, above, -above, 1.0 - 1e-9, 1.0 + 1e-9, -1.0 + 1e-9, -1.0 - 1e-9, 0.5, -0.5, 3.0, -7.25]
  rng = np.random.default_rng(2)
  t = torch.from_numpy(np.concatenate([rng.uniform(-3, 3, len(edge)), rng.uniform(-3, 3, 200)]))
  d = torch.from_numpy(np.concatenate([edge, rng.uniform(-2.5, 2.5, 200)]))
  y = (t + d).clone().requires_grad_(True)
  # (y - t reproduces the chosen residuals exactly only where the sum was exact: take the residuals torch itself sees)
  seen = (y.detach() - t)
  assert (seen[:3] == torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)).all()
  assert bool((seen.abs() < 1).any()) and bool((seen.abs() > 1).any()) and bool((seen.abs() == 1).any())
  fn = torch.nn.SmoothL1Loss(reduction='none') if kind == 'Huber' else torch.nn.MSELoss(reduction='none')
  want = fn(y, t)
  wts = torch.from_numpy(rng.uniform(0.2, 1.0, y.numel()))
  (wts * want).sum().backward()
  l, dl = restate_loss(kind, y.detach(), t)
  assert torch.allclose(l, want.detach(), rtol=1e-15, atol=1e-16)
  assert torch.allclose(wts * dl, y.grad, rtol=1e-15, atol=1e-16)


# ------------------------------------------------------------------------------------------------ against the reference (g9)
def g9_run(tmp_path, device_flag, loss, w_tol, far_frac, loss_tol, err_tol=2e-4, far_tol=2e-6):
  """two Learner.update_weights steps on g9_learner_scalar_w0's weights and g5_learner_lunar's batch against g9_learner_<loss>_lunar
  (the reference's --no_support steps): every weight within w_tol, at most far_frac of them further than far_tol; loss sums; priority
  refreshes"""
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
  from make_optimizer_goldens import decode_weights
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  g5 = np.load(os.path.join(G, 'g5_learner_lunar.npz'))
  g9 = np.load(os.path.join(G, 'g9_learner_%s_lunar.npz' % loss.lower()))
  gw = np.load(os.path.join(G, 'g9_learner_scalar_w0.npz'))
  w0 = {k[3:]: gw[k] for k in gw.files}
  want = decode_weights(g9, w0)
  cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '256', '--no_support', '--seed', '0', '--use_gpu_for'] + device_flag +
                    ['--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'g9'] + LOSSES[loss])
  sink = Sink()
  learner = Learner(cfg, sink, sink)
  for k, v in learner.network.state_dict().items():          # (the goldens' initial weights are this repository's under --seed 0)
    assert np.array_equal(v.cpu().numpy(), w0[k]), k
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
  losses = np.array([learner.losses_to_log[k] for k in ('reward', 'value', 'policy')])
  errs = max(float(np.abs(err - ref).max()) for (_, err), ref in zip(sink.updates, g9['new_errors']))
  print('--no_support %s learner on %s: max |dw| %.3g after two AdamW steps, %.4f %% of the weights further than %g, max |dloss| %.3g, '
        'max |d new_errors| %.3g' % (loss, learner.device, worst, 100.0 * far / total, far_tol, np.abs(losses - g9['losses']).max(), errs))
  assert far <= far_frac * total, (far, total)
  assert np.abs(losses - g9['losses']).max() <= loss_tol
  assert len(sink.updates) == 2
  for (idxs, err), ref in zip(sink.updates, g9['new_errors']):
    assert idxs == [int(i) for i in g5['sample_idxs']]
    assert np.abs(err - ref).max() <= err_tol
  return learner


@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
def test_pytorch_learner_matches_reference_no_support(tmp_path, loss):
  """the PyTorch learner on the CPU against the reference's two --no_support steps (g9), under the bounds
  test_pytorch_learner_matches_reference_sgd_rmsprop holds SGD to: every weight within 2e-6, loss sums within 1e-5, priority refreshes
  within 2e-4 (measured where the goldens were made: max |dw| 3.0e-8, loss sums 2.6e-8, refreshes 2.4e-7)"""
  g9_run(tmp_path, ['actors'], loss, 2e-6, 0.0, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
def test_native_scalar_step_matches_reference_at_the_benched_shapes(tmp_path, loss):
  """... and THROUGH THE NATIVE STEP on the MI355X in scalar mode, under the bounds test_native_step_matches_reference_at_the_benched_shapes
  applies to g5_learner_lunar (same shapes, optimiser and rate: the same lr / eps amplification of Adam): 99 % of the weights within
  2e-6, all within 2.5 learning rates, loss sums within 5e-5, refreshes within 2e-4.  Figures on the MI355X: not measured yet (printed with -s)."""
  learner = g9_run(tmp_path, ['actors', 'learner'], loss, 2e-3, 0.01, 5e-5)
  assert learner.device.type == 'cuda' and learner._native is not None


# ------------------------------------------------------------------------------------------------ eligibility
def _stand_in_learner(flags, device):
  """what _NativeFC.eligible looks at, without a GPU: the configuration, an FCNetwork (on the host), the optimiser as the learner builds
  it for a GPU (a device-tensor rate for Adam / AdamW: the capturable form), and the device it would run on"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import make_optimizer
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '16'] + flags)
  cfg.obs_space, cfg.action_space = (8,), 4
  net = get_network(cfg, torch.device('cpu'))
  adam = cfg.optimizer in ('AdamW', 'Adam')
  opt = make_optimizer(cfg, net.parameters(), capturable=False)
  if adam:
    opt.param_groups[0]['lr'] = torch.tensor(float(opt.param_groups[0]['lr']))
  graph = not getattr(cfg, 'no_graph_learner', False)
  return types.SimpleNamespace(config=cfg, network=net, optimizer=opt, device=torch.device(device), use_graph=adam and graph,
                               native_only=(not adam) and graph and not getattr(cfg, 'no_native_learner', False))


def test_no_support_is_eligible_for_the_native_step():
  """_NativeFC.eligible accepts --no_support with both scalar losses and every optimiser family; the switches that select the PyTorch
  paths and a learner that is not on a GPU still decline (a stand-in for the learner: eligible reads its configuration, network,
  optimiser and device, and touches no device)"""
  from model_based_rl_amd.learners import _NativeFC
  host = _random_batch(np.random.default_rng(0), 16, 5, 8, 4)
  for loss in LOSSES.values():
    for opt in ([], ['--optimizer', 'Adam'], ['--optimizer', 'SGD'], ['--optimizer', 'RMSprop', '--momentum', '0']):
      assert _NativeFC.eligible(_stand_in_learner(['--no_support'] + loss + opt, 'cuda'), host), (loss, opt)
      assert not _NativeFC.eligible(_stand_in_learner(['--no_support', '--no_native_learner'] + loss + opt, 'cuda'), host)
      assert not _NativeFC.eligible(_stand_in_learner(['--no_support', '--no_graph_learner'] + loss + opt, 'cuda'), host)
      assert not _NativeFC.eligible(_stand_in_learner(['--no_support'] + loss + opt, 'cpu'), host)
  assert _NativeFC.eligible(_stand_in_learner([], 'cuda'), host)                      # (the categorical default, as before)
  odd = _stand_in_learner(['--no_support'], 'cuda')
  odd.config.scalar_loss = 'L1'                                                        # (no such kind in the native step)
  assert not _NativeFC.eligible(odd, host)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
def test_no_support_learner_takes_the_native_step(tmp_path, loss):
  """on the GPU: eligible, and Learner.update_weights builds the native step; --no_native_learner and --no_graph_learner keep the
  PyTorch paths"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner, _NativeFC
  h = _random_batch(np.random.default_rng(5), 16, 5, 8, 4)
  batch = ((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(16)), h['w'])
  for extra, native in (([], True), (['--no_native_learner'], False), (['--no_graph_learner'], False)):
    cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '16', '--no_support', '--use_gpu_for', 'actors', 'learner',
                       '--runs_dir', str(tmp_path / ('r%d' % len(extra))), '--run_tag', 'x', '--no_tune_gemms'] + LOSSES[loss] + extra)
    cfg.obs_space, cfg.action_space = (8,), 4
    ln = Learner(cfg, Sink(), Sink())
    assert _NativeFC.eligible(ln, h) == native, extra
    ln.update_weights(batch)
    assert (ln._native is not None) == native, extra
    assert (ln._graph is not None) == (extra == ['--no_native_learner']), extra
    if ln._native is not None:
      ln._native.close()


# ------------------------------------------------------------------------------------------------ gradients against autograd
def scalar_forward(net, obs, act, masks=None, margins=None):
  """the K-step unroll (learners.py:174,198-206) -> value [K + 1][bs], policy logits [K + 1][bs][A], reward [K][bs]; masks: the ReLU
  on / off patterns (chain fc1, hidden states, the heads' fc1) to use instead of the pre-activations' own signs -- and then the
  largest |pre-activation| (relative to its layer's scale) whose own sign disagrees with the pattern comes back too; margins: a list
  that receives every ReLU's smallest |pre-activation|"""
  K, A = act.shape[1], net.action_space
  m_a1c, m_h, m_a1h = masks if masks is not None else ([None] * (K + 1), [None] * (K + 1), [[None] * (K + 1)] * 3)
  worst_flip = [0.0]
  def relu_as(pre, mask):
    if margins is not None:
      margins.append(float(pre.detach().abs().min()))
    if mask is None:
      return torch.relu(pre)
    mine = pre > 0
    if bool((mine != mask).any()):
      worst_flip[0] = max(worst_flip[0], float(pre.detach()[mine != mask].abs().max()) / (1.0 + float(pre.detach().abs().max())))
    return pre * mask.to(pre.dtype)
  onehot = torch.nn.functional.one_hot(act.to(torch.int64), A).to(torch.float32)
  h = relu_as(net.LN(net.representation_head.out(relu_as(net.representation_head.fc1(obs), m_a1c[0]))), m_h[0])
  hs, xs = [h], []
  for i in range(K):
    x = torch.cat((h, onehot[:, i]), dim=1)
    xs.append(x)
    h = relu_as(net.LN(net.transition_head.out(relu_as(net.transition_head.fc1(x), m_a1c[i + 1]))), m_h[i + 1])
    if h.requires_grad:
      h.register_hook(lambda grad: grad * 0.5)
    hs.append(h)
  value = torch.stack([net.value_head.value(relu_as(net.value_head.fc1(hs[p]), m_a1h[0][p])) for p in range(K + 1)]).squeeze(2)
  policy = torch.stack([net.policy_head.policy(relu_as(net.policy_head.fc1(hs[p]), m_a1h[1][p])) for p in range(K + 1)])
  reward = torch.stack([net.reward_head.reward(relu_as(net.reward_head.fc1(xs[p - 1]), m_a1h[2][p])) for p in range(1, K + 1)]).squeeze(2)
  return value, policy, reward, worst_flip[0]


def scalar_targets(cfg, t_val, t_rew):
  from model_based_rl_amd.learners import scalar_transform
  return (t_val, t_rew) if cfg.no_target_transform else (scalar_transform(t_val), scalar_transform(t_rew))


def scalar_masked_reference(learner, nat, dev):
  """the scalar-loss sibling of test_learner.masked_reference: PyTorch autograd over the learner's parameters (learners.py:164-214 with
  --no_support written out: torch's own MSELoss / SmoothL1Loss on the transformed targets, importance weights, the 0.5 and 1 / K
  hooks) with every ReLU's on / off pattern taken from the native step's tapes; wherever PyTorch's own pattern differs the
  pre-activation must be within 2e-5 of zero.  Returns (gradients by name, new_errors, the three loss means)."""
  cfg, net = learner.config, learner.network
  obs, act, t_rew, t_val, t_pol, w = dev
  bs, K = obs.shape[0], act.shape[1]
  K1, device = K + 1, obs.device
  masks = ((native_tape(nat, 1, 512) > 0).to(device), (native_tape(nat, 4, 64)[:, :, :50] > 0).to(device),
           (native_tape(nat, 7, 512) > 0).to(device).reshape(3, K1, bs, 512))
  for p_ in net.parameters():
    p_.grad = None
  value, policy, reward, worst_flip = scalar_forward(net, obs, act, masks)
  with torch.no_grad():
    new_errors = value[0] - t_val[:, 0]                                  # learners.py:182: the raw output, the untransformed target
    tv, tr = scalar_targets(cfg, t_val, t_rew)
  fn = torch.nn.SmoothL1Loss(reduction='none') if cfg.scalar_loss == 'Huber' else torch.nn.MSELoss(reduction='none')
  value_loss = fn(value, tv.transpose(0, 1)).sum(0)
  reward_loss = fn(reward, tr.transpose(0, 1)[1:]).sum(0)
  policy_loss = (-t_pol.transpose(0, 1) * torch.log_softmax(policy, dim=2)).sum(2).sum(0)
  losses = [(w * reward_loss).mean(), (w * value_loss).mean(), (w * policy_loss).mean()]
  total = losses[0] + losses[1] + losses[2]
  total.register_hook(lambda grad: grad * (1 / K))
  total.backward()
  assert worst_flip <= 2e-5, worst_flip
  grads = {k: p_.grad.detach().cpu().clone() for k, p_ in net.named_parameters()}
  for p_ in net.parameters():
    p_.grad = None
  return grads, new_errors.detach(), [float(x.detach()) for x in losses]


def _scalar_learner(tmp_path, env, O, A, bs, K, extra, device_flag, tag):
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  cfg = make_config(['--environment', env, '--seed', '3', '--batch_size', str(bs), '--num_unroll_steps', str(K), '--no_support', '--use_gpu_for'] +
                    device_flag + ['--runs_dir', str(tmp_path / tag), '--run_tag', 'x', '--no_tune_gemms'] + extra)
  cfg.obs_space, cfg.action_space = (O,), A
  learner = Learner(cfg, Sink(), Sink())
  net = learner.network
  assert net.action_space == A and net.representation_head.fc1.in_features == O and net.value_head.value.out_features == 1
  with torch.no_grad():                              # away from the initialisation: LayerNorm and biases not at 1 / 0
    g = torch.Generator().manual_seed(5)
    for p in net.parameters():
      p.add_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))
  return learner


def _scalar_gradients_vs_autograd(tmp_path, env, O, A, bs, K, extra, loss):
  """mz_fcl_step in scalar mode against PyTorch autograd over the same parameters and batch: every parameter's gradient, the priority
  refresh and the three loss sums, with the ReLU patterns of the native run (scalar_masked_reference).  Targets from _random_batch with
  lo = -18, hi = 18.  For Huber the batch must exercise BOTH branches in BOTH scalar heads: checked on PyTorch's own forward pass on
  the host, before the GPU is touched."""
  from model_based_rl_amd.learners import _NativeFC, _GraphedUpdate
  flags = extra + LOSSES[loss]
  rng = np.random.default_rng(bs * 10 + K)
  host = _random_batch(rng, bs, K, O, A, lo=-18.0, hi=18.0)
  cpu = _scalar_learner(tmp_path, env, O, A, bs, K, flags, ['actors'], 'c')
  assert cpu.device.type == 'cpu'
  with torch.no_grad():
    value, _, reward, _ = scalar_forward(cpu.network, torch.from_numpy(host['obs']), torch.from_numpy(host['act']))
    tv, tr = scalar_targets(cpu.config, torch.from_numpy(host['t_val']), torch.from_numpy(host['t_rew']))
    fracs = []
    for d in ((value - tv.transpose(0, 1)).abs(), (reward - tr.transpose(0, 1)[1:]).abs()):
      fracs += [float((d < 1).float().mean()), float((d > 1).float().mean())]
  if loss == 'Huber':          # at least 5 % of the (sample, position) residuals on each side of |d| = 1, value and reward head
    assert min(fracs) >= 0.05, fracs
  learner = _scalar_learner(tmp_path, env, O, A, bs, K, flags, ['actors', 'learner'], 'g')
  net = learner.network
  for (k, a), b in zip(net.state_dict().items(), cpu.network.state_dict().values()):
    assert torch.equal(a.cpu(), b), k
  assert _NativeFC.eligible(learner, host)
  dev = [torch.from_numpy(host[k]).to(learner.device) for k in _GraphedUpdate.ORDER]
  before = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
  nat = _NativeFC(learner, host)
  learner._loss_dev.zero_()
  got_errors = nat.step(*dev, no_update=True)
  got = nat.grad()
  got_l = learner._loss_dev.tolist()
  want, new_errors, losses = scalar_masked_reference(learner, nat, dev)
  worst = grads_close(got, want)
  derr = (got_errors - new_errors).abs().max().item()
  print('native scalar-loss step vs autograd (%s, %s, batch %d, K %d): worst relative gradient difference %.2g, refresh %.2g; residuals below / above 1: '
        'value %.2f / %.2f, reward %.2f / %.2f' % (loss, env, bs, K, worst, derr, fracs[0], fracs[1], fracs[2], fracs[3]))
  assert all(float(want[k].abs().max()) > 0 for k in want)
  assert derr <= 1e-5 * (1 + new_errors.abs().max().item())          # (no inverse transform in this mode: no staircase)
  for a, b in zip(got_l, losses):
    assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (got_l, losses)
  for k, p in net.named_parameters():                # no_update: nothing moved
    assert torch.equal(p.detach().cpu(), before[k]), k
  nat.close()


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
@pytest.mark.parametrize('env,O,A,bs,K,extra', [('LunarLander-v2', 8, 4, 16, 1, []), ('TicTacToe', 9, 9, 16, 5, ['--no_target_transform']),
                                                 ('Pong-ramNoFrameskip-v4', 128, 6, 32, 3, []), ('LunarLander-v2', 8, 4, 64, 7, [])])
def test_native_scalar_step_gradients_equal_autograd(tmp_path, env, O, A, bs, K, extra, loss):
  _scalar_gradients_vs_autograd(tmp_path, env, O, A, bs, K, extra, loss)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
@pytest.mark.parametrize('knobs', [{'MZ_FCL_GROUPS': '2', 'MZ_FCL_SLABS': '2'}, {'MZ_FCL_GROUPS': '4', 'MZ_FCL_SLABS': '4'},
                                   {'MZ_FCL_FUSE_FWD': '0'}, {'MZ_FCL_FUSE_FB': '0'}, {'MZ_FCL_SLABS': '3'}])
def test_native_scalar_step_launch_structures_of_other_batch_sizes(tmp_path, monkeypatch, knobs, loss):
  """the launch structures the step takes at other batch sizes, forced at batch 64 (k_fcl_heads_scalar as a launch of its own with row
  slabs and groups, the fused forward launch without the backward chain, the forward pass as two launches): the same gradient check"""
  for k, val in knobs.items():
    monkeypatch.setenv(k, val)
  _scalar_gradients_vs_autograd(tmp_path, 'LunarLander-v2', 8, 4, 64, 7, [], loss)


@pytest.mark.gpu
@pytest.mark.parametrize('loss', ['MSE', 'Huber'])
def test_scalar_loss_launch_structures_give_the_same_bits(tmp_path, monkeypatch, loss):
  """batch 256: the two-launch step (k_fcl_fb + k_fcl_dwa), the three-launch one (MZ_FCL_FUSE_FB=0) and the four-launch one
  (MZ_FCL_FUSE_FWD=0) give the same weights, moments, refreshes and loss sums bit for bit after two updates of the golden batch"""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  g5 = np.load(os.path.join(G, 'g5_learner_lunar.npz'))
  batch = ((g5['sample_obs'].copy(), g5['sample_actions'].tolist(),
            (g5['sample_target_rewards'].copy(), g5['sample_target_values'].copy(), g5['sample_target_policies'].copy())),
           g5['sample_idxs'].tolist(), g5['sample_is_weights'].copy())

  def run(tag):
    cfg = make_config(['--environment', 'LunarLander-v2', '--batch_size', '256', '--no_support', '--seed', '0', '--use_gpu_for', 'actors',
                       'learner', '--runs_dir', str(tmp_path / tag), '--run_tag', 'x'] + LOSSES[loss])
    sink = Sink()
    ln = Learner(cfg, sink, sink)
    for _ in range(2):
      ln.update_weights(batch)
    assert ln._native is not None
    out = (ln._native.flat.cpu().numpy().copy(), ln._native.m.cpu().numpy().copy(), ln._native.v.cpu().numpy().copy(),
           [np.asarray(e).copy() for _, e in sink.updates], [ln.losses_to_log[k] for k in ('reward', 'value', 'policy')])
    ln._native.close()
    return out
  base = run('fb')
  assert base[1].any() and base[2].any() and np.isfinite(base[0]).all()
  for knobs in ({'MZ_FCL_FUSE_FB': '0'}, {'MZ_FCL_FUSE_FWD': '0'}):
    with monkeypatch.context() as m:
      for k, val in knobs.items():
        m.setenv(k, val)
      other = run('k' + ''.join(knobs))
    for x, y in zip(base[:3], other[:3]):
      assert np.array_equal(x, y), knobs
    assert all(np.array_equal(x, y) for x, y in zip(base[3], other[3])) and base[4] == other[4], knobs


# ------------------------------------------------------------------------------------------------ lock-step with the PyTorch learner
LOCKSTEP_FLAGS = [[], ['--scalar_loss', 'Huber', '--optimizer', 'SGD'], ['--optimizer', 'RMSprop', '--momentum', '0'],
                  ['--scalar_loss', 'Huber', '--clip_grad', '1']]


@pytest.mark.gpu
@pytest.mark.parametrize('flags', LOCKSTEP_FLAGS, ids=['-'.join(f[1::2]) or 'AdamW' for f in LOCKSTEP_FLAGS])
def test_native_no_support_learner_equals_the_pytorch_learner(tmp_path, flags):
  """three updates on changing random batches, LunarLander shapes, batch 16: the native step against the PyTorch learner
  (--no_native_learner: the captured graph for AdamW, the eager step for SGD / RMSprop), in lock-step -- after every update the
  weights, the optimiser's state, the priority refreshes and the loss sums are compared, then the PyTorch learner's state is copied
  into the native one.  Bounds: those of test_native_learner_equals_the_pytorch_learner (AdamW: every weight within 2.5 learning
  rates) and test_native_sgd_rmsprop_learner_equals_the_eager_learner (every weight within 2.5 times the update's largest move); both:
  98 % of the weights within 1e-6, state within 3e-2 of its scale, refreshes within 5e-4, loss sums within 1e-4.
  Input condition, asserted on the PyTorch learner's own forward pass before every update: no ReLU of the unroll has a pre-activation
  within 1e-6 of zero.  The two learners sum in different orders, so their float32 pre-activations (64 to 512 terms of about 0.1, up to
  13 layers deep: a few 1e-7) may differ in sign that close to zero, and at batch 16 with a residual-sized gradient ONE (sample, position)
  of a flipped unit is several per cent of its row of the head's fc1 gradient (batch seed 11 had a value-head pre-activation of -6e-8 in
  the third update, one float32 step at that layer's scale: that unit on or off moves its row of exp_avg by 0.048 of the matrix's
  scale, computed on the host, which is the whole difference the two learners then showed), a property of the batch, not of either learner.  The batch seed is
  chosen so that the condition holds for all four runs."""
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  L = {}
  for name, extra in (('native', []), ('torch', ['--no_native_learner'])):
    cfg = make_config(['--environment', 'LunarLander-v2', '--seed', '1', '--batch_size', '16', '--no_support', '--use_gpu_for', 'actors', 'learner',
                       '--runs_dir', str(tmp_path / name), '--run_tag', 'x', '--no_tune_gemms'] + flags + extra)
    cfg.obs_space, cfg.action_space = (8,), 4
    sink = Sink()
    L[name] = (Learner(cfg, sink, sink), sink, cfg)
  a, b = L['native'][0], L['torch'][0]
  kind = a.config.optimizer
  grp = b.optimizer.param_groups[0]
  if kind == 'AdamW':
    keys = ['exp_avg', 'exp_avg_sq']
  else:
    keys = (['momentum_buffer'] if float(grp['momentum']) else []) + (['square_avg'] if kind == 'RMSprop' else [])
  rng = np.random.default_rng(95)
  for step in range(3):
    h = _random_batch(rng, 16, 5, 8, 4, lo=-18.0, hi=18.0)
    batch = ((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(16)), h['w'])
    margins = []
    with torch.no_grad():
      scalar_forward(b.network, torch.from_numpy(h['obs']).to(b.device), torch.from_numpy(h['act']).to(b.device), margins=margins)
    assert min(margins) >= 1e-6, (step, min(margins))
    before = [p.detach().clone() for p in b.network.parameters()]
    for ln in (a, b):
      ln.update_weights(batch)
      ln.training_step += 1
    assert a._native is not None and b._native is None
    lr = float(b.optimizer.param_groups[0]['lr'])
    assert abs(float(a.optimizer.param_groups[0]['lr']) - lr) <= 1e-6 * lr
    moved = max((pb.detach() - q).abs().max().item() for pb, q in zip(b.network.parameters(), before))
    dws = []
    for (k, pa), pb in zip(a.network.named_parameters(), b.network.parameters()):
      sa, sb = a.optimizer.state.get(pa, {}), b.optimizer.state.get(pb, {})
      assert set(sa) == set(sb), (k, set(sa), set(sb))
      if 'step' in sb:
        assert float(sa['step']) == float(sb['step']) == step + 1
      d = (pa - pb).abs().reshape(-1)
      dws.append(d)
      assert d.max().item() <= (2.5 * lr if kind == 'AdamW' else 2.5 * moved + 1e-6), (step, k, d.max().item(), moved)
      for key in keys:
        dm = (sa[key] - sb[key]).abs().max().item() / (sb[key].abs().max().item() + 1e-30)
        assert dm <= 3e-2, (step, k, key, dm)
    frac = (torch.cat(dws) > 1e-6).float().mean().item()
    assert frac <= 0.02, (step, frac)
    ea, eb = L['native'][1].updates[-1][1], L['torch'][1].updates[-1][1]
    assert np.abs(ea - eb).max() <= 5e-4
    la, lb = dict(a.losses_to_log), dict(b.losses_to_log)
    assert all(abs(la[k] - lb[k]) <= 1e-4 * max(1.0, abs(lb[k])) for k in lb), (la, lb)
    with torch.no_grad():                       # lock-step: the PyTorch learner's state into the native learner's flat vectors
      for pa, pb in zip(a.network.parameters(), b.network.parameters()):
        pa.copy_(pb)
        for key in keys:
          a.optimizer.state[pa][key].copy_(b.optimizer.state[pb][key])
  assert lb['value'] > 0 and lb['reward'] > 0
  a._native.close()


# ------------------------------------------------------------------------------------------------ the native loop
@pytest.mark.gpu
def test_native_loop_with_no_support_equals_the_per_update_path(tmp_path):
  """Learner.learn through mz_fcl_run (the loop body in native code) with --no_support against the per-update path driven from Python
  in the same order on twin replays: the same weights, moments and priorities bit for bit after 21 updates"""
  import random
  from collections import deque
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine, flatten_weights
  from model_based_rl_amd.learners import Learner
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = make_config(['--environment', 'LunarLander-v2', '--seed', '2', '--batch_size', '64', '--num_envs', '256', '--num_simulations', '8', '--no_support',
                     '--window_size', '16384', '--stored_before_train', '1000', '--use_gpu_for', 'actors', 'learner', '--send_weights_frequency', '16',
                     '--learner_log_frequency', '10', '--save_state_frequency', '1000000', '--beta', '0.6', '--runs_dir', str(tmp_path), '--run_tag', 'x'])
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

  n = 21
  a, ra = world()
  slots = a._native.lib.mz_fcl_slots(a._native.h)
  owed = deque()
  assert a._scheduled_lrs(n) is None
  for i in range(n):
    if len(owed) == slots:
      ix, slot = owed.popleft()
      ra.update(ix, a._native.errors(slot))
    host, ix = a._host_batch(ra.sample_batch_arrays())
    owed.append((ix, a._native.launch(host)))
  while owed:
    ix, slot = owed.popleft()
    ra.update(ix, a._native.errors(slot))
  c, rc = world()
  c.learn(max_steps=n)
  assert c.training_step == 1 + n and c.native_loop_updates == n > 0
  for name, t_a, t_c in (('weights', a._native.flat, c._native.flat), ('exp_avg', a._native.m, c._native.m), ('exp_avg_sq', a._native.v, c._native.v),
                         ('steps', a._native.steps, c._native.steps)):
    assert torch.equal(t_a, t_c), (name, (t_a - t_c).abs().max().item())
  assert np.array_equal(ra.tree.leaves(), rc.tree.leaves())
  assert np.isfinite(a._native.flat.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ C ABI, hand-over to the actor
@pytest.mark.gpu
def test_set_scalar_loss_refusals_and_the_two_one_output_modes(tmp_path):
  """mz_fcl_set_scalar_loss refuses a null handle, an unknown kind and a scalar kind on a handle with 31-bin supports, naming the
  problem.  On a handle with one output per head (supports (3, 3) and (0, 0)) the categorical reading (kind 0: one bin, whose softmax is
  1 and whose gradient is zero) and the scalar one (kind 1) are different modes: same weights, same batch, other value-head gradients."""
  from model_based_rl_amd import _abi
  from model_based_rl_amd.engine import WEIGHT_ORDER
  from model_based_rl_amd.learners import _NativeFC, _GraphedUpdate
  lib = _abi.load()
  assert lib.mz_fcl_set_scalar_loss(C.c_void_p(), 1) != 0
  with pytest.raises(Exception, match='null'):
    _abi.check(lib.mz_fcl_set_scalar_loss(C.c_void_p(), 1), 'mz_fcl_set_scalar_loss')
  learner = _scalar_learner(tmp_path, 'LunarLander-v2', 8, 4, 16, 5, [], ['actors', 'learner'], 'a')
  host = _random_batch(np.random.default_rng(3), 16, 5, 8, 4, lo=-18.0, hi=18.0)
  nat = _NativeFC(learner, host)
  for kind in (3, -1):
    assert lib.mz_fcl_set_scalar_loss(nat.h, kind) != 0
    with pytest.raises(Exception, match='kind'):
      _abi.check(lib.mz_fcl_set_scalar_loss(nat.h, kind), 'mz_fcl_set_scalar_loss')
  wide = C.c_void_p()
  with torch.cuda.device(learner.device):
    _abi.check(lib.mz_fcl_create(16, 5, 8, 4, -15, 15, -15, 15, 0, C.byref(wide)), 'mz_fcl_create')
  for kind in (1, 2):
    assert lib.mz_fcl_set_scalar_loss(wide, kind) != 0
    with pytest.raises(Exception, match='one output per head'):
      _abi.check(lib.mz_fcl_set_scalar_loss(wide, kind), 'mz_fcl_set_scalar_loss')
  assert lib.mz_fcl_set_scalar_loss(wide, 0) == 0
  lib.mz_fcl_destroy(wide)
  # one output per head: value support (3, 3), reward support (0, 0), on the native learner's own flat vectors
  one = C.c_void_p()
  with torch.cuda.device(learner.device):
    _abi.check(lib.mz_fcl_create(16, 5, 8, 4, 3, 3, 0, 0, 0, C.byref(one)), 'mz_fcl_create')
  assert lib.mz_fcl_num_params(one) == nat.flat.numel()
  ptr = lambda t: C.c_void_p(t.data_ptr())
  stream = C.c_void_p(torch.cuda.current_stream(learner.device).cuda_stream)
  _abi.check(lib.mz_fcl_bind(one, ptr(nat.flat), ptr(nat.m), ptr(nat.v), ptr(nat.steps), len(nat.params), ptr(nat.lr), stream), 'mz_fcl_bind')
  obs, act, t_rew, t_val, t_pol, w = [torch.from_numpy(host[k]).to(learner.device) for k in _GraphedUpdate.ORDER]
  errs, loss = torch.empty(16, dtype=torch.float32, device=learner.device), torch.zeros(3, dtype=torch.float64, device=learner.device)
  grads = {}
  for kind in (0, 1):
    _abi.check(lib.mz_fcl_set_scalar_loss(one, kind), 'mz_fcl_set_scalar_loss')
    _abi.check(lib.mz_fcl_step(one, ptr(obs), ptr(act), 0, ptr(t_rew), ptr(t_val), ptr(t_pol), ptr(w), 1, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, 1,
                               ptr(errs), ptr(loss), stream), 'mz_fcl_step')
    out = np.empty(nat.flat.numel(), np.float32)
    _abi.check(lib.mz_fcl_read_grad(one, out.ctypes.data_as(C.c_void_p), out.size), 'mz_fcl_read_grad')
    off = 0
    for k, p in zip(WEIGHT_ORDER, nat.params):
      grads[(kind, k)] = out[off:off + p.numel()].copy()
      off += p.numel()
  for k in ('value_head.value.weight', 'value_head.value.bias', 'value_head.fc1.weight'):
    assert not grads[(0, k)].any(), k                       # one bin: the softmax is 1, the target is 1
    assert grads[(1, k)].any() and np.isfinite(grads[(1, k)]).all(), k
  assert np.array_equal(grads[(0, 'policy_head.policy.weight')], grads[(1, 'policy_head.policy.weight')])      # (the policy head: categorical in both)
  lib.mz_fcl_destroy(one)
  nat.close()


@pytest.mark.gpu
def test_native_no_support_weights_reach_the_actor(tmp_path):
  """after native --no_support updates Learner._host_weights() (one copy of the flat vector) has the state_dict's keys, shapes and
  values, and an Engine built with no_support takes them"""
  from model_based_rl_amd.engine import Engine
  learner = _scalar_learner(tmp_path, 'LunarLander-v2', 8, 4, 16, 5, [], ['actors', 'learner'], 'a')
  rng = np.random.default_rng(4)
  for _ in range(2):
    h = _random_batch(rng, 16, 5, 8, 4, lo=-18.0, hi=18.0)
    learner.update_weights(((h['obs'], h['act'], (h['t_rew'], h['t_val'], h['t_pol'])), list(range(16)), h['w']))
  assert learner._native is not None
  hw, sd = learner._host_weights(), learner.network.state_dict()
  assert list(hw) == list(sd)
  for k, v in sd.items():
    assert tuple(hw[k].shape) == tuple(v.shape) and torch.equal(hw[k], v.cpu()), k
  assert tuple(hw['value_head.value.weight'].shape) == (1, 512) and tuple(hw['reward_head.reward.bias'].shape) == (1,)
  eng = Engine(16, 8, 4, 8, device='cuda:0', no_support=True)
  eng.set_weights(hw)
  eng.close()
  learner._native.close()
