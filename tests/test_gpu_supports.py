"""Every device kernel that computes an FCNetwork output, at value / reward supports other than (-15, 15) for both heads,
against the float64 network of tests/fc64.py.

The support-to-scalar step exists three times on the device (mz_support_to_scalar in mz_net.hip.h: k_net_recurrent_rows,
k_net_recurrent_tree, k_eval_rows; mz_support_to_scalar16 in k_root; mz_support_to_scalar_q in k_search_fused and
k_search_h2, whose bins past the support size are MZ_PAD_BIN padding), and the host packs the two output layers at their own
sizes.  The shapes below have Sv != Sr in both orientations, 32 bins (no padding bin), 16 / 17 bins at the 16-row tile
edge, a one-bin support at smin = 3 and a non-negative support, each with and without the target transform.

Bounds (the float64 network is the truth):
  hidden state, policy logits            |d| <= 1e-5 (tests/test_oracle_net.py TOL; split-f16 included)
  value, reward, --no_target_transform   |d| <= 1e-5 max(1, M / 15), M = max(|smin|, |smax|): the 1e-5 bar at 31 bins scaled
                                         with the magnitude of the support values the expectation sums
  value, reward with the transform       |d| <= 2e-4 (1 + |v|) on every row: one float32 step of the reference's own
                                         formula (tests/test_oracle_net.py:test_inverse_transform_large_values)
The weight set whose support-head biases are moved by -200 has its logits near -200, where a float32 ulp is 2^-16 and every
float32 evaluation rounds each logit (the final bias add alone by half an ulp): a logit error e_i moves the expectation by
sum_i p_i e_i (s_i - x), at most max |e| sum_i p_i |s_i - x| (fc64.support_spread).  Without the transform its bound adds two
ulps, 2^-15, times that spread of the float64 softmax (measured before: up to 6e-5 against the 1e-5 bar at 31 bins); the
transform's bound covers it as it is.
"""
import types

import numpy as np
import pytest

from tests.fc64 import FC64, scalar_bound
from tests.parity_util import env_switches
from tests.test_oracle_net import TOL

pytestmark = pytest.mark.gpu
O = 12

SHAPES = {
    # name: (value support, reward support, action_space)
    'v31_r31_control': ((-15, 15), (-15, 15), 4),
    'v15_r5': ((-7, 7), (-2, 2), 2),            # Sv != Sr, the policy path of A <= 4
    'v5_r15': ((-2, 2), (-7, 7), 6),            # the same sizes swapped
    'v32_r32pos': ((-16, 15), (0, 31), 9),      # 32 bins: no padding bin; a non-negative support (values up to ~1000)
    'v1at3_r3': ((3, 3), (-1, 1), 18),          # one bin at smin = 3 (not --no_support); two policy tiles
    'v16_r17': ((-20, -5), (-8, 8), 13),        # 16 / 17 bins at the 16-row tile edge; the widest split-f16 action space
}
NT = [False, True]
NT_IDS = ['transform', 'no_target_transform']


def weights(vs, rs, A, nt, seed=7, shift=0.0, scale_heads=3.0):
  """a PyTorch-initialised FCNetwork of these supports, output heads times 3 (the values leave the near-zero regime);
  shift: added to every real bin's bias of both support heads (softmax does not see it)"""
  import torch
  from model_based_rl_amd.networks import FCNetwork
  cfg = types.SimpleNamespace(value_support=vs, reward_support=rs, no_support=False, no_target_transform=nt)
  torch.manual_seed(seed)
  w = {k: v.numpy().copy() for k, v in FCNetwork(O, A, torch.device('cpu'), cfg).state_dict().items()}
  for k in ('value_head.value', 'reward_head.reward'):
    w[k + '.weight'] = (w[k + '.weight'] * scale_heads).astype(np.float32)
    w[k + '.bias'] = (w[k + '.bias'] + np.float32(shift)).astype(np.float32)
  return w


def engine(B, vs, rs, A, nt, sims=24, seed=3, switches=None, split=False):
  from model_based_rl_amd.engine import Engine
  with env_switches(**(switches or {})):
    return Engine(B, O, A, sims, value_support=vs, reward_support=rs, no_target_transform=nt, seed=seed, split_f16=split)


class Errors(object):
  """worst |d| and worst |d| / bound per quantity; asserts every bound"""

  def __init__(self, tag, vs, rs, nt, shifted=False):
    self.tag, self.vs, self.rs, self.nt, self.worst = tag, vs, rs, nt, {}
    self.logit_eps = 2.0 ** -15 if shifted else 0.0      # (module docstring: the -200 bias set)

  def _put(self, what, d, ratio):
    old = self.worst.get(what, (0.0, 0.0))
    self.worst[what] = (max(old[0], float(np.max(d, initial=0.0))), max(old[1], float(np.max(ratio, initial=0.0))))

  def exact(self, what, got, want):
    d = np.abs(np.asarray(got, np.float64) - want)
    self._put(what, d, d / TOL)
    assert d.max() <= TOL, (self.tag, what, d.max())

  def scalar(self, what, got, want, support, spread=None):
    d = np.abs(np.asarray(got, np.float64).reshape(-1) - want.reshape(-1))
    bound = scalar_bound(want.reshape(-1), support, not self.nt)
    if self.nt and self.logit_eps:
      bound = bound + self.logit_eps * np.asarray(spread).reshape(-1)
    self._put(what, d, d / bound)
    assert np.all(np.isfinite(got)) and np.all(d <= bound), (self.tag, what, d.max(), int(np.argmax(d / bound)))

  def report(self):
    print('%-44s ' % self.tag + '  '.join('%s %.2e (%.2f of bound)' % (k, v[0], v[1]) for k, v in sorted(self.worst.items())))


def spread_check(v, support):
  """the float64 values of a head with more than one bin are spread over its support, not stuck near zero"""
  S = support[1] - support[0] + 1
  if S > 1:
    assert np.ptp(v) > 0.02 * (S - 1) and np.abs(v).max() > 0.05, (support, np.ptp(v))


@pytest.mark.parametrize('shift', [0.0, -200.0], ids=['bias', 'bias_minus_200'])
@pytest.mark.parametrize('nt', NT, ids=NT_IDS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_inference_kernels_vs_float64(shape, nt, shift):
  """k_root (mz_initial_inference), k_net_recurrent_rows (mz_recurrent_inference) and k_eval_rows (mz_eval_lookahead
  --only_value: bit-identical to the recurrent rows, mz_eval.hip.h) on ragged batches.  bias_minus_200: the same network with
  both support heads' biases moved by -200 on every real bin; the float64 values do not move, and a kernel that dropped the
  max subtraction, or let a padding bin into the maximum, would be far off."""
  vs, rs, A = SHAPES[shape]
  B = 203
  rng = np.random.RandomState(11)
  w = weights(vs, rs, A, nt, shift=shift)
  ref = FC64(w, O, A, vs, rs, nt)
  if shift:
    base = FC64(weights(vs, rs, A, nt), O, A, vs, rs, nt)
    obs0 = rng.standard_normal((8, O))
    _, r1, v1, _ = ref.recurrent(ref.initial(obs0)[0], np.arange(8) % A)
    _, r0, v0, _ = base.recurrent(base.initial(obs0)[0], np.arange(8) % A)
    assert np.all(np.abs(v1 - v0) <= 1e-3 * (1 + np.abs(v0))) and np.all(np.abs(r1 - r0) <= 1e-3 * (1 + np.abs(r0)))
  err = Errors('%s %s %s' % (shape, NT_IDS[nt], 'shift-200' if shift else 'inference'), vs, rs, nt, bool(shift))
  eng = engine(B, vs, rs, A, nt, sims=4)
  eng.set_weights(w)
  obs = (rng.standard_normal((B, O)) * 2).astype(np.float32)
  eng.initial_inference(obs)
  v, lg, h = [x.cpu().numpy() for x in eng.root_outputs()]
  ho, vo, lgo = ref.initial(obs)
  err.exact('root hidden', h, ho)
  err.exact('root logits', lg, lgo)
  err.scalar('root value', v, vo, vs, ref.value_spread(ho))
  act = rng.randint(0, A, B).astype(np.int32)
  h2, r2, v2, lg2 = [x.cpu().numpy() for x in eng.recurrent_inference(h, act)]
  h2o, r2o, v2o, lg2o = ref.recurrent(h, act)
  err.exact('rec hidden', h2, h2o)
  err.exact('rec logits', lg2, lg2o)
  err.scalar('rec value', v2, v2o, vs, ref.value_spread(h2o))
  err.scalar('rec reward', r2, r2o, rs, ref.reward_spread(h, act))
  if nt:
    spread_check(v2o, vs)
    spread_check(r2o, rs)
  # the evaluation lookahead's rows: every (root, action) pair
  eng.root_prepare(None, None, None, device_rng=True, move=0)
  out = {k: x.cpu().numpy() for k, x in eng.eval_lookahead('only_value', rows=True).items()}
  hr, ar = np.repeat(h, A, 0), np.tile(np.arange(A, dtype=np.int32), B)
  _, rr, vr, _ = [x.cpu().numpy() for x in eng.recurrent_inference(hr, ar)]
  assert np.array_equal(out['row_reward'].reshape(-1).view(np.uint32), rr.view(np.uint32))
  assert np.array_equal(out['row_value'].reshape(-1).view(np.uint32), vr.view(np.uint32))
  hro, rro, vro, _ = ref.recurrent(hr, ar)
  err.scalar('lookahead value', out['row_value'], vro, vs, ref.value_spread(hro))
  err.scalar('lookahead reward', out['row_reward'], rro, rs, ref.reward_spread(hr, ar))
  err.report()
  eng.close()


def slots_of(t, A, sims):
  """per tree and slot s = 1..sims (the node expanded by simulation s): its parent's slot and the action that led to it"""
  E = t['E']
  B = E.shape[0]
  assert np.all((E > 0).sum(1) == sims)
  node = np.zeros((B, sims + 1), np.int64)
  bs, ks = np.nonzero(E > 0)
  node[bs, E[bs, ks]] = ks
  assert np.all(node[:, 1:] >= 1)
  return node[:, 1:], (node[:, 1:] - 1) // A, (node[:, 1:] - 1) % A


def check_simulations(err, ref, t, io, A, sims, vs, rs):
  """every simulation of every tree: the reward and the new hidden state against float64 recurrent(hidden[parent], a) on
  the device's own parent state, the value and logits (io: the sim_io log of the move, or None) against float64
  prediction(hidden[s])"""
  B = t['E'].shape[0]
  node, parent, act = slots_of(t, A, sims)
  hid = t['hidden'].astype(np.float64)
  hp = hid[np.arange(B)[:, None], parent].reshape(-1, hid.shape[2])
  hn, r = ref.dynamics(hp, act.reshape(-1))
  err.exact('sim hidden', hid[:, 1:].reshape(-1, hid.shape[2]), hn)
  rspread = ref.reward_spread(hp, act.reshape(-1))
  err.scalar('tree reward', t['R'][np.arange(B)[:, None], node], r, rs, rspread)
  if io is not None:
    v, lg = ref.prediction(hid[:, 1:].reshape(-1, hid.shape[2]))
    err.scalar('sim reward', io[:, 1:, 1], r, rs, rspread)
    err.scalar('sim value', io[:, 1:, 0], v, vs, ref.value_spread(hid[:, 1:].reshape(-1, hid.shape[2])))
    err.exact('sim logits', io[:, 1:, 2:].reshape(-1, A), lg)


VARIANTS = {
    # name: (switches at mz_create, split_f16, kernel kind, LDS placement (None: by fit), bias shift)
    'lds': ({}, False, 'fused', None, 0.0),
    'lds_shift': ({}, False, 'fused', None, -200.0),
    'pool': ({'MZ_NO_LDS_TREES': '1'}, False, 'fused', 0, 0.0),
    'split_f16': ({}, True, 'split_f16', None, 0.0),
    'standalone': ({'MZ_NO_FUSED': '1'}, False, 'standalone', None, 0.0),
}


@pytest.mark.parametrize('nt', NT, ids=NT_IDS)
@pytest.mark.parametrize('shape,variant', [(s, v) for s in sorted(SHAPES) for v in VARIANTS
                                           if not (VARIANTS[v][1] and SHAPES[s][2] > 13)])      # (k_search_h2: A <= 13)
def test_search_every_simulation_vs_float64(shape, nt, variant):
  """mz_search with 24 simulations: the network outputs of every simulation of every tree, logged by the fused kernels
  (sim_io) and read from the exported tree -- no tie margin is involved, the tree the device built is the input.  The
  stand-alone kernels (MZ_NO_FUSED) do not log: their rewards and hidden states come from the tree, and the value from
  the child's value sum after a one-simulation search."""
  vs, rs, A = SHAPES[shape]
  sw, split, kind, lt, shift = VARIANTS[variant]
  B, sims = 157, 24
  rng = np.random.RandomState(5)
  w = weights(vs, rs, A, nt, seed=9, shift=shift)
  ref = FC64(w, O, A, vs, rs, nt)
  err = Errors('%s %s %s' % (shape, NT_IDS[nt], variant), vs, rs, nt, bool(shift))
  eng = engine(B, vs, rs, A, nt, sims=sims, switches=sw, split=split)
  eng.set_weights(w)
  info = eng.search_kernel_info()
  assert info['kind'] == kind, info
  if lt is not None:
    assert info['lt'] == lt, info
  obs = (rng.standard_normal((B, O)) * 2).astype(np.float32)
  noise = rng.dirichlet([0.25] * A, size=B)
  log = eng.sim_io('log', keep_moves=1) if kind != 'standalone' else None
  eng.initial_inference(obs)
  eng.root_prepare(None, None, noise)
  eng.search()
  t = eng.export_tree(hidden=True)
  err.exact('root hidden', t['hidden'][:, 0], ref.initial(obs)[0])
  check_simulations(err, ref, t, None if log is None else log[0].cpu().numpy(), A, sims, vs, rs)
  if log is None:
    eng.initial_inference(obs)
    eng.root_prepare(None, None, noise)
    eng.search(1)
    t1 = eng.export_tree(hidden=True)
    child = np.argmax(t1['N'][:, 1:1 + A], 1)
    assert np.all(t1['N'][:, 1:1 + A].sum(1) == 1)
    h1, r1, v1, _ = ref.recurrent(t1['hidden'][:, 0], child)
    err.scalar('sim value', t1['W'][np.arange(B), 1 + child], v1, vs, ref.value_spread(h1))
    err.scalar('sim reward', t1['R'][np.arange(B), 1 + child], r1, rs, ref.reward_spread(t1['hidden'][:, 0], child))
  else:
    eng.sim_io('off')
  err.report()
  eng.close()


@pytest.mark.parametrize('nt', NT, ids=NT_IDS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_selfplay_launch_vs_float64(shape, nt):
  """whole moves inside one launch (mz_selfplay_steps): the root of every tree of every move against float64 initial
  inference on the move's recorded observation, and every simulation of the last move"""
  import torch
  from model_based_rl_amd.engine import records_view
  vs, rs, A = SHAPES[shape]
  B, sims, T, moves = 101, 24, 5, 6
  w = weights(vs, rs, A, nt, seed=13)
  ref = FC64(w, O, A, vs, rs, nt)
  err = Errors('%s %s selfplay' % (shape, NT_IDS[nt]), vs, rs, nt)
  eng = engine(B, vs, rs, A, nt, sims=sims, seed=21)
  eng.set_weights(w)
  assert eng.search_kernel_info()['kind'] == 'fused' and eng.selfplay_moves_per_launch() == 16
  eng.selfplay_reset(T, 1.0)
  log = eng.sim_io('log', keep_moves=moves)
  eng.selfplay_export_trees(True)
  eng.selfplay_steps(moves)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == moves
  rv = records_view(buf[:n].numpy().copy(), O, A)
  io = log.cpu().numpy()
  for m in range(moves):
    obs = rv['obs'][m]
    assert np.array_equal(obs[B - 1], eng.synth_obs(B - 1, int(rv['episode'][m, B - 1]), int(rv['step'][m, B - 1]))[0])
    ho, vo, lgo = ref.initial(obs)
    err.scalar('root value', io[m, :, 0, 0], vo, vs, ref.value_spread(ho))
    err.exact('root logits', io[m, :, 0, 2:], lgo)
  check_simulations(err, ref, eng.export_tree(hidden=True), io[moves - 1], A, sims, vs, rs)
  eng.sim_io('off')
  err.report()
  eng.close()


@pytest.mark.parametrize('vs,rs', [((-7, 7), (-2, 2)), ((-2, 2), (-7, 7))], ids=['Sv15_Sr5', 'Sv5_Sr15'])
def test_relu_scale_decision_with_unequal_heads(vs, rs):
  """The clamp-ReLU scale decision when Sv != Sr: the largest consuming-layer weight planted in the last real row of the
  larger output head, then of the smaller one, once above the limit both sides apply (k_relu_scale refuses from
  w2max >= 2^(100-k)) and once well inside it.  The device's own decision (set_weights(sync=True): weight_scale(),
  search_kernel_info()) equals the host's (Engine.weights_scale_ok); the asynchronous pull, which hands the host's
  decision to the device, searches without a NaN.
  'Well inside' is 2^(24-k): the activations the weight multiplies stay below 2^k, so the logit it adds stays below 2^24.
  Admitted weights up to 2^(97-k) can put a support logit more than ~1.5e9 below the row's maximum, where the fused
  kernels' written-out expf (mz_support_to_scalar_q) returns NaN (the stand-alone kernels do not); planted at 2^(60-k) ..
  2^(90-k) in the reward head this test saw NaN rewards.  A per-bin cap of exp2's argument removes it but costs the
  headline kernel 16 bytes of scratch (test_abi.py:test_headline_kernel_keeps_its_register_budget), so it is not in."""
  import torch
  from model_based_rl_amd.engine import flatten_weights
  from tests.test_abi import host_scale_exponent
  A, B, sims = 6, 64, 8
  sd = weights(vs, rs, A, False, seed=1, scale_heads=1.0)
  k = host_scale_exponent(sd, A)
  sv, sr = vs[1] - vs[0] + 1, rs[1] - rs[0] + 1
  heads = sorted([('value_head.value.weight', sv), ('reward_head.reward.weight', sr)], key=lambda h: -h[1])
  rng = np.random.RandomState(2)
  obs = (rng.standard_normal((B, O)) * 2).astype(np.float32)
  noise = rng.dirichlet([0.25] * A, size=B)
  eng = engine(B, vs, rs, A, False, sims=sims)
  for key, rows in heads:
    for val, want in ((2.0 ** (102 - k), 0), (2.0 ** (24 - k), 1)):
      g = {n: v.copy() for n, v in sd.items()}
      g[key][rows - 1, 511] = -val
      host = eng.weights_scale_ok(flatten_weights(g))
      assert host == want, (key, val)
      eng.set_weights(g, sync=True)
      scale = eng.weight_scale()
      assert scale[3] == host and eng.search_kernel_info()['kind'] == ('fused' if host else 'standalone'), (key, val, scale)
      eng.set_weights(g)
      assert eng.search_kernel_info()['kind'] == ('fused' if host else 'standalone')
      eng.initial_inference(obs)
      eng.root_prepare(None, None, noise)
      eng.search()
      out = {n: x.cpu().numpy() for n, x in eng.finalize(1.0, rng.uniform(size=B)).items()}
      torch.cuda.synchronize()
      t = eng.export_tree()
      assert np.all(np.isfinite(out['root_value'])) and np.all(np.isfinite(t['W'])) and np.all(np.isfinite(t['R'])), (key, val)
  eng.close()


def test_set_weights_checks_every_tensor_shape():
  """a state_dict of swapped supports -- the same total count -- is refused by name; the engine's own is accepted; a flat
  vector keeps the count check"""
  from model_based_rl_amd.engine import flatten_weights
  vs, rs, A = SHAPES['v15_r5']
  eng = engine(16, vs, rs, A, False, sims=4)
  good, swapped = weights(vs, rs, A, False), weights(rs, vs, A, False)
  assert flatten_weights(good).numel() == flatten_weights(swapped).numel() == eng.num_weights
  with pytest.raises(ValueError, match='value_head.value.weight'):
    eng.set_weights(swapped)
  eng.set_weights(good)
  eng.set_weights(flatten_weights(good))
  with pytest.raises(ValueError, match='expected'):
    eng.set_weights(flatten_weights(good)[:-1])
  eng.close()


class _Sink(object):
  def update(self, idxs, errors): pass
  def store_weights(self, w, step): pass
  def get_stats(self, key=None): return {0: 3}
  def add_initial_throughput(self, f, g): pass
  def get_throughput(self): return {'frames': 0, 'games': 0}


def _learner(tmp_path, *flags):
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.learners import Learner
  cfg = make_config(['--environment', 'LunarLander-v2', '--seed', '3', '--num_simulations', '8', '--runs_dir', str(tmp_path),
                     '--run_tag', 'sup'] + list(flags))
  return cfg, Learner(cfg, _Sink(), _Sink())


def test_config_supports_reach_the_engine(tmp_path):
  """--value_support -7 7 --reward_support -2 2 through a Learner's network and Engine.from_config: the engine's outputs
  equal the learner network's eval-mode forward (in float64) within the bounds above"""
  import copy
  import torch
  from model_based_rl_amd.engine import Engine
  cfg, learner = _learner(tmp_path, '--value_support', '-7', '7', '--reward_support', '-2', '2')
  assert learner.device.type == 'cpu'
  net = learner.network
  with torch.no_grad():
    net.value_head.value.weight.mul_(3.0)
    net.reward_head.reward.weight.mul_(3.0)
  net64 = copy.deepcopy(net).double().eval()
  O_, A, B = int(np.prod(cfg.obs_space)), int(cfg.action_space), 93
  eng = Engine.from_config(cfg, B)
  eng.set_weights(net.state_dict())
  rng = np.random.RandomState(4)
  obs = (rng.standard_normal((B, O_)) * 2).astype(np.float32)
  act = rng.randint(0, A, B)
  eng.initial_inference(obs)
  v, lg, h = [x.cpu().numpy() for x in eng.root_outputs()]
  h2, r2, v2, lg2 = [x.cpu().numpy() for x in eng.recurrent_inference(h, act.astype(np.int32))]
  with torch.no_grad():
    o0 = net64.initial_inference(torch.from_numpy(obs).double())
    o1 = net64.recurrent_inference(torch.from_numpy(h).double(), act)
  err = Errors('config -7..7 / -2..2', (-7, 7), (-2, 2), False)
  err.exact('root hidden', h, o0.hidden_state.numpy())
  err.exact('root logits', lg, o0.policy_logits.numpy())
  err.scalar('root value', v, o0.value.numpy(), (-7, 7))
  err.exact('rec hidden', h2, o1.hidden_state.numpy())
  err.exact('rec logits', lg2, o1.policy_logits.numpy())
  err.scalar('rec value', v2, o1.value.numpy(), (-7, 7))
  err.scalar('rec reward', r2, o1.reward.numpy(), (-2, 2))
  err.report()
  eng.close()


def test_config_with_33_bins_is_refused_by_the_engine(tmp_path):
  """the learner takes a 33-bin support; mz_create refuses it and names its limit of 32"""
  from model_based_rl_amd.engine import Engine
  cfg, learner = _learner(tmp_path, '--value_support', '-16', '16')
  assert learner.network.value_head.value.weight.shape[0] == 33
  with pytest.raises(RuntimeError, match=r'support size must be in \[1,32\] \(value 33, reward 31\)'):
    Engine.from_config(cfg, 16)
