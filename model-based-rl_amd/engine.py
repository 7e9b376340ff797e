"""Batched device engine: B search trees in lock-step on one MI355X, through the C ABI.

torch is used for device memory and streams only; every computation below is a HIP kernel in
csrc/ reached through libmz_hip.so.  Mirrors, batched over B environments, what one reference Actor
does per move (actors.py:131-153): initial inference, root expand + noise, MCTS.run, select_action."""
import ctypes as C
import os

import numpy as np
import torch

from . import _abi
from .envs import BOARD_KINDS, KIND_OF_ENV, SELFPLAY_KINDS

H = 50

WEIGHT_ORDER = [
    'representation_head.fc1.weight', 'representation_head.fc1.bias',
    'representation_head.out.weight', 'representation_head.out.bias',
    'value_head.fc1.weight', 'value_head.fc1.bias', 'value_head.value.weight', 'value_head.value.bias',
    'policy_head.fc1.weight', 'policy_head.fc1.bias', 'policy_head.policy.weight', 'policy_head.policy.bias',
    'reward_head.fc1.weight', 'reward_head.fc1.bias', 'reward_head.reward.weight', 'reward_head.reward.bias',
    'transition_head.fc1.weight', 'transition_head.fc1.bias', 'transition_head.out.weight', 'transition_head.out.bias',
    'LN.weight', 'LN.bias',
]


def flatten_weights(weights):
  """state_dict (reference key names, networks.py:137-144) -> one float32 vector in ABI order.
  Copied with numpy: torch.cat parallelises over its intra-op pool once a tensor passes 32 K elements (the 128 x 512 first
  layer of the -ram- shapes), and the pool's threads spin after every call -- 7 of 16 host cores busy at a pull every 0.1 s."""
  parts = []
  for k in WEIGHT_ORDER:
    v = weights[k]
    parts.append(v.detach().to('cpu', torch.float32).numpy().reshape(-1) if torch.is_tensor(v)
                 else np.ascontiguousarray(v, np.float32).reshape(-1))
  out = np.empty(sum(p.size for p in parts), np.float32)
  pos = 0
  for p in parts:
    out[pos:pos + p.size] = p
    pos += p.size
  return torch.from_numpy(out)


def weight_shapes(obs_dim, action_space, value_outputs, reward_outputs):
  """{WEIGHT_ORDER key: shape} of an FCNetwork state_dict (networks.py:122-140) with these output sizes"""
  O, A, F = int(obs_dim), int(action_space), 512
  layers = {'representation_head.fc1': (F, O), 'representation_head.out': (H, F), 'value_head.fc1': (F, H),
            'value_head.value': (int(value_outputs), F), 'policy_head.fc1': (F, H), 'policy_head.policy': (A, F),
            'reward_head.fc1': (F, H + A), 'reward_head.reward': (int(reward_outputs), F), 'transition_head.fc1': (F, H + A),
            'transition_head.out': (H, F)}
  out = {}
  for k, s in layers.items():
    out[k + '.weight'], out[k + '.bias'] = s, s[:1]
  out['LN.weight'] = out['LN.bias'] = (H,)
  return out


def check_weight_shapes(weights, obs_dim, action_space, value_outputs, reward_outputs):
  """ValueError naming the first key of a state_dict that is missing or whose shape is not the one these sizes need: the
  flat vector's length alone cannot tell a (15, 5) support pair from (5, 15), nor (32, 30) from (31, 31)."""
  for k, want in weight_shapes(obs_dim, action_space, value_outputs, reward_outputs).items():
    if k not in weights:
      raise ValueError('weights: %s is missing' % k)
    got = tuple(weights[k].shape)
    if got != want:
      raise ValueError('weights: %s has shape %s, expected %s (obs_dim %d, action_space %d, value outputs %d, reward outputs %d)'
                       % (k, got, want, obs_dim, action_space, value_outputs, reward_outputs))


def weights_scale_ok(flat_host, obs_dim, action_space, value_outputs, reward_outputs):
  """mz_weights_scale_ok (include/mz_engine.h): does this weight set admit the search kernel's clamp-ReLU scale?  Host
  arithmetic on a host copy of the flat weights (engine.WEIGHT_ORDER); no GPU."""
  w = flat_host if torch.is_tensor(flat_host) else torch.from_numpy(np.ascontiguousarray(flat_host, np.float32))
  w = w.detach().to('cpu', torch.float32).contiguous().reshape(-1)
  rc = _abi.load().mz_weights_scale_ok(C.c_void_p(w.data_ptr()), w.numel(), int(obs_dim), int(action_space), int(value_outputs),
                                       int(reward_outputs))
  if rc < 0:
    _abi.check(rc, 'mz_weights_scale_ok')
  return int(rc)


def config_scale_check(config):
  """flat host weights -> mz_weights_scale_ok for a Config's FCNetwork shapes (None for the torch networks)"""
  if getattr(config, 'architecture', 'FCNetwork') != 'FCNetwork':
    return None
  O, A = int(np.prod(config.obs_space)), int(config.action_space)
  if getattr(config, 'no_support', False):
    sv = sr = 1
  else:
    sv = int(config.value_support[1]) - int(config.value_support[0]) + 1
    sr = int(config.reward_support[1]) - int(config.reward_support[0]) + 1
  return lambda flat: weights_scale_ok(flat, O, A, sv, sr)


from .record import REC_EXTRA, rec_floats, records_view  # noqa: E402,F401  (the record's layout: record.py; callers import these from here)


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def mz_config(num_envs, obs_dim, action_space, num_simulations, two_players=False, known_bounds=(None, None),
              value_support=(-15, 15), reward_support=(-15, 15), no_target_transform=False, no_support=False, discount=0.997,
              pb_c_base=19652, pb_c_init=1.25, init_value_score=0.0, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
              seed=0, env_id_offset=0, split_f16=False):
  """the mz_config (include/mz_engine.h) of an engine with these arguments (Engine.__init__'s); needs no GPU"""
  lo, hi = known_bounds
  return _abi.MzConfig(
      int(num_envs), int(obs_dim), int(action_space), int(num_simulations), int(bool(two_players)), int(lo is not None),
      int(hi is not None), int(value_support[0]), int(value_support[1]), int(reward_support[0]), int(reward_support[1]),
      int(bool(no_target_transform)), 0.0 if lo is None else float(lo), 0.0 if hi is None else float(hi),
      float(discount), float(pb_c_base), float(pb_c_init), float(init_value_score), float(root_dirichlet_alpha),
      float(root_exploration_fraction), int(seed), int(env_id_offset), int(bool(no_support)), int(bool(split_f16)))


_TM_EVAL = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))


def tm_search_host(cfg, kind, boards, turn, step, root_logits, eval_fn, num_simulations=None, noise=None):
  """mz_tm_search_host (include/mz_engine_debug.h): the true-rules search of n positions as sequential C++ on the host, no
  GPU.  cfg: an mz_config (mz_config(...) above; its num_simulations sizes the trees); kind 1 / 3; boards [n, 42], turn [n],
  step [n]; root_logits [n, A] float32; noise [n, A] float64 or None; eval_fn(obs [n, O] float32) -> (value [n], logits
  [n, A]) is called once per simulation on the leaves' observations.  Returns a dict of numpy arrays: the trees as
  export_tree's (N, W, P, R, E, TP [n, NN], legal [n], minmax [n, 2]), nexp [n], the side state per expansion slot as
  tm_export's (boards [n, sims + 1, 42], mover, step, mask, finished [n, sims + 1]), leaf_depth [n, sims] and EX [n, NN]."""
  lib = _abi.load()
  k = KIND_OF_ENV[kind] if isinstance(kind, str) else int(kind)
  bd = np.ascontiguousarray(boards, np.int8)
  tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
  n, A, O, S = bd.shape[0], cfg.action_space, cfg.obs_dim, cfg.num_simulations
  lg = np.ascontiguousarray(root_logits, np.float32)
  nz = None if noise is None else np.ascontiguousarray(noise, np.float64)
  if bd.shape != (n, 42) or tn.shape != (n,) or st.shape != (n,) or lg.shape != (n, A) or (nz is not None and nz.shape != (n, A)):
    raise ValueError('tm_search_host: boards [n, 42], turn [n], step [n], root_logits [n, A], noise [n, A]')
  sims = S if num_simulations is None else int(num_simulations)
  NN = 1 + (S + 1) * A
  d = dict(N=np.zeros((n, NN), np.int32), W=np.zeros((n, NN)), P=np.zeros((n, NN)), R=np.zeros((n, NN), np.float32),
           E=np.zeros((n, NN), np.int32), TP=np.zeros((n, NN), np.int8), legal=np.zeros(n, np.uint32), minmax=np.zeros((n, 2)),
           nexp=np.zeros(n, np.int32), boards=np.zeros((n, S + 1, 42), np.int8), mover=np.zeros((n, S + 1), np.int8),
           step=np.zeros((n, S + 1), np.int32), mask=np.zeros((n, S + 1), np.uint32), finished=np.zeros((n, S + 1), np.uint8),
           leaf_depth=np.zeros((n, S), np.int32))
  failure = []

  def cb(_ctx, obs, rows, value, logits):
    try:
      v, l = eval_fn(np.ctypeslib.as_array(obs, (rows, O)).copy())
      np.ctypeslib.as_array(value, (rows,))[:] = np.asarray(v, np.float32).reshape(rows)
      np.ctypeslib.as_array(logits, (rows, A))[:] = np.asarray(l, np.float32).reshape(rows, A)
    except Exception as ex:      # (an exception cannot cross the C frames)
      failure.append(ex)
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
  cb_c = _TM_EVAL(cb)      # (kept alive across the call)
  _abi.check(lib.mz_tm_search_host(C.byref(cfg), k, n, p(bd), p(tn), p(st), p(lg), p(nz), sims, C.cast(cb_c, C.c_void_p), None,
                                   *[p(d[key]) for key in ('N', 'W', 'P', 'R', 'E', 'TP', 'legal', 'minmax', 'nexp', 'boards', 'mover',
                                                           'step', 'mask', 'finished', 'leaf_depth')]), 'mz_tm_search_host')
  if failure:
    raise failure[0]
  d['EX'] = tm_exists(d['mask'], d['nexp'], A, NN)
  return d


def tm_exists(mask, nexp, A, NN):
  """EX [n, NN] of a true-rules tree: the root, and child a of every taken expansion slot whose mask has bit a"""
  n = mask.shape[0]
  EX = np.zeros((n, NN), np.uint8)
  EX[:, 0] = 1
  for b in range(n):
    for e in range(int(nexp[b])):
      for a in range(A):
        EX[b, 1 + e * A + a] = (int(mask[b, e]) >> a) & 1
  return EX


_GZ_EVAL = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_float),
                       C.POINTER(C.c_float), C.POINTER(C.c_float))


def gz_seq(m, n):
  """mz_gz_seq_host: seq(m, n), the visit count a root action must have to be considered at each of n simulations when
  sequential halving starts from m actions (mctx's get_sequence_of_considered_visits); needs no GPU"""
  out = np.zeros(int(n), np.int32)
  _abi.check(_abi.load().mz_gz_seq_host(int(m), int(n), out.ctypes.data_as(C.c_void_p)), 'mz_gz_seq_host')
  return out


def gz_search_host(cfg, root_value, root_logits, eval_fn, to_play=None, legal=None, gumbel=None, max_considered=16,
                   c_visit=50.0, c_scale=1.0, gumbel_scale=0.0, num_simulations=None):
  """mz_gz_search_host (include/mz_engine_debug.h): the Gumbel search of n roots as sequential C++ on the host, no GPU.  cfg:
  an mz_config (its num_simulations sizes the trees); root_value [n], root_logits [n, A] float32; to_play [n] (None: 1), legal
  [n, A] (None: all), gumbel [n, A] float64 = G (needed unless gumbel_scale is 0); eval_fn(sim, parent_slot [n], action [n]) ->
  (value [n], reward [n], logits [n, A]) is called once per simulation.  Returns a dict of numpy arrays: the trees as
  export_tree's (N, W, P, R, E, TP [n, NN], legal [n], minmax [n, 2]), vhat [n, sims + 1], sel_slot / sel_action / plens
  [n, sims], paths [n, sims, sims + 2], action [n], pred_reward [n], pi [n, A], v_mix [n] and min_gap (a float)."""
  lib = _abi.load()
  A, S = cfg.action_space, cfg.num_simulations
  rv = np.ascontiguousarray(root_value, np.float32)
  lg = np.ascontiguousarray(root_logits, np.float32)
  n = rv.shape[0]
  tp = None if to_play is None else np.ascontiguousarray(to_play, np.int8)
  lm = None if legal is None else np.ascontiguousarray(legal, np.uint8)
  gm = None if gumbel is None else np.ascontiguousarray(gumbel, np.float64)
  if rv.shape != (n,) or lg.shape != (n, A) or (tp is not None and tp.shape != (n,)) or (lm is not None and lm.shape != (n, A)) or \
      (gm is not None and gm.shape != (n, A)):
    raise ValueError('gz_search_host: root_value [n], root_logits [n, A], to_play [n], legal [n, A], gumbel [n, A]')
  sims = S if num_simulations is None else int(num_simulations)
  NN = 1 + (S + 1) * A
  d = dict(N=np.zeros((n, NN), np.int32), W=np.zeros((n, NN)), P=np.zeros((n, NN)), R=np.zeros((n, NN), np.float32),
           E=np.zeros((n, NN), np.int32), TP=np.zeros((n, NN), np.int8), legal=np.zeros(n, np.uint32), minmax=np.zeros((n, 2)),
           vhat=np.zeros((n, S + 1), np.float32), sel_slot=np.zeros((n, S), np.int32), sel_action=np.zeros((n, S), np.int32),
           paths=np.full((n, S, S + 2), -1, np.int32), plens=np.zeros((n, S), np.int32), action=np.zeros(n, np.int32),
           pred_reward=np.zeros(n, np.float32), pi=np.zeros((n, A)), v_mix=np.zeros(n), min_gap=np.zeros(1))
  failure = []

  def cb(_ctx, sim, slot, act, rows, value, reward, logits):
    try:
      v, r, l = eval_fn(int(sim), np.ctypeslib.as_array(slot, (rows,)).copy(), np.ctypeslib.as_array(act, (rows,)).copy())
      np.ctypeslib.as_array(value, (rows,))[:] = np.asarray(v, np.float32).reshape(rows)
      np.ctypeslib.as_array(reward, (rows,))[:] = np.asarray(r, np.float32).reshape(rows)
      np.ctypeslib.as_array(logits, (rows, A))[:] = np.asarray(l, np.float32).reshape(rows, A)
    except Exception as ex:      # (an exception cannot cross the C frames)
      failure.append(ex)
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
  cb_c = _GZ_EVAL(cb)      # (kept alive across the call)
  _abi.check(lib.mz_gz_search_host(C.byref(cfg), n, p(tp), p(lm), p(rv), p(lg), p(gm), int(max_considered), float(c_visit),
                                   float(c_scale), float(gumbel_scale), sims, C.cast(cb_c, C.c_void_p), None,
                                   *[p(d[key]) for key in ('N', 'W', 'P', 'R', 'E', 'TP', 'legal', 'minmax', 'vhat', 'sel_slot',
                                                           'sel_action', 'paths', 'plens', 'action', 'pred_reward', 'pi', 'v_mix',
                                                           'min_gap')]), 'mz_gz_search_host')
  if failure:
    raise failure[0]
  d['min_gap'] = float(d['min_gap'][0])
  return d


class Engine(object):

  def __init__(self, num_envs, obs_dim, action_space, num_simulations, two_players=False,
               known_bounds=(None, None), value_support=(-15, 15), reward_support=(-15, 15),
               no_target_transform=False, no_support=False, discount=0.997, pb_c_base=19652, pb_c_init=1.25, init_value_score=0.0,
               root_dirichlet_alpha=0.25, root_exploration_fraction=0.25, seed=0, env_id_offset=0, device=None,
               split_f16=False):
    if not torch.cuda.is_available():
      raise RuntimeError('model_based_rl_amd.Engine needs a HIP device (torch.cuda.is_available() is False); '
                         'there is no CPU path.')
    self.lib = _abi.load()
    self.device = torch.device(device if device is not None else 'cuda:0')
    if self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    torch.cuda.set_device(self.device)
    lo, hi = known_bounds
    self.B, self.O, self.A, self.sims = int(num_envs), int(obs_dim), int(action_space), int(num_simulations)
    # outputs of the value / reward heads: the support sizes, one scalar each with --no_support (networks.py:135-136)
    self._outputs = (1, 1) if no_support else (int(value_support[1]) - int(value_support[0]) + 1,
                                                int(reward_support[1]) - int(reward_support[0]) + 1)
    self.cfg = mz_config(self.B, self.O, self.A, self.sims, two_players, known_bounds, value_support, reward_support,
                         no_target_transform, no_support, discount, pb_c_base, pb_c_init, init_value_score,
                         root_dirichlet_alpha, root_exploration_fraction, seed, env_id_offset, split_f16)
    # (the library also honours MZ_SPLIT_F16=1, for running the parity suite on that kernel)
    self.split_f16 = bool(split_f16) or os.environ.get('MZ_SPLIT_F16', '0')[:1] == '1'
    h = C.c_void_p()
    _abi.check(self.lib.mz_create(C.byref(self.cfg), C.byref(h)), 'mz_create')
    self._h = h
    self.NN = self.lib.mz_nodes_per_tree(self._h)
    self.num_weights = self.lib.mz_num_weights(self._h)
    self._keep = []
    self.obs_packed = False

  @classmethod
  def from_config(cls, config, num_envs, device=None, seed=None, env_id_offset=0):
    """Build from a reference-style Config (config.py:87-231 attribute names)."""
    obs_dim = int(np.prod(config.obs_space))
    return cls(num_envs, obs_dim, config.action_space, config.num_simulations,
               two_players=getattr(config, 'two_players', False),
               known_bounds=tuple(getattr(config, 'known_bounds', (None, None))),
               value_support=tuple(getattr(config, 'value_support', (-15, 15))),
               reward_support=tuple(getattr(config, 'reward_support', (-15, 15))),
               no_target_transform=getattr(config, 'no_target_transform', False),
               no_support=getattr(config, 'no_support', False), discount=config.discount,
               pb_c_base=config.pb_c_base, pb_c_init=config.pb_c_init,
               init_value_score=getattr(config, 'init_value_score', 0.0),
               root_dirichlet_alpha=config.root_dirichlet_alpha,
               root_exploration_fraction=config.root_exploration_fraction,
               seed=(config.seed if seed is None else seed) or 0, env_id_offset=env_id_offset, device=device,
               split_f16=getattr(config, 'split_f16', False))

  def close(self):
    if getattr(self, '_h', None):
      self.lib.mz_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  @property
  def stream(self):
    return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  def _dev(self, x, dtype):
    if x is None:
      return None
    if not torch.is_tensor(x):
      x = torch.as_tensor(np.ascontiguousarray(x))
    x = x.to(self.device, dtype).contiguous()
    self._keep.append(x)
    if len(self._keep) > 64:
      del self._keep[:32]
    return x

  # ---- weights (networks.py:36-37, actors.py:81-85)
  def set_weights(self, weights, scale_ok=None, sync=False):
    """Weights on the HOST (a state_dict, a numpy array, a CPU tensor): mz_set_weights_async -- the repack is queued in
    stream order and the call returns without waiting for the moves queued before it (which kernel set the weights run on
    is decided on the host copy, mz_weights_scale_ok).  Weights on the DEVICE (the buffer a broadcast filled): the same
    when the caller passes `scale_ok` (the learner rank's mz_weights_scale_ok on its host copy; the tensor must stay valid
    until the stream has passed the call), else mz_set_weights, which reads the decision back and so waits for the stream.
    sync: force mz_set_weights.  A state_dict's tensors must have this engine's shapes; a flat vector, its length."""
    if isinstance(weights, dict):
      check_weight_shapes(weights, self.O, self.A, *self._outputs)
      weights = flatten_weights(weights)
    if not torch.is_tensor(weights):
      weights = torch.from_numpy(np.ascontiguousarray(weights, np.float32))
    weights = weights.reshape(-1)
    if weights.numel() != self.num_weights:
      raise ValueError('expected %d weights, got %d' % (self.num_weights, weights.numel()))
    on_dev = weights.is_cuda
    w = weights.to(torch.float32).contiguous()
    sync = sync or os.environ.get('MZ_SYNC_WEIGHTS', '0')[:1] == '1'      # (A/B runs against the synchronous pull)
    if not on_dev and scale_ok is None and not sync:
      scale_ok = self.weights_scale_ok(w)
    if scale_ok is None or sync:
      _abi.check(self.lib.mz_set_weights(self._h, _ptr(w), w.numel(), int(on_dev), self.stream), 'mz_set_weights')
    else:
      _abi.check(self.lib.mz_set_weights_async(self._h, _ptr(w), w.numel(), int(on_dev), int(bool(scale_ok)), self.stream),
                 'mz_set_weights_async')
    self._weights_dev = w if on_dev else None      # (the one device buffer of the last pull stays alive; nothing accumulates)

  def weights_scale_ok(self, flat_host):
    """mz_weights_scale_ok for this engine's shapes on a host copy of the flat weights"""
    return weights_scale_ok(flat_host, self.O, self.A, self._outputs[0], self._outputs[1])

  def weight_scale(self):
    """(1, 2^-k, 2^k, chosen) of the last set_weights (mz_weight_scale): the power of two the search kernel's weight
    stream is scaled by so that its ReLU can be a clamp."""
    out = np.zeros(4, np.float32)
    _abi.check(self.lib.mz_weight_scale(self._h, out.ctypes.data, self.stream), 'mz_weight_scale')
    return out

  # ---- network
  def initial_inference(self, obs):
    obs = self._dev(obs, torch.float32).reshape(self.B, self.O)
    _abi.check(self.lib.mz_initial_inference(self._h, _ptr(obs), self.stream), 'mz_initial_inference')

  def root_load(self, value, logits, hidden=None):
    value = self._dev(value, torch.float32); logits = self._dev(logits, torch.float32)
    hidden = self._dev(hidden, torch.float32)
    _abi.check(self.lib.mz_root_load(self._h, _ptr(hidden), _ptr(value), _ptr(logits), self.stream), 'mz_root_load')

  def root_outputs(self):
    v = torch.empty(self.B, dtype=torch.float32, device=self.device)
    lg = torch.empty(self.B, self.A, dtype=torch.float32, device=self.device)
    h = torch.empty(self.B, H, dtype=torch.float32, device=self.device)
    _abi.check(self.lib.mz_root_outputs(self._h, _ptr(v), _ptr(lg), _ptr(h), self.stream), 'mz_root_outputs')
    return v, lg, h

  def recurrent_inference(self, hidden, action):
    hidden = self._dev(hidden, torch.float32).reshape(-1, H)
    action = self._dev(action, torch.int32)
    n = hidden.shape[0]
    ho = torch.empty(n, H, dtype=torch.float32, device=self.device)
    r = torch.empty(n, dtype=torch.float32, device=self.device)
    v = torch.empty(n, dtype=torch.float32, device=self.device)
    lg = torch.empty(n, self.A, dtype=torch.float32, device=self.device)
    _abi.check(self.lib.mz_recurrent_inference(self._h, _ptr(hidden), _ptr(action), n, _ptr(ho), _ptr(r), _ptr(v),
                                               _ptr(lg), self.stream), 'mz_recurrent_inference')
    return ho, r, v, lg

  # ---- tree
  def root_prepare(self, to_play=None, legal=None, noise=None, device_rng=False, move=0):
    to_play = self._dev(to_play, torch.int8)
    legal = self._dev(legal, torch.uint8)
    noise = self._dev(noise, torch.float64)
    _abi.check(self.lib.mz_root_prepare(self._h, _ptr(to_play), _ptr(legal), _ptr(noise), int(device_rng), int(move),
                                        self.stream), 'mz_root_prepare')

  def root_set_priors(self, priors, to_play=None, legal=None):
    to_play = self._dev(to_play, torch.int8); legal = self._dev(legal, torch.uint8)
    priors = self._dev(priors, torch.float64)
    _abi.check(self.lib.mz_root_set_priors(self._h, _ptr(to_play), _ptr(legal), _ptr(priors), self.stream),
               'mz_root_set_priors')

  def last_paths(self):
    paths = torch.empty(self.B, self.sims + 2, dtype=torch.int32, device=self.device)
    lens = torch.empty(self.B, dtype=torch.int32, device=self.device)
    _abi.check(self.lib.mz_last_paths(self._h, _ptr(paths), _ptr(lens), self.stream), 'mz_last_paths')
    return paths, lens

  def search(self, num_simulations=None):
    n = self.sims if num_simulations is None else int(num_simulations)
    _abi.check(self.lib.mz_search(self._h, n, self.stream), 'mz_search')

  def search_profiled(self, num_simulations=None):
    """-> (ms of all recurrent-inference launches, ms of all tree-step launches) for one search."""
    n = self.sims if num_simulations is None else int(num_simulations)
    ms = (C.c_float * 2)()
    _abi.check(self.lib.mz_search_profiled(self._h, n, ms, self.stream), 'mz_search_profiled')
    return float(ms[0]), float(ms[1])

  def search_timed(self, num_simulations=None):
    """mz_search with events around the search kernel's own dispatch; returns milliseconds (synchronous)."""
    n = self.sims if num_simulations is None else int(num_simulations)
    ms = (C.c_float * 1)()
    _abi.check(self.lib.mz_search_timed(self._h, n, ms, self.stream), 'mz_search_timed')
    return float(ms[0])

  def search_phase_profile(self, num_simulations=None):
    n = self.sims if num_simulations is None else int(num_simulations)
    out = np.zeros((4, 14), np.uint64)
    _abi.check(self.lib.mz_search_phase_profile(self._h, n, out.ctypes.data_as(C.c_void_p), self.stream),
               'mz_search_phase_profile')
    return out

  def search_phase_spread(self):
    """(mean, min, max) over the workgroups of a workgroup's total cycles in the last search_phase_profile"""
    out = (C.c_double * 3)()
    _abi.check(self.lib.mz_search_phase_spread(self._h, out), 'mz_search_phase_spread')
    return tuple(float(x) for x in out)

  def select(self):
    out = self._selection_out(4)
    _abi.check(self.lib.mz_select(self._h, *[_ptr(o) for o in out], self.stream), 'mz_select')
    return out   # leaf_node, parent_slot, action, depth

  def tree_pair_timed(self, value, reward, logits):
    """one simulation's select + expand_backup with events around each kernel's own dispatch; returns (ms, ms), synchronous"""
    value = self._dev(value, torch.float32); reward = self._dev(reward, torch.float32); logits = self._dev(logits, torch.float32)
    ms = (C.c_float * 2)()
    _abi.check(self.lib.mz_tree_pair_timed(self._h, _ptr(value), _ptr(reward), _ptr(logits), ms, self.stream), 'mz_tree_pair_timed')
    return float(ms[0]), float(ms[1])

  def gather_hidden(self):
    h = torch.empty(self.B, H, dtype=torch.float32, device=self.device)
    _abi.check(self.lib.mz_gather_hidden(self._h, _ptr(h), self.stream), 'mz_gather_hidden')
    return h

  def _tree_step(self, name, inputs, outputs=None, n_out=0):
    """the ABI call `name` of one simulation's tree step: inputs as float32 device tensors (None: NULL), then the n_out
    pointers of an *_expand_backup_select -- of the tensors in `outputs`, or NULL each (None: the move's last simulation);
    returns outputs"""
    ins = [_ptr(self._dev(x, torch.float32)) for x in inputs]
    outs = [None] * n_out if outputs is None else [_ptr(o) for o in outputs]
    _abi.check(getattr(self.lib, name)(self._h, *ins, *outs, self.stream), name)
    return outputs

  def _selection_out(self, n):
    return [torch.empty(self.B, dtype=torch.int32, device=self.device) for _ in range(n)]

  def expand_backup(self, value, reward, logits, hidden=None):
    self._tree_step('mz_expand_backup', (value, reward, logits, hidden))

  def expand_backup_select(self, value, reward, logits, hidden=None, last=False):
    """expand_backup of this simulation and select of the next in one launch (mz_expand_backup_select); returns what
    select() returns, or None after the move's last simulation (`last`: the caller's count of simulations)"""
    return self._tree_step('mz_expand_backup_select', (value, reward, logits, hidden), None if last else self._selection_out(4), 4)

  # ---- the true-rules search (mz_set_true_model, mz_tm_*, include/mz_engine.h; DESIGN s7g)
  def set_true_model(self, kind):
    """mz_set_true_model: kind 0 / None off, an EVAL_ENVS name or 1 (TicTacToe) / 3 (Connect Four).  While set,
    eval_env_moves and Match.plies search the games' real positions on this engine."""
    k = 0 if not kind else (self.EVAL_ENVS[kind] if isinstance(kind, str) else int(kind))
    _abi.check(self.lib.mz_set_true_model(self._h, k), 'mz_set_true_model')
    self.true_model = k

  def tm_root(self, boards, turn, step):
    """mz_tm_root (after root_prepare): the roots' positions, boards [B, 42] int8, turn [B] int8, step [B] int32"""
    bd = self._dev(np.ascontiguousarray(boards, np.int8).reshape(self.B, 42), torch.int8)
    tn = self._dev(np.ascontiguousarray(turn, np.int8).reshape(self.B), torch.int8)
    st = self._dev(np.ascontiguousarray(step, np.int32).reshape(self.B), torch.int32)
    _abi.check(self.lib.mz_tm_root(self._h, _ptr(bd), _ptr(tn), _ptr(st), self.stream), 'mz_tm_root')

  def _tm_leaf_out(self):
    return (torch.empty(self.B, self.O, dtype=torch.float32, device=self.device),
            torch.empty(self.B, dtype=torch.uint8, device=self.device))

  def tm_select(self):
    """mz_tm_select -> (obs [B, O] float32: the leaves' observations, zeros where finished; finished [B] uint8)"""
    obs, fin = self._tm_leaf_out()
    _abi.check(self.lib.mz_tm_select(self._h, _ptr(obs), _ptr(fin), self.stream), 'mz_tm_select')
    return obs, fin

  def tm_expand_backup(self, value, logits):
    self._tree_step('mz_tm_expand_backup', (value, logits))

  def tm_expand_backup_select(self, value, logits, last=False):
    """tm_expand_backup of this simulation and tm_select of the next in one launch; returns what tm_select returns, or None
    after the move's last simulation (`last`: the caller's count of simulations)"""
    return self._tree_step('mz_tm_expand_backup_select', (value, logits), None if last else self._tm_leaf_out(), 2)

  def tm_search(self, num_simulations=None):
    n = self.sims if num_simulations is None else int(num_simulations)
    _abi.check(self.lib.mz_tm_search(self._h, n, self.stream), 'mz_tm_search')

  def tm_search_fused(self, num_simulations=None):
    """mz_tm_search_fused (DESIGN s7k): tm_search's simulations in one launch, bit-identical trees"""
    n = self.sims if num_simulations is None else int(num_simulations)
    _abi.check(self.lib.mz_tm_search_fused(self._h, n, self.stream), 'mz_tm_search_fused')

  def tm_export(self):
    """mz_tm_export -> dict of numpy arrays per expansion slot: boards [B, sims + 1, 42], mover, step, mask, finished
    [B, sims + 1], and nexp [B]; EX [B, NN]: the nodes that exist (export_tree's EX counts every child of an expanded node)"""
    B, S = self.B, self.sims + 1
    d = dict(boards=np.zeros((B, S, 42), np.int8), mover=np.zeros((B, S), np.int8), step=np.zeros((B, S), np.int32),
             mask=np.zeros((B, S), np.uint32), finished=np.zeros((B, S), np.uint8), nexp=np.zeros(B, np.int32))
    _abi.check(self.lib.mz_tm_export(self._h, *[d[k].ctypes.data_as(C.c_void_p) for k in ('boards', 'mover', 'step', 'mask', 'finished', 'nexp')]),
               'mz_tm_export')
    d['EX'] = tm_exists(d['mask'], d['nexp'], self.A, self.NN)
    return d

  # ---- the Gumbel search (mz_set_gumbel, mz_gz_*, include/mz_engine.h; DESIGN s7h)
  def set_gumbel(self, on=True, max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=0.0):
    """mz_set_gumbel: while on, eval_env_moves and Match.plies search with the Gumbel search on this engine.
    gumbel_scale 0 (the evaluation default) draws nothing; 1 is the acting setting of the paper."""
    _abi.check(self.lib.mz_set_gumbel(self._h, int(bool(on)), int(max_considered), float(c_visit), float(c_scale),
                                      float(gumbel_scale)), 'mz_set_gumbel')
    self.gumbel = bool(on)

  def gz_root(self, gumbel=None, move=0):
    """mz_gz_root (after root_prepare without noise): gumbel [B, A] float64 = G, or None: drawn on the device, `move` in the key"""
    g = None if gumbel is None else self._dev(gumbel, torch.float64).reshape(self.B, self.A)
    _abi.check(self.lib.mz_gz_root(self._h, _ptr(g), int(move), self.stream), 'mz_gz_root')

  def gz_select(self):
    """mz_gz_select -> (parent_slot [B], action [B]) int32; gather_hidden() gives the parents' hidden states"""
    out = self._selection_out(2)
    _abi.check(self.lib.mz_gz_select(self._h, _ptr(out[0]), _ptr(out[1]), self.stream), 'mz_gz_select')
    return out

  def gz_expand_backup(self, value, reward, logits, hidden=None):
    self._tree_step('mz_gz_expand_backup', (value, reward, logits, hidden))

  def gz_expand_backup_select(self, value, reward, logits, hidden=None, last=False):
    """gz_expand_backup of this simulation and gz_select of the next in one launch; returns what gz_select returns, or None
    after the move's last simulation (`last`: the caller's count of simulations)"""
    return self._tree_step('mz_gz_expand_backup_select', (value, reward, logits, hidden), None if last else self._selection_out(2), 2)

  def gz_search(self, num_simulations=None):
    n = self.sims if num_simulations is None else int(num_simulations)
    _abi.check(self.lib.mz_gz_search(self._h, n, self.stream), 'mz_gz_search')

  def gz_pick(self):
    """mz_gz_pick -> (action [B] int32, pred_reward [B] float32, improved_policy [B, A] float64, v_mix [B] float64)"""
    a = torch.empty(self.B, dtype=torch.int32, device=self.device)
    r = torch.empty(self.B, dtype=torch.float32, device=self.device)
    pi = torch.empty(self.B, self.A, dtype=torch.float64, device=self.device)
    vm = torch.empty(self.B, dtype=torch.float64, device=self.device)
    _abi.check(self.lib.mz_gz_pick(self._h, _ptr(a), _ptr(r), _ptr(pi), _ptr(vm), self.stream), 'mz_gz_pick')
    return a, r, pi, vm

  def gz_export(self):
    """mz_gz_export -> dict of numpy arrays: G [B, A] float64 (this move's draws), vhat [B, sims + 1] float32"""
    d = dict(G=np.zeros((self.B, self.A)), vhat=np.zeros((self.B, self.sims + 1), np.float32))
    _abi.check(self.lib.mz_gz_export(self._h, d['G'].ctypes.data_as(C.c_void_p), d['vhat'].ctypes.data_as(C.c_void_p)), 'mz_gz_export')
    return d

  def finalize(self, temperature, uniform=None, move=0):
    if torch.is_tensor(temperature):
      t = temperature.to(self.device, torch.float64).expand(self.B)
    else:
      t = torch.as_tensor(np.broadcast_to(np.asarray(temperature, np.float64), (self.B,)).copy())
    t = self._dev(t, torch.float64)
    u = self._dev(uniform, torch.float64)
    action = torch.empty(self.B, dtype=torch.int32, device=self.device)
    cv = torch.empty(self.B, self.A, dtype=torch.float64, device=self.device)
    rv = torch.empty(self.B, dtype=torch.float64, device=self.device)
    err = torch.empty(self.B, dtype=torch.float64, device=self.device)
    vc = torch.empty(self.B, self.A, dtype=torch.int32, device=self.device)
    _abi.check(self.lib.mz_finalize(self._h, _ptr(t), _ptr(u), int(move), _ptr(action), _ptr(cv), _ptr(rv), _ptr(err),
                                    _ptr(vc), self.stream), 'mz_finalize')
    return dict(action=action, child_visits=cv, root_value=rv, error=err, visit_counts=vc)

  # ---- evaluation (evaluate.py:278-327; csrc/mz_eval.hip.h)
  def eval_walk(self, max_actions, temperature, uniform=None, move=0, path_lengths=True):
    """mz_eval_walk: after a search, the up to max_actions actions Evaluator.play_game applies (evaluate.py:314-326) and
    their predicted rewards, and len(search_path) of every simulation (evaluate.py:306-307).  temperature: scalar or [B];
    uniform [B, max_actions] float64 (the draws of select_action) or None = device RNG keyed (seed, env, move, step).
    Returns dict(actions [B, M] int32 (-1 past n_actions), pred_rewards [B, M] float32, n_actions [B] int32,
    path_lengths [B, sims] int32 or None), device tensors."""
    M = int(max_actions)
    if torch.is_tensor(temperature):
      t = self._dev(temperature.to(self.device, torch.float64).expand(self.B), torch.float64)
    else:
      t = self._dev(torch.as_tensor(np.broadcast_to(np.asarray(temperature, np.float64), (self.B,)).copy()), torch.float64)
    u = self._dev(None if uniform is None else np.asarray(uniform, np.float64).reshape(self.B, M), torch.float64)
    out = dict(actions=torch.empty(self.B, M, dtype=torch.int32, device=self.device),
               pred_rewards=torch.empty(self.B, M, dtype=torch.float32, device=self.device),
               n_actions=torch.empty(self.B, dtype=torch.int32, device=self.device),
               path_lengths=torch.empty(self.B, self.sims, dtype=torch.int32, device=self.device) if path_lengths else None)
    _abi.check(self.lib.mz_eval_walk(self._h, M, _ptr(t), _ptr(u), int(move), _ptr(out['actions']), _ptr(out['pred_rewards']),
                                     _ptr(out['n_actions']), _ptr(out['path_lengths']), self.stream), 'mz_eval_walk')
    return out

  EVAL_MODES = {'only_prior': 1, 'only_value': 2}

  def eval_lookahead(self, mode, rows=False):
    """mz_eval_lookahead: --only_prior / --only_value (evaluate.py:278-304) on the prepared roots, no search.  Returns
    dict(action [B] int32, pred_reward [B] float32, child_visits [B, A] float64) and with rows=True the rows' reward and value
    (row_reward / row_value: [B, A] for only_value, [B] for only_prior), device tensors."""
    m = self.EVAL_MODES[mode] if isinstance(mode, str) else int(mode)
    shape = (self.B, self.A) if m == 2 else (self.B,)
    out = dict(action=torch.empty(self.B, dtype=torch.int32, device=self.device),
               pred_reward=torch.empty(self.B, dtype=torch.float32, device=self.device),
               child_visits=torch.empty(self.B, self.A, dtype=torch.float64, device=self.device))
    if rows:
      out['row_reward'] = torch.empty(shape, dtype=torch.float32, device=self.device)
      out['row_value'] = torch.empty(shape, dtype=torch.float32, device=self.device)
    _abi.check(self.lib.mz_eval_lookahead(self._h, m, _ptr(out['action']), _ptr(out['pred_reward']), _ptr(out['child_visits']),
                                          _ptr(out.get('row_reward')), _ptr(out.get('row_value')), self.stream),
               'mz_eval_lookahead')
    return out

  # ---- evaluation games on the device environments (mz_eval_env_*, include/mz_engine.h)
  EVAL_ENVS = KIND_OF_ENV      # (envs.DEVICE_GAMES)

  def eval_env_reset(self, kind, max_steps, time_limit=0, random_opp=None, keep_history=False):
    """mz_eval_env_reset: B evaluation games of `kind` (an EVAL_ENVS name or 1 / 2 / 3) at their start; game b has the seed
    env_id_offset + b.  random_opp: +1 / -1 / None."""
    k = self.EVAL_ENVS[kind] if isinstance(kind, str) else int(kind)
    _abi.check(self.lib.mz_eval_env_reset(self._h, k, int(max_steps), int(time_limit), int(random_opp or 0),
                                          int(bool(keep_history)), self.stream), 'mz_eval_env_reset')
    self.eval_log_cap = int(self.lib.mz_eval_env_log_capacity(self._h))
    self._eval_keep = bool(keep_history)
    self._eval_draws = None

  def eval_env_set_draws(self, walk=None, noise=None, opp=None, start_states=None):
    """mz_eval_env_set_draws: walk [B, moves, M] float64, noise [B, moves, A] float64, opp [B, n] int32, start_states [B, 4]
    float64 (CartPole); uploaded once, kept alive by this object until the next reset"""
    dev = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(self.device, dt).contiguous()
    w, nz, op, st = dev(walk, torch.float64), dev(noise, torch.float64), dev(opp, torch.int32), dev(start_states, torch.float64)
    for t, shape in ((w, (self.B, None, None)), (nz, (self.B, None, self.A)), (op, (self.B, None)), (st, (self.B, 4))):
      if t is not None and (t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise ValueError('eval_env_set_draws: shape %s does not match %s' % (tuple(t.shape), shape))
    self._eval_draws = (w, nz, op, st)
    _abi.check(self.lib.mz_eval_env_set_draws(
        self._h, _ptr(w), 0 if w is None else w.shape[1], 0 if w is None else w.shape[2], _ptr(nz),
        0 if nz is None else nz.shape[1], _ptr(op), 0 if op is None else op.shape[1], _ptr(st), self.stream), 'mz_eval_env_set_draws')

  def eval_env_moves(self, n, mode=0, max_actions=1, temperature=0.0, noise_on=False):
    """mz_eval_env_moves: n whole moves enqueued back to back, one synchronisation at the end; returns the games still live.
    mode: 0 search + walk, 'only_prior' / 1, 'only_value' / 2."""
    m = self.EVAL_MODES[mode] if isinstance(mode, str) else int(mode)
    live = C.c_int(0)
    _abi.check(self.lib.mz_eval_env_moves(self._h, int(n), m, int(max_actions), float(temperature), int(bool(noise_on)),
                                          C.byref(live), self.stream), 'mz_eval_env_moves')
    return int(live.value)

  def eval_env_results(self, logs=None):
    """mz_eval_env_results -> dict of numpy arrays: step, n_moves [B], sum_reward, sum_pred_reward, sum_pred_value,
    sum_root_value, depth_mean [B] float64, depth_max [B, sims]; with logs (default: whether they were kept) also actions,
    rewards, mover, pred_rewards, pred_values, root_values, n_actions [B, cap], child_visits [B, cap, A], depths [B, cap, sims]"""
    B, A, L, S = self.B, self.A, self.eval_log_cap, self.sims
    logs = self._eval_keep if logs is None else bool(logs)
    out = dict(step=np.zeros(B, np.int32), n_moves=np.zeros(B, np.int32), acc=np.zeros((5, B), np.float64),
               depth_max=np.zeros((B, S), np.int32))
    names = ['step', 'n_moves', 'acc', 'depth_max']
    if logs:
      out.update(actions=np.zeros((B, L), np.int32), rewards=np.zeros((B, L), np.float64), mover=np.zeros((B, L), np.int8),
                 pred_rewards=np.zeros((B, L), np.float32), pred_values=np.zeros((B, L), np.float32),
                 root_values=np.zeros((B, L), np.float64), child_visits=np.zeros((B, L, A), np.float64),
                 n_actions=np.zeros((B, L), np.int32), depths=np.zeros((B, L, S), np.int32))
      names += ['actions', 'rewards', 'mover', 'pred_rewards', 'pred_values', 'root_values', 'child_visits', 'n_actions', 'depths']
    ptrs = [out[k].ctypes.data_as(C.c_void_p) for k in names] + [None] * (13 - len(names))
    _abi.check(self.lib.mz_eval_env_results(self._h, *ptrs, self.stream), 'mz_eval_env_results')
    acc = out.pop('acc')
    for i, k in enumerate(('sum_reward', 'sum_pred_reward', 'sum_pred_value', 'sum_root_value', 'depth_mean')):
      out[k] = acc[i]
    return out

  # ---- the playout-search (UCT) opponent (mz_playout_plan, mz_eval_env_set_opponent, include/mz_engine.h)
  def eval_env_set_opponent(self, playouts):
    """mz_eval_env_set_opponent (after eval_env_reset with a random_opp seat, before the first move): that seat's moves are
    planned by a playout search of `playouts` playouts per move on the true rules; 0: the uniformly random mover"""
    _abi.check(self.lib.mz_eval_env_set_opponent(self._h, int(playouts), self.stream), 'mz_eval_env_set_opponent')

  def playout_plan(self, kind, boards, turn, step, playouts, move=0):
    """mz_playout_plan: one playout-search move for each of n <= B positions of `kind` (an EVAL_ENVS name or 1 / 3): boards
    [n, 42] (TicTacToe: the first 9 cells of a row), turn [n] +1 / -1, step [n] plies played; position i is the game with
    the seed env_id_offset + i.  Returns numpy arrays: action [n], visits [n, A], wins [n, A] (2 * wins + draws of the
    mover), all int32."""
    k = self.EVAL_ENVS[kind] if isinstance(kind, str) else int(kind)
    bd = np.ascontiguousarray(boards, np.int8)
    tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
    n = bd.shape[0]
    if bd.shape != (n, 42) or tn.shape != (n,) or st.shape != (n,):
      raise ValueError('playout_plan: boards [n, 42], turn [n], step [n]; got %s, %s, %s' % (bd.shape, tn.shape, st.shape))
    action, visits, wins = np.zeros(n, np.int32), np.zeros((n, self.A), np.int32), np.zeros((n, self.A), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _abi.check(self.lib.mz_playout_plan(self._h, k, p(bd), p(tn), p(st), n, int(playouts), int(move), p(action), p(visits),
                                        p(wins), self.stream), 'mz_playout_plan')
    return action, visits, wins

  SOLVE_NODES = 4096      # the default node budget of one (position, action): derived from profiles/solve_bench.json (README, "Grading moves")

  def solve(self, kind, boards, turn, step, max_nodes=SOLVE_NODES, table=False):
    """mz_solve, or with table=True mz_solve_tt (the table search: the same exact values from far fewer nodes, so `nodes`
    counts another search and fewer units are unsolved at a given max_nodes): the exact outcome of every action of n positions of `kind` (an EVAL_ENVS name or 1 / 3; any n): boards
    [n, 42], turn [n], step [n] as playout_plan's, none with a finished line.  Returns numpy arrays: values [n, A] int8 (+1 /
    0 / -1 for the mover after the action, -2 illegal, -3 not solved within max_nodes nodes) and nodes [n, A] uint32."""
    k = self.EVAL_ENVS[kind] if isinstance(kind, str) else int(kind)
    bd = np.ascontiguousarray(boards, np.int8)
    tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
    n = bd.shape[0]
    if bd.shape != (n, 42) or tn.shape != (n,) or st.shape != (n,):
      raise ValueError('solve: boards [n, 42], turn [n], step [n]; got %s, %s, %s' % (bd.shape, tn.shape, st.shape))
    values, nodes = np.zeros((n, self.A), np.int8), np.zeros((n, self.A), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    name = 'mz_solve_tt' if table else 'mz_solve'
    _abi.check(getattr(self.lib, name)(self._h, k, p(bd), p(tn), p(st), n, int(max_nodes), p(values), p(nodes), self.stream), name)
    return values, nodes

  # ---- the learned model by unroll depth (mz_unroll, include/mz_engine.h)
  UNROLL_MAX_K = 16
  UNROLL_TERMS = ('live', 'transition', 'position', 'reward_true', 'reward', 'reward_err', 'value', 'value_fresh', 'value_drift',
                  'policy_tv', 'top1_agree', 'illegal_mass', 'illegal_mass_fresh', 'solved', 'vstar', 'value_err', 'value_err_fresh',
                  'sign', 'sign_fresh', 'optimal_mass', 'optimal_mass_fresh')      # csrc/mz_unroll.hip.h MzUnrollTerm

  def unroll(self, kind, boards, turn, step, actions, truth=None, raw=False):
    """mz_unroll: the model unrolled along the actions of n rows (any n) next to the real positions those actions lead to.
    kind: an EVAL_ENVS name or 1 / 3; boards [n, 42], turn [n], step [n] as solve's; actions [n, K] int32, -1 as padding, K in
    0 .. 16; truth [n, K + 1, A] int8 or None: solve's values of the actions of p_k.  Returns a dict of numpy arrays: depth [n]
    (the actions applied), terms [n, K + 1, len(UNROLL_TERMS)] float64 (the scalars of every (row, k), named by UNROLL_TERMS;
    values are in the view of p_k's mover) and, with raw=True, obs [n, K + 1, O], hidden_u [n, K + 1, 50], logits_u / logits_f
    [n, K + 1, A], value_u / reward_u / value_f / reward_true [n, K + 1] (float32), legal [n, K + 1, A] and terminal [n, K + 1]
    (uint8).  Past a row's depth everything is zero.  ValueError if a row holds an action that is illegal in its position."""
    k = self.EVAL_ENVS[kind] if isinstance(kind, str) else int(kind)
    bd = np.ascontiguousarray(boards, np.int8)
    tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
    ac = np.ascontiguousarray(actions, np.int32)
    n = bd.shape[0]
    if bd.shape != (n, 42) or tn.shape != (n,) or st.shape != (n,) or ac.ndim != 2 or ac.shape[0] != n:
      raise ValueError('unroll: boards [n, 42], turn [n], step [n], actions [n, K]; got %s, %s, %s, %s' % (bd.shape, tn.shape, st.shape, ac.shape))
    K = ac.shape[1]
    th = None
    if truth is not None:
      th = np.ascontiguousarray(truth, np.int8)
      if th.shape != (n, K + 1, self.A):
        raise ValueError('unroll: truth [n, K + 1, A] = %s, got %s' % ((n, K + 1, self.A), th.shape))
    NT, W = len(self.UNROLL_TERMS), self.O + H + 2 * self.A + 4
    assert NT == self.lib.mz_unroll_num_terms() and W == self.lib.mz_unroll_raw_floats(self._h)
    terms = np.zeros((n, K + 1, NT), np.float64)
    depth, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rec = np.zeros((n, K + 1, W), np.float32) if raw else None
    meta = np.zeros((n, K + 1, 2), np.int32) if raw else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _abi.check(self.lib.mz_unroll(self._h, k, p(bd), p(tn), p(st), p(ac), n, K, p(th), p(terms), p(depth), p(flags), p(rec), p(meta),
                                  self.stream), 'mz_unroll')
    if flags.any():
      raise ValueError('unroll: row %d holds an action that is illegal in its position' % int(np.flatnonzero(flags)[0]))
    out = dict(depth=depth, terms=terms)
    if raw:
      O, A = self.O, self.A
      out.update(obs=rec[..., :O], hidden_u=rec[..., O:O + H], logits_u=rec[..., O + H:O + H + A], logits_f=rec[..., O + H + A:O + H + 2 * A],
                 value_u=rec[..., W - 4], reward_u=rec[..., W - 3], value_f=rec[..., W - 2], reward_true=rec[..., W - 1],
                 legal=((meta[..., 0:1] >> np.arange(A)) & 1).astype(np.uint8), terminal=meta[..., 1].astype(np.uint8))
    return out

  # ---- Reanalyse of stored replay rows (mz_reanalyse, include/mz_engine.h)
  def reanalyse(self, rows, fresh, n_rows, kind, num_simulations=None):
    """mz_reanalyse: rows [>= n_rows, rec_floats(O, A)] and fresh [>= n_rows, A + 2], both PINNED float32 host tensors; the
    first n_rows rows are searched again under the current weights in chunks of B, without exploration noise, and fresh
    receives child_visits (float32) and root_value (float64 in two slots) per row -- what PrioritizedReplay.reanalyse_write
    takes.  kind: an ENVS / EVAL_ENVS name or 0..3.  Returns when the last chunk has been stored."""
    kind, n_rows, sims = self._reanalyse_args('reanalyse', rows, fresh, n_rows, kind, num_simulations)
    _abi.check(self.lib.mz_reanalyse(self._h, kind, _ptr(rows), int(rows.shape[1]), n_rows, _ptr(fresh), sims, self.stream),
               'mz_reanalyse')

  def _reanalyse_args(self, fn, rows, fresh, n_rows, kind, num_simulations):
    """the tensor checks of reanalyse / reanalyse_gumbel -> (kind, n_rows, num_simulations) as ints"""
    if isinstance(kind, str):
      kind = self.ENVS[kind] if kind in self.ENVS else self.EVAL_ENVS[kind]
    n_rows = int(n_rows)
    for t, name, width in ((rows, 'rows', None), (fresh, 'fresh', self.A + 2)):
      if not (torch.is_tensor(t) and t.dtype == torch.float32 and not t.is_cuda and t.is_pinned() and t.is_contiguous() and t.dim() == 2):
        raise ValueError('%s: %s must be a contiguous pinned float32 host tensor [rows, floats]' % (fn, name))
      if t.shape[0] < n_rows or (width is not None and t.shape[1] != width):
        raise ValueError('%s: %s has shape %s for %d rows of %s floats' % (fn, name, tuple(t.shape), n_rows, width or 'rec_floats'))
    return int(kind), n_rows, self.sims if num_simulations is None else int(num_simulations)

  def reanalyse_gumbel(self, rows, fresh, n_rows, kind, num_simulations=None, value='mean', draw_key=0):
    """mz_reanalyse_gumbel (DESIGN s7j; set_gumbel first): reanalyse's buffers and chunks, searched with the Gumbel search; fresh
    receives the root's improved policy pi' (float32, exactly 0 at illegal actions) and, as the float64, the root's mean value
    ('mean') or its v_mix ('vmix') -- what a record of selfplay_set_gumbel holds.  draw_key: with a gumbel_scale above 0 a row's
    draws are keyed (engine seed, row index in the pass, draw_key, action), so a pass does not depend on B; at scale 0 nothing
    is drawn."""
    if value not in self.SELFPLAY_GUMBEL_VALUES:
      raise ValueError("reanalyse_gumbel: value is 'mean' or 'vmix', got %r" % (value,))
    kind, n_rows, sims = self._reanalyse_args('reanalyse_gumbel', rows, fresh, n_rows, kind, num_simulations)
    _abi.check(self.lib.mz_reanalyse_gumbel(self._h, kind, _ptr(rows), int(rows.shape[1]), n_rows, _ptr(fresh), sims,
                                            self.SELFPLAY_GUMBEL_VALUES[value], int(draw_key) & 0xFFFFFFFFFFFFFFFF, self.stream),
               'mz_reanalyse_gumbel')

  def reanalyse_true_model(self, rows, fresh, n_rows, kind, num_simulations=None, fused=True):
    """mz_reanalyse_true_model (DESIGN s7n; set_true_model with the game's kind first): reanalyse's buffers, chunks and stored
    fields -- visit shares and the root's mean value, what a record of selfplay_set_true_model holds --, searched on the true
    rules of TicTacToe / Connect Four from the position the stored observation and the record's mover determine.  fused: the
    simulations of a chunk in one launch (tm_search_fused), else tm_search's two launches per simulation; the same bits."""
    kind, n_rows, sims = self._reanalyse_args('reanalyse_true_model', rows, fresh, n_rows, kind, num_simulations)
    _abi.check(self.lib.mz_reanalyse_true_model(self._h, kind, _ptr(rows), int(rows.shape[1]), n_rows, _ptr(fresh), sims,
                                                int(bool(fused)), self.stream), 'mz_reanalyse_true_model')

  def export_tree(self, hidden=False):
    B, NN, A = self.B, self.NN, self.A
    d = dict(N=np.zeros((B, NN), np.int32), W=np.zeros((B, NN)), P=np.zeros((B, NN)),
             R=np.zeros((B, NN), np.float32), E=np.zeros((B, NN), np.int32), TP=np.zeros((B, NN), np.int8),
             legal=np.zeros(B, np.uint32), minmax=np.zeros((B, 2)), noise=np.zeros((B, A)))
    hp = np.zeros((B, self.sims + 1, H), np.float32) if hidden else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _abi.check(self.lib.mz_export_tree(self._h, p(d['N']), p(d['W']), p(d['P']), p(d['R']), p(d['E']), p(d['TP']),
                                       p(d['legal']), p(d['minmax']), p(d['noise']), p(hp)), 'mz_export_tree')
    if hidden:
      d['hidden'] = hp
    # EX (node exists): root, legal root children, and every child slab of an expanded node
    EX = np.zeros((B, NN), np.uint8)
    EX[:, 0] = 1
    for a in range(A):
      EX[:, 1 + a] = (d['legal'] >> a) & 1
    exp_idx = d['E']
    for b in range(B):
      for e in np.unique(exp_idx[b][exp_idx[b] > 0]):
        EX[b, 1 + e * A:1 + (e + 1) * A] = 1
    d['EX'] = EX
    return d

  # ---- on-device self-play (actors.py:126-176 on synthetic envs)
  def selfplay_reset(self, episode_len, temperature=1.0, stagger=False):
    _abi.check(self.lib.mz_selfplay_reset(self._h, int(episode_len), float(temperature), int(stagger), self.stream),
               'mz_selfplay_reset')
    self.rec_floats = self.lib.mz_selfplay_rec_floats(self._h)
    self.ring_moves = self.lib.mz_selfplay_ring_moves(self._h)

  def selfplay_set_temperature(self, temperature):
    """Temperature every environment's next game starts with (actors.py:128-129); games in progress keep theirs."""
    _abi.check(self.lib.mz_selfplay_set_temperature(self._h, float(temperature), self.stream),
               'mz_selfplay_set_temperature')

  def selfplay_set_moves(self, moves):
    """every environment's move counter (RNG key, record placement); the device ring must be drained"""
    _abi.check(self.lib.mz_selfplay_set_moves(self._h, int(moves)), 'mz_selfplay_set_moves')

  def selfplay_set_obs(self, uint8_obs=False, obs_min=None, obs_range=None, packed=False):
    """Synthetic observations as bytes (the -ram- envs) and / or --norm_obs (actors.py:55-58,134-137): obs_min and
    obs_range are broadcast to obs_dim like numpy does in the reference's (obs - min) / range.  packed: the experience
    records carry the byte observations four per float slot (records_view(..., obs_u8=True), a replay with obs_u8)."""
    mn = rg = None
    if obs_min is not None:
      mn = np.ascontiguousarray(np.broadcast_to(np.asarray(obs_min, np.float32).reshape(-1), (self.O,)))
      rg = np.ascontiguousarray(np.broadcast_to(np.asarray(obs_range, np.float32).reshape(-1), (self.O,)))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if packed and not uint8_obs:
      raise ValueError('packed records need byte-valued observations (uint8_obs=True)')
    _abi.check(self.lib.mz_selfplay_set_obs(self._h, 2 if packed else int(bool(uint8_obs)), p(mn), p(rg)), 'mz_selfplay_set_obs')
    self.obs_packed = bool(packed)
    self.rec_floats = self.lib.mz_selfplay_rec_floats(self._h)

  ENVS = SELFPLAY_KINDS      # (envs.DEVICE_GAMES)

  def selfplay_set_env(self, kind):
    """'synthetic' (default), 'tictactoe' (the reference's custom_environments/tic_tac_toe.py on the device), 'cartpole'
    (envs.CartPole on the device; selfplay_reset's episode_len is its time limit) or 'connect_four' (envs.ConnectFour on
    the device); before selfplay_reset"""
    _abi.check(self.lib.mz_selfplay_set_env(self._h, self.ENVS[kind] if isinstance(kind, str) else int(kind)), 'mz_selfplay_set_env')

  def selfplay_set_draws(self, noise=None, uniform=None):
    """parity runs of a game environment: the next moves use these Dirichlet draws [B, A] / select_action uniforms [B]"""
    noise = self._dev(noise, torch.float64); uniform = self._dev(uniform, torch.float64)
    _abi.check(self.lib.mz_selfplay_set_draws(self._h, _ptr(noise), _ptr(uniform), self.stream), 'mz_selfplay_set_draws')

  SELFPLAY_GUMBEL_VALUES = {'mean': 0, 'vmix': 1}
  selfplay_search = 'puct'      # how the self-play loop searches a move: 'puct', 'gumbel' or 'true_rules' (selfplay_set_gumbel / _true_model)

  def selfplay_set_gumbel(self, on=True, value='mean'):
    """mz_selfplay_set_gumbel (DESIGN s7i): while on, the self-play moves of a device game are searched with the Gumbel search
    (set_gumbel first, with gumbel_scale 1 for training) and their records carry pi' of the root in the policy slots, the
    Gumbel pick as the action and, as root_value, the root's mean value ('mean') or its v_mix ('vmix').  After
    selfplay_set_env, with the ring drained."""
    if value not in self.SELFPLAY_GUMBEL_VALUES:
      raise ValueError("selfplay_set_gumbel: value is 'mean' or 'vmix', got %r" % (value,))
    _abi.check(self.lib.mz_selfplay_set_gumbel(self._h, int(bool(on)), self.SELFPLAY_GUMBEL_VALUES[value]), 'mz_selfplay_set_gumbel')
    self._selfplay_switched('gumbel', on)

  def selfplay_set_true_model(self, on=True, fused=True):
    """mz_selfplay_set_true_model (DESIGN s7k): while on, the self-play moves of a device board game are PUCT moves searched on
    the true rules (set_true_model with the game's kind first); fused: a move's simulations in one launch (tm_search_fused),
    else tm_search's two launches per simulation, with the same records.  After selfplay_set_env, with the ring drained."""
    _abi.check(self.lib.mz_selfplay_set_true_model(self._h, int(bool(on)), int(bool(fused))), 'mz_selfplay_set_true_model')
    self._selfplay_switched('true_rules', on)

  def _selfplay_switched(self, mode, on):      # (switching off a mode that is not on leaves the current one)
    self.selfplay_search = mode if on else 'puct' if self.selfplay_search == mode else self.selfplay_search
  selfplay_gumbel = property(lambda self: self.selfplay_search == 'gumbel')
  selfplay_true_model = property(lambda self: self.selfplay_search == 'true_rules')

  def selfplay_export_trees(self, keep=True):
    _abi.check(self.lib.mz_selfplay_export_trees(self._h, int(bool(keep))), 'mz_selfplay_export_trees')

  def selfplay_noise_log(self, keep=True):
    """Keep every move's Dirichlet draw (test instrumentation; selfplay_noise(move) reads one move's draws)."""
    _abi.check(self.lib.mz_selfplay_noise_log(self._h, int(bool(keep))), 'mz_selfplay_noise_log')

  def selfplay_noise(self, move):
    out = np.zeros((self.B, self.A), np.float64)
    _abi.check(self.lib.mz_selfplay_read_noise(self._h, int(move), out.ctypes.data_as(C.c_void_p)), 'mz_selfplay_read_noise')
    return out

  SIM_IO = {'off': 0, 'log': 1, 'inject': 2}

  def sim_io(self, mode, keep_moves=1, values=None):
    """Test instrumentation of the fused search kernels (mz_sim_io): 'log' -> returns the device tensor
    [keep_moves, B, sims + 1, 2 + A] float32 the kernels fill with (value, reward, logits) per tree and simulation (slot 0 =
    the root of a self-play move); 'inject' -> `values` ([B, sims + 1, 2 + A] or [1, B, ...]) are what mz_search's simulations
    consume instead of their own network outputs; 'off' -> production state."""
    m = self.SIM_IO[mode] if isinstance(mode, str) else int(mode)
    buf = None
    if m == 1:
      buf = torch.zeros(int(keep_moves), self.B, self.sims + 1, 2 + self.A, dtype=torch.float32, device=self.device)
    elif m == 2:
      buf = torch.as_tensor(np.ascontiguousarray(values, np.float32)).reshape(1, self.B, self.sims + 1, 2 + self.A)
      buf = buf.to(self.device).contiguous()
      keep_moves = 1
    torch.cuda.synchronize(self.device)
    _abi.check(self.lib.mz_sim_io(self._h, m, _ptr(buf), int(keep_moves)), 'mz_sim_io')
    self._sim_io_buf = buf          # (the engine reads / writes it until the mode changes)
    return buf

  def search_kernel_info(self):
    """dict(kind='standalone' | 'fused' | 'split_f16', lt=LDS placement of the trees, ks1, G) of the kernel mz_search /
    mz_selfplay_steps launch right now (mz_search_kernel_info)"""
    out = (C.c_int * 4)()
    _abi.check(self.lib.mz_search_kernel_info(self._h, out), 'mz_search_kernel_info')
    return dict(kind=('standalone', 'fused', 'split_f16')[out[0]], lt=int(out[1]), ks1=int(out[2]), G=int(out[3]))

  def selfplay_steps(self, moves):
    _abi.check(self.lib.mz_selfplay_steps(self._h, int(moves), self.stream), 'mz_selfplay_steps')

  def selfplay_steps_into(self, out, moves):
    """moves self-play moves whose records the kernels write straight into `out` (pinned host tensor
    [>= moves, B, rec_floats]); complete when the work queued on the current stream behind this call is."""
    if not out.is_pinned() or out.dtype != torch.float32 or not out.is_contiguous() \
        or out.numel() < int(moves) * self.B * self.rec_floats:
      raise ValueError('selfplay_steps_into: out must be a pinned contiguous float32 tensor of [moves, B, rec_floats]')
    _abi.check(self.lib.mz_selfplay_steps_into(self._h, int(moves), C.c_void_p(out.data_ptr()), self.stream),
               'mz_selfplay_steps_into')

  def selfplay_steps_timed(self, moves):
    """moves self-play moves launched eagerly back to back, events around every search-kernel dispatch;
    returns the durations in milliseconds (synchronous)."""
    ms = (C.c_float * int(moves))()
    _abi.check(self.lib.mz_selfplay_steps_timed(self._h, int(moves), ms, self.stream), 'mz_selfplay_steps_timed')
    return [float(x) for x in ms]

  def selfplay_moves_per_launch(self):
    """16 where selfplay_steps plays whole moves inside one launch of the search kernel, 0 where every move is a root
    kernel + a search kernel (two-player games, trees in the global pool, MZ_NO_PERSIST)."""
    return int(self.lib.mz_selfplay_moves_per_launch(self._h))

  SELFPLAY_PHASES = ('root_stage0', 'root_rep_ln', 'root_prediction', 'root_tree', 'resident+tree_setup', 'ring+barrier',
                     'simulations', 'end_of_move')

  def selfplay_phase_profile(self, moves=16):
    """Shader cycles per move and phase of the persistent self-play launch (diagnostic, synchronous): dict phase -> cycles."""
    out = (C.c_double * 8)()
    _abi.check(self.lib.mz_selfplay_phase_profile(self._h, int(moves), out, self.stream), 'mz_selfplay_phase_profile')
    return dict(zip(self.SELFPLAY_PHASES, [float(x) for x in out]))

  def selfplay_drain(self, out=None, max_moves=None, copy_stream=None):
    """Asynchronous D2H of the records produced since the last drain into pinned memory; returns
    (host tensor [n_moves, B, rec_floats], n_moves).  Synchronise the stream before reading.
    copy_stream: issue the copy there, ordered after the work queued on the current stream so far -- the next
    moves on the current stream then overlap the copy (the ring keeps them in different slots)."""
    max_moves = self.ring_moves if max_moves is None else int(max_moves)
    if out is None:
      out = torch.empty(max_moves, self.B, self.rec_floats, dtype=torch.float32).pin_memory()
    n = C.c_int(0)
    stream = self.stream
    if copy_stream is not None:
      copy_stream.wait_stream(torch.cuda.current_stream(self.device))
      stream = C.c_void_p(copy_stream.cuda_stream)
    _abi.check(self.lib.mz_selfplay_drain(self._h, C.c_void_p(out.data_ptr()), max_moves, C.byref(n), stream),
               'mz_selfplay_drain')
    return out, n.value

  def cartpole_reset_state(self, env, episode):
    """float64 state [4] episode `episode` of (global) environment `env` of the device CartPole starts from"""
    out = np.zeros(4, np.float64)
    _abi.check(self.lib.mz_cartpole_reset_state(self._h, int(env), int(episode), out.ctypes.data_as(C.c_void_p)),
               'mz_cartpole_reset_state')
    return out

  def selfplay_env_state(self):
    """[B, 4] float64: the current states of the device CartPole environments (synchronous)"""
    out = np.zeros((self.B, 4), np.float64)
    _abi.check(self.lib.mz_selfplay_env_state(self._h, out.ctypes.data_as(C.c_void_p)), 'mz_selfplay_env_state')
    return out

  def selfplay_set_env_state(self, env, state):
    """replace the state of device CartPole environment `env` (tests: a start next to a threshold); after selfplay_reset"""
    st = np.ascontiguousarray(state, np.float64).reshape(4)
    _abi.check(self.lib.mz_selfplay_set_env_state(self._h, int(env), st.ctypes.data_as(C.c_void_p)), 'mz_selfplay_set_env_state')

  def selfplay_board_state(self):
    """[B, 44] int8: 42 cells, turn and step of every device Connect Four environment (synchronous)"""
    out = np.zeros((self.B, 44), np.int8)
    _abi.check(self.lib.mz_selfplay_board_state(self._h, out.ctypes.data_as(C.c_void_p)), 'mz_selfplay_board_state')
    return out

  def selfplay_set_board_state(self, env, board, turn):
    """place a position into device Connect Four environment `env` (its step = the number of stones); after selfplay_reset"""
    bd = np.ascontiguousarray(board, np.int8).reshape(42)
    _abi.check(self.lib.mz_selfplay_set_board_state(self._h, int(env), bd.ctypes.data_as(C.c_void_p), int(turn)),
               'mz_selfplay_set_board_state')

  def synth_obs(self, env, episode, t):
    obs = np.zeros(self.O, np.float32)
    r = C.c_float(0)
    _abi.check(self.lib.mz_synth_obs(self._h, env, episode, t, obs.ctypes.data_as(C.c_void_p), C.byref(r)),
               'mz_synth_obs')
    return obs, float(r.value)


class Match(object):
  """A match between two networks on the device games (mz_match_*, include/mz_engine.h): a handle over two Engines, network
  0 and network 1, each with its own weights and num_simulations.  The engines must share device, num_envs, shapes, seed
  and env_id_offset; the match holds them and is closed before them."""
  KINDS = BOARD_KINDS      # (envs.DEVICE_GAMES)
  MODES = {'search': 0, 'only_prior': 1, 'only_value': 2}

  def __init__(self, engine0, engine1, kind, max_steps, keep_history=False):
    self.engines = (engine0, engine1)
    self.lib = engine0.lib
    self.device = engine0.device
    self.B, self.A = engine0.B, engine0.A
    self.S = max(engine0.sims, engine1.sims)
    self.keep = bool(keep_history)
    k = KIND_OF_ENV.get(kind, 0) if isinstance(kind, str) else int(kind)      # (CartPole's 2 gets mz_match_create's own refusal)
    h = C.c_void_p()
    _abi.check(self.lib.mz_match_create(engine0._h, engine1._h, k, int(max_steps), int(self.keep), C.byref(h)), 'mz_match_create')
    self._h = h
    self.log_cap = int(self.lib.mz_match_log_capacity(self._h))
    self._draws = None

  def close(self):
    if getattr(self, '_h', None):
      self.lib.mz_match_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  @property
  def stream(self):
    return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  def reset(self, first_net=0, opening_plies=0):
    """mz_match_reset: every game at its start; network `first_net` moves at ply `opening_plies`, after the opening"""
    _abi.check(self.lib.mz_match_reset(self._h, int(first_net), int(opening_plies), self.stream), 'mz_match_reset')
    self._draws = None

  def set_draws(self, walk=None, noise=None, opening=None):
    """mz_match_set_draws: walk [B, plies] (or [B, plies, 1]) float64, noise [B, plies, A] float64 -- both indexed by the
    ply, opening plies counted -- and opening [B, k] int32; uploaded once, kept alive by this object until the next reset"""
    dev = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(self.device, dt).contiguous()
    w, nz, op = dev(walk, torch.float64), dev(noise, torch.float64), dev(opening, torch.int32)
    if w is not None and w.dim() == 3 and w.shape[2] == 1:
      w = w.reshape(w.shape[0], w.shape[1])
    for t, shape in ((w, (self.B, None)), (nz, (self.B, None, self.A)), (op, (self.B, None))):
      if t is not None and (t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise ValueError('Match.set_draws: shape %s does not match %s' % (tuple(t.shape), shape))
    self._draws = (w, nz, op)
    _abi.check(self.lib.mz_match_set_draws(self._h, _ptr(w), 0 if w is None else w.shape[1], _ptr(nz),
                                           0 if nz is None else nz.shape[1], _ptr(op), 0 if op is None else op.shape[1],
                                           self.stream), 'mz_match_set_draws')

  def plies(self, n, modes=(0, 0), temperatures=(0.0, 0.0), noise_on=(False, False)):
    """mz_match_plies: the opening (once) and n plies enqueued back to back, one synchronisation at the end; returns the
    games still live.  modes / temperatures / noise_on: per network; a mode is 0 / 'search', 1 / 'only_prior', 2 / 'only_value'."""
    md = (C.c_int * 2)(*[self.MODES[m] if isinstance(m, str) else int(m) for m in modes])
    tp = (C.c_double * 2)(*[float(t) for t in temperatures])
    nz = (C.c_int * 2)(*[int(bool(x)) for x in noise_on])
    live = C.c_int(0)
    _abi.check(self.lib.mz_match_plies(self._h, int(n), md, tp, nz, C.byref(live), self.stream), 'mz_match_plies')
    return int(live.value)

  def results(self, logs=None):
    """mz_match_results -> dict of numpy arrays: result [B] int8 (for player +1, the first mover), length [B]; per network
    n_searched [2, B], sum_pred_reward / sum_pred_value / sum_root_value / depth_mean [2, B] float64, depth_max [2, B, S];
    with logs (default: whether they were kept), per ply: actions, mover, net, rewards, pred_rewards, pred_values,
    root_values [B, cap], child_visits [B, cap, A], depths [B, cap, S]"""
    B, A, L, S = self.B, self.A, self.log_cap, self.S
    logs = self.keep if logs is None else bool(logs)
    out = dict(result=np.zeros(B, np.int8), length=np.zeros(B, np.int32), n_searched=np.zeros((2, B), np.int32),
               acc=np.zeros((2, 4, B), np.float64), depth_max=np.zeros((2, B, S), np.int32))
    names = ['result', 'length', 'n_searched', 'acc', 'depth_max']
    if logs:
      out.update(actions=np.zeros((B, L), np.int32), mover=np.zeros((B, L), np.int8), net=np.zeros((B, L), np.int8),
                 rewards=np.zeros((B, L), np.float64), pred_rewards=np.zeros((B, L), np.float32),
                 pred_values=np.zeros((B, L), np.float32), root_values=np.zeros((B, L), np.float64),
                 child_visits=np.zeros((B, L, A), np.float64), depths=np.zeros((B, L, S), np.int32))
      names += ['actions', 'mover', 'net', 'rewards', 'pred_rewards', 'pred_values', 'root_values', 'child_visits', 'depths']
    ptrs = [out[k].ctypes.data_as(C.c_void_p) for k in names] + [None] * (14 - len(names))
    _abi.check(self.lib.mz_match_results(self._h, *ptrs, self.stream), 'mz_match_results')
    acc = out.pop('acc')
    for i, k in enumerate(('sum_pred_reward', 'sum_pred_value', 'sum_root_value', 'depth_mean')):
      out[k] = acc[:, i]
    return out
