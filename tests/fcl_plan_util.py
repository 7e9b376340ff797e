"""What tests/test_fcl_plan_cpu.py and tests/test_gpu_fcl_plan.py share: the record mz_fcl_plan / mz_fcl_plan_host fill
(include/mz_engine_debug.h), the MZ_FCL_* knob sets, the cases of the two goldens and one step case run to a SHA-256.

The goldens were recorded on the MI355X with a library built from the commit BEFORE the plan existed, never from the code under test:
  tests/golden/fcl_plan_parent.json    a scratch copy of that commit got one added hook that copies a created handle's G, S, nwg, nln,
                                       fuse_fwd, fuse_fb, fb_jobs, view.tr.ks1 (KP), lds_bytes, lds_bwd_dw, njobs, njobs_heads, stage_bytes
                                       and the device's CU count out; per row of plan_cases(): mz_fcl_create under the row's knobs
                                       (knobs_set), the hook, mz_fcl_destroy
  tests/golden/fcl_plan_sha256.json    {step_key(c): run_step_case(lib, c) for c in step_cases()} with that commit's library, written in
                                       two separate processes; the two files were equal"""
import ctypes as C
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# the integers of the record, in order (MZ_FCL_PLAN_FIELDS of them)
FIELDS = ('G', 'S', 'nwg', 'nln', 'fuse_fwd', 'fuse_fb', 'fb_jobs', 'KP', 'lds_bytes', 'lds_bwd_dw', 'njobs', 'njobs_heads',
          'stage_bytes', 'fwd', 'bwd', 'lds_dwa', 'cus', 'tape_floats', 'tapes_fit', 'nflags')
PARENT_FIELDS = FIELDS[:13]      # what the golden holds

KNOB_ORDER = ('MZ_FCL_GROUPS', 'MZ_FCL_SLABS', 'MZ_FCL_FUSE_FWD', 'MZ_FCL_FUSE_FB', 'MZ_FCL_FB_JOBS')
KNOB_SETS = {
    'none': {},
    'fuse_fb0': {'MZ_FCL_FUSE_FB': '0'},
    'fuse_fwd0': {'MZ_FCL_FUSE_FWD': '0'},
    'fuse_fwd1': {'MZ_FCL_FUSE_FWD': '1'},
    'fb_jobs0': {'MZ_FCL_FB_JOBS': '0'},
    'g2s2': {'MZ_FCL_GROUPS': '2', 'MZ_FCL_SLABS': '2'},
    'g4s4': {'MZ_FCL_GROUPS': '4', 'MZ_FCL_SLABS': '4'},
    's3': {'MZ_FCL_SLABS': '3'},
    's2': {'MZ_FCL_SLABS': '2'},
}

# optimiser kinds as the kernels are instantiated: FCL_ADAM, FCL_SGD, FCL_SGD | FCL_MOM, FCL_RMSPROP, FCL_RMSPROP | FCL_MOM
OPT_KINDS = (0, 1, 5, 2, 6)
SHAPES = ((8, 4), (42, 7), (128, 6))      # (obs_dim, actions): KD = 54, 57, 56


def knobs_of(env):
  """the five integers of mz_fcl_plan_host's knobs as mz_fcl_create reads them from the environment: -1 = not set; groups and
  slabs by atoi, the three switches 1 where the value starts with '1'"""
  out = []
  for name in KNOB_ORDER:
    if name not in env:
      out.append(-1)
    elif name in ('MZ_FCL_GROUPS', 'MZ_FCL_SLABS'):
      out.append(int(env[name]))
    else:
      out.append(1 if env[name][:1] == '1' else 0)
  return (C.c_int * 5)(*out)


def plan_cases():
  """the rows of tests/golden/fcl_plan_parent.json: (batch, K, obs_dim, actions, Sv, Sr, knob set)"""
  rows = [(b, 5, o, a, 31, 31, 'none') for b in (16, 256, 272, 512, 528, 1024, 2048, 4096) for o, a in SHAPES]
  rows += [(b, 5, 8, 4, 31, 31, k) for b in (64, 256, 2048) for k in ('fuse_fb0', 'fuse_fwd0', 'fuse_fwd1', 'fb_jobs0', 'g2s2', 'g4s4', 's3')]
  rows += [(256, 5, 8, 4, 1, 1, 'none'), (16, 5, 1024, 4, 31, 31, 'none')]
  return rows


def plan_key(row):
  return 'b%d_K%d_O%d_A%d_S%d_%d_%s' % tuple(row)


def _names(buf):
  return [n for n in buf.value.decode().split('\n') if n]


def plan_host(lib, batch, K, O, A, Sv, Sr, cus, env, opt=0, scalar=0):
  """(record as a dict, kernel names) of mz_fcl_plan_host, or None where mz_fcl_create refuses the shape"""
  out, names = (C.c_longlong * len(FIELDS))(), C.create_string_buffer(2048)
  if lib.mz_fcl_plan_host(batch, K, O, A, Sv, Sr, cus, knobs_of(env), opt, scalar, out, names, len(names)) != 0:
    return None
  return dict(zip(FIELDS, out)), _names(names)


def plan_of(lib, handle, opt=0, scalar=0):
  from model_based_rl_amd import _abi
  out, names = (C.c_longlong * len(FIELDS))(), C.create_string_buffer(2048)
  _abi.check(lib.mz_fcl_plan(handle, opt, scalar, out, names, len(names)), 'mz_fcl_plan')
  return dict(zip(FIELDS, out)), _names(names)


def launched(names, S, clip):
  """of the kernels the resolver returns for a plan, the ones a step with an update launches: k_fcl_grad only with clipping,
  k_fcl_adam only where the update is not fused into the weight-gradient jobs (row slabs, or clipping)"""
  return [n for n in names if not (n == 'k_fcl_grad' and not clip) and not (n.startswith('k_fcl_adam<') and S == 1 and not clip)]


class knobs_set:
  """the knob set's variables in the process environment for the length of a `with` (mz_fcl_create reads them)"""

  def __init__(self, env):
    self.env = env

  def __enter__(self):
    self.old = {k: os.environ.get(k) for k in KNOB_ORDER}
    for k in KNOB_ORDER:
      os.environ.pop(k, None)
    os.environ.update(self.env)

  def __exit__(self, *exc):
    for k, v in self.old.items():
      os.environ.pop(k, None)
      if v is not None:
        os.environ[k] = v


# ---------------------------------------------------------------------------------------------- step cases
def step_cases():
  """(batch, knob set, actions, optimiser kind, scalar loss, clip_grad): the smallest batch that reaches each form of the step,
  thinned so that every kernel the resolver can return is launched by a case (test_fcl_plan_cpu asserts that)"""
  cases = [(16, 'none', a, ok, sc, 5.0 if (a == 7 and ok in (0, 6)) else 0.0) for a in (4, 7) for ok in OPT_KINDS for sc in (0, 1)]
  cases += [(16, 'fb_jobs0', 4, 0, 0, 0.0), (16, 'fb_jobs0', 7, 5, 1, 0.0), (16, 'fb_jobs0', 4, 2, 1, 5.0), (16, 'fb_jobs0', 7, 0, 0, 0.0)]
  cases += [(16, 'fuse_fb0', 4, 0, 0, 0.0), (16, 'fuse_fb0', 7, 1, 1, 0.0), (16, 'fuse_fb0', 4, 5, 1, 0.0), (16, 'fuse_fb0', 7, 2, 0, 0.0),
            (16, 'fuse_fb0', 4, 6, 0, 0.0), (16, 'fuse_fb0', 7, 0, 0, 5.0)]
  cases += [(16, 'fuse_fwd0', 4, 0, 0, 0.0), (16, 'fuse_fwd0', 7, 2, 1, 5.0), (16, 'fuse_fwd0', 7, 5, 0, 0.0)]
  cases += [(32, 'g2s2', 4, 0, 0, 0.0), (32, 'g2s2', 7, 1, 1, 5.0), (32, 'g2s2', 4, 5, 0, 0.0), (32, 'g2s2', 7, 2, 0, 0.0), (32, 'g2s2', 4, 6, 1, 5.0)]
  cases += [(64, 'g4s4', 4, 0, 0, 5.0), (64, 'g4s4', 7, 6, 1, 0.0)]
  # (row slabs with ONE group per chain workgroup -- k_fcl_chain_bwd4<1>, the step of batch 1024 -- is reached by none of the above)
  cases += [(32, 's2', 4, 1, 0, 0.0), (32, 's2', 7, 0, 1, 5.0)]
  return cases


def step_key(case):
  return 'b%d_%s_A%d_opt%d_sc%d_clip%g' % tuple(case)


K, OBS = 5, 8


def run_step_case(lib, case, device='cuda:0', check_plan=None):
  """two updates of a fixed seeded batch through mz_fcl_step on a fresh handle; the SHA-256 of the flat weights, both optimiser
  buffers, the step counters and, after each update, the new errors and the loss sums.  check_plan(handle, plan inputs): called
  on the created handle"""
  import torch
  from model_based_rl_amd import _abi
  batch, knobs, A, ok, sc, clip = case
  sup = (0, 0, 0, 0) if sc else (-15, 15, -15, 15)
  rng = np.random.Generator(np.random.PCG64(1234 + batch + 7 * A))
  h = C.c_void_p()
  with torch.cuda.device(device), knobs_set(KNOB_SETS[knobs]):
    _abi.check(lib.mz_fcl_create(batch, K, OBS, A, sup[0], sup[1], sup[2], sup[3], 0, C.byref(h)), 'mz_fcl_create')
  try:
    if check_plan is not None:
      check_plan(h, (batch, K, OBS, A, sup[1] - sup[0] + 1, sup[3] - sup[2] + 1), KNOB_SETS[knobs], ok, sc)
    if sc:
      _abi.check(lib.mz_fcl_set_scalar_loss(h, 1 + (A == 7)), 'mz_fcl_set_scalar_loss')      # (MSE at 4 actions, Huber at 7)
    _abi.check(lib.mz_fcl_set_optimizer(h, ok & 3, 0.9 if ok & 4 else 0.0, 0.99 if (ok & 3) == 2 else 0.0), 'mz_fcl_set_optimizer')
    n = lib.mz_fcl_num_params(h)
    dev = lambda x: torch.from_numpy(x).to(device)
    flat = dev((0.05 * rng.standard_normal(n)).astype(np.float32))
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    steps = torch.zeros(22, dtype=torch.float32, device=device)
    lr = torch.tensor(1e-3, dtype=torch.float32, device=device)
    obs = dev(rng.standard_normal((batch, OBS)).astype(np.float32))
    act = dev(rng.integers(0, A, (batch, K)).astype(np.int64))
    t_rew = dev(rng.uniform(-3, 3, (batch, K + 1)).astype(np.float32))
    t_val = dev(rng.uniform(-8, 8, (batch, K + 1)).astype(np.float32))
    pol = rng.random((batch, K + 1, A)) + 0.05
    t_pol = dev((pol / pol.sum(-1, keepdims=True)).astype(np.float32))
    w = dev(rng.uniform(0.1, 1.0, batch))
    errs = torch.zeros(batch, dtype=torch.float32, device=device)
    loss = torch.zeros(3, dtype=torch.float64, device=device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _abi.check(lib.mz_fcl_bind(h, ptr(flat), ptr(m), ptr(v), ptr(steps), 22, ptr(lr), stream), 'mz_fcl_bind')
    sha = hashlib.sha256()
    eps = 1e-8 if ok == 0 else 0.01
    for _ in range(2):
      _abi.check(lib.mz_fcl_step(h, ptr(obs), ptr(act), 0, ptr(t_rew), ptr(t_val), ptr(t_pol), ptr(w), 1, 0.9, 0.999, eps, 1e-4, clip, 1, 0,
                                 ptr(errs), ptr(loss), stream), 'mz_fcl_step')
      torch.cuda.synchronize(device)
      sha.update(errs.cpu().numpy().tobytes())
      sha.update(loss.cpu().numpy().tobytes())
    for t in (flat, m, v, steps):
      sha.update(t.cpu().numpy().tobytes())
    assert np.isfinite(flat.cpu().numpy()).all() and steps.cpu().numpy().any()
    return sha.hexdigest()
  finally:
    lib.mz_fcl_destroy(h)
