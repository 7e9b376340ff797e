#!/usr/bin/env python3
"""Reference goldens of the --no_support learner steps (TEST INFRASTRUCTURE, runs where the reference is mounted).

Two Learner.update_weights steps of the UNMODIFIED reference at the LunarLander bench shapes (seed 11, batch 256, K = 5, AdamW at
the reference's defaults) with --no_support (scalar value / reward heads trained with torch.nn.MSELoss, utils.py:61-70) and with
--no_support --scalar_loss Huber (SmoothL1Loss), through oracle/make_goldens.py's own gen_learner_synth, unchanged.  The batch is
that of g5_learner_lunar.npz -- checked here, and left out of the new files.  The initial weights (one-output heads: 167 630
parameters) are the same for both runs and equal what this repository's FCNetwork builds under --seed 0 -- both checked here; they are
stored once, in tests/golden/g9_learner_scalar_w0.npz.  g9_learner_mse_lunar.npz and g9_learner_huber_lunar.npz hold w1 and w2 as
ulp steps (make_optimizer_goldens.encode_step / decode_weights), losses, new_errors and the scalars gen_learner_synth records.
The archives are written with fixed member order and time stamps: a re-run writes byte-identical files.

usage: python scripts/make_scalar_loss_goldens.py [outdir]      (default tests/golden)"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_optimizer_goldens import LUNAR, SHARED, decode_weights, encode_step, mg, write_npz  # noqa: E402

RUNS = (('g9_learner_mse_lunar', ['--no_support']), ('g9_learner_huber_lunar', ['--no_support', '--scalar_loss', 'Huber']))
W0 = 'g9_learner_scalar_w0'


def own_initial_weights(O, A):
  """what this repository's FCNetwork holds under --seed 0 --no_support (train.py seeds torch before get_network)"""
  sys.path.insert(0, ROOT)
  import torch
  import model_based_rl_amd  # noqa: F401  (import alias)
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'LunarLander-v2', '--no_support', '--seed', '0'])
  cfg.obs_space, cfg.action_space = (O,), A
  torch.manual_seed(0)
  return {k: v.detach().numpy().copy() for k, v in get_network(cfg, torch.device('cpu')).state_dict().items()}


def main(outdir):
  mg._stand_in_modules()
  g5 = np.load(os.path.join(outdir, 'g5_learner_lunar.npz'))
  env_argv, O, A, bs, seed = LUNAR
  w0 = None
  for name, flags in RUNS:
    with tempfile.TemporaryDirectory() as tmp:
      mg.gen_learner_synth(tmp, name, env_argv + flags, O, A, bs, seed)
      got = dict(np.load(os.path.join(tmp, name + '.npz')))
    run_w0 = {k[3:]: v for k, v in got.items() if k.startswith('w0.')}
    if w0 is None:
      w0 = run_w0
      assert sum(v.size for v in w0.values()) == 167630
    assert set(run_w0) == set(w0) and all(np.array_equal(run_w0[k], w0[k]) for k in w0), '%s: other initial weights' % name
    out = {}
    for k, v in got.items():
      if k.startswith(SHARED):
        assert k in g5.files and np.array_equal(v, g5[k]) and v.dtype == g5[k].dtype, '%s: %s differs from g5_learner_lunar' % (name, k)
      elif k.startswith('w1.'):
        out['d1.' + k[3:]] = encode_step(w0[k[3:]], v)
        out['d2.' + k[3:]] = encode_step(v, got['w2.' + k[3:]])
      elif not k.startswith(('w0.', 'w2.')):
        out[k] = v
    assert all(('w1.' + k) in got and ('w2.' + k) in got for k in w0)
    path = os.path.join(outdir, name + '.npz')
    write_npz(path, out)
    back = decode_weights(np.load(path), w0)
    assert all(np.array_equal(back[k], got[k]) for k in back), 'the stored steps do not restore the weights'
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print('%s (%s): losses %s, %d bytes' % (name, ' '.join(flags), out['losses'], os.path.getsize(path)))
  own = own_initial_weights(O, A)
  assert list(own) == list(w0) and all(np.array_equal(own[k], w0[k]) and own[k].dtype == w0[k].dtype for k in w0), \
      'the reference\'s initial weights are not this repository\'s under --seed 0'
  path = os.path.join(outdir, W0 + '.npz')
  write_npz(path, {'w0.' + k: v for k, v in w0.items()})
  assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
  print('%s: %d parameters, %d bytes' % (W0, sum(v.size for v in w0.values()), os.path.getsize(path)))


if __name__ == '__main__':
  main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden'))
