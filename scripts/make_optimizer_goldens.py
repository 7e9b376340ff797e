#!/usr/bin/env python3
"""Reference goldens of the SGD and RMSprop learner steps (TEST INFRASTRUCTURE, runs where the reference is mounted).

Two Learner.update_weights steps of the UNMODIFIED reference at the LunarLander bench shapes (seed 11, batch 256, K = 5, the
reference's defaults: lr 0.0008, momentum 0.9, weight decay 1e-4), once with --optimizer SGD and once with --optimizer RMSprop,
through oracle/make_goldens.py's own gen_learner_synth (its stand-in modules for ray / gym / cv2 / tensorboard, the direct
FCNetwork construction).  The initial weights and the batch are those of g5_learner_lunar.npz -- checked here, and left out of the
new files: tests/golden/g8_learner_sgd_lunar.npz and g8_learner_rmsprop_lunar.npz hold w1 and w2, losses, new_errors and the
scalars gen_learner_synth records.  The weights are stored losslessly as steps, to stay under the 1 MiB a committed file may take
(plain, the two weight sets are 1.5 MB): d1.<name> / d2.<name> are the int32 differences of the float32 bit patterns w1 - w0 and
w2 - w1 (a weight's step in ulps), as four byte planes [4][n] (uint8), LZMA-compressed; decode_weights() below restores them.
The archives are written with fixed member order and time stamps: a re-run writes byte-identical files.

usage: python scripts/make_optimizer_goldens.py [outdir]      (default tests/golden)"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import make_goldens as mg  # noqa: E402

RUNS = (('g8_learner_sgd_lunar', 'SGD'), ('g8_learner_rmsprop_lunar', 'RMSprop'))
SHARED = ('sample_',)          # the batch: equal to g5's, left out
LUNAR = (['--environment', 'LunarLander-v2'], 8, 4, 256, 11)


def write_npz(path, arrays):
  """an .npz (np.load reads it) with sorted members, a fixed date and LZMA (numpy stamps the current time into every member)"""
  with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_LZMA) as zf:
    for k in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
      info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_LZMA
      info.external_attr = 0o644 << 16
      zf.writestr(info, buf.getvalue())


def encode_step(a, b):
  """b - a in ulps (int32 difference of the float32 bit patterns; wraps), as byte planes [4][n]"""
  d = b.astype(np.float32).reshape(-1).view(np.int32) - a.astype(np.float32).reshape(-1).view(np.int32)
  return np.ascontiguousarray(d.view(np.uint8).reshape(-1, 4).T)


def decode_weights(g8, w0):
  """{w1.<name>, w2.<name>} of a g8 file from w0 = {name: float32 array} (g5_learner_lunar's w0.*)"""
  out = {}
  for name, a in w0.items():
    prev = np.asarray(a, np.float32)
    for t in (1, 2):
      d = np.ascontiguousarray(g8['d%d.%s' % (t, name)].T).view(np.int32).reshape(-1)
      prev = (prev.reshape(-1).view(np.int32) + d).view(np.float32).reshape(prev.shape)
      out['w%d.%s' % (t, name)] = prev
  return out


def main(outdir):
  mg._stand_in_modules()
  g5 = np.load(os.path.join(outdir, 'g5_learner_lunar.npz'))
  env_argv, O, A, bs, seed = LUNAR
  for name, opt in RUNS:
    with tempfile.TemporaryDirectory() as tmp:
      mg.gen_learner_synth(tmp, name, env_argv + ['--optimizer', opt], O, A, bs, seed)
      got = dict(np.load(os.path.join(tmp, name + '.npz')))
    out = {}
    for k, v in got.items():
      if k.startswith('w0.') or k.startswith(SHARED):
        assert k in g5.files and np.array_equal(v, g5[k]) and v.dtype == g5[k].dtype, '%s: %s differs from g5_learner_lunar' % (name, k)
      elif k.startswith('w1.'):
        out['d1.' + k[3:]] = encode_step(g5['w0.' + k[3:]], v)
        out['d2.' + k[3:]] = encode_step(v, got['w2.' + k[3:]])
      elif not k.startswith('w2.'):
        out[k] = v
    w0 = {k[3:]: g5[k] for k in g5.files if k.startswith('w0.')}
    assert all(('w1.' + k) in got and ('w2.' + k) in got for k in w0)
    path = os.path.join(outdir, name + '.npz')
    write_npz(path, out)
    back = decode_weights(np.load(path), w0)
    assert all(np.array_equal(back[k], got[k]) for k in back), 'the stored steps do not restore the weights'
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print('%s (--optimizer %s): losses %s, %d bytes' % (name, opt, out['losses'], os.path.getsize(path)))


if __name__ == '__main__':
  main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden'))
