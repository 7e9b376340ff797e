"""The weight streams' gather tables without a GPU (csrc/mz_pack.inc, DESIGN s3.1):
  parent      mz_pack_host's record and tables equal, digest by digest, what mz_create built BEFORE pack_plan existed
              (tests/golden/pack_sha256.json; scripts/make_pack_goldens.py says how it was made)
  streams     what the kernels rely on, with numpy: the four waves' fused streams name every weight of the search's layers exactly once
              (but for the small MFMA's replicas) under one scale class, the split-f16 stream every weight once as a high and once as a
              low part, and every length is the schedule's own for the row
  sanitizers  tests/pack_host.cpp -- the packing's own file in a stand-alone program -- under AddressSanitizer + UBSan"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.pack_util import pack_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIONS = (1, 2, 4, 5, 6, 8, 9, 10, 13, 14, 16, 17, 21, 22, 32)      # both edges of every row of mz_kernels.inc
OBS = (1, 4, 27, 128, 257)
SUPPORTS = ((31, 31), (1, 1), (32, 32), (21, 5))                    # (1, 1): no_support
CASES = [(o, a, sv, sr, 1 if a <= 13 else 0) for a in ACTIONS for o in OBS for sv, sr in SUPPORTS]
# mz_kernels.inc: (largest action count, KS1, JTP, G)
ROWS = ((4, 14, 1, 4), (6, 14, 1, 8), (8, 15, 1, 8), (10, 15, 1, 16), (13, 16, 1, 16), (16, 18, 1, 16), (21, 18, 2, 32), (32, 21, 2, 32))
H, F = 50, 512


@pytest.fixture(scope='module')
def lib():
  from model_based_rl_amd import _abi
  _abi.build()
  return _abi.load()


@pytest.fixture(scope='module')
def plans(lib):
  """case -> (record, its dict, [idx, idx2, idx_h2]).  Built on demand and not kept: a case's tables are ~7 MB and pack_plan takes
  a few milliseconds"""
  return lambda case, tables=True: pack_host(lib, *case, tables=tables)


def test_tables_equal_what_create_built_before_the_plan(plans):
  with open(os.path.join(ROOT, 'tests', 'golden', 'pack_sha256.json')) as f:
    golden = json.load(f)['cases']
  assert sorted(golden) == sorted('O%d_A%d_Sv%d_Sr%d_h%d' % c for c in CASES) and len(CASES) == 300
  sha = lambda a: None if a is None else hashlib.sha256(a.tobytes()).hexdigest()
  for case in CASES:
    rec, _, (idx, idx2, idx_h2) = plans(case)
    got = {'record': sha(rec.astype('<i8')), 'idx': sha(idx), 'idx2': sha(idx2), 'idx_h2': sha(idx_h2)}
    assert got == golden['O%d_A%d_Sv%d_Sr%d_h%d' % case], case


def layout(O, A, Sv, Sr):
  """offsets of the 22 tensors in the flat vector (engine.WEIGHT_ORDER) -> ({name: (offset, rows, columns)}, total)"""
  K = H + A
  shapes = (('rep_w1', F, O), ('rep_b1', 1, F), ('rep_w2', H, F), ('rep_b2', 1, H), ('val_w1', F, H), ('val_b1', 1, F), ('val_w2', Sv, F),
            ('val_b2', 1, Sv), ('pol_w1', F, H), ('pol_b1', 1, F), ('pol_w2', A, F), ('pol_b2', 1, A), ('rew_w1', F, K), ('rew_b1', 1, F),
            ('rew_w2', Sr, F), ('rew_b2', 1, Sr), ('tr_w1', F, K), ('tr_b1', 1, F), ('tr_w2', H, F), ('tr_b2', 1, H), ('ln_w', 1, H), ('ln_b', 1, H))
  L, off = {}, 0
  for name, r, c in shapes:
    L[name] = (off, r, c)
    off += r * c
  return L, off


def test_fused_streams_name_every_weight_once_under_one_class(plans):
  for case in CASES:
    O, A, Sv, Sr, _ = case
    _, p, (idx, idx2, _) = plans(case)
    L, total = layout(O, A, Sv, Sr)
    assert total == p['n_flat'], case
    want = np.zeros(total, np.int64)      # how often an element sits in the four waves' streams (action tables included)
    cls = np.zeros(total, np.int64)       # ... and under which scale class
    for name, c in (('rew_w1', 1), ('tr_w1', 1), ('val_w1', 1), ('val_b1', 1), ('pol_w1', 1), ('pol_b1', 1), ('rew_w2', 2), ('tr_w2', 2),
                    ('val_w2', 2), ('pol_w2', 2)):
      off, r, k = L[name]
      want[off:off + r * k] = 1
      cls[off:off + r * k] = c
    # the small MFMA replicates its A operand across its four lane blocks: rows 48, 49 of the next hidden state; the policy head at A <= 4
    want[L['tr_w2'][0] + 48 * F:L['tr_w2'][0] + 50 * F] = 4
    if A <= 4:
      want[L['pol_w2'][0]:L['pol_w2'][0] + A * F] = 4
    s = idx[p['ws']:p['ws'] + 4 * p['wstride']]
    s2 = idx2[p['ws']:p['ws'] + 4 * p['wstride']]
    live = s >= 0
    el = s[live] & ((1 << 29) - 1)
    assert np.array_equal(np.bincount(el, minlength=total), want), case
    assert np.array_equal(s[live] >> 29, cls[el]), case
    # idx2: the row's fc1 bias on the dynamics' one-hot columns (the table's entries are such columns), -1 everywhere else
    K = H + A
    onehot = np.zeros(total, bool)
    bias = np.full(total, -1, np.int64)
    for w1, b1 in (('rew_w1', 'rew_b1'), ('tr_w1', 'tr_b1')):
      off = L[w1][0]
      e = np.arange(F * K)
      onehot[off:off + F * K] = e % K >= H
      bias[off:off + F * K] = np.where(e % K >= H, L[b1][0] + e // K, -1)
    assert np.all(s2[~live] == -1) and np.array_equal(s2[live], bias[el]), case
    # ... over the whole table too: only the fused kernel's dynamics fc1 pack and the streams carry a second element
    has2 = np.flatnonzero(idx2 >= 0)
    assert np.all((has2 >= p['w1f']) & (has2 < p['h4'])) and not np.any((has2 >= p['w3f']) & (has2 < p['ws'])), case
    assert np.all(idx[has2] >= 0) and np.array_equal(idx2[has2], bias[idx[has2] & ((1 << 29) - 1)]), case
    assert onehot[el].sum() == 2 * F * A, case


def test_split_stream_names_every_weight_once_high_and_once_low(plans):
  seen = 0
  for case in CASES:
    O, A, Sv, Sr, split = case
    _, p, (_, _, h2) = plans(case)
    if not split:
      assert h2 is None and p['n_packed_h2'] == 0
      continue
    seen += 1
    L, total = layout(O, A, Sv, Sr)
    want = np.zeros(total, np.int64)
    for head in ('rew', 'tr', 'val', 'pol'):
      for part in ('_w1', '_b1', '_w2'):
        off, r, k = L[head + part]
        want[off:off + r * k] = 1
    live = h2 >= 0
    el, low = h2[live] & ((1 << 29) - 1), (h2[live] >> 30) & 1
    assert np.all((h2[live] >> 29) & 1 == 0), case
    for part in (0, 1):
      assert np.array_equal(np.bincount(el[low == part], minlength=total), want), (case, part)
  assert seen == 9 * len(OBS) * len(SUPPORTS)


def test_lengths_are_the_schedules_own(plans):
  """FusedSched::NSTEPS, RootSched::NS and H2Sched::NGROUPS for the case's row, restated here from the kernels' descriptions: dynamics
  fc1 (13 steps with the action table, else the row's KS1) + 12 + 13 + 2 (2 + JTP) steps, the first RS resident, the others padded to the
  ring of 4; the root: (obs_dim + 1 columns, two k-steps per step) + 8 + 13 + 2 (2 + JTP); 25 groups"""
  for case in CASES:
    O, A, Sv, Sr, split = case
    _, p, _ = plans(case, tables=False)
    _, ks1, jtp, g = next(r for r in ROWS if A <= r[0])
    atab = (ks1, jtp, g) == (14, 1, 4)
    real = (13 if atab else ks1) + 12 + 13 + 2 * (2 + jtp)
    rs = 9 if jtp > 1 else (11 if ks1 > 16 else (12 if ks1 > 14 else 13))
    assert p['nsteps'] == rs + (real - rs + 3) // 4 * 4, case
    assert p['wstride'] == p['nsteps'] * 1024 + (1024 if atab else 0), case
    assert p['nst0'] == ((O + 1 + 3) // 4 + 1) // 2 and p['nroot'] == p['nst0'] + 8 + 13 + 2 * (2 + jtp), case
    assert p['ngroups'] == (25 if split else 0) and p['n_packed_h2'] == p['ngroups'] * 4 * 8 * 512, case
    assert (p['ks0'], p['ks1'], p['ks3']) == ((O + 3) // 4, (H + A + 3) // 4, 13), case


def test_refusals(lib):
  rec = np.zeros(29, np.int64)
  assert lib.mz_pack_host(8, 33, 31, 31, 0, rec.ctypes.data, 0, None, 0) != 0      # no row
  assert lib.mz_pack_host(8, 14, 31, 31, 1, rec.ctypes.data, 0, None, 0) != 0      # split-f16 covers action_space <= 13
  assert lib.mz_pack_host(1 << 20, 4, 31, 31, 0, rec.ctypes.data, 0, None, 0) != 0
  assert 'weights do not fit the gather index' in lib.mz_last_error().decode()
  small = np.zeros(16, np.int32)
  assert lib.mz_pack_host(8, 4, 31, 31, 0, rec.ctypes.data, 0, small.ctypes.data, 16) != 0


def test_plan_under_the_sanitizers(tmp_path):
  """tests/pack_host.cpp: the whole case grid through pack_plan itself, under AddressSanitizer + UBSan"""
  import subprocess
  exe = str(tmp_path / 'pack_host')
  cmd = ['hipcc', '-x', 'c++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
         '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'model-based-rl_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'pack_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.strip() == 'ok 300'
