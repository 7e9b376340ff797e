"""The learner step's plan without a GPU (csrc/mz_fcl_plan.inc, DESIGN s3.6):
  parent     mz_fcl_plan_host equals, field by field, what mz_fcl_create decided BEFORE the plan existed, on the committed cases at
             the CU count they were recorded with (tests/golden/fcl_plan_parent.json; tests/fcl_plan_util.py says how it was made)
  invariants over every multiple of 16 up to 1024, four CU counts and every knob set: what the step's code relies on
  coverage   every kernel name the resolver can return for any plan is launched by a step case of tests/test_gpu_fcl_plan.py
  sanitizers tests/fcl_plan_host.cpp -- the plan's own file in a stand-alone program -- under AddressSanitizer + UBSan"""
import json
import os

import pytest

from tests import fcl_plan_util as u


@pytest.fixture(scope='module')
def lib():
  from model_based_rl_amd import _abi
  _abi.build()
  return _abi.load()


def test_plan_equals_what_create_decided_before_the_plan(lib):
  with open(os.path.join(u.GOLDEN, 'fcl_plan_parent.json')) as f:
    golden = json.load(f)
  rows = u.plan_cases()
  assert sorted(golden) == sorted(u.plan_key(r) for r in rows) and len(rows) == 47
  for row in rows:
    batch, K, O, A, Sv, Sr, knobs = row
    want = golden[u.plan_key(row)]
    got = u.plan_host(lib, batch, K, O, A, Sv, Sr, want['cus'], u.KNOB_SETS[knobs])
    assert got is not None, row
    assert {f: got[0][f] for f in u.PARENT_FIELDS} == {f: want[f] for f in u.PARENT_FIELDS}, row
    assert got[0]['cus'] == want['cus']
  # the cases reach both instantiations of the transition's input and every form of the step
  seen = [golden[u.plan_key(r)] for r in rows]
  assert {g['KP'] for g in seen} == {56, 64} and {g['G'] for g in seen} == {1, 2, 4}
  assert {(g['fuse_fwd'], g['fuse_fb'], g['S'] > 1) for g in seen} == {(1, 1, False), (1, 0, False), (0, 0, False), (0, 0, True)}


GRID = [(b, o, a, cus, k) for b in range(16, 1025, 16) for o, a in u.SHAPES for cus in (64, 128, 256, 304) for k in u.KNOB_SETS]


@pytest.fixture(scope='module')
def grid(lib):
  """per grid point the plan's record"""
  out = {}
  for b, o, a, cus, k in GRID:
    got = u.plan_host(lib, b, 5, o, a, 31, 31, cus, u.KNOB_SETS[k])
    assert got is not None, (b, o, a, cus, k)      # (mz_fcl_create accepts all of these)
    out[b, o, a, cus, k] = got[0]
  return out


def test_invariants_the_step_relies_on(grid):
  for key, p in grid.items():
    batch = key[0]
    assert p['nwg'] * 4 * p['G'] == batch and p['nln'] * 4 == batch, key
    assert p['S'] != 1 or p['G'] == 1, key
    assert not p['fuse_fb'] or p['fuse_fwd'], key
    assert max(p['lds_bytes'], p['lds_bwd_dw'], p['lds_dwa']) <= 160 * 1024, key
    assert 0 < p['njobs_heads'] <= p['njobs'], key
    assert (p['fwd'], p['bwd']) in ((0, 0), (1, 1), (2, 1), (2, 2)) and (p['bwd'] == 2) == (p['S'] > 1), key
    assert p['fuse_fwd'] == (p['fwd'] != 2) and p['fuse_fb'] == (p['fwd'] == 0), key


def test_refused_shapes_are_refused_with_creates_words(lib):
  from model_based_rl_amd import _abi
  for args, word in (((24, 5, 8, 4, 31, 31), 'multiple of 16'), ((16, 8, 8, 4, 31, 31), 'unroll steps'), ((16, 5, 8, 15, 31, 31), 'actions'),
                     ((16, 5, 8, 4, 65, 31), 'bins'), ((16, 5, 1025, 4, 31, 31), 'observation features')):
    assert u.plan_host(lib, *args, 256, {}) is None
    assert word in lib.mz_last_error().decode() and lib.mz_last_error().decode().startswith('mz_fcl_create: ')


def test_every_kernel_the_resolver_can_return_is_launched_by_a_step_case(lib, grid):
  """the universe: the names over the whole grid, the large default batches and both supports' widths, under all ten (optimiser kind,
  loss form); a step case launches what the resolver returns for ITS plan at the MI355X's 256 CUs, less the kernels its clipping
  setting leaves out (fcl_plan_util.launched)"""
  points = [(b, o, a, cus, k, 31) for b, o, a, cus, k in GRID if b % 64 == 16 or b in (256, 512, 1024)]
  points += [(b, o, a, 256, 'none', s) for b in (2048, 4096) for o, a in u.SHAPES for s in (31, 1)]
  universe = set()
  for b, o, a, cus, k, s in points:
    for ok in u.OPT_KINDS:
      for sc in (0, 1):
        universe |= set(u.plan_host(lib, b, 5, o, a, s, s, cus, u.KNOB_SETS[k], ok, sc)[1])
  assert len(universe) == 57, sorted(universe)      # 20 k_fcl_fb, 4 k_fcl_fwd, 6 k_fcl_chain_fwd4, 2 heads, 5 k_fcl_bwd_dw, 10 k_fcl_dwa, 3 k_fcl_chain_bwd4, k_fcl_dwt, k_fcl_grad, 5 k_fcl_adam
  covered = set()
  for case in u.step_cases():
    batch, knobs, a, ok, sc, clip = case
    s = 1 if sc else 31
    plan, names = u.plan_host(lib, batch, u.K, u.OBS, a, s, s, 256, u.KNOB_SETS[knobs], ok, sc)
    covered |= set(u.launched(names, plan['S'], clip))
  assert universe <= covered, sorted(universe - covered)


def test_step_cases_have_their_digests():
  with open(os.path.join(u.GOLDEN, 'fcl_plan_sha256.json')) as f:
    golden = json.load(f)
  keys = [u.step_key(c) for c in u.step_cases()]
  assert len(set(keys)) == len(keys) and sorted(keys) == sorted(golden)


def test_plan_under_the_sanitizers(tmp_path):
  """tests/fcl_plan_host.cpp: the wide grid through fcl_plan itself, under AddressSanitizer + UBSan"""
  import subprocess
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  exe = str(tmp_path / 'fcl_plan_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(root, 'include'),
         '-I', os.path.join(root, 'model-based-rl_amd', 'csrc'), os.path.join(root, 'tests', 'fcl_plan_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.startswith('ok ')
