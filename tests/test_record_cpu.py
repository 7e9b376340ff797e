"""The experience record's one statement (include/mz_record.h) against everything that repeats it, without a GPU.

tests/record_host.cpp writes records through the C++ accessors (csrc/mz_record.h) in a stand-alone program under AddressSanitizer +
UBSan and prints each row's words.  Here the rows are decoded with THE OFFSETS WRITTEN OUT -- this file is the one pin of the
numbers outside the header -- and with record.records_view, bit for bit against what went in; record.records_fill writes the same
rows again.  The header's #defines are held to the Python module's constants and to what the two public headers expose."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def host_rows(tmp_path_factory):
  """the rows tests/record_host.cpp printed: a list of dicts of inputs and the row's words"""
  exe = str(tmp_path_factory.mktemp('record_host') / 'record_host')
  cmd = ['hipcc', '-x', 'c++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Xarch_host', '-fsanitize=address,undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'model-based-rl_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'record_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  lines = run.stdout.splitlines()
  assert lines[-1] == 'ok %d' % (len(lines) - 1)
  rows = []
  for line in lines[:-1]:
    head, scal, obs, cv, words = [p.split() for p in line.split('|')]
    assert head[0] == 'row'
    h = lambda x: int(x, 16)
    rows.append(dict(O=int(head[1]), packed=bool(int(head[2])), A=int(head[3]), flags=h(scal[0]), action=h(scal[1]), step=h(scal[2]),
                     env_id=h(scal[3]), episode=h(scal[4]), reward=h(scal[5]), root_value=h(scal[6]), error=h(scal[7]),
                     obs=[h(x) for x in obs], child_visits=[h(x) for x in cv], words=np.array([h(x) for x in words], np.uint32)))
  return rows


def test_the_host_program_covers_the_cases(host_rows):
  shapes = {(r['O'], r['packed'], r['A']) for r in host_rows}
  assert shapes == {(O, p, A) for O in (1, 3, 4, 5, 9, 128) for p in (False, True) for A in (2, 7, 18)}
  f64 = lambda v: int(np.array([v], np.float64).view(np.uint64)[0])
  specials = {f64(0.0), f64(-0.0), 5, f64(1e300), 0x7ff8dead0000beef}      # 0.0, -0.0, a denormal, 1e300, a NaN with a payload
  for s in shapes:
    mine = [r for r in host_rows if (r['O'], r['packed'], r['A']) == s]
    assert {r['flags'] for r in mine} == {0, 1, 2, 3}
    assert {r['root_value'] for r in mine} == specials and {r['error'] for r in mine} == specials
    assert {(r['flags'], r['root_value']) for r in mine} == {(f, v) for f in range(4) for v in specials}
    assert any(r['action'] == 2 ** 31 - 1 for r in mine) and any(r['episode'] == 2 ** 31 - 1 for r in mine)
    assert any(r['env_id'] == 2 ** 31 - 1 for r in mine)


def test_rows_decode_with_the_offsets_written_out(host_rows):
  """obs | child_visits[A] | root_value f64 | error f64 | reward | action, flags, step, env_id, episode: the literal numbers"""
  for r in host_rows:
    O, A, w = r['O'], r['A'], r['words']
    OS = (O + 3) // 4 if r['packed'] else O
    assert len(w) == OS + A + 10
    if r['packed']:
      by = w[:OS].view(np.uint8)
      assert list(by[:O]) == r['obs'] and not by[O:].any()      # four bytes per slot, low byte first; the last slot's rest is 0
    else:
      assert list(w[:O]) == r['obs']
    assert list(w[OS:OS + A]) == r['child_visits']
    t = OS + A
    assert int(w[t + 0]) | int(w[t + 1]) << 32 == r['root_value']      # float64, low word first
    assert int(w[t + 2]) | int(w[t + 3]) << 32 == r['error']
    assert w[t + 4] == r['reward']
    assert (w[t + 5], w[t + 6], w[t + 7], w[t + 8], w[t + 9]) == (r['action'], r['flags'], r['step'], r['env_id'], r['episode'])


def _by_shape(rows):
  out = {}
  for r in rows:
    out.setdefault((r['O'], r['packed'], r['A']), []).append(r)
  return out


def test_records_view_and_records_fill_agree_with_the_host_rows(host_rows):
  from model_based_rl_amd.record import rec_floats, records_fill, records_view
  for (O, packed, A), rows in _by_shape(host_rows).items():
    rec = np.stack([r['words'] for r in rows]).view(np.float32)
    assert rec.shape == (len(rows), rec_floats(O, A, packed))
    col = lambda k, dt: np.array([r[k] for r in rows], dt)
    v = records_view(rec, O, A, packed)
    want_obs = np.array([r['obs'] for r in rows], np.uint8 if packed else np.uint32)
    assert np.array_equal(v['obs'] if packed else v['obs'].view(np.uint32), want_obs)
    assert np.array_equal(v['child_visits'].view(np.uint32), np.array([r['child_visits'] for r in rows], np.uint32))
    assert np.array_equal(v['root_value'].view(np.uint64), col('root_value', np.uint64))
    assert np.array_equal(v['error'].view(np.uint64), col('error', np.uint64))
    assert np.array_equal(np.ascontiguousarray(v['reward']).view(np.uint32), col('reward', np.uint32))
    for k in ('action', 'step', 'env_id', 'episode'):
      assert v[k].dtype == np.int32 and np.array_equal(v[k], col(k, np.int64)), k
    flags = col('flags', np.int32)
    assert np.array_equal(v['done'], flags & 1) and np.array_equal(v['to_play'], np.where(flags & 2, -1, 1))
    # the writer: the same inputs give the same words; and what it wrote reads back through the view
    out = np.full_like(rec, -7.0)
    got = records_fill(out, O, A, packed, obs=want_obs if packed else want_obs.view(np.float32),
                       child_visits=np.array([r['child_visits'] for r in rows], np.uint32).view(np.float32),
                       root_value=col('root_value', np.uint64).view(np.float64), error=col('error', np.uint64).view(np.float64),
                       reward=col('reward', np.uint32).view(np.float32), action=col('action', np.int32), flags=flags,
                       step=col('step', np.int32), env_id=col('env_id', np.int32), episode=col('episode', np.int32))
    assert got is out
    if packed and O % 4:      # (records_fill writes the O bytes it is given; the host program zeroes the last slot's rest)
      out.view(np.uint8)[:, O:4 * ((O + 3) // 4)] = 0
    assert np.array_equal(out.view(np.uint32), rec.view(np.uint32))
    back = records_view(out, O, A, packed)
    assert all(np.array_equal(np.ascontiguousarray(back[k]).view(np.uint8), np.ascontiguousarray(v[k]).view(np.uint8)) for k in v)


def test_records_fill_leaves_fields_not_given_and_takes_torch_tensors():
  import torch
  from model_based_rl_amd.record import rec_floats, records_fill, records_view
  O, A, n = 5, 3, 4
  rng = np.random.RandomState(0)
  for packed in (False, True):
    kw = dict(obs=rng.randint(0, 256, (n, O)).astype(np.uint8 if packed else np.float32), child_visits=rng.rand(n, A).astype(np.float32),
              root_value=rng.standard_normal(n), error=rng.standard_normal(n), reward=rng.rand(n).astype(np.float32),
              action=rng.randint(0, A, n).astype(np.int32), flags=np.array([0, 1, 2, 3], np.int32), step=np.arange(n, dtype=np.int32),
              env_id=np.arange(n, dtype=np.int32) + 7, episode=np.full(n, 3, np.int32))
    full = records_fill(np.zeros((n, rec_floats(O, A, packed)), np.float32), O, A, packed, **kw)
    t = records_fill(torch.zeros(n, rec_floats(O, A, packed)), O, A, packed, **{k: torch.from_numpy(x) for k, x in kw.items()})
    assert np.array_equal(t.numpy().view(np.uint32), full.view(np.uint32))
    part = records_fill(np.full_like(full, 9.0), O, A, packed, error=kw['error'], flags=kw['flags'])
    v = records_view(part, O, A, packed)
    assert np.array_equal(v['error'], kw['error']) and np.array_equal(v['done'], kw['flags'] & 1)
    untouched = np.ones(part.shape[1], bool)
    OS = (O + 3) // 4 if packed else O
    untouched[[OS + A + 2, OS + A + 3, OS + A + 6]] = False
    assert np.all(part[:, untouched] == 9.0)


def _defines(path):
  text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
  return {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define\s+(\w+)\s+(\d+)\s*$', text, re.M)}


def test_constants_of_the_header_the_module_and_the_public_headers(tmp_path):
  from model_based_rl_amd import record
  d = _defines(os.path.join(ROOT, 'include', 'mz_record.h'))
  assert d == dict(MZ_REC_ROOT_VALUE=0, MZ_REC_ERROR=2, MZ_REC_REWARD=4, MZ_REC_ACTION=5, MZ_REC_FLAGS=6, MZ_REC_STEP=7, MZ_REC_ENV_ID=8,
                   MZ_REC_EPISODE=9, MZ_REC_EXTRA=10, MZ_REC_FLAG_DONE=1, MZ_REC_FLAG_P2=2)
  for name in ('ROOT_VALUE', 'ERROR', 'REWARD', 'ACTION', 'FLAGS', 'STEP', 'ENV_ID', 'EPISODE', 'FLAG_DONE', 'FLAG_P2'):
    assert getattr(record, name) == d['MZ_REC_' + name], name
  assert record.REC_EXTRA == d['MZ_REC_EXTRA']
  # what the two public headers expose, and the width formula, as C computes them
  shapes = [(O, A, p) for O in (1, 3, 4, 5, 9, 128) for A in (2, 18) for p in (0, 1)]
  widths = ''.join('printf(" %%d %%d", MZ_REC_OBS_SLOTS(%d, %d), MZ_REC_FLOATS(%d, %d, %d));' % (O, p, O, A, p) for O, A, p in shapes)
  src = '#include <stdio.h>\n#include "HEADER"\nint main(void){printf("%d %d", NAME, MZ_REC_EXTRA);' + widths + 'return 0;}\n'
  for header, name in (('mz_engine.h', 'MZ_REC_EXTRA'), ('mz_replay.h', 'MZR_REC_EXTRA')):
    exe = str(tmp_path / ('extra_' + name))
    subprocess.run(['gcc', '-std=c99', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe], input=src.replace('HEADER', header).replace('NAME', name).encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[:2] == [record.REC_EXTRA, record.REC_EXTRA], header
    assert got[2:] == [f for O, A, p in shapes for f in (record.obs_slots(O, bool(p)), record.rec_floats(O, A, bool(p)))], header
  subprocess.check_call(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'mz_record.h')])      # plain C
  from model_based_rl_amd import engine
  assert engine.records_view is record.records_view and engine.REC_EXTRA == record.REC_EXTRA
