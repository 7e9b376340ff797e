"""The self-play ring's bookkeeping without a GPU (csrc/mz_selfplay_ring.inc, DESIGN s2): tests/selfplay_ring_host.cpp -- the struct's
own file in a stand-alone program, held to a brute-force model of the drains' reads -- under AddressSanitizer + UBSan."""
import os
import subprocess


def test_ring_bookkeeping_under_the_sanitizers(tmp_path):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  exe = str(tmp_path / 'selfplay_ring_host')
  # (hipcc as the host compiler, like tests/test_fcl_plan_cpu.py, but on plain C++: no HIP header can come in; the sanitizers are
  # the host's alone)
  cmd = ['hipcc', '-x', 'c++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
         '-I', os.path.join(root, 'model-based-rl_amd', 'csrc'),
         os.path.join(root, 'tests', 'selfplay_ring_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.startswith('ok ')
