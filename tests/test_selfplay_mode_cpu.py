"""The self-play loop's search mode without a GPU (csrc/mz_selfplay_mode.inc, DESIGN s7l): tests/selfplay_mode_host.cpp -- the file of
the mode table, the refusal sentence and the switch decision in a stand-alone program, held to a flat restatement of the rules over
every combination of the facts -- under AddressSanitizer + UBSan."""
import os
import subprocess


def test_mode_switches_and_sentences_under_the_sanitizers(tmp_path):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  exe = str(tmp_path / 'selfplay_mode_host')
  # (hipcc as the host compiler on plain C++, like tests/test_selfplay_ring_cpu.py: no HIP header can come in; the sanitizers are the host's alone)
  cmd = ['hipcc', '-x', 'c++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
         '-I', os.path.join(root, 'model-based-rl_amd', 'csrc'),
         os.path.join(root, 'tests', 'selfplay_mode_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.startswith('ok ')
