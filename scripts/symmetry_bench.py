#!/usr/bin/env python3
"""What --symmetry costs the learner: updates/s through Learner.launch (the native loop, mz_fcl_run) at batch 256 and 2048 with the
TicTacToe and Connect Four shapes, each learner set up as bench_learner.setup wires it (replay filled by the product's Actor on the
device game), for three configurations:
  parent   this tree's Python on the PREVIOUS commit's library (--parent_lib PATH: a libmz_hip.so built from that commit; left out
           without it), flag off
  off      this commit, flag off
  on       this commit, --symmetry
Every figure comes from a child process of its own (one per configuration and game, both batch sizes in it; the median of RUNS timed
runs of 1000 updates after a warm-up), and the configurations take their turns in alternating blocks: parent, off, on, parent, ...
Per game, batch size and configuration: every block's figure, the median, the spread (max - min) / median; off / parent and on / off
with `within_spread` (off against the parent's own spread: a flag that is off must cost nothing; on against the larger of the two
spreads: one small launch per update is the flag's price).  The `on` children also time the kernel alone (HIP events around 200
mz_fcl_symmetry_apply launches on device arrays).

Prints one JSON line; --out FILE writes it too (profiles/symmetry_bench.json).

usage: python scripts/symmetry_bench.py [--blocks 5] [--runs 3] [--parent_lib PATH] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

BATCHES = (256, 2048)
GAMES = {'TicTacToe': ['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--td_steps', '10'],
         'ConnectFour': ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--td_steps', '10']}
UPDATES = 1000


def child(game, symmetry, runs):
  import contextlib
  import ctypes as C
  import numpy as np
  import torch
  import bench_learner
  out = {}
  with contextlib.redirect_stdout(sys.stderr):
    for bs in BATCHES:
      cfg, storage, replay, handle = bench_learner.setup(GAMES[game] + ['--batch_size', str(bs)] + (['--symmetry'] if symmetry else []))
      lrn = handle._obj
      lrn.launch(30)                                    # warm-up: builds the step
      assert lrn._native is not None and bool(lrn._native.sym_kind) == bool(symmetry)
      rates = []
      for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lrn.launch(UPDATES)
        torch.cuda.synchronize()
        rates.append(UPDATES / (time.perf_counter() - t0))
      point = {'updates_per_second': float(np.median(rates)), 'runs': rates, 'native_loop_updates': int(lrn.native_loop_updates)}
      if symmetry:                                      # the kernel alone
        nat = lrn._native
        lrn.flush_priorities()
        host = lrn._host_batch(getattr(replay, '_obj', replay).sample_batch_arrays())[0]
        dev = [torch.from_numpy(host[k]).to(nat.dev) for k in ('obs', 'act', 't_pol')]
        outs = [torch.empty_like(t) for t in dev]
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(nat.dev).cuda_stream)
        call = lambda: nat.lib.mz_fcl_symmetry_apply(nat.h, p(dev[0]), p(dev[1]), int(dev[1].dtype == torch.int32), p(dev[2]), 0, p(outs[0]),
                                                     p(outs[1]), p(outs[2]), None, stream)
        assert call() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(200):
          call()
        e1.record(); torch.cuda.synchronize()
        point['kernel_us'] = 1000.0 * e0.elapsed_time(e1) / 200
        point['kernel_bytes_moved'] = int(2 * sum(t.numel() * t.element_size() for t in dev))
      out[str(bs)] = point
      lrn._native.close()
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--blocks', type=int, default=5)
  ap.add_argument('--runs', type=int, default=3)
  ap.add_argument('--parent_lib', default=None, help='libmz_hip.so built from the previous commit')
  ap.add_argument('--out', default=None)
  ap.add_argument('--child', nargs=2, default=None, help=argparse.SUPPRESS)      # GAME on|off
  a = ap.parse_args()
  if a.child:
    return child(a.child[0], a.child[1] == 'on', a.runs)
  if a.blocks < 5:
    raise SystemExit('symmetry_bench: at least five blocks per configuration')
  configs = ([('parent', 'off', {'MZ_HIP_LIB': os.path.abspath(a.parent_lib), 'MZ_HIP_LIB_OLD': '1'})] if a.parent_lib else []) + \
            [('off', 'off', {}), ('on', 'on', {})]
  res = {g: {str(bs): {name: [] for name, _, _ in configs} for bs in BATCHES} for g in GAMES}
  kernel = {g: {str(bs): [] for bs in BATCHES} for g in GAMES}
  for game in GAMES:
    for block in range(a.blocks):
      for name, flag, env in configs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--runs', str(a.runs), '--child', game, flag], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:
          raise SystemExit('symmetry_bench: the %s child of %s ended with status %d' % (name, game, r.returncode))
        point = json.loads(r.stdout.strip().splitlines()[-1])
        print('symmetry_bench: %s block %d %s: %s' % (game, block, name, {bs: round(point[str(bs)]['updates_per_second']) for bs in BATCHES}),
              file=sys.stderr, flush=True)
        for bs in BATCHES:
          res[game][str(bs)][name].append(point[str(bs)]['updates_per_second'])
          if 'kernel_us' in point[str(bs)]:
            kernel[game][str(bs)].append(point[str(bs)]['kernel_us'])
            kernel_bytes = point[str(bs)]['kernel_bytes_moved']
            res[game][str(bs)]['kernel_bytes_moved'] = kernel_bytes
  med = lambda v: sorted(v)[len(v) // 2]
  out = {'blocks': a.blocks, 'runs': a.runs, 'updates_per_run': UPDATES, 'parent_lib': bool(a.parent_lib), 'games': {}}
  for game in GAMES:
    out['games'][game] = {}
    for bs in BATCHES:
      cell = res[game][str(bs)]
      point = {}
      for name, _, _ in configs:
        v = cell[name]
        point[name] = {'blocks': v, 'median': med(v), 'spread': (max(v) - min(v)) / med(v)}
      if 'parent' in point:
        point['off_vs_parent'] = point['off']['median'] / point['parent']['median']
        point['off_within_parents_spread'] = bool(abs(1.0 - point['off_vs_parent']) <= point['parent']['spread'])
      point['on_vs_off'] = point['on']['median'] / point['off']['median']
      point['on_within_spread'] = bool(1.0 - point['on_vs_off'] <= max(point['on']['spread'], point['off']['spread']))
      point['kernel_us'] = {'blocks': kernel[game][str(bs)], 'median': med(kernel[game][str(bs)])}
      point['kernel_bytes_moved'] = cell.get('kernel_bytes_moved')
      out['games'][game][str(bs)] = point
  line = json.dumps(out)
  print(line)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
  main()
