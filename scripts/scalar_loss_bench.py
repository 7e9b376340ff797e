#!/usr/bin/env python3
"""The learner under --no_support (scalar value / reward heads, --scalar_loss MSE or Huber; utils.py:61-70) at batch 256 and 2048,
LunarLander shapes, each learner set up as bench_learner.setup wires it (replay filled by the product's Actor).  Only the public
Learner surface is used, so the same script runs on a commit whose native step does not take --no_support (there every figure is
that of the PyTorch step the flag then selects, and part (a) is left out).

(a) GPU microseconds per update (HIP events around 50 _native.launch calls: kernels only) of the native MSE and Huber steps against
    the native categorical step, in the same process, in alternating blocks (categorical, MSE, Huber, categorical, ...).  Per batch
    size: every block's figure, the medians, their ratios to the categorical median, and the spread of the repeated categorical
    blocks ((max - min) / median) -- the scalar heads do less work, so a ratio should not exceed 1 by more than that spread
    ("within_spread").
(b) updates/s through Learner.launch with --no_support (the median of RUNS runs; 1000 updates on the native step, 200 on a PyTorch
    step), as the commit runs it by default and with --no_native_learner.

Prints one JSON line (profiles/learner_scalar_loss.json holds this commit's line and, under "parent", the previous commit's).

usage: python scripts/scalar_loss_bench.py [runs] [blocks]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import bench_learner  # noqa: E402

BATCHES = (256, 2048)
VARIANTS = (('categorical', []), ('MSE', ['--no_support']), ('Huber', ['--no_support', '--scalar_loss', 'Huber']))


def timed(learner, n):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  learner.launch(n)
  torch.cuda.synchronize()
  return n / (time.perf_counter() - t0)


def gpu_us(learner, host, n=50):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  learner._native.launch(host)
  torch.cuda.synchronize(); e0.record()
  for _ in range(n):
    learner._native.launch(host)
  e1.record(); torch.cuda.synchronize()
  return 1000.0 * e0.elapsed_time(e1) / n


def main(runs, blocks):
  import contextlib
  out = {'runs': runs, 'blocks': blocks, 'gpu_us_per_update': {}, 'updates_per_second': {}}
  with contextlib.redirect_stdout(sys.stderr):
    for bs in BATCHES:
      made = {}
      for name, flags in VARIANTS:
        cfg, storage, replay, handle = bench_learner.setup(flags + ['--batch_size', str(bs)])
        lrn = handle._obj
        lrn.launch(30)                                    # warm-up: builds the step
        made[name] = (lrn, getattr(replay, '_obj', replay))
      native = all(getattr(l, '_native', None) is not None for l, _ in made.values())
      # (b) the default path of --no_support, the variants taking their runs in turn
      rates = {name: [] for name in made}
      for _ in range(runs):
        for name, (lrn, rep) in made.items():
          rates[name].append(timed(lrn, 1000 if getattr(lrn, '_native', None) is not None else 200))
      for name, (lrn, rep) in made.items():
        out['updates_per_second']['%s_%d' % (name, bs)] = {
            'updates_per_second': float(np.median(rates[name])), 'runs': rates[name],
            'step': 'native' if getattr(lrn, '_native', None) is not None else ('graph' if getattr(lrn, '_graph', None) is not None else 'eager'),
            'native_loop_updates': int(getattr(lrn, 'native_loop_updates', 0))}
      # (a) kernels only, alternating blocks
      if native:
        hosts = {}
        for name, (lrn, rep) in made.items():
          lrn.flush_priorities()
          hosts[name] = lrn._host_batch(rep.sample_batch_arrays())[0]
        us = {name: [] for name in made}
        for _ in range(blocks):
          for name, (lrn, rep) in made.items():
            us[name].append(gpu_us(lrn, hosts[name]))
        for lrn, rep in made.values():
          lrn.flush_priorities()
        med = {name: float(np.median(v)) for name, v in us.items()}
        spread = (max(us['categorical']) - min(us['categorical'])) / med['categorical']
        point = {'blocks': us, 'median': med, 'categorical_spread': spread}
        for name in ('MSE', 'Huber'):
          point['%s_vs_categorical' % name] = med[name] / med['categorical']
        point['within_spread'] = all(point['%s_vs_categorical' % n] <= 1.0 + spread for n in ('MSE', 'Huber'))
        out['gpu_us_per_update'][str(bs)] = point
      for lrn, rep in made.values():
        if getattr(lrn, '_native', None) is not None:
          lrn._native.close()
      made.clear()
      # (b) ... and with --no_native_learner (the captured PyTorch graph)
      for name, flags in VARIANTS[1:]:
        cfg, storage, replay, handle = bench_learner.setup(flags + ['--batch_size', str(bs), '--no_native_learner'])
        lrn = handle._obj
        lrn.launch(10)
        assert lrn._native is None
        r = [timed(lrn, 200) for _ in range(runs)]
        out['updates_per_second']['%s_%d_no_native_learner' % (name, bs)] = {
            'updates_per_second': float(np.median(r)), 'runs': r, 'step': 'graph' if lrn._graph is not None else 'eager'}
  if not out['gpu_us_per_update']:
    out['gpu_us_per_update'] = 'not measured: --no_support does not take the native step on this commit'
  print(json.dumps(out))


if __name__ == '__main__':
  main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
