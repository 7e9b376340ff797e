#!/usr/bin/env python3
"""The learner's optimisers on the native step: AdamW, SGD and RMSprop (utils.py:73-83, the reference's defaults: momentum 0.9,
weight decay 1e-4) at batch 256 and 2048, LunarLander shapes, each learner set up as bench_learner.setup wires it (replay filled by
the product's Actor).  Per variant: updates/s through Learner.launch (the median of RUNS runs of 1000 updates; the variants take
their runs in turn, so that a drift of the machine spreads over all of them) and GPU microseconds per update (HIP events around 50
_native.launch calls).  SGD and RMSprop also on their eager PyTorch step (--no_native_learner: what they ran before the native
step took them; 200 updates).  Prints one JSON line (profiles/learner_optimizers.json).

usage: python scripts/optimizer_bench.py [runs]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import bench_learner  # noqa: E402

OPTS = ('AdamW', 'SGD', 'RMSprop')
BATCHES = (256, 2048)


def timed(learner, n):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  learner.launch(n)
  torch.cuda.synchronize()
  return n / (time.perf_counter() - t0)


def gpu_us(learner, replay):
  host = learner._host_batch(replay.sample_batch_arrays())[0]
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  learner._native.launch(host)
  torch.cuda.synchronize(); e0.record()
  for _ in range(50):
    learner._native.launch(host)
  e1.record(); torch.cuda.synchronize()
  learner.flush_priorities()
  return 1000.0 * e0.elapsed_time(e1) / 50


def main(runs):
  import contextlib
  out = {'runs': runs, 'updates_per_run': 1000, 'native': {}, 'eager': {}}
  with contextlib.redirect_stdout(sys.stderr):
    native = {}
    for bs in BATCHES:
      for opt in OPTS:
        cfg, storage, replay, handle = bench_learner.setup(['--optimizer', opt, '--batch_size', str(bs)])
        lrn = handle._obj
        lrn.launch(30)                                    # warm-up: builds the native step
        assert lrn._native is not None, (opt, bs)
        native[(opt, bs)] = (lrn, getattr(replay, '_obj', replay), [])
    for _ in range(runs):
      for key, (lrn, rep, rates) in native.items():
        rates.append(timed(lrn, 1000))
    for (opt, bs), (lrn, rep, rates) in native.items():
      out['native']['%s_%d' % (opt, bs)] = {'updates_per_second': float(np.median(rates)), 'runs': rates, 'gpu_us_per_update': gpu_us(lrn, rep),
                                             'native_loop_updates': lrn.native_loop_updates}
      lrn._native.close()
    native.clear()
    for bs in BATCHES:
      for opt in OPTS[1:]:
        cfg, storage, replay, handle = bench_learner.setup(['--optimizer', opt, '--batch_size', str(bs), '--no_native_learner'])
        lrn = handle._obj
        lrn.launch(10)
        assert lrn._native is None and lrn._graph is None
        out['eager']['%s_%d' % (opt, bs)] = {'updates_per_second': timed(lrn, 200)}
  for bs in BATCHES:
    base = out['native']['AdamW_%d' % bs]['gpu_us_per_update']
    for opt in OPTS[1:]:
      k = '%s_%d' % (opt, bs)
      out['native'][k]['gpu_us_vs_adamw'] = out['native'][k]['gpu_us_per_update'] / base
      out['native'][k]['speedup_over_eager'] = out['native'][k]['updates_per_second'] / out['eager'][k]['updates_per_second']
  print(json.dumps(out))


if __name__ == '__main__':
  main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
