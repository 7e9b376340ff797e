"""Rate of MuZero Reanalyse (reanalyse.Reanalyser.run: replay pick -> Engine.reanalyse, whole chunks enqueued -> replay write)
beside the same work done step by step from Python on the same engine (pick, then per chunk initial_inference / root_prepare /
search / finalize with host copies, then write), and the self-play rate of the same build for scale; writes
profiles/reanalyse_bench.json.

LunarLander shapes (obs 8, actions 4), B = 4096, 30 simulations.  Every measurement is a child process of its own (a fresh
engine and a fresh replay filled by 64 self-play moves with --max_history_length 32, so that slices with ignored tails exist);
the three kinds of block alternate (chunked, stepwise, selfplay, chunked, ...) at least five times.  A block times three passes
of 16 chunks (65536 rows) after one unmeasured pass and reports their median; the file has, per kind, the median of the blocks
with minimum and maximum.  There is no pass mark: the figures are recorded as they come out.

usage: python scripts/reanalyse_bench.py [--blocks 5] [--out profiles/reanalyse_bench.json]
       python scripts/reanalyse_bench.py --not_measured     (no GPU time: the file then says so)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SIMS, CHUNKS, PASSES = 4096, 30, 16, 3
FLAGS = ['--environment', 'LunarLander-v2', '--num_envs', str(B), '--num_simulations', str(SIMS), '--window_size', '400000',
         '--max_history_length', '32', '--seed', '0']


def _setup():
  """-> (config, replay filled by 64 self-play moves, the engine that played them, weights)"""
  import torch
  import model_based_rl_amd  # noqa: F401
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  cfg = make_config(FLAGS)
  torch.manual_seed(0)
  w = get_network(cfg, torch.device('cpu')).state_dict()
  replay = PrioritizedReplay(cfg)
  eng = Engine.from_config(cfg, B)
  eng.set_weights(w)
  eng.selfplay_reset(cfg.episode_length, 1.0, stagger=True)
  for _ in range(4):
    eng.selfplay_steps(16)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    replay.ingest_records(buf[:n].numpy().copy(), n, B)
  return cfg, replay, eng, w


def block(kind):
  import torch
  from model_based_rl_amd.reanalyse import Reanalyser
  cfg, replay, eng, w = _setup()
  rows_max = CHUNKS * B
  rates = []
  if kind == 'selfplay':
    for i in range(PASSES + 1):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(4):
        eng.selfplay_steps(16)
      torch.cuda.synchronize()
      rates.append(64 * B / (time.perf_counter() - t0))
      eng.selfplay_drain()
    return {'env_steps_per_s': float(np.median(rates[1:]))}
  re = Reanalyser(cfg, replay, max_rows=rows_max)
  re.set_weights(w)
  O, A = re.O, re.A
  if kind == 'chunked':
    for i in range(PASSES + 1):
      out = re.run(rows_max)
      rates.append(out['rows'] / out['seconds'])
    return {'rows_per_s': float(np.median(rates[1:])), 'rows': out['rows']}
  e = re.engine
  to_play, legal = np.ones(B, np.int8), np.ones((B, A), np.uint8)
  for i in range(PASSES + 1):
    t0 = time.perf_counter()
    pick = replay.reanalyse_pick(rows_max, re.rows)
    n = pick['n_rows']
    rows, fresh = re.rows.numpy(), re.fresh.numpy()
    for at in range(0, n, B):
      m = min(B, n - at)
      obs = np.zeros((B, O), np.float32)
      obs[:m] = rows[at:at + m, :O]
      e.initial_inference(obs)
      e.root_prepare(to_play, legal, None, device_rng=False)
      e.search()
      out = e.finalize(0.0, np.zeros(B))
      fresh[at:at + m, :A] = out['child_visits'].cpu().numpy()[:m]
      fresh[at:at + m, A:] = out['root_value'].cpu().numpy()[:m, None].view(np.float32)
    st = replay.reanalyse_write(pick['ticket'], re.fresh[:n])
    rates.append(st['rows'] / (time.perf_counter() - t0))
  return {'rows_per_s': float(np.median(rates[1:])), 'rows': st['rows']}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--blocks', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reanalyse_bench.json'))
  ap.add_argument('--block', default=None, choices=['chunked', 'stepwise', 'selfplay'], help='(a child: one block, one JSON line)')
  ap.add_argument('--not_measured', action='store_true')
  a = ap.parse_args()
  if a.block:
    print('MZ_BLOCK ' + json.dumps(block(a.block)), flush=True)
    return
  what = ('rows per second of Reanalyser.run (chunks enqueued on the device) beside the same passes driven step by step from Python '
          'on the same engine, and self-play env-steps per second of the same build; LunarLander shapes, B = 4096, 30 simulations, '
          'child-process blocks alternating, median [min, max] over the blocks')
  if a.not_measured:
    out = {'what': what, 'result': 'not measured'}
  else:
    got = {'chunked': [], 'stepwise': [], 'selfplay': []}
    for _ in range(max(5, a.blocks)):
      for kind in ('chunked', 'stepwise', 'selfplay'):      # one child at a time: this process never opens the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--block', kind], capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith('MZ_BLOCK ')]
        if r.returncode != 0 or not line:
          raise SystemExit('block %s failed (exit %d): %s' % (kind, r.returncode, r.stderr[-2000:]))
        got[kind].append(json.loads(line[-1][len('MZ_BLOCK '):]))
        print(kind, got[kind][-1], flush=True)
    res = {}
    for kind, key in (('chunked', 'rows_per_s'), ('stepwise', 'rows_per_s'), ('selfplay', 'env_steps_per_s')):
      v = [b[key] for b in got[kind]]
      res[kind] = {key + '_median': float(np.median(v)), key + '_min': float(min(v)), key + '_max': float(max(v)), 'blocks': v}
    res['rows_per_pass'] = got['chunked'][-1]['rows']
    res['ratio_chunked_to_stepwise'] = res['chunked']['rows_per_s_median'] / res['stepwise']['rows_per_s_median']
    res['chunked_ahead_beyond_stepwise_spread'] = bool(res['chunked']['rows_per_s_min'] > res['stepwise']['rows_per_s_max'])
    out = {'what': what, 'result': res}
  print(json.dumps(out))
  with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)


if __name__ == '__main__':
  main()
