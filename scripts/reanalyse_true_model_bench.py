"""Time of one Reanalyse pass on the true rules (Engine.reanalyse_true_model, DESIGN s7n), in its two forms, beside the learned-model
pass (Engine.reanalyse) on the same rows; writes profiles/reanalyse_true_model_bench.json.

Workload: one pass over 16 x 4096 Connect Four rows on a B = 4096 engine.  The rows are the records of 16 self-play moves of 4096
device games (PUCT at 8 simulations, seed 0, the same in every child), the weights a fresh FCNetwork's (torch seed 0).  Arms, all
at 30 simulations:
  puct30     Engine.reanalyse (the fused search kernel on the learned model): the point of comparison
  true_fused Engine.reanalyse_true_model, fused=True: all simulations of a chunk in one launch of k_tm_search
  true_loop  the same with fused=False: two launches per simulation
Every measurement is a child process of its own (fresh engines); a child makes one unmeasured pass, then times one.  The arms
alternate (puct30, true_fused, true_loop, puct30, ...) for seven rounds after one unmeasured round.  Reported per arm: the median of
the seven passes with minimum and maximum, in milliseconds and rows per second; round by round the ratios of the two true-rules
forms to puct30; and s7k's rule for the form reanalyse.Reanalyser uses: the fused form stays if its median is below the loop's by
more than the loop's own min-max spread.

usage: python scripts/reanalyse_true_model_bench.py [--rounds 7] [--out profiles/reanalyse_true_model_bench.json]
       python scripts/reanalyse_true_model_bench.py --not_measured     (no GPU time: the file then says so)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CHUNKS, SIMS = 4096, 16, 30
ARMS = {'puct30': None, 'true_fused': True, 'true_loop': False}      # arm: None the learned model, else reanalyse_true_model's fused
ORDER = ('puct30', 'true_fused', 'true_loop')
FLAGS = ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--num_envs', str(B), '--seed', '0']


def block(arm):
  import torch
  import model_based_rl_amd  # noqa: F401
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.networks import get_network
  fused = ARMS[arm]
  torch.manual_seed(0)
  play = make_config(FLAGS + ['--num_simulations', '8'])
  w = get_network(play, torch.device('cpu')).state_dict()
  eng = Engine.from_config(play, B)
  eng.set_weights(w)
  eng.selfplay_set_env('connect_four')
  eng.selfplay_reset(42, 1.0, stagger=True)
  played = []
  for _ in range(CHUNKS // 4):
    eng.selfplay_steps(4)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == 4
    played.append(buf[:n].clone())
  rows = torch.cat(played).reshape(CHUNKS * B, -1).contiguous().pin_memory()
  eng.close()
  eng = Engine.from_config(make_config(FLAGS + ['--num_simulations', str(SIMS)]), B)
  eng.set_weights(w)
  if fused is not None:
    eng.set_true_model('ConnectFour')
  fresh = torch.zeros(CHUNKS * B, eng.A + 2, dtype=torch.float32).pin_memory()
  seconds = []
  for _ in range(2):      # (the first pass allocates, loads the kernels and is not reported)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if fused is None:
      eng.reanalyse(rows, fresh, CHUNKS * B, 'connect_four', SIMS)
    else:
      eng.reanalyse_true_model(rows, fresh, CHUNKS * B, 'connect_four', SIMS, fused=fused)
    seconds.append(time.perf_counter() - t0)
  pol = fresh.numpy()[:, :eng.A]
  assert np.abs(pol.sum(1) - 1).max() <= 1e-5 and np.all(pol[rows.numpy()[:, 35:42] != 0] == 0)      # (the pass did its work)
  eng.close()
  return {'seconds': seconds[-1], 'rows': CHUNKS * B}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reanalyse_true_model_bench.json'))
  ap.add_argument('--block', default=None, choices=sorted(ARMS), help='(a child: one pass, one JSON line)')
  ap.add_argument('--not_measured', action='store_true')
  a = ap.parse_args()
  if a.block:
    print('MZ_BLOCK ' + json.dumps(block(a.block)), flush=True)
    return
  what = ('seconds of one Reanalyse pass over 16 x 4096 Connect Four rows on a B = 4096 engine at 30 simulations: Engine.reanalyse '
          '(puct30) beside Engine.reanalyse_true_model in one launch per chunk (true_fused) and in the two-launch loop (true_loop); '
          'child-process passes alternating, seven rounds after an unmeasured one, median [min, max] per arm, the ratios to puct30 '
          'round by round, and the form the rule of DESIGN s7k keeps')
  if a.not_measured:
    out = {'what': what, 'result': 'not measured'}
  else:
    got = {arm: [] for arm in ARMS}
    for rnd in range(1 + max(1, a.rounds)):
      for arm in ORDER:      # one child at a time: this process never opens the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--block', arm], capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith('MZ_BLOCK ')]
        if r.returncode != 0 or not line:
          raise SystemExit('block %s failed (exit %d): %s' % (arm, r.returncode, r.stderr[-2000:]))
        if rnd:      # (round 0 warms the machine up)
          got[arm].append(json.loads(line[-1][len('MZ_BLOCK '):]))
        print(rnd, arm, line[-1], flush=True)
    res = {'rows_per_pass': CHUNKS * B, 'simulations': SIMS}
    for arm, runs in got.items():
      s = [b['seconds'] for b in runs]
      res[arm] = {'ms_median': 1e3 * float(np.median(s)), 'ms_min': 1e3 * min(s), 'ms_max': 1e3 * max(s),
                  'rows_per_s_median': CHUNKS * B / float(np.median(s)), 'ms_per_chunk_median': 1e3 * float(np.median(s)) / CHUNKS,
                  'ms_runs': [1e3 * v for v in s]}
    for arm in ('true_fused', 'true_loop'):
      ratios = [g['seconds'] / p['seconds'] for g, p in zip(got[arm], got['puct30'])]
      res['ratio_%s_to_puct30' % arm] = {'median': float(np.median(ratios)), 'min': min(ratios), 'max': max(ratios), 'runs': ratios}
    gain = res['true_loop']['ms_median'] - res['true_fused']['ms_median']
    spread = res['true_loop']['ms_max'] - res['true_loop']['ms_min']
    res['rule'] = {'loop_median_minus_fused_median_ms': gain, 'loop_spread_ms': spread, 'fused_stays': bool(gain > spread)}
    out = {'what': what, 'result': res}
  print(json.dumps(out))
  with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)


if __name__ == '__main__':
  main()
