"""The unroll diagnostic (csrc/mz_unroll.hip.h, DESIGN s7f "Grading by unroll depth") on the device; writes ONE JSON line
(default profiles/unroll_bench.json).  No figure here is a pass mark.

  unroll  Engine.unroll at K = 5 on the rows of 4096 Connect Four evaluation games (30 simulations, untrained weights, seed 0,
          both sides the network -- the configuration scripts/solve_bench.py plays): every position of every game with the
          next five actions and the solver's truth at the default scope.  HIP events around the whole call (upload, the
          lines, 1 + 2 K inference launches a chunk, the terms, the copy back), seven runs after one warm-up: minimum / median
          / maximum of the call, and the time per row
  games   evaluate --device_env --grade on the same 4096 games with and without --grade_unroll 5, in alternating
          repetitions after a warm-up of both: wall time of Evaluator.play_games each (it ends in the gradings' own
          synchronisations), the spread, and the ratio.  The point of comparison is the run without the flag in this script

Each part runs in a fresh child process under its own time limit; a part that fails or runs out is recorded as such.

usage: python scripts/unroll_bench.py [--reps 7] [--games 4096] [--sims 30] [--K 5] [--out FILE] [--part unroll|games]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C4_FLAGS = ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1']
PART_SECONDS = {'unroll': 300, 'games': 420}


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def _evaluator(sims, games, unroll):
  import torch
  from model_based_rl_amd import solver
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.networks import get_network
  cfg = make_config(C4_FLAGS + ['--num_simulations', str(sims)])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games, verbose=False,
                   opp_playouts=0, grade=True, grade_empties=solver.DEFAULT_EMPTIES, grade_nodes=solver.DEFAULT_NODES,
                   grade_table=False, grade_unroll=unroll).items():
    setattr(cfg, k, v)
  ev = Evaluator(state)
  ev.load_network()
  return ev


def bench_unroll(reps, games, sims, K):
  import torch
  from model_based_rl_amd import solver
  from model_based_rl_amd.engine import Engine
  ev = _evaluator(sims, games, None)
  played = ev.play_games(games, list(range(games)), device_env=True)
  pos = solver.positions_of(played, 3)
  P = len(pos['turn'])
  eng = Engine.from_config(ev.config, games, device='cuda:0', seed=0)
  eng.set_weights(ev.weights)
  scope = 42 - pos['step'] <= solver.DEFAULT_EMPTIES
  values = np.full((P, 7), solver.UNSOLVED, np.int8)
  values[scope] = eng.solve(3, pos['boards'][scope], pos['turn'][scope], pos['step'][scope])[0]
  at = {(int(g), int(p)): i for i, (g, p) in enumerate(zip(pos['game'], pos['ply']))}
  actions, truth = np.full((P, K), -1, np.int32), np.full((P, K + 1, 7), solver.UNSOLVED, np.int8)
  for i in range(P):
    g, p = int(pos['game'][i]), int(pos['ply'][i])
    nxt = played[g].history.actions[p:p + K]
    actions[i, :len(nxt)] = nxt
    for j in range(K + 1):
      q = at.get((g, p + j))
      if q is not None:
        truth[i, j] = values[q]
  args = (3, pos['boards'], pos['turn'], pos['step'], actions)
  first = eng.unroll(*args, truth=truth)      # warm-up: code objects, the call's buffers
  ms = []
  for _ in range(reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    again = eng.unroll(*args, truth=truth)
    t1.record()
    t1.synchronize()
    assert np.array_equal(again['terms'], first['terms']) and np.array_equal(again['depth'], first['depth'])
    ms.append(t0.elapsed_time(t1))
  eng.close()
  T = {name: i for i, name in enumerate(Engine.UNROLL_TERMS)}
  return dict(device=torch.cuda.get_device_name(0), games=games, simulations=sims, K=K, rows=P, chunks=-(-P // games),
              mean_length=float(np.mean([g.step for g in played])), repetitions=reps, call_ms=_spread(ms),
              us_per_row=_spread([1e3 * x / P for x in ms]), mean_depth=float(first['depth'].mean()),
              solved_share_by_depth=[float(first['terms'][:, k, T['solved']].sum() / max(1.0, first['terms'][:, k, T['position']].sum()))
                                     for k in range(K + 1)])


def bench_games(reps, games, sims, K):
  evs = {'graded': _evaluator(sims, games, None), 'graded_unroll': _evaluator(sims, games, K)}
  seeds = list(range(games))
  for ev in evs.values():      # warm-up: library load, allocator, code objects
    ev.play_games(64, seeds[:64], device_env=True)
  wall = {k: [] for k in evs}
  for _ in range(reps):
    for name, ev in evs.items():
      t0 = time.perf_counter()
      ev.play_games(games, seeds, device_env=True)
      wall[name].append(time.perf_counter() - t0)
  out = dict(games=games, simulations=sims, K=K, repetitions=reps)
  for name in evs:
    out[name] = dict(games_per_s=_spread([games / w for w in wall[name]]), wall_s=_spread(wall[name]))
  out['unroll_over_graded_wall'] = out['graded_unroll']['wall_s']['median'] / out['graded']['wall_s']['median']
  out['unroll_report_seconds'] = evs['graded_unroll'].grade_unroll_report['seconds']
  a, b = dict(evs['graded'].grade_report), dict(evs['graded_unroll'].grade_report)
  a.pop('seconds'); b.pop('seconds')
  out['grade_report_unchanged'] = a == b
  out['report'] = evs['graded_unroll'].grade_unroll_report
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--sims', type=int, default=30)
  ap.add_argument('--K', type=int, default=5)
  ap.add_argument('--part', default=None, choices=['unroll', 'games'], help='run this part alone and print its JSON (what the children run)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unroll_bench.json'))
  a = ap.parse_args()
  if a.part:
    part = bench_unroll if a.part == 'unroll' else bench_games
    print('RESULT ' + json.dumps(part(a.reps, a.games, a.sims, a.K)), flush=True)
    return
  try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
  except Exception:
    commit = None
  line = dict(what='the learned model by unroll depth (scripts/unroll_bench.py)', git_head=commit)
  for part in ('unroll', 'games'):      # a fresh process each, under its own time limit
    cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--reps', str(a.reps), '--games', str(a.games), '--sims', str(a.sims),
           '--K', str(a.K)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=PART_SECONDS[part])
      got = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
      line[part] = json.loads(got[-1][7:]) if r.returncode == 0 and got else dict(failed=r.returncode, stderr=r.stderr[-2000:])
    except subprocess.TimeoutExpired:
      line[part] = dict(failed='ran past its limit of %d s' % PART_SECONDS[part])
    print(part, json.dumps(line[part]), flush=True)
    if 'failed' in line[part]:
      break      # nothing more is started on the device after a part that failed
  s = json.dumps(line)
  print(s)
  with open(a.out, 'w') as f:
    f.write(s + '\n')
  sys.exit(1 if any('failed' in line.get(p, {}) for p in ('unroll', 'games')) else 0)


if __name__ == '__main__':
  main()
