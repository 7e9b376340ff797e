"""The true-rules search (csrc/mz_truemodel.hip.h, DESIGN s7g) against the plain search on the device; writes ONE JSON line
(default profiles/true_model_bench.json).  No figure here is a pass mark: the point of comparison is the plain path in
this same run.

  games   evaluate --device_env on 4096 Connect Four games (30 simulations, untrained weights, seed 0, both sides the
          network) with and without --true_model, in alternating repetitions after a warm-up of both: wall time of
          Evaluator.play_games each, median and range, moves per second, and the ratio of the medians
  search  HIP events around Engine.tm_search alone (and around Engine.search on the same roots) on 4096 roots, the empty
          board: ms per move and simulations per second, seven runs after a warm-up
  sync    one condition: a chunk of eight moves with the flag still synchronises once (Evaluator.device_syncs over the moves
          played) and the host touches no game in between -- a count, not a measurement

Each part runs in a fresh child process under its own time limit; a part that fails or runs out is recorded as such.

usage: python scripts/true_model_bench.py [--reps 7] [--games 4096] [--sims 30] [--out FILE] [--part games|search]"""
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
PART_SECONDS = {'games': 420, 'search': 180}


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def _state(sims, games):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(C4_FLAGS + ['--num_simulations', str(sims)])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games, verbose=False).items():
    setattr(cfg, k, v)
  return state


def bench_games(reps, games, sims):
  from model_based_rl_amd.evaluate import Evaluator, MOVES_PER_SYNC
  ev = Evaluator(_state(sims, games))
  ev.load_network()
  seeds = list(range(games))
  wall = {False: [], True: []}
  moves, syncs = {}, {}
  for rep in range(reps + 1):      # repetition 0 warms both paths up
    for tm in (False, True):
      s0 = ev.device_syncs
      t0 = time.perf_counter()
      played = ev.play_games(games, seeds, device_env=True, true_model=tm)
      dt = time.perf_counter() - t0
      if rep:
        wall[tm].append(dt)
      moves[tm], syncs[tm] = int(sum(g.step for g in played)), ev.device_syncs - s0
  out = {}
  for tm, name in ((False, 'learned_model'), (True, 'true_rules')):
    out[name] = dict(seconds=_spread(wall[tm]), moves=moves[tm], moves_per_s=moves[tm] / float(np.median(wall[tm])),
                     host_synchronisations=syncs[tm])
  out['ratio_true_over_learned'] = dict(
      median=float(np.median(wall[True]) / np.median(wall[False])),
      range=[float(np.min(wall[True]) / np.max(wall[False])), float(np.max(wall[True]) / np.min(wall[False]))])
  longest = max(g.step for g in played)
  out['sync'] = dict(moves_per_chunk=MOVES_PER_SYNC, longest_game=int(longest), synchronisations=syncs[True],
                     one_per_chunk=bool(syncs[True] == -(-longest // MOVES_PER_SYNC)))
  return out


def bench_search(reps, games, sims):
  import torch
  from model_based_rl_amd.engine import Engine, flatten_weights
  state = _state(sims, games)
  eng = Engine.from_config(state['config'], games, seed=0)
  eng.set_weights(flatten_weights(state['weights']))
  obs = np.zeros((games, 42), np.float32)
  boards, turn, step = np.zeros((games, 42), np.int8), np.ones(games, np.int8), np.zeros(games, np.int32)
  ms = {False: [], True: []}
  for rep in range(reps + 1):
    for tm in (False, True):
      eng.set_true_model(3 if tm else 0)
      eng.initial_inference(obs)
      eng.root_prepare(turn, None, None)
      if tm:
        eng.tm_root(boards, turn, step)
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      eng.tm_search() if tm else eng.search()
      e1.record()
      torch.cuda.synchronize()
      if rep:
        ms[tm].append(e0.elapsed_time(e1))
  eng.close()
  return {name: dict(ms_per_move=_spread(ms[tm]), simulations_per_s=games * sims / (float(np.median(ms[tm])) * 1e-3))
          for tm, name in ((False, 'search'), (True, 'tm_search'))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--sims', type=int, default=30)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'true_model_bench.json'))
  ap.add_argument('--part', default=None, choices=sorted(PART_SECONDS))
  a = ap.parse_args()
  if a.part:      # a child: one part, its result on the last line of stdout
    fn = bench_games if a.part == 'games' else bench_search
    print(json.dumps(fn(a.reps, a.games, a.sims)))
    return
  out = dict(workload='%d Connect Four evaluation games, %d simulations, untrained weights, both sides the network' % (a.games, a.sims),
             reps=a.reps)
  for part in ('search', 'games'):
    cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--reps', str(a.reps), '--games', str(a.games), '--sims', str(a.sims)]
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=PART_SECONDS[part])
    except subprocess.TimeoutExpired:
      out[part] = dict(failed='ran out of its %d s' % PART_SECONDS[part])
      break      # (nothing more is started on the device after a part that hung)
    if r.returncode != 0:
      out[part] = dict(failed=r.returncode, stderr=r.stderr[-600:])
      break
    out[part] = json.loads(r.stdout.strip().splitlines()[-1])
  line = json.dumps(out)
  print(line)
  with open(a.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
