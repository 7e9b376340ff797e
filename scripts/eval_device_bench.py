"""The evaluator's device-environment path (--device_env) against its host-environment path, end to end; writes ONE JSON
line (default profiles/eval_device_bench.json).

Three workloads, every one played by both paths in the same process on the same checkpoint (random weights, seed 0) and
the same seeds, the two paths in alternating repetitions after one warm-up run of each:
  tictactoe     4096 TicTacToe games against the random opponent, the agent moving first and second
  connect_four  4096 ConnectFour games likewise
  cartpole      1024 CartPole-v1 games
Per workload and path: games/s and wall time as the median over the repetitions with their minimum and maximum, the host
synchronisations per game batch (device path: one per chunk of moves; host path: at least one per move, counted as the
moves played) and, for the device path, the share of wall time inside Engine.eval_env_moves.  The host path is untouched by
the device path, so its figure is the parent commit's; the statement is the ratio with both spreads beside it.  The two
paths draw the random opponent from different streams (numpy per game on the host, the counter RNG on the device), so
they play different games of the same distribution; CartPole's start states differ likewise.

usage: python scripts/eval_device_bench.py [--reps 5] [--sims 30] [--out profiles/eval_device_bench.json] [--only NAME]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    'tictactoe': (['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'], 4096, (-1, 1)),
    'connect_four': (['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'], 4096, (-1, 1)),
    'cartpole': (['--environment', 'CartPole-v1'], 1024, (None,)),
}


def _evaluator(flags, sims, games, side):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.networks import get_network
  cfg = make_config(flags + ['--num_simulations', str(sims)])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=side,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games, verbose=False).items():
    setattr(cfg, k, v)
  ev = Evaluator(state)
  ev.load_network()
  return ev


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def bench(name, reps, sims):
  from model_based_rl_amd.evaluate import MOVES_PER_SYNC, game_return
  flags, games, sides = WORKLOADS[name]
  out = {}
  for side in sides:
    ev = _evaluator(flags, sims, games, side)
    seeds = list(range(games))
    for dev in (False, True):      # warm-up: library load, graph capture, allocator
      ev.play_games(64, seeds[:64], device_env=dev)
    wall = {False: [], True: []}
    share, syncs, length, ret = [], [], {}, {}
    for _ in range(reps):
      for dev in (False, True):
        ev.device_seconds, ev.device_syncs = 0.0, 0
        t0 = time.perf_counter()
        played = ev.play_games(games, seeds, device_env=dev)
        w = time.perf_counter() - t0
        wall[dev].append(w)
        length[dev] = float(np.mean([g.step for g in played]))
        r = np.array([game_return(g) for g in played])
        ret[dev] = dict(mean=float(r.mean()), wins=int((r > 0).sum()), draws=int((r == 0).sum()), losses=int((r < 0).sum()))
        if dev:
          share.append(ev.device_seconds / w)
          syncs.append(ev.device_syncs)
        else:
          host_moves = max(len(g.history.child_visits) for g in played)
    key = 'single_player' if side is None else ('agent_first' if side == -1 else 'agent_second')
    gps = {d: [games / w for w in wall[d]] for d in wall}
    out[key] = dict(
        games=games, simulations=sims, repetitions=reps,
        device_path=dict(games_per_s=_spread(gps[True]), wall_s=_spread(wall[True]), syncs_per_batch=_spread(syncs),
                         moves_per_sync=MOVES_PER_SYNC, share_in_eval_env_moves=_spread(share), mean_length=length[True],
                         result=ret[True]),
        host_path=dict(games_per_s=_spread(gps[False]), wall_s=_spread(wall[False]), syncs_per_batch_at_least=host_moves,
                       mean_length=length[False], result=ret[False]),
        device_over_host=float(np.median(gps[True]) / np.median(gps[False])))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--sims', type=int, default=30)
  ap.add_argument('--only', default=None, choices=sorted(WORKLOADS))
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_device_bench.json'))
  a = ap.parse_args()
  if a.reps < 5:
    raise SystemExit('--reps: at least 5 repetitions of each path')
  import torch
  try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
  except Exception:
    commit = None
  line = dict(what='evaluation games on the device environments against the host-environment path (scripts/eval_device_bench.py)',
              device=torch.cuda.get_device_name(0), git_head=commit)
  for name in ([a.only] if a.only else list(WORKLOADS)):
    line[name] = bench(name, a.reps, a.sims)
  s = json.dumps(line)
  print(s)
  with open(a.out, 'w') as f:
    f.write(s + '\n')


if __name__ == '__main__':
  main()
