"""The playout-search opponent (csrc/mz_playout.hip.h, DESIGN s7d) on the device; writes ONE JSON line (default
profiles/playout_opp_bench.json).

  plan   Engine.playout_plan on 4096 Connect Four positions (after 0 .. 30 random plies, seed 0) at 1024 and at 16384
         playouts per move: HIP events around the call (the upload of the positions, the planner's one launch, the copy of
         the plans back), the median over the repetitions with their minimum and maximum after one warm-up call of each
         budget, and from it the time per planned move and the playouts per second
  games  Connect Four evaluation games (random weights, seed 0) against the uniformly random mover and against the
         playout opponent, the agent moving first: games/s of Evaluator.play_games(device_env=True), the two opponents in
         alternating blocks after one warm-up run of each.  The planner is extra work inside the same chunks of moves, so the
         random opponent's figure is the parent path's; the two play different games, and their mean lengths and results are
         beside the rates.

usage: python scripts/playout_opp_bench.py [--reps 7] [--games 4096] [--sims 30] [--opp_playouts 1024] [--out FILE]"""
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
POSITIONS, BUDGETS = 4096, (1024, 16384)


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def _positions(n):
  """n Connect Four positions after 0 .. 30 uniformly random legal plies in which the game has not ended"""
  from model_based_rl_amd.envs import ConnectFour
  rng = np.random.RandomState(0)
  boards, turn, step = np.zeros((n, 42), np.int8), np.zeros(n, np.int8), np.zeros(n, np.int32)
  env, i = ConnectFour(), 0
  while i < n:
    env.reset()
    plies, done = i % 31, False
    for _ in range(plies):
      legal = env.legal_actions()
      _, _, done, _ = env.step(int(legal[rng.randint(len(legal))]))
      if done:
        break
    if not done:
      boards[i], turn[i], step[i] = env.board, env.turn, plies
      i += 1
  return boards, turn, step


def bench_plan(reps):
  import torch
  from model_based_rl_amd.engine import Engine
  boards, turn, step = _positions(POSITIONS)
  eng = Engine(POSITIONS, 42, 7, 4, two_players=True, known_bounds=(-1, 1), discount=1.0, seed=0, device='cuda:0')
  out = {}
  for n in BUDGETS:
    eng.playout_plan(3, boards, turn, step, n)      # warm-up: code object, the planner's buffers
  ms = {n: [] for n in BUDGETS}
  for r in range(reps):
    for n in BUDGETS:      # the two budgets in alternating blocks
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      action, visits, _ = eng.playout_plan(3, boards, turn, step, n, move=r)
      t1.record()
      t1.synchronize()
      assert np.all(visits.sum(1) == n)
      ms[n].append(t0.elapsed_time(t1))
  eng.close()
  for n in BUDGETS:
    med = float(np.median(ms[n]))
    out[str(n)] = dict(positions=POSITIONS, playouts_per_move=n, repetitions=reps, call_ms=_spread(ms[n]),
                       us_per_planned_move=med * 1e3 / POSITIONS, playouts_per_s=POSITIONS * n / (med * 1e-3))
  return out


def _evaluator(sims, games, opp_playouts):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.networks import get_network
  cfg = make_config(C4_FLAGS + ['--num_simulations', str(sims)])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=-1,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games, verbose=False,
                   opp_playouts=opp_playouts).items():
    setattr(cfg, k, v)
  ev = Evaluator(state)
  ev.load_network()
  return ev


def bench_games(reps, games, sims, opp_playouts):
  from model_based_rl_amd.evaluate import game_return
  evs = {'random': _evaluator(sims, games, 0), 'playout': _evaluator(sims, games, opp_playouts)}
  seeds = list(range(games))
  for ev in evs.values():      # warm-up: library load, graph capture, allocator
    ev.play_games(64, seeds[:64], device_env=True)
  wall, info = {k: [] for k in evs}, {}
  for _ in range(reps):
    for name, ev in evs.items():
      t0 = time.perf_counter()
      played = ev.play_games(games, seeds, device_env=True)
      wall[name].append(time.perf_counter() - t0)
      r = np.array([game_return(g) for g in played])
      info[name] = dict(mean_length=float(np.mean([g.step for g in played])), wins=int((r > 0).sum()), draws=int((r == 0).sum()),
                        losses=int((r < 0).sum()))
  out = dict(games=games, simulations=sims, repetitions=reps, opp_playouts=opp_playouts, agent='first')
  for name in evs:
    out[name] = dict(games_per_s=_spread([games / w for w in wall[name]]), wall_s=_spread(wall[name]), **info[name])
  out['playout_over_random'] = out['playout']['games_per_s']['median'] / out['random']['games_per_s']['median']
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--sims', type=int, default=30)
  ap.add_argument('--opp_playouts', type=int, default=1024)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'playout_opp_bench.json'))
  a = ap.parse_args()
  if a.reps < 5:
    raise SystemExit('--reps: at least 5 repetitions of each block')
  import torch
  try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
  except Exception:
    commit = None
  line = dict(what='the playout-search opponent of the device evaluation games (scripts/playout_opp_bench.py)',
              device=torch.cuda.get_device_name(0), git_head=commit)
  line['plan'] = bench_plan(a.reps)
  line['games'] = bench_games(a.reps, a.games, a.sims, a.opp_playouts)
  s = json.dumps(line)
  print(s)
  with open(a.out, 'w') as f:
    f.write(s + '\n')


if __name__ == '__main__':
  main()
