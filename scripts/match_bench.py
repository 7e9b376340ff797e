"""Rate of a match of a network against itself (match.play_match) beside today's single-network device evaluation
(Evaluator.play_games(device_env=True)) on the same network and seeds; writes profiles/match_bench.json.

Per game (ConnectFour, TicTacToe): 4096 seeds, 30 simulations, temperature 0.5 (so that games differ), no opening.  The
match plays every seed twice (once per seating) on two engines, the evaluation once on one; both are measured in plies
applied per second of wall time, in the same process, in alternating repetitions (evaluation, match, evaluation, ...)
after one unmeasured repetition of each.  Reported: the two rates as median with minimum and maximum over the
repetitions, and the ratio of the medians.  There is no pass mark.

usage: python scripts/match_bench.py [--reps 5] [--games 4096] [--out profiles/match_bench.json]
       python scripts/match_bench.py --not_measured     (no GPU time: the file then says so)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENV_FLAGS = ['--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--num_simulations', '30']


def _state(env):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', env] + ENV_FLAGS)
  for k, v in dict(temperature=0.5, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, render=False,
                   save_mcts=False, save_gif_as='', random_opp=None, human_opp=None, label='bench', verbose=False).items():
    setattr(cfg, k, v)
  torch.manual_seed(0)
  return {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}


def bench(env, games, reps):
  import torch
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.match import play_match
  state = _state(env)
  state['config'].batch = games
  seeds = list(range(games))
  ev = Evaluator(state)
  ev.load_network()

  def evaluation():
    t0 = time.perf_counter()
    played = ev.play_games(games, seeds, device_env=True)
    torch.cuda.synchronize()
    return sum(g.step for g in played) / (time.perf_counter() - t0)

  def match():
    t0 = time.perf_counter()
    played, _ = play_match(state, state, games, seeds, batch=games)
    torch.cuda.synchronize()
    return sum(g.step for g in played) / (time.perf_counter() - t0)
  evaluation(), match()
  rates = {'evaluation': [], 'match': []}
  for _ in range(reps):
    rates['evaluation'].append(evaluation())
    rates['match'].append(match())
  out = {k: dict(plies_per_s_median=float(np.median(v)), plies_per_s_min=float(min(v)), plies_per_s_max=float(max(v)),
                 repetitions=[float(x) for x in v]) for k, v in rates.items()}
  out['ratio_match_to_evaluation'] = out['match']['plies_per_s_median'] / out['evaluation']['plies_per_s_median']
  out.update(games=games, simulations=30, temperature=0.5)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_bench.json'))
  ap.add_argument('--not_measured', action='store_true')
  a = ap.parse_args()
  what = ('plies applied per second of a match of a network against itself (both seatings, two engines) beside '
          'Evaluator.play_games(device_env=True) on the same network and seeds, same process, alternating repetitions')
  if a.not_measured:
    out = {'what': what, 'result': 'not measured'}
  else:
    out = {'what': what, 'result': {env: bench(env, a.games, a.reps) for env in ('ConnectFour', 'TicTacToe')}}
  print(json.dumps(out))
  with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)


if __name__ == '__main__':
  main()
