"""The Gumbel search (csrc/mz_gumbel.hip.h, DESIGN s7h) against the plain PUCT search on the device; writes ONE JSON line
(default profiles/gumbel_bench.json).  No figure here is a pass mark: the point of comparison is the plain path in this same
run, alternating.

  search    HIP events around Engine.gz_search alone (and around Engine.search on the same roots) on 4096 empty Connect Four
            boards at n = 8, 16 and 30 simulations: ms per move, seven runs after a warm-up, median and range
  games     Evaluator.play_games(device_env=True) on 4096 Connect Four games (30 simulations, untrained weights, both sides
            the network) with and without gumbel, in alternating repetitions after a warm-up of both: wall time, plies
  strength  one checkpoint against itself, PUCT on one side and Gumbel on the other (match.play_match(gumbel=(0, 1)),
            TicTacToe, temperature 0, gumbel_scale 0, two random opening plies, every seed from both seats), at equal n in
            {4, 8, 16, 30} and Gumbel at 8 against PUCT at 30: the Elo difference of the GUMBEL side with match.score_summary's
            interval; and --grade's optimal-move rate of that checkpoint's games against the random mover (the network moves
            first) with and without gumbel at n = 8 and 30.
            --checkpoint FILE: the same again on a saved state (scripts/tictactoe_learning.py --keep_checkpoint), recorded
            as strength_trained beside the untrained weights' strength

Each part runs in a fresh child process under its own time limit; a part that fails or runs out is recorded as such.

usage: python scripts/gumbel_bench.py [--reps 7] [--games 4096] [--seeds 1024] [--checkpoint FILE] [--out FILE] [--part NAME]"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = {'ConnectFour': ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1'],
         'TicTacToe': ['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1']}
PART_SECONDS = {'search': 180, 'games': 300, 'strength': 420, 'strength_trained': 420}
SEARCH_SIMS = (8, 16, 30)


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def _state(env, sims, batch, checkpoint=None, **over):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  if checkpoint:      # (a checkpoint kept by scripts/tictactoe_learning.py --keep_checkpoint carries weights alone: its recipe's config)
    state = torch.load(checkpoint, map_location=torch.device('cpu'), weights_only=False)
    cfg = copy.copy(state['config']) if 'config' in state else make_config(FLAGS[env] + ['--num_simulations', str(sims)])
    state = dict(state, config=cfg)
    cfg.num_simulations = int(sims)
  else:
    cfg = make_config(FLAGS[env] + ['--num_simulations', str(sims)])
    torch.manual_seed(0)
    state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=batch, verbose=False).items():
    setattr(cfg, k, v)
  for k, v in over.items():
    setattr(cfg, k, v)
  return state


def bench_search(a):
  import torch
  from model_based_rl_amd.engine import Engine, flatten_weights
  out = {}
  for sims in SEARCH_SIMS:
    state = _state('ConnectFour', sims, a.games)
    eng = Engine.from_config(state['config'], a.games, seed=0)
    eng.set_weights(flatten_weights(state['weights']))
    obs, turn = np.zeros((a.games, 42), np.float32), np.ones(a.games, np.int8)
    ms = {False: [], True: []}
    for rep in range(a.reps + 1):      # repetition 0 warms both paths up
      for gz in (False, True):
        eng.set_gumbel(gz)
        eng.initial_inference(obs)
        eng.root_prepare(turn, None, None)
        if gz:
          eng.gz_root()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.gz_search() if gz else eng.search()
        e1.record()
        torch.cuda.synchronize()
        if rep:
          ms[gz].append(e0.elapsed_time(e1))
    eng.close()
    out['n_%d' % sims] = dict(search_ms=_spread(ms[False]), gz_search_ms=_spread(ms[True]),
                              ratio_gumbel_over_puct=float(np.median(ms[True]) / np.median(ms[False])))
  return out


def bench_games(a):
  from model_based_rl_amd.evaluate import Evaluator
  ev = Evaluator(_state('ConnectFour', 30, a.games))
  ev.load_network()
  seeds = list(range(a.games))
  wall, plies = {False: [], True: []}, {}
  for rep in range(a.reps + 1):
    for gz in (False, True):
      t0 = time.perf_counter()
      played = ev.play_games(a.games, seeds, device_env=True, gumbel=gz)
      dt = time.perf_counter() - t0
      if rep:
        wall[gz].append(dt)
      plies[gz] = int(sum(g.step for g in played))
  out = {name: dict(seconds=_spread(wall[gz]), plies=plies[gz]) for gz, name in ((False, 'puct'), (True, 'gumbel'))}
  out['ratio_gumbel_over_puct'] = float(np.median(wall[True]) / np.median(wall[False]))
  return out


def bench_strength(a):
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.match import play_match
  seeds = list(range(a.seeds))
  out = dict(checkpoint=os.path.basename(a.checkpoint) if a.checkpoint else 'untrained weights (seed 0)', seeds=a.seeds,
             opening_plies=2, matches={}, graded={})
  for n_puct, n_gz in ((4, 4), (8, 8), (16, 16), (30, 30), (30, 8)):
    sa, sb = _state('TicTacToe', n_puct, a.seeds, a.checkpoint), _state('TicTacToe', n_gz, a.seeds, a.checkpoint)
    _, s = play_match(sa, sb, a.seeds, seeds, opening_plies=2, gumbel=(0, 1))
    # play_match scores side A (PUCT); the Gumbel side's Elo is its negative
    lo, hi = s['elo_interval']
    neg = lambda v: None if v is None else -v
    out['matches']['puct_%d_vs_gumbel_%d' % (n_puct, n_gz)] = dict(
        gumbel_wins=s['losses'], draws=s['draws'], gumbel_losses=s['wins'], gumbel_score=1.0 - s['score'], gumbel_elo=neg(s['elo']),
        gumbel_elo_interval=[neg(hi), neg(lo)], mean_length=s['mean_length'])
  for n in (8, 30):
    for gz in (0, 1):
      state = _state('TicTacToe', n, a.seeds, a.checkpoint, grade=True, grade_table=False, grade_empties=12, grade_nodes=4096,
                     grade_unroll=None, device_env=True, gumbel=gz, random_opp=-1)
      ev = Evaluator(state)
      ev.load_network()
      ev.play_games(a.seeds, seeds)
      r = ev.grade_report
      out['graded']['%s_%d' % ('gumbel' if gz else 'puct', n)] = dict(graded=r['graded'], optimal=r['optimal'], optimal_rate=r['optimal_rate'],
                                                                   blunders=r['blunders'])
  return out


PARTS = {'search': bench_search, 'games': bench_games, 'strength': bench_strength, 'strength_trained': bench_strength}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--seeds', type=int, default=1024)
  ap.add_argument('--checkpoint', default=None)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gumbel_bench.json'))
  ap.add_argument('--part', default=None, choices=sorted(PARTS))
  a = ap.parse_args()
  if a.part:      # a child: one part, its result on the last line of stdout
    print(json.dumps(PARTS[a.part](a)))
    return
  out = dict(workload='%d empty Connect Four roots / evaluation games, untrained weights; TicTacToe matches of %d seeds from both seats'
                      % (a.games, a.seeds), reps=a.reps)
  for part in ('search', 'games', 'strength') + (('strength_trained',) if a.checkpoint else ()):
    cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--reps', str(a.reps), '--games', str(a.games), '--seeds', str(a.seeds)]
    if part == 'strength_trained':
      cmd += ['--checkpoint', a.checkpoint]
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
