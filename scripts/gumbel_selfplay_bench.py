"""Self-play with the Gumbel search (train --selfplay_gumbel, DESIGN s7i) against PUCT self-play, through Actor.launch on the
device games; writes ONE JSON line (default profiles/gumbel_selfplay_bench.json).  No figure here is a pass mark: the points of
comparison are the PUCT runs of this same call, alternating.

Per game (TicTacToe, ConnectFour) at --num_envs environments (4096), untrained weights (seed 0), four configurations:
  puct30         PUCT at 30 simulations, whole moves inside one launch: the loop as it is trained with today
  puct30_steps   the same with MZ_NO_PERSIST=1: one launch per step of a move, the form the Gumbel moves run in -- the fair
                 baseline of this path
  gumbel8        --selfplay_gumbel at 8 simulations
  gumbel16       --selfplay_gumbel at 16 simulations
Every run is a fresh child process: an Actor built as train builds it (a storage that holds the weights, the native replay, no
learner) plays --warm moves per environment, then --moves timed ones (Actor.last_run: launch to the last chunk ingested).
Repetition 0 of every configuration warms the box up and is dropped; then --reps repetitions, the configurations alternating
inside each; median and range of moves/s and env-steps/s, and the ratios gumbel8 / puct30 and gumbel8 / puct30_steps run by run.
A child that fails or runs out of its time limit ends the call: nothing more is started on the device.

--bench_a / --bench_b: two lines of `python bench.py --gpus 1` results (files with one JSON line per run, this commit's and its
parent's, taken alternating, each from its own checkout: MZ_HIP_LIB alone does not do, this commit's _abi.py asks the library for
mz_selfplay_set_gumbel) are recorded beside them under mode_off: the whole-moves path compiles the same kernels with the
same argument structs, and the acceptance is that this commit's median lies inside the parent's own range.

usage: python scripts/gumbel_selfplay_bench.py [--reps 7] [--num_envs 4096] [--moves 1024] [--warm 128] [--games TicTacToe ConnectFour]
                                               [--bench_a FILE --bench_b FILE] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--td_steps', '10', '--seed', '0', '--window_size', '200000']
# name -> (simulations, extra train flags, MZ_NO_PERSIST)
CONFIGS = {'puct30': (30, [], None), 'puct30_steps': (30, [], '1'), 'gumbel8': (8, ['--selfplay_gumbel'], None),
           'gumbel16': (16, ['--selfplay_gumbel'], None)}
ORDER = ('puct30', 'puct30_steps', 'gumbel8', 'gumbel16')
CHILD_SECONDS = 240


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def child(a):
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.selfplay_search import refuse_selfplay_gumbel
  from model_based_rl_amd.shared_storage import SharedStorage
  sims, extra, _ = CONFIGS[a.child]
  cfg = make_config(['--environment', a.game] + RECIPE + ['--num_envs', str(a.num_envs), '--num_simulations', str(sims),
                                                        '--runs_dir', a.runs_dir, '--run_tag', a.child] + extra)
  refuse_selfplay_gumbel(cfg, 1)
  torch.manual_seed(0)
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  storage.store_weights(get_network(cfg, torch.device('cpu')).state_dict(), 1)
  actor = Actor(0, cfg, storage, replay)
  actor.launch(max_moves=a.warm)
  actor.launch(max_moves=a.moves)
  run = dict(actor.last_run)
  out = dict(moves=int(run['moves']), seconds=float(run['seconds']), moves_per_launch=actor.engine.selfplay_moves_per_launch(),
             gumbel=bool(getattr(actor.engine, 'selfplay_gumbel', False)), games=int(actor.games_played))
  actor.close(); actor.engine.close()
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--num_envs', type=int, default=4096)
  ap.add_argument('--moves', type=int, default=1024)
  ap.add_argument('--warm', type=int, default=128)
  ap.add_argument('--games', nargs='+', default=['TicTacToe', 'ConnectFour'], choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--bench_a', default=None, help='bench.py result lines of this commit, one JSON line per run')
  ap.add_argument('--bench_b', default=None, help='bench.py result lines of the parent commit, taken alternating with --bench_a')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gumbel_selfplay_bench.json'))
  ap.add_argument('--child', default=None, choices=sorted(CONFIGS))
  ap.add_argument('--game', default='TicTacToe')
  ap.add_argument('--runs_dir', default=os.path.join('/tmp', 'mz_gumbel_selfplay_bench_%d' % os.getpid()))
  a = ap.parse_args()
  if a.child:
    return child(a)
  out = dict(workload='Actor.launch, %d environments, %d timed moves per environment after %d, untrained weights' % (a.num_envs, a.moves, a.warm),
             reps=a.reps, games={})
  failed = False
  for game in a.games:
    runs = {name: [] for name in ORDER}
    res = out['games'][game] = {}
    for rep in range(a.reps + 1):      # repetition 0 warms every configuration up
      for name in ORDER:
        env = dict(os.environ)
        env.pop('MZ_NO_PERSIST', None)
        if CONFIGS[name][2]:
          env['MZ_NO_PERSIST'] = CONFIGS[name][2]
        cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--game', game, '--num_envs', str(a.num_envs),
               '--moves', str(a.moves), '--warm', str(a.warm), '--runs_dir', a.runs_dir]
        try:
          r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS, env=env)
        except subprocess.TimeoutExpired:
          res['failed'] = '%s repetition %d ran out of its %d s' % (name, rep, CHILD_SECONDS)
          failed = True
          break
        if r.returncode != 0:
          res['failed'] = dict(run='%s repetition %d' % (name, rep), code=r.returncode, stderr=r.stderr[-600:])
          failed = True
          break
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert got['gumbel'] == bool(CONFIGS[name][1]) and (got['moves_per_launch'] == 16) == (name == 'puct30'), (name, got)
        if rep:
          runs[name].append(got)
      if failed:
        break
    for name in ORDER:
      if runs[name]:
        mps = [g['moves'] / g['seconds'] for g in runs[name]]
        res[name] = dict(simulations=CONFIGS[name][0], moves_per_second=_spread(mps),
                         env_steps_per_second=_spread([x * a.num_envs for x in mps]))
    n = min(len(runs[k]) for k in ('puct30', 'puct30_steps', 'gumbel8'))
    if n:
      rate = lambda k, i: runs[k][i]['moves'] / runs[k][i]['seconds']
      res['gumbel8_over_puct30'] = _spread([rate('gumbel8', i) / rate('puct30', i) for i in range(n)])
      res['gumbel8_over_puct30_steps'] = _spread([rate('gumbel8', i) / rate('puct30_steps', i) for i in range(n)])
    if failed:
      break      # (nothing more is started on the device after a run that failed or hung)
  if a.bench_a and a.bench_b:
    read = lambda p: [json.loads(l) for l in open(p) if l.strip().startswith('{')]
    A, Bp = read(a.bench_a), read(a.bench_b)
    va, vb = [float(x['value']) for x in A], [float(x['value']) for x in Bp]
    out['mode_off'] = dict(metric=A[0]['metric'], this_commit=_spread(va), parent=_spread(vb),
                           median_inside_parents_range=bool(min(vb) <= float(np.median(va)) <= max(vb)))
  line = json.dumps(out)
  print(line)
  with open(a.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
