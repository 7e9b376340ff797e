"""Self-play on the true rules (train --selfplay_true_model, DESIGN s7k): what the one-launch search costs against the two-launch
loop, and what the mode costs against PUCT self-play; writes ONE JSON line (default profiles/true_model_selfplay_bench.json).  No
figure here is a pass mark: the points of comparison are the other configurations of this same call, alternating.

  search    HIP events around the search alone on 4096 roots, the empty Connect Four board, at 16 and at 30 simulations:
            Engine.tm_search (two launches per simulation) against Engine.tm_search_fused (one launch), Engine.search beside them
  selfplay  per game (TicTacToe, ConnectFour) at --num_envs environments (4096), untrained weights (seed 0), through Actor.launch:
              puct30        PUCT at 30 simulations, whole moves inside one launch: the loop as it is trained with today
              puct30_steps  the same with MZ_NO_PERSIST=1: one launch per step of a move
              true30_loop   --selfplay_true_model --selfplay_true_model_loop: two launches per simulation
              true30_fused  --selfplay_true_model: one launch for a move's simulations
            --warm moves per environment, then --moves timed ones (Actor.last_run: launch to the last chunk ingested)
Every run is a fresh child process under its own time limit.  Repetition 0 of every configuration warms the box up and is dropped;
then --reps repetitions, the configurations alternating inside each; median and range.  fused_default: whether the one-launch
form's median rate lies above the loop's by more than the loop's own min-max spread, per game -- the rule DESIGN s7k keeps the
default by.  A child that fails or runs out of its time limit ends the call: nothing more is started on the device.

--bench_a / --bench_b: `python bench.py --gpus 1` result lines of this commit and of its parent (one JSON line per run, taken
alternating, each from its own checkout) are recorded under mode_off.

usage: python scripts/true_model_selfplay_bench.py [--reps 7] [--num_envs 4096] [--moves 1024] [--warm 128] [--games TicTacToe ConnectFour]
                                                   [--parts search selfplay] [--base FILE] [--bench_a FILE --bench_b FILE] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = ['--two_players', '--discount', '1', '--known_bounds', '-1', '1', '--td_steps', '10', '--seed', '0', '--window_size', '200000']
# name -> (extra train flags, MZ_NO_PERSIST)
CONFIGS = {'puct30': ([], None), 'puct30_steps': ([], '1'),
           'true30_loop': (['--selfplay_true_model', '--selfplay_true_model_loop'], None), 'true30_fused': (['--selfplay_true_model'], None)}
ORDER = ('puct30', 'puct30_steps', 'true30_loop', 'true30_fused')
SEARCHES = ('search', 'tm_search', 'tm_search_fused')
CHILD_SECONDS = 240


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def child_selfplay(a):
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.selfplay_search import refuse_selfplay_true_model
  from model_based_rl_amd.shared_storage import SharedStorage
  extra, _ = CONFIGS[a.child]
  cfg = make_config(['--environment', a.game] + RECIPE + ['--num_envs', str(a.num_envs), '--num_simulations', '30',
                                                        '--runs_dir', a.runs_dir, '--run_tag', a.child] + extra)
  refuse_selfplay_true_model(cfg, 1)
  torch.manual_seed(0)
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  storage.store_weights(get_network(cfg, torch.device('cpu')).state_dict(), 1)
  actor = Actor(0, cfg, storage, replay)
  actor.launch(max_moves=a.warm)
  actor.launch(max_moves=a.moves)
  run = dict(actor.last_run)
  out = dict(moves=int(run['moves']), seconds=float(run['seconds']), moves_per_launch=actor.engine.selfplay_moves_per_launch(),
             true_model=bool(getattr(actor.engine, 'selfplay_true_model', False)), games=int(actor.games_played))
  actor.close(); actor.engine.close()
  print(json.dumps(out))


def child_search(a):
  """ms of the search alone, per simulation count and search, --reps runs after a warm-up, the three alternating"""
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import Engine, flatten_weights
  from model_based_rl_amd.networks import get_network
  n = a.num_envs
  obs = np.zeros((n, 42), np.float32)
  boards, turn, step = np.zeros((n, 42), np.int8), np.ones(n, np.int8), np.zeros(n, np.int32)
  out = {}
  for sims in (16, 30):
    cfg = make_config(['--environment', 'ConnectFour'] + RECIPE + ['--num_simulations', str(sims)])
    torch.manual_seed(0)
    eng = Engine.from_config(cfg, n, seed=0)
    eng.set_weights(flatten_weights(get_network(cfg, torch.device('cpu')).state_dict()))
    ms = {k: [] for k in SEARCHES}
    for rep in range(a.reps + 1):
      for k in SEARCHES:
        eng.set_true_model(0 if k == 'search' else 3)
        eng.initial_inference(obs)
        eng.root_prepare(turn, None, None)
        if k != 'search':
          eng.tm_root(boards, turn, step)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        getattr(eng, k)()
        e1.record()
        torch.cuda.synchronize()
        if rep:
          ms[k].append(e0.elapsed_time(e1))
    eng.close()
    out['sims%d' % sims] = {k: dict(ms_per_move=_spread(ms[k]), simulations_per_s=n * sims / (float(np.median(ms[k])) * 1e-3)) for k in SEARCHES}
    out['sims%d' % sims]['fused_over_loop'] = float(np.median(ms['tm_search_fused']) / np.median(ms['tm_search']))
  print(json.dumps(out))


def _child(a, args, env=None):
  """one child -> (result, None) or (None, what failed)"""
  cmd = [sys.executable, os.path.abspath(__file__), '--num_envs', str(a.num_envs), '--moves', str(a.moves), '--warm', str(a.warm),
         '--reps', str(a.reps), '--runs_dir', a.runs_dir] + args
  try:
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS, env=env)
  except subprocess.TimeoutExpired:
    return None, 'ran out of its %d s' % CHILD_SECONDS
  if r.returncode != 0:
    return None, dict(code=r.returncode, stderr=r.stderr[-600:])
  return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--num_envs', type=int, default=4096)
  ap.add_argument('--moves', type=int, default=1024)
  ap.add_argument('--warm', type=int, default=128)
  ap.add_argument('--games', nargs='+', default=['TicTacToe', 'ConnectFour'], choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--parts', nargs='*', default=['search', 'selfplay'], choices=['search', 'selfplay'])
  ap.add_argument('--base', default=None, help='a result line of an earlier call to start from (with --parts naming what to measure again, or nothing)')
  ap.add_argument('--bench_a', default=None, help='bench.py result lines of this commit, one JSON line per run')
  ap.add_argument('--bench_b', default=None, help='bench.py result lines of the parent commit, taken alternating with --bench_a')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'true_model_selfplay_bench.json'))
  ap.add_argument('--child', default=None, choices=sorted(CONFIGS) + ['search'])
  ap.add_argument('--game', default='TicTacToe')
  ap.add_argument('--runs_dir', default=os.path.join('/tmp', 'mz_true_model_selfplay_bench_%d' % os.getpid()))
  a = ap.parse_args()
  if a.child:
    return child_search(a) if a.child == 'search' else child_selfplay(a)
  out = dict(workload='search: %d empty Connect Four boards; selfplay: Actor.launch, %d environments, %d timed moves per environment after %d, '
                      'untrained weights' % (a.num_envs, a.num_envs, a.moves, a.warm), reps=a.reps)
  if a.base:
    out = json.loads(open(a.base).read())
  failed = False
  if 'search' in a.parts:
    out['search'], why = _child(a, ['--child', 'search'])
    if why:
      out['search'], failed = dict(failed=why), True
  if 'selfplay' in a.parts and not failed:
    out['selfplay'] = {}
    for game in a.games:
      runs = {name: [] for name in ORDER}
      res = out['selfplay'][game] = {}
      for rep in range(a.reps + 1):      # repetition 0 warms every configuration up
        for name in ORDER:
          env = dict(os.environ)
          env.pop('MZ_NO_PERSIST', None)
          if CONFIGS[name][1]:
            env['MZ_NO_PERSIST'] = CONFIGS[name][1]
          got, why = _child(a, ['--child', name, '--game', game], env)
          print('%s %s repetition %d: %s' % (game, name, rep, why or '%.0f moves/s' % (got['moves'] / got['seconds'])), file=sys.stderr, flush=True)
          if why:
            res['failed'], failed = dict(run='%s repetition %d' % (name, rep), why=why), True
            break
          assert got['true_model'] == bool(CONFIGS[name][0]) and (got['moves_per_launch'] == 16) == (name == 'puct30'), (name, got)
          if rep:
            runs[name].append(got)
        if failed:
          break
      rate = {name: [g['moves'] / g['seconds'] for g in runs[name]] for name in ORDER}
      for name in ORDER:
        if rate[name]:
          res[name] = dict(moves_per_second=_spread(rate[name]), env_steps_per_second=_spread([x * a.num_envs for x in rate[name]]))
      if rate['true30_loop'] and rate['true30_fused']:
        loop, fused = rate['true30_loop'], rate['true30_fused']
        n = min(len(loop), len(fused), len(rate['puct30']), len(rate['puct30_steps']))
        res['fused_over_loop'] = _spread([fused[i] / loop[i] for i in range(n)])
        res['fused_over_puct30'] = _spread([fused[i] / rate['puct30'][i] for i in range(n)])
        res['fused_over_puct30_steps'] = _spread([fused[i] / rate['puct30_steps'][i] for i in range(n)])
        # the rule of the default: the fused median above the loop's by more than the loop's own min-max spread
        res['fused_default'] = bool(np.median(fused) - np.median(loop) > np.max(loop) - np.min(loop))
      if failed:
        break      # (nothing more is started on the device after a run that failed or hung)
    if not failed and all('fused_default' in out['selfplay'][g] for g in a.games):
      out['fused_is_the_default_by_the_rule'] = bool(all(out['selfplay'][g]['fused_default'] for g in a.games))
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
