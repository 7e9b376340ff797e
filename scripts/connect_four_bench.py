"""Self-play speed of the device Connect Four environment (mz_selfplay_set_env kind 3): the whole-moves form against the
launch-per-step form (MZ_NO_PERSIST=1), in alternating blocks, with TicTacToe's whole-moves figure of the same run beside
them and the mean depth of the leaves a search expands.  4096 environments, 30 simulations, random-init FCNetwork weights.

  python scripts/connect_four_bench.py [--blocks 5] [--launches 12] [--out profiles/connect_four_selfplay.json]

Every block is a fresh child process under a time limit of its own (MZ_NO_PERSIST is read at mz_create): it creates the
engine, plays two launches of 16 moves to warm up, then times `--launches` more, synchronising and draining the record ring
after each (the drain is outside the clock).  A form's figure is the median of its blocks, its spread their min and max."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS, SIMS, CHUNK = 4096, 30, 16
GAMES = {'connect_four': (42, 7, 42), 'tictactoe': (9, 9, 9)}      # obs_dim, action_space, episode_len
BLOCK_LIMIT = 120      # seconds a child may take


def leaf_depths(E, A):
  """depths of the expanded nodes of every tree (scripts/tree_depth.py: node n = 1 + e_parent * A + a, expansion indices are
  assigned in order, so parents precede children)"""
  import numpy as np
  d = []
  for b in range(E.shape[0]):
    order = sorted((int(E[b, n]), int(n)) for n in np.flatnonzero(E[b] >= 0) if n != 0)
    dep = {0: 0}
    for e, n in order:
      dep[e] = dep[(n - 1) // A] + 1
    d += [v for k, v in dep.items() if k != 0]
  return np.array(d)


def child(game, launches, depth):
  import types
  import numpy as np
  import torch
  import model_based_rl_amd      # noqa: F401  (import alias)
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.networks import FCNetwork
  O, A, T = GAMES[game]
  torch.manual_seed(0)
  net = FCNetwork(O, A, torch.device('cpu'), types.SimpleNamespace()).eval()
  eng = Engine(ENVS, O, A, SIMS, seed=1, two_players=True, known_bounds=(-1.0, 1.0), discount=1.0)
  eng.set_weights(net.state_dict())
  eng.selfplay_set_env(game)
  if depth:
    eng.selfplay_export_trees(True)
  eng.selfplay_reset(T, 1.0)
  out = dict(game=game, moves_per_launch=eng.selfplay_moves_per_launch(), kernel=eng.search_kernel_info())
  for _ in range(2):
    eng.selfplay_steps(CHUNK); eng.selfplay_drain(); torch.cuda.synchronize()
  if depth:      # the trees of the last move played (positions from the middle of the games)
    d = leaf_depths(eng.export_tree()['E'][:1024], A)
    out.update(mean_leaf_depth=float(d.mean()), max_leaf_depth=int(d.max()))
  else:
    seconds = 0.0
    for _ in range(launches):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      eng.selfplay_steps(CHUNK)
      torch.cuda.synchronize()
      seconds += time.perf_counter() - t0
      eng.selfplay_drain(); torch.cuda.synchronize()
    moves = launches * CHUNK
    out.update(moves=moves, us_per_move=1e6 * seconds / moves, env_steps_per_s=ENVS * moves / seconds)
  eng.close()
  print('RESULT ' + json.dumps(out), flush=True)


def run_child(game, launches, no_persist=False, depth=False):
  env = {k: v for k, v in os.environ.items() if k not in ('MZ_NO_PERSIST', 'MZ_NO_LDS_TREES', 'MZ_NO_LDS_HYBRID', 'MZ_SPLIT_F16', 'MZ_NO_FUSED')}
  if no_persist:
    env['MZ_NO_PERSIST'] = '1'
  cmd = [sys.executable, os.path.abspath(__file__), '--child', game, '--launches', str(launches)] + (['--depth'] if depth else [])
  r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=BLOCK_LIMIT)
  lines = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
  if r.returncode != 0 or not lines:      # a failed block ends the run: nothing more is started on the GPU
    raise SystemExit('block %s failed (exit %s)\n%s\n%s' % (cmd, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
  return json.loads(lines[-1][7:])


def figure(blocks):
  import numpy as np
  us = sorted(b['us_per_move'] for b in blocks)
  return dict(us_per_move=float(np.median(us)), us_per_move_min=us[0], us_per_move_max=us[-1],
              env_steps_per_s=ENVS * 1e6 / float(np.median(us)), moves_per_launch=blocks[0]['moves_per_launch'],
              kernel=blocks[0]['kernel'], blocks=[b['us_per_move'] for b in blocks])


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--child')
  p.add_argument('--depth', action='store_true')
  p.add_argument('--blocks', type=int, default=5)
  p.add_argument('--launches', type=int, default=12)
  p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'connect_four_selfplay.json'))
  a = p.parse_args()
  if a.child:
    return child(a.child, a.launches, a.depth)
  assert a.blocks >= 5, 'at least five blocks per form'
  whole, steps, ttt = [], [], []
  for k in range(a.blocks):      # alternating blocks: drift of the box reaches both forms alike
    whole.append(run_child('connect_four', a.launches))
    steps.append(run_child('connect_four', a.launches, no_persist=True))
    if k < 3:
      ttt.append(run_child('tictactoe', a.launches))
    print('block %d: whole moves %.1f us/move, launch per step %.1f us/move' % (k, whole[-1]['us_per_move'], steps[-1]['us_per_move']), flush=True)
  assert whole[0]['moves_per_launch'] == CHUNK and steps[0]['moves_per_launch'] == 0 and ttt[0]['moves_per_launch'] == CHUNK
  res = dict(what='device Connect Four self-play, %d environments, %d simulations, random-init weights; us per move of all environments'
                  % (ENVS, SIMS),
             whole_moves=figure(whole), launch_per_step=figure(steps), tictactoe_whole_moves=figure(ttt),
             connect_four_depth=run_child('connect_four', 0, depth=True), tictactoe_depth=run_child('tictactoe', 0, depth=True))
  w, s = res['whole_moves'], res['launch_per_step']
  res['whole_moves_ahead_by_us'] = s['us_per_move'] - w['us_per_move']
  res['launch_per_step_spread_us'] = s['us_per_move_max'] - s['us_per_move_min']
  res['whole_moves_ahead_by_more_than_the_spread'] = bool(w['us_per_move_max'] < s['us_per_move_min'] and
                                                          res['whole_moves_ahead_by_us'] > res['launch_per_step_spread_us'])
  with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
  print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
  for k in ('whole_moves', 'launch_per_step', 'tictactoe_whole_moves'):
    print('%-24s %8.1f us/move (%.1f .. %.1f)  %.2f M env-steps/s' % (k, res[k]['us_per_move'], res[k]['us_per_move_min'],
                                                                       res[k]['us_per_move_max'], res[k]['env_steps_per_s'] / 1e6))
  print('mean leaf depth: Connect Four %.2f, TicTacToe %.2f' % (res['connect_four_depth']['mean_leaf_depth'], res['tictactoe_depth']['mean_leaf_depth']))


if __name__ == '__main__':
  main()
