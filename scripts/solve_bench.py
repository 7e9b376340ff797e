"""The exact game solver (csrc/mz_solve.hip.h, DESIGN s7f) on the device; writes ONE JSON line (default
profiles/solve_bench.json).  No figure here is a pass mark.

  solve  Engine.solve on 4096 Connect Four positions from uniformly random play (seed 0) at 8, 12, 16 and 20 empty cells,
         at a budget of 2^20 nodes (the share of units a smaller budget would leave unsolved follows from the node counts:
         a unit is cut at b exactly when it needs more than b nodes, and is given for b = 2^10 .. 2^20, the default among them): HIP events around the whole call (upload, the launches, the copy back), seven runs
         after one warm-up, minimum / median / maximum; nodes per second, the share of (position, action) units and of
         positions left unsolved, and the host hook's single-thread time on the first 256 of them
  games  4096 Connect Four evaluation games (random weights, seed 0, both sides the network) with and without --grade at
         the default scope, in alternating repetitions: games/s of Evaluator.play_games(device_env=True) each, their spread
         and the ratio; then the grading alone (Evaluator.grade on the kept games: the host's replay of the positions and
         the solve) at every even scope from 8 to 20 empty cells
  derived  the default scope: the largest even count of empty cells at which grading took less time than the games
         themselves; the default budget: the largest power of two at which a launch of 4096 positions whose every unit ran
         to the budget would last under a second at the measured nodes per second (computed, never run)


--table: the table search (Engine.solve(table=True), DESIGN s7f "The table search") beside the plain one; writes
profiles/solve_table_bench.json instead.
  solve  the same positions, also at 24 empty cells, at the default budget and at 2^20: plain and table calls alternate,
         seven runs each after a warm-up of both, HIP events around the whole call; per depth, budget and search the time
         with its spread, the total nodes, the largest unit, the share of unsolved units and of positions with one, and
         the time of a call over its largest unit's nodes (the cost of a stone on the lane that bounds the launch); the host
         hooks' single-thread rates on the first 256 positions at the default budget
  games  the games without grading, and the grading alone with the table search at every even scope from 8 to 24
  derived  the largest even scope at which grading with the table search took less time than the games themselves

usage: python scripts/solve_bench.py [--table] [--reps 7] [--games 4096] [--sims 30] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C4_FLAGS = ['--environment', 'ConnectFour', '--two_players', '--discount', '1', '--known_bounds', '-1', '1']
POSITIONS, EMPTIES, HOST_POSITIONS, SCOPES = 4096, (8, 12, 16, 20), 256, (8, 10, 12, 14, 16, 18, 20)
DEFAULT_SCOPE = 12      # evaluate --grade_empties' default
MEASURE_NODES = 1 << 20      # the budget the solve part measures at: far above the default, so the tail of the units shows
BUDGETS = tuple(1 << k for k in range(10, 21, 2))


def _spread(v):
  return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=[float(x) for x in v])


def _positions(n, plies, rng):
  """n Connect Four positions after `plies` uniformly random legal plies in which the game has not ended"""
  from model_based_rl_amd.envs import ConnectFour
  boards, turn, step = np.zeros((n, 42), np.int8), np.zeros(n, np.int8), np.full(n, plies, np.int32)
  env, i = ConnectFour(), 0
  while i < n:
    env.reset()
    done = False
    for _ in range(plies):
      legal = env.legal_actions()
      _, _, done, _ = env.step(int(legal[rng.randint(len(legal))]))
      if done:
        break
    if not done:
      boards[i], turn[i] = env.board, env.turn
      i += 1
  return boards, turn, step


def _host_seconds(boards, turn, step, max_nodes, table=False):
  from model_based_rl_amd import _abi
  lib = _abi.load()
  hook = lib.mz_solve_tt_host if table else lib.mz_solve_host
  n = len(turn)
  values, nodes = np.zeros((n, 7), np.int8), np.zeros((n, 7), np.uint32)
  p = lambda a: a.ctypes.data_as(C.c_void_p)
  t0 = time.perf_counter()
  _abi.check(hook(3, 7, p(boards), p(turn), p(step), n, int(max_nodes), p(values), p(nodes)), 'the host hook')
  return time.perf_counter() - t0, values, nodes


def bench_solve(reps, max_nodes):
  import torch
  from model_based_rl_amd.engine import Engine
  rng = np.random.RandomState(0)
  eng = Engine(POSITIONS, 42, 7, 4, two_players=True, known_bounds=(-1, 1), discount=1.0, seed=0, device='cuda:0')
  out = {}
  for empties in EMPTIES:
    boards, turn, step = _positions(POSITIONS, 42 - empties, rng)
    values, nodes = eng.solve(3, boards, turn, step, max_nodes=max_nodes)      # warm-up: code object, the solver's buffers
    ms = []
    for _ in range(reps):
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      again = eng.solve(3, boards, turn, step, max_nodes=max_nodes)
      t1.record()
      t1.synchronize()
      assert np.array_equal(again[0], values) and np.array_equal(again[1], nodes)
      ms.append(t0.elapsed_time(t1))
    hs, hv, hn = _host_seconds(boards[:HOST_POSITIONS], turn[:HOST_POSITIONS], step[:HOST_POSITIONS], max_nodes)
    assert np.array_equal(hv, values[:HOST_POSITIONS]) and np.array_equal(hn, nodes[:HOST_POSITIONS])
    total = int(nodes.astype(np.uint64).sum())
    per_position = nodes.astype(np.uint64).sum(1)
    legal = values != -2
    out[str(empties)] = dict(
        positions=POSITIONS, empty_cells=empties, max_nodes=max_nodes, repetitions=reps, call_ms=_spread(ms), nodes=total,
        nodes_per_position=dict(mean=float(per_position.mean()), max=int(per_position.max())), unit_nodes_max=int(nodes.max()),
        nodes_per_s=total / (float(np.median(ms)) * 1e-3), unsolved_units=float((values == -3).sum() / legal.sum()),
        unsolved_positions=float((values == -3).any(1).mean()),
        unsolved_at={str(b): dict(units=float(((nodes > b) | (values == -3))[legal].mean()),
                                  positions=float(((nodes > b) | (values == -3)).any(1).mean())) for b in BUDGETS},
        host_hook=dict(positions=HOST_POSITIONS, seconds=hs, nodes_per_s=int(hn.astype(np.uint64).sum()) / hs))
    print(empties, json.dumps(out[str(empties)]), flush=True)
  eng.close()
  return out


TABLE_EMPTIES, TABLE_SCOPES = (8, 12, 16, 20, 24), (8, 10, 12, 14, 16, 18, 20, 22, 24)


def bench_table_solve(reps, budgets):
  import torch
  from model_based_rl_amd.engine import Engine
  rng = np.random.RandomState(0)
  eng = Engine(POSITIONS, 42, 7, 4, two_players=True, known_bounds=(-1, 1), discount=1.0, seed=0, device='cuda:0')
  out = {}
  for empties in TABLE_EMPTIES:
    boards, turn, step = _positions(POSITIONS, 42 - empties, rng)
    out[str(empties)] = {}
    for budget in budgets:
      first = {t: eng.solve(3, boards, turn, step, max_nodes=budget, table=t) for t in (False, True)}      # warm-up of both
      solved = (first[False][0] != -3) & (first[True][0] != -3)
      both = np.all(solved)
      assert np.array_equal(first[False][0][solved], first[True][0][solved])      # where both solve, one value
      ms = {False: [], True: []}
      for _ in range(reps):
        for t in (False, True):
          t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          t0.record()
          again = eng.solve(3, boards, turn, step, max_nodes=budget, table=t)
          t1.record()
          t1.synchronize()
          assert np.array_equal(again[0], first[t][0]) and np.array_equal(again[1], first[t][1])
          ms[t].append(t0.elapsed_time(t1))
      row = dict(positions=POSITIONS, empty_cells=empties, max_nodes=budget, repetitions=reps, every_unit_solved_by_both=bool(both))
      for t, name in ((False, 'plain'), (True, 'table')):
        values, nodes = first[t]
        legal = values != -2
        total, med = int(nodes.astype(np.uint64).sum()), float(np.median(ms[t]))
        row[name] = dict(call_ms=_spread(ms[t]), nodes=total, nodes_per_position=float(nodes.astype(np.uint64).sum(1).mean()),
                         unit_nodes_max=int(nodes.max()), nodes_per_s=total / (med * 1e-3),
                         call_us_per_node_of_largest_unit=med * 1e3 / int(nodes.max()),
                         unsolved_units=float((values == -3).sum() / legal.sum()), unsolved_positions=float((values == -3).any(1).mean()))
      row['table_over_plain'] = dict(call_ms=row['table']['call_ms']['median'] / row['plain']['call_ms']['median'],
                                     nodes=row['table']['nodes'] / row['plain']['nodes'])
      if budget == budgets[0]:      # the host hooks, single thread, at the default budget (bounded: 256 * 7 * budget nodes)
        for t, name in ((False, 'plain'), (True, 'table')):
          hs, hv, hn = _host_seconds(boards[:HOST_POSITIONS], turn[:HOST_POSITIONS], step[:HOST_POSITIONS], budget, table=t)
          assert np.array_equal(hv, first[t][0][:HOST_POSITIONS]) and np.array_equal(hn, first[t][1][:HOST_POSITIONS])
          row[name]['host_hook'] = dict(positions=HOST_POSITIONS, seconds=hs, nodes_per_s=int(hn.astype(np.uint64).sum()) / hs)
      out[str(empties)][str(budget)] = row
      print(empties, budget, json.dumps(row), flush=True)
  eng.close()
  return out


def bench_table_games(reps, games, sims, max_nodes):
  plain = _evaluator(sims, games, False, max_nodes)
  graded = _evaluator(sims, games, True, max_nodes)
  graded.config.grade_table = True
  seeds = list(range(games))
  plain.play_games(64, seeds[:64], device_env=True)
  wall = []
  for _ in range(reps):
    t0 = time.perf_counter()
    plain.play_games(games, seeds, device_env=True)
    wall.append(time.perf_counter() - t0)
  played = graded.play_games(games, seeds, device_env=True)      # kept histories; its report is the default scope's
  out = dict(games=games, simulations=sims, repetitions=reps, max_nodes=max_nodes, mean_length=float(np.mean([g.step for g in played])),
             plain=dict(games_per_s=_spread([games / w for w in wall]), wall_s=_spread(wall)), report=graded.grade_report)
  scopes = {}
  for e in TABLE_SCOPES:
    graded.config.grade_empties = e
    secs, rep = [], None
    for _ in range(3):
      t0 = time.perf_counter()
      rep = graded.grade(played)
      secs.append(time.perf_counter() - t0)
    scopes[str(e)] = dict(seconds=_spread(secs), graded=rep['graded'], unsolved=rep['unsolved'], nodes=rep['nodes'],
                          optimal_rate=rep['optimal_rate'])
    print('scope', e, json.dumps(scopes[str(e)]), flush=True)
  out['grading_alone_table'] = scopes
  return out


def _evaluator(sims, games, grade, max_nodes):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.networks import get_network
  cfg = make_config(C4_FLAGS + ['--num_simulations', str(sims)])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                   human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games, verbose=False,
                   opp_playouts=0, grade=grade, grade_empties=DEFAULT_SCOPE, grade_nodes=max_nodes).items():
    setattr(cfg, k, v)
  ev = Evaluator(state)
  ev.load_network()
  return ev


def bench_games(reps, games, sims, max_nodes):
  evs = {'plain': _evaluator(sims, games, False, max_nodes), 'graded': _evaluator(sims, games, True, max_nodes)}
  seeds = list(range(games))
  for ev in evs.values():      # warm-up: library load, allocator, the solver's code object
    ev.play_games(64, seeds[:64], device_env=True)
  wall = {k: [] for k in evs}
  for _ in range(reps):
    for name, ev in evs.items():
      t0 = time.perf_counter()
      played = ev.play_games(games, seeds, device_env=True)
      wall[name].append(time.perf_counter() - t0)
  out = dict(games=games, simulations=sims, repetitions=reps, max_nodes=max_nodes, mean_length=float(np.mean([g.step for g in played])),
             scope_of_graded=DEFAULT_SCOPE)
  for name in evs:
    out[name] = dict(games_per_s=_spread([games / w for w in wall[name]]), wall_s=_spread(wall[name]))
  out['graded_over_plain'] = out['graded']['games_per_s']['median'] / out['plain']['games_per_s']['median']
  out['report'] = evs['graded'].grade_report
  # the grading alone on the kept games, per scope (three runs each: the replay on the host is the steady part)
  ev, scopes = evs['graded'], {}
  for e in SCOPES:
    ev.config.grade_empties = e
    secs, rep = [], None
    for _ in range(3):
      t0 = time.perf_counter()
      rep = ev.grade(played)
      secs.append(time.perf_counter() - t0)
    scopes[str(e)] = dict(seconds=_spread(secs), graded=rep['graded'], unsolved=rep['unsolved'], nodes=rep['nodes'],
                          optimal_rate=rep['optimal_rate'])
    print('scope', e, json.dumps(scopes[str(e)]), flush=True)
  out['grading_alone'] = scopes
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--games', type=int, default=4096)
  ap.add_argument('--sims', type=int, default=30)
  ap.add_argument('--table', action='store_true', help='the table search beside the plain one -> profiles/solve_table_bench.json')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  a.out = a.out or os.path.join(ROOT, 'profiles', 'solve_table_bench.json' if a.table else 'solve_bench.json')
  import torch
  from model_based_rl_amd.engine import Engine
  try:
    commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
  except Exception:
    commit = None
  max_nodes = Engine.SOLVE_NODES
  assert max_nodes in BUDGETS
  line = dict(what='the exact game solver that grades evaluation moves (scripts/solve_bench.py)',
              device=torch.cuda.get_device_name(0), git_head=commit)
  if a.table:
    line['what'] = 'the table search of the exact game solver beside the plain one (scripts/solve_bench.py --table)'
    line['solve'] = bench_table_solve(a.reps, (max_nodes, MEASURE_NODES))
    line['games'] = bench_table_games(a.reps, a.games, a.sims, max_nodes)
    games_s = line['games']['plain']['wall_s']['median']
    cheaper = [e for e in TABLE_SCOPES if line['games']['grading_alone_table'][str(e)]['seconds']['median'] < games_s]
    line['derived'] = dict(games_wall_s=games_s, largest_scope_cheaper_than_the_games=max(cheaper) if cheaper else None)
    s = json.dumps(line)
    print(s)
    with open(a.out, 'w') as f:
      f.write(s + '\n')
    return
  line['solve'] = bench_solve(a.reps, MEASURE_NODES)
  line['games'] = bench_games(a.reps, a.games, a.sims, max_nodes)
  games_s = line['games']['plain']['wall_s']['median']
  cheaper = [e for e in SCOPES if line['games']['grading_alone'][str(e)]['seconds']['median'] < games_s]
  rate = line['solve'][str(EMPTIES[-1])]['nodes_per_s']
  budget = 1
  while 2 * budget * POSITIONS * 7 / rate < 1.0:
    budget *= 2
  line['derived'] = dict(games_wall_s=games_s, default_scope=max(cheaper) if cheaper else None,
                         nodes_per_s_used=rate, default_budget=budget, seconds_if_every_unit_ran_out=budget * POSITIONS * 7 / rate)
  s = json.dumps(line)
  print(s)
  with open(a.out, 'w') as f:
    f.write(s + '\n')


if __name__ == '__main__':
  main()
