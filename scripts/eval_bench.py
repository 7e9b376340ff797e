"""Cost of the evaluator's device work (csrc/mz_eval.hip.h) and its end-to-end rate; prints ONE JSON line.

  walk       B = 4096 LunarLander shapes (obs 8, 4 actions), 30 simulations: initial inference + root, the search, and
             mz_eval_walk (apply_mcts_actions 1, with the per-simulation search depths) timed with HIP events, each as the
             median over `reps` moves; the walk as a fraction of the search (estimate to report against: <= 3 %)
  lookahead  mz_eval_lookahead('only_value'): the B*A recurrent rows + the choice, against ONE mz_recurrent_inference
             launch on the same B*A rows (estimate: <= 1.5x)
  games      4096 TicTacToe games against a uniformly random opponent, the agent moving first and second
             (evaluate.Evaluator.play_games, 30 simulations, temperature 0): games/s and the share of wall time spent in
             host environment stepping

usage: python scripts/eval_bench.py [--reps 50] [--out line.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _weights(O, A, seed):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'LunarLander-v2'], action_space=A, obs_space=(O,))
  torch.manual_seed(seed)
  return get_network(cfg, torch.device('cpu')).state_dict()


def _timed(fn, reps, warmup=5):
  import torch
  for _ in range(warmup):
    fn()
  ms = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return float(np.median(ms))


def bench_walk(reps, B=4096, O=8, A=4, sims=30):
  import torch
  from model_based_rl_amd.engine import Engine
  eng = Engine(B, O, A, sims, seed=1)
  eng.set_weights(_weights(O, A, 0))
  obs = torch.randn(B, O, device=eng.device)
  temp = torch.zeros(B, dtype=torch.float64, device=eng.device)

  def root():
    eng.initial_inference(obs)
    eng.root_prepare(None, None, None)
  root()
  eng.search()
  root_ms = _timed(root, reps)
  search_ms = _timed(lambda: (root(), eng.search()), reps) - root_ms
  from model_based_rl_amd import _abi
  from model_based_rl_amd.engine import _ptr
  w = eng.eval_walk(1, temp)           # (the raw call on these buffers below: no allocation inside the timed region)

  def walk():
    _abi.check(eng.lib.mz_eval_walk(eng._h, 1, _ptr(temp), None, 5, _ptr(w['actions']), _ptr(w['pred_rewards']),
                                    _ptr(w['n_actions']), _ptr(w['path_lengths']), eng.stream), 'mz_eval_walk')
  walk_ms = _timed(walk, reps)
  eng.close()
  return dict(B=B, obs=O, actions=A, sims=sims, root_us=1e3 * root_ms, search_us=1e3 * search_ms, walk_us=1e3 * walk_ms,
              walk_over_search=walk_ms / search_ms)


def bench_lookahead(reps, B=4096, O=8, A=4):
  import torch
  from model_based_rl_amd.engine import Engine, H
  eng = Engine(B, O, A, 5, seed=1)
  eng.set_weights(_weights(O, A, 0))
  eng.initial_inference(torch.randn(B, O, device=eng.device))
  eng.root_prepare(None, None, None)
  n = B * A
  hid = eng.root_outputs()[2].repeat_interleave(A, 0).contiguous()
  act = torch.arange(A, dtype=torch.int32, device=eng.device).repeat(B)
  ho = torch.empty(n, H, device=eng.device); r = torch.empty(n, device=eng.device); v = torch.empty(n, device=eng.device)
  lg = torch.empty(n, A, device=eng.device)
  from model_based_rl_amd import _abi
  from model_based_rl_amd.engine import _ptr

  def rows():
    _abi.check(eng.lib.mz_recurrent_inference(eng._h, _ptr(hid), _ptr(act), n, _ptr(ho), _ptr(r), _ptr(v), _ptr(lg),
                                              eng.stream), 'mz_recurrent_inference')
  out = eng.eval_lookahead('only_value')

  def look():
    _abi.check(eng.lib.mz_eval_lookahead(eng._h, 2, _ptr(out['action']), _ptr(out['pred_reward']), _ptr(out['child_visits']),
                                         None, None, eng.stream), 'mz_eval_lookahead')
  rows_ms, look_ms = _timed(rows, reps), _timed(look, reps)
  eng.close()
  return dict(B=B, actions=A, rows=n, recurrent_rows_us=1e3 * rows_ms, lookahead_us=1e3 * look_ms,
              lookahead_over_rows=look_ms / rows_ms)


def bench_games(games=4096, sims=30):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.networks import get_network
  out = {}
  for side in (-1, 1):        # random_opp -1: the agent moves first
    cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1',
                       '--num_simulations', str(sims)])
    torch.manual_seed(0)
    state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 0}
    for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=side,
                     human_opp=None, render=False, save_mcts=False, save_gif_as='', label='bench', batch=games).items():
      setattr(cfg, k, v)
    ev = Evaluator(state)
    ev.load_network()
    ev.play_games(64, list(range(64)))          # (warm-up: library load, graph capture)
    ev.host_seconds = 0.0
    t0 = time.perf_counter()
    played = ev.play_games(games, list(range(games)))
    wall = time.perf_counter() - t0
    ret = np.array([sum(g.history.rewards) for g in played])
    out['agent_first' if side == -1 else 'agent_second'] = dict(
        games=games, games_per_s=games / wall, host_share=ev.host_seconds / wall, wall_s=wall,
        wins=int((ret > 0).sum()), draws=int((ret == 0).sum()), losses=int((ret < 0).sum()), mean_length=float(np.mean([g.step for g in played])))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  import torch
  line = dict(what='evaluator device work and end-to-end rate (scripts/eval_bench.py)', device=torch.cuda.get_device_name(0),
              walk=bench_walk(a.reps), lookahead=bench_lookahead(a.reps), tictactoe_vs_random=bench_games(),
              targets=dict(walk_over_search_max=0.03, lookahead_over_rows_max=1.5))
  line['targets']['walk_met'] = line['walk']['walk_over_search'] <= 0.03
  line['targets']['lookahead_met'] = line['lookahead']['lookahead_over_rows'] <= 1.5
  s = json.dumps(line)
  print(s)
  if a.out:
    with open(a.out, 'w') as f:
      f.write(s + '\n')


if __name__ == '__main__':
  main()
