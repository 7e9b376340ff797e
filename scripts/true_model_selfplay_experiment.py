"""The experiment --selfplay_true_model was built for (DESIGN s7k): scripts/tictactoe_learning.py, seed 0, one run per arm -- PUCT
self-play at 30 simulations as today, and self-play searched on the true rules at 30 -- and the final checkpoints compared, each
under the plain search and under the true-rules search (evaluate --true_model 1): against the random mover, against the
1024-playout search, graded against the exact solver with the model's unroll by depth (--grade --grade_unroll 5), and the mutual
match (256 seeds, both seats, two random opening plies) under both searches.  What separates the arms at equal learner steps is
the learned model's share of the search targets.  Writes ONE JSON line (default profiles/true_model_selfplay_tictactoe_learning.json).
An observation of one seed, not a claim.

Every training run is a fresh child process under its own time limit; a run that fails or runs out ends the call.

usage: python scripts/true_model_selfplay_experiment.py [--training_steps 3000] [--environment TicTacToe] [--out FILE]"""
import argparse
import copy
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = {'puct30': [], 'true_rules30': ['--selfplay_true_model']}
RUN_SECONDS = 420


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--training_steps', type=int, default=3000)
  ap.add_argument('--environment', default='TicTacToe', choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--seeds', type=int, default=256)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'true_model_selfplay_tictactoe_learning.json'))
  a = ap.parse_args()
  tmp = tempfile.mkdtemp(prefix='mz_true_model_selfplay_')
  out = dict(environment=a.environment, training_steps=a.training_steps, seed=0, runs={}, matches={})
  kept = {}
  for name, flags in RUNS.items():
    report, ckpt = os.path.join(tmp, name + '.json'), os.path.join(tmp, name + '.pt')
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'), '--environment', a.environment, '--training_steps',
           str(a.training_steps), '--grade', '--grade_unroll', '5', '--true_model', '--opp_playouts', '1024', '--keep_checkpoint', ckpt,
           '--out', report] + flags
    t0 = time.time()
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_SECONDS)
    except subprocess.TimeoutExpired:
      out['runs'][name] = dict(failed='ran out of its %d s' % RUN_SECONDS)
      break      # (nothing more is started on the device after a run that hung)
    if r.returncode != 0 or not os.path.exists(report):
      out['runs'][name] = dict(failed=r.returncode, stderr=r.stderr[-800:])
      break
    print('%s: trained and evaluated in %.0f s' % (name, time.time() - t0), file=sys.stderr, flush=True)
    rep = json.load(open(report))

    def graded(key):
      g = rep.get(key, {}).get('trained', {})
      return dict(optimal_move_rate={k: v.get('optimal_rate') for k, v in g.items()}, blunders={k: v.get('blunders') for k, v in g.items()},
                  unroll={k: v.get('unroll') for k, v in g.items() if v.get('unroll') is not None})
    out['runs'][name] = dict(
        recipe=rep['recipe'], wall_seconds=time.time() - t0, train_seconds=rep['train_seconds'], selfplay_frames=rep['selfplay_frames'],
        selfplay_games=rep['selfplay_games'],
        evaluated_plain=dict(vs_random_512_games=rep['vs_random_512_games']['trained'],
                             vs_1024_playout_search_512_games=rep.get('vs_1024_playout_search_512_games', {}).get('trained'),
                             graded=graded('graded_vs_random_512_games')),
        evaluated_true_rules=dict(vs_random_512_games=rep.get('true_model_vs_random_512_games (win, draw, loss)', {}).get('trained'),
                                  graded=graded('true_model_graded_vs_random_512_games')))
    kept[name] = ckpt
  if len(kept) == len(RUNS):
    import torch
    from model_based_rl_amd.config import make_config
    from model_based_rl_amd.match import play_match
    spec = importlib.util.spec_from_file_location('tictactoe_learning', os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'))
    learning = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(learning)
    flags = ['--environment', a.environment, '--two_players', '--architecture', 'FCNetwork', '--td_steps', '10', '--discount', '1',
             '--known_bounds', '-1', '1', '--seed', '0', '--num_simulations', '30']
    states = {name: torch.load(kept[name], map_location='cpu', weights_only=False) for name in RUNS}
    for name in RUNS:      # the playout opponent under the true-rules search (the learning script plays it under the plain one)
      out['runs'][name]['evaluated_true_rules']['vs_1024_playout_search_512_games'] = {
          key: learning.play_vs_random_device(make_config(flags), states[name]['weights'], side, opp_playouts=1024, true_model=True)
          for side, key in ((1, 'agent_first (win, draw, loss)'), (-1, 'agent_second'))}

    def side(name):
      cfg = copy.copy(make_config(flags))
      for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                       human_opp=None).items():
        setattr(cfg, k, v)
      return {'config': cfg, 'weights': states[name]['weights'], 'training_step': states[name]['training_step']}
    x, y = list(RUNS)
    for label, tm in (('plain', (0, 0)), ('true_rules', (1, 1))):
      _, s = play_match(side(x), side(y), a.seeds, list(range(a.seeds)), opening_plies=2, batch=a.seeds, true_model=tm)
      out['matches']['%s_vs_%s_evaluated_%s' % (x, y, label)] = {
          k: s[k] for k in ('wins', 'draws', 'losses', 'score', 'elo', 'elo_interval', 'mean_length') if k in s}
  line = json.dumps(out)
  print(line)
  with open(a.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
