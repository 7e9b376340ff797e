"""The experiment --reanalyse_true_model was built for (DESIGN s7n): scripts/tictactoe_learning.py, seed 0, one run per arm --
  puct30                      PUCT self-play at 30 simulations as today
  puct30_reanalyse_true       the same with --reanalyse_rows 4096 --reanalyse_true_model: stored targets refreshed on the true rules
  true_rules30                self-play searched on the true rules (--selfplay_true_model)
  true_rules30_reanalyse_true the same with --reanalyse_rows 4096 --reanalyse_true_model
-- and the final checkpoints compared as the s7k table does, under the plain search: against the random mover, against the
1024-playout search, graded against the exact solver with the model's unroll by depth (--grade --grade_unroll 5), and every mutual
match (256 seeds, both seats, two random opening plies).  Writes ONE JSON line (default
profiles/true_model_reanalyse_tictactoe_learning.json).  An observation of one seed, not a claim.

Every training run is a fresh child process under its own time limit; a run that fails or runs out ends the call.

usage: python scripts/true_model_reanalyse_experiment.py [--training_steps 3000] [--environment TicTacToe] [--out FILE]"""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REANALYSE = ['--reanalyse_rows', '4096', '--reanalyse_true_model']
RUNS = {'puct30': [], 'puct30_reanalyse_true': REANALYSE, 'true_rules30': ['--selfplay_true_model'],
        'true_rules30_reanalyse_true': ['--selfplay_true_model'] + REANALYSE}
RUN_SECONDS = 420
UNROLL_KEYS = ('k', 'positions', 'reward_mae', 'value_mae', 'value_sign', 'policy_tv', 'top1_agree', 'illegal_mass', 'optimal_mass')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--training_steps', type=int, default=3000)
  ap.add_argument('--environment', default='TicTacToe', choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--seeds', type=int, default=256)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'true_model_reanalyse_tictactoe_learning.json'))
  a = ap.parse_args()
  tmp = tempfile.mkdtemp(prefix='mz_true_model_reanalyse_')
  out = dict(environment=a.environment, training_steps=a.training_steps, seed=0, runs={}, matches={})
  kept = {}
  for name, flags in RUNS.items():
    report, ckpt = os.path.join(tmp, name + '.json'), os.path.join(tmp, name + '.pt')
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'), '--environment', a.environment, '--training_steps',
           str(a.training_steps), '--grade', '--grade_unroll', '5', '--opp_playouts', '1024', '--keep_checkpoint', ckpt,
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
    g = rep.get('graded_vs_random_512_games', {}).get('trained', {})
    out['runs'][name] = dict(
        recipe=rep['recipe'], wall_seconds=time.time() - t0, train_seconds=rep['train_seconds'], selfplay_frames=rep['selfplay_frames'],
        selfplay_games=rep['selfplay_games'], reanalyse=rep.get('reanalyse'), vs_random_512_games=rep['vs_random_512_games']['trained'],
        vs_1024_playout_search_512_games=rep.get('vs_1024_playout_search_512_games', {}).get('trained'),
        optimal_move_rate={k: v.get('optimal_rate') for k, v in g.items()}, blunders={k: v.get('blunders') for k, v in g.items()},
        unroll={k: [{u: d.get(u) for u in UNROLL_KEYS} for d in v['unroll']['depth']] for k, v in g.items() if v.get('unroll')})
    kept[name] = ckpt
  if len(kept) == len(RUNS):
    import torch
    from model_based_rl_amd.config import make_config
    from model_based_rl_amd.match import play_match
    flags = ['--environment', a.environment, '--two_players', '--architecture', 'FCNetwork', '--td_steps', '10', '--discount', '1',
             '--known_bounds', '-1', '1', '--seed', '0', '--num_simulations', '30']
    states = {name: torch.load(kept[name], map_location='cpu', weights_only=False) for name in RUNS}

    def side(name):
      cfg = copy.copy(make_config(flags))
      for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                       human_opp=None).items():
        setattr(cfg, k, v)
      return {'config': cfg, 'weights': states[name]['weights'], 'training_step': states[name]['training_step']}
    names = list(RUNS)
    for i, x in enumerate(names):
      for y in names[i + 1:]:
        _, s = play_match(side(x), side(y), a.seeds, list(range(a.seeds)), opening_plies=2, batch=a.seeds)
        out['matches']['%s_vs_%s' % (x, y)] = {
            k: s[k] for k in ('wins', 'draws', 'losses', 'score', 'elo', 'elo_interval', 'mean_length') if k in s}
  line = json.dumps(out)
  print(line)
  with open(a.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
