"""The experiment --selfplay_gumbel was built for (DESIGN s7i): scripts/tictactoe_learning.py, seed 0, four ways -- PUCT self-play
at 30 simulations as today, Gumbel self-play at 8 with the mean root value, Gumbel self-play at 8 with v_mix, and the mean-value run
with Gumbel Reanalyse (--reanalyse_rows 4096 --reanalyse_gumbel, DESIGN s7j) -- and the final
checkpoints compared: the mutual matches (256 seeds, both seats, two random opening plies) evaluated with PUCT at 30 and with the
Gumbel search at 8, and from each run's own report the --grade optimal-move rates, the scores against the 1024-playout search and
the wall-clock.  Writes ONE JSON line (default profiles/gumbel_selfplay_tictactoe_learning.json).  An observation, not a claim.

Every training run is a fresh child process under its own time limit; a run that fails or runs out ends the call.

usage: python scripts/gumbel_selfplay_experiment.py [--training_steps 3000] [--environment TicTacToe] [--out FILE]"""
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

RUNS = {'puct30': [], 'gumbel8_mean': ['--selfplay_gumbel', '--num_simulations', '8'],
        'gumbel8_vmix': ['--selfplay_gumbel', '--num_simulations', '8', '--selfplay_gumbel_value', 'vmix'],
        # (DESIGN s7j: the gumbel8_mean run with its stored targets refreshed by Gumbel Reanalyse passes of 4096 rows)
        'gumbel8_mean_reanalyse': ['--selfplay_gumbel', '--num_simulations', '8', '--reanalyse_rows', '4096', '--reanalyse_gumbel']}
RUN_SECONDS = 420


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--training_steps', type=int, default=3000)
  ap.add_argument('--environment', default='TicTacToe', choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--seeds', type=int, default=256)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gumbel_selfplay_tictactoe_learning.json'))
  a = ap.parse_args()
  tmp = tempfile.mkdtemp(prefix='mz_gumbel_selfplay_')
  out = dict(environment=a.environment, training_steps=a.training_steps, seed=0, runs={}, matches={})
  kept = {}
  for name, flags in RUNS.items():
    report, ckpt = os.path.join(tmp, name + '.json'), os.path.join(tmp, name + '.pt')
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'), '--environment', a.environment, '--training_steps',
           str(a.training_steps), '--grade', '--opp_playouts', '1024', '--keep_checkpoint', ckpt, '--out', report] + flags
    t0 = time.time()
    try:
      r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_SECONDS)
    except subprocess.TimeoutExpired:
      out['runs'][name] = dict(failed='ran out of its %d s' % RUN_SECONDS)
      break      # (nothing more is started on the device after a run that hung)
    if r.returncode != 0 or not os.path.exists(report):
      out['runs'][name] = dict(failed=r.returncode, stderr=r.stderr[-800:])
      break
    rep = json.load(open(report))
    graded = rep.get('graded_vs_random_512_games', {}).get('trained', {})
    out['runs'][name] = dict(
        recipe=rep['recipe'], wall_seconds=time.time() - t0, train_seconds=rep['train_seconds'], selfplay_frames=rep['selfplay_frames'],
        selfplay_games=rep['selfplay_games'], vs_random_512_games=rep['vs_random_512_games']['trained'],
        vs_1024_playout_search_512_games=rep.get('vs_1024_playout_search_512_games', {}).get('trained'),
        optimal_move_rate={k: v.get('optimal_rate') for k, v in graded.items()},
        blunders={k: v.get('blunders') for k, v in graded.items()})
    kept[name] = ckpt
  if len(kept) == len(RUNS):
    import torch
    from model_based_rl_amd.config import make_config
    from model_based_rl_amd.match import play_match
    flags = ['--environment', a.environment, '--two_players', '--architecture', 'FCNetwork', '--td_steps', '10', '--discount', '1',
             '--known_bounds', '-1', '1', '--seed', '0']

    def side(name, sims):
      st = torch.load(kept[name], map_location='cpu', weights_only=False)
      cfg = copy.copy(make_config(flags + ['--num_simulations', str(sims)]))
      for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                       human_opp=None).items():
        setattr(cfg, k, v)
      return {'config': cfg, 'weights': st['weights'], 'training_step': st['training_step']}
    names = list(RUNS)
    for i, x in enumerate(names):
      for y in names[i + 1:]:
        for label, sims, gz in (('puct30', 30, None), ('gumbel8', 8, (1, 1))):
          _, s = play_match(side(x, sims), side(y, sims), a.seeds, list(range(a.seeds)), opening_plies=2, batch=a.seeds, gumbel=gz)
          out['matches']['%s_vs_%s_evaluated_%s' % (x, y, label)] = {
              k: s[k] for k in ('wins', 'draws', 'losses', 'score', 'elo', 'elo_interval', 'mean_length') if k in s}
  line = json.dumps(out)
  print(line)
  with open(a.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
