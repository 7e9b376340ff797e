"""End-to-end check that the stack LEARNS: MuZero on TicTacToe with the reference's recipe (README: --two_players
--td_steps 10 --discount 1 --known_bounds -1 1, FCNetwork, 30 simulations) -- the games played by the device environment
(whole moves inside the two-player launch), the native replay with sign-flipped n-step targets, the stock-PyTorch learner
on the same GPU -- then the trained network's MCTS agent (temperature 0, no exploration noise) against a uniformly random
opponent on the host's TicTacToe rules, 512 games as each side, next to the untrained network.

  python scripts/tictactoe_learning.py [--training_steps 3000] [--num_envs 1024] [--no_support [--scalar_loss Huber]]
                                       [--environment ConnectFour] [--out profiles/r03_tictactoe_learning.json]
                                       [--opp_playouts 1024] [--symmetry] [--grade [--grade_table] [--grade_unroll K]] [--true_model] [--gumbel]
                                       [--selfplay_gumbel [--num_simulations 8] [--selfplay_gumbel_value vmix] ...]
                                       [--selfplay_true_model [--selfplay_true_model_loop]]
                                       [--reanalyse_rows N [--reanalyse_every K] [--reanalyse_gumbel [--reanalyse_gumbel_scale S]]
                                                           [--reanalyse_true_model]]
--reanalyse_rows / --reanalyse_every / --reanalyse_gumbel / --reanalyse_gumbel_scale / --reanalyse_true_model are train's flags, passed
on to the training run (--reanalyse_gumbel: Reanalyse with the Gumbel search for a --selfplay_gumbel run; --reanalyse_true_model:
Reanalyse on the game's true rules, with --selfplay_true_model or with plain PUCT self-play; reanalyse.py).
--selfplay_gumbel adds train's flag (self-play searched with the Gumbel search, the learner trained on pi'; selfplay_search.py) with
its --selfplay_gumbel_* parameters, and --num_simulations sets the simulations of the TRAINING run's self-play; the evaluation
blocks below stay as they are -- PUCT at 30 simulations unless --gumbel is given.
--selfplay_true_model adds train's flag (self-play searched on the game's true rules below the root, selfplay_search.py;
--selfplay_true_model_loop: its two-launch form) to the training run; the evaluation blocks stay as they are.
--environment ConnectFour runs the same recipe on the device Connect Four environment and plays the matches through the
evaluator's device-environment path (evaluate.Evaluator.play_games(device_env=True): the games never leave the GPU).
--symmetry adds train's flag (every sample trained on one of the equivalent images of its position, symmetry.py) to the training run.
--no_support adds the flag (scalar value / reward heads, MSE or Huber loss) to the recipe, for training and for the matches."""
import argparse, json, os, sys, time, types
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LINES = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 3, 6], [1, 4, 7], [2, 5, 8], [0, 4, 8], [2, 4, 6]])


def play_vs_random(weights, agent_side, games=512, sims=30, seed=0, no_support=False):
  """agent (MCTS, T = 0, no noise) vs a uniformly random opponent, `games` boards in lock-step through the stepwise ABI;
  returns (wins, draws, losses) of the agent.  agent_side: +1 moves first, -1 second."""
  from model_based_rl_amd.engine import Engine
  rng = np.random.RandomState(seed)
  eng = Engine(games, 9, 9, sims, two_players=True, known_bounds=(-1.0, 1.0), discount=1.0, seed=seed, no_support=no_support)
  eng.set_weights(weights)
  board = np.zeros((games, 9), np.int64); turn = np.ones(games, np.int64); live = np.ones(games, bool)
  result = np.zeros(games, np.int64)          # +1 agent won, -1 agent lost, 0 draw
  for ply in range(9):
    if not live.any():
      break
    legal = (board == 0)
    act = np.zeros(games, np.int64)
    agent_moves = live & (turn == agent_side)
    if agent_moves.any():
      obs = (turn[:, None] * board).astype(np.float32)
      lg = legal.astype(np.uint8); lg[~live] = 1               # (finished boards: any mask, their result is not read)
      eng.initial_inference(obs)
      eng.root_prepare(turn.astype(np.int8), lg, None, device_rng=False)
      eng.search()
      out = eng.finalize(0.0, np.full(games, 0.5))
      act = out['action'].cpu().numpy().astype(np.int64)
    rnd = np.array([rng.choice(np.flatnonzero(legal[i])) if live[i] and legal[i].any() else 0 for i in range(games)])
    act = np.where(agent_moves, act, rnd)
    idx = np.flatnonzero(live)
    assert np.all(board[idx, act[idx]] == 0)
    board[idx, act[idx]] = turn[idx]
    won = np.any(np.abs(board[:, LINES].sum(-1)) == 3, axis=1) & live
    result[won] = np.where(turn[won] == agent_side, 1, -1)
    full = ~(board == 0).any(1)
    live &= ~won & ~full
    turn = -turn
  eng.close()
  return int((result == 1).sum()), int((result == 0).sum()), int((result == -1).sum())


def play_vs_random_device(config, weights, agent_side, games=512, seed=0, opp_playouts=0, grade=None, grade_table=False,
                          grade_unroll=None, true_model=False, gumbel=False):
  """the same match through the evaluator's device-environment path (any environment with a device form); `weights` a
  state_dict.  Returns (wins, draws, losses) of the agent.  agent_side: +1 moves first, -1 second.  opp_playouts > 0: the
  opponent is the playout search of that budget (evaluate --opp_playouts) instead of the random mover.  grade: a list that
  receives the report of the agent's moves graded against the exact solver (evaluate --grade), or None: no grading;
  grade_table: with the table search (evaluate --grade_table); grade_unroll: K, the report then carries the model by unroll
  depth under 'unroll' (evaluate --grade_unroll K); true_model: the agent searches the true rules of the game instead of its
  learned model (evaluate --true_model); gumbel: the agent searches with the Gumbel search instead of PUCT (evaluate --gumbel,
  its default parameters)."""
  import copy
  from model_based_rl_amd.evaluate import Evaluator, game_return
  cfg = copy.copy(config)
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1,
                   random_opp=-agent_side, human_opp=None, render=False, save_mcts=False, save_gif_as='', label='vs random',
                   verbose=False, batch=games, device_env=True, keep_history=False, opp_playouts=int(opp_playouts), grade=grade is not None,
                   grade_table=bool(grade_table) and grade is not None,
                   grade_unroll=int(grade_unroll) if grade_unroll and grade is not None else None, true_model=int(bool(true_model)), gumbel=int(bool(gumbel))).items():
    setattr(cfg, k, v)
  ev = Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  ret = np.array([game_return(g) for g in ev.play_games(games, list(range(seed, seed + games)))])
  if grade is not None:
    grade.append(ev.grade_report if ev.grade_unroll_report is None else dict(ev.grade_report, unroll=ev.grade_unroll_report))
  return int((ret > 0).sum()), int((ret == 0).sum()), int((ret < 0).sum())


def build_parser():
  ap = argparse.ArgumentParser()
  ap.add_argument('--environment', default='TicTacToe', choices=['TicTacToe', 'ConnectFour'])
  ap.add_argument('--training_steps', type=int, default=3000)
  ap.add_argument('--num_envs', type=int, default=1024)
  ap.add_argument('--out', default=None)
  ap.add_argument('--no_support', action='store_true')
  ap.add_argument('--scalar_loss', default='MSE', choices=['MSE', 'Huber'])
  ap.add_argument('--reanalyse_rows', type=int, default=0, help='train --reanalyse_rows (0: off)')
  ap.add_argument('--reanalyse_every', type=int, default=None, help='train --reanalyse_every')
  ap.add_argument('--reanalyse_gumbel', action='store_true',
                  help='train --reanalyse_gumbel: with --selfplay_gumbel and --reanalyse_rows, the passes search with the Gumbel search and write pi\'')
  ap.add_argument('--reanalyse_gumbel_scale', type=float, default=None, help='train --reanalyse_gumbel_scale')
  ap.add_argument('--reanalyse_true_model', action='store_true',
                  help='train --reanalyse_true_model: with --reanalyse_rows, the passes search the stored positions on the true rules')
  ap.add_argument('--keep_checkpoint', default=None, help='copy the run\'s last checkpoint to this file')
  ap.add_argument('--match_against', default=None, help='a checkpoint kept by another run: the last checkpoint also plays it, from both seats')
  ap.add_argument('--opp_playouts', type=int, default=0,
                  help='also play the 512 games per side against a playout search of this many playouts per move (evaluate --opp_playouts)')
  ap.add_argument('--symmetry', action='store_true', help='train --symmetry: board-symmetry augmentation of the training batches')
  ap.add_argument('--grade', action='store_true',
                  help='also grade the agent\'s moves of 512 games per side against the exact solver (evaluate --grade), before and after training')
  ap.add_argument('--grade_table', action='store_true', help='--grade: solve with the table search (evaluate --grade_table)')
  ap.add_argument('--grade_unroll', type=int, default=None, metavar='K',
                  help='--grade: also the model unrolled K steps along the graded games, by depth (evaluate --grade_unroll K)')
  ap.add_argument('--true_model', action='store_true',
                  help='also play (and with --grade, grade) the 512 games per side with the search on the true rules of the game '
                       '(evaluate --true_model): next to the plain games, the difference is what the learned model costs')
  ap.add_argument('--gumbel', action='store_true',
                  help='also play (and with --grade, grade) the 512 games per side with the Gumbel search (evaluate --gumbel, default '
                       'parameters) at the same number of simulations: next to the plain games, what the search rule changes')
  ap.add_argument('--num_simulations', type=int, default=None,
                  help='simulations per move of the training run\'s self-play (default: the recipe\'s 30); the evaluation blocks keep 30')
  ap.add_argument('--selfplay_gumbel', action='store_true',
                  help='train --selfplay_gumbel: self-play with the Gumbel search, pi\' as the policy target (use with --num_simulations 8 or 16)')
  ap.add_argument('--selfplay_gumbel_considered', type=int, default=None, help='train --selfplay_gumbel_considered')
  ap.add_argument('--selfplay_gumbel_c_visit', type=float, default=None, help='train --selfplay_gumbel_c_visit')
  ap.add_argument('--selfplay_gumbel_c_scale', type=float, default=None, help='train --selfplay_gumbel_c_scale')
  ap.add_argument('--selfplay_gumbel_scale', type=float, default=None, help='train --selfplay_gumbel_scale')
  ap.add_argument('--selfplay_gumbel_value', default=None, choices=['mean', 'vmix'], help='train --selfplay_gumbel_value')
  ap.add_argument('--selfplay_true_model', action='store_true',
                  help='train --selfplay_true_model: self-play searched on the true rules below the root; the evaluation blocks are unchanged')
  ap.add_argument('--selfplay_true_model_loop', action='store_true', help='train --selfplay_true_model_loop')
  return ap


def recipe(a):
  """(base, extra) of the parsed arguments: base is the recipe the evaluation blocks build their configs from, base + extra the
  training run's flags (a flag given again in extra overrides base's)"""
  base = ['--environment', a.environment, '--two_players', '--architecture', 'FCNetwork', '--td_steps', '10', '--discount', '1',
          '--known_bounds', '-1', '1', '--num_simulations', '30', '--seed', '0', '--num_envs', str(a.num_envs)]
  if a.no_support:
    base += ['--no_support', '--scalar_loss', a.scalar_loss]
  extra = ['--reanalyse_rows', str(a.reanalyse_rows)] if a.reanalyse_rows else []
  if a.reanalyse_rows and a.reanalyse_every:
    extra += ['--reanalyse_every', str(a.reanalyse_every)]
  if a.reanalyse_gumbel:      # (given without --reanalyse_rows or --selfplay_gumbel: train's preflight says so)
    extra += ['--reanalyse_gumbel']
    if a.reanalyse_gumbel_scale is not None:
      extra += ['--reanalyse_gumbel_scale', str(a.reanalyse_gumbel_scale)]
  if a.reanalyse_true_model:      # (given without --reanalyse_rows: train's preflight says so)
    extra += ['--reanalyse_true_model']
  if a.symmetry:
    extra += ['--symmetry']
  if a.num_simulations is not None:
    extra += ['--num_simulations', str(a.num_simulations)]
  if a.selfplay_gumbel:
    extra += ['--selfplay_gumbel']
    for k in ('considered', 'c_visit', 'c_scale', 'scale', 'value'):
      v = getattr(a, 'selfplay_gumbel_' + k)
      if v is not None:
        extra += ['--selfplay_gumbel_' + k, str(v)]
  if a.selfplay_true_model:
    extra += ['--selfplay_true_model'] + (['--selfplay_true_model_loop'] if a.selfplay_true_model_loop else [])
  return base, extra


def main():
  ap = build_parser()
  a = ap.parse_args()
  if a.grade_table and not a.grade:
    ap.error('--grade_table: it chooses the search that --grade solves with and grades nothing without --grade.')
  if a.grade_unroll is not None and not a.grade:
    ap.error('--grade_unroll: it unrolls the model along the games --grade keeps and does nothing without --grade.')
  if a.grade_unroll is not None and not 1 <= a.grade_unroll <= 16:
    ap.error('--grade_unroll: the depth is 1 to 16 dynamics steps, got %d.' % a.grade_unroll)
  from model_based_rl_amd import train
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  from model_based_rl_amd.engine import flatten_weights
  if not a.selfplay_gumbel and any(getattr(a, 'selfplay_gumbel_' + k) is not None for k in ('considered', 'c_visit', 'c_scale', 'scale', 'value')):
    ap.error('--selfplay_gumbel_*: parameters of --selfplay_gumbel, which is not given.')
  if a.selfplay_true_model_loop and not a.selfplay_true_model:
    ap.error('--selfplay_true_model_loop: an option of --selfplay_true_model, which is not given.')
  base, extra = recipe(a)
  torch.manual_seed(0)
  untrained_sd = get_network(make_config(base), torch.device('cpu')).state_dict()
  if a.environment == 'TicTacToe':
    match = lambda sd, side: play_vs_random(flatten_weights(sd), side, no_support=a.no_support)
  else:
    match = lambda sd, side: play_vs_random_device(make_config(base), sd, side)
  before = {side: match(untrained_sd, side) for side in (1, -1)}
  saves = os.path.join('/tmp', 'mz_%s_learning_%d' % ('ttt' if a.environment == 'TicTacToe' else 'c4', os.getpid()))
  t0 = time.time()
  thr = train.main(base + extra + ['--max_moves', '-1', '--training_steps', str(a.training_steps), '--stored_before_train', '20000',
                           '--batch_size', '256', '--window_size', '200000', '--send_weights_frequency', '100',
                           '--weight_sync_frequency', '16', '--use_gpu_for', 'actors', 'learner', '--gpu_turns', '--runs_dir', saves,
                           '--run_tag', 'learn', '--save_state_frequency', str(a.training_steps), '--learner_log_frequency', '500'])
  seconds = time.time() - t0
  import glob
  kept = sorted(glob.glob(os.path.join(saves, '**', 'saves', '*'), recursive=True), key=os.path.getmtime)
  state = torch.load(kept[-1], map_location='cpu', weights_only=False)
  after = {side: match(state['weights'], side) for side in (1, -1)}
  if a.opp_playouts:      # an absolute line: the same games against a search whose strength ignores the weights
    vs_playouts = {name: {side: play_vs_random_device(make_config(base), sd, side, opp_playouts=a.opp_playouts) for side in (1, -1)}
                   for name, sd in (('untrained', untrained_sd), ('trained', state['weights']))}
  if a.grade:      # the absolute line per evaluation point: optimal-move rate, blunders, value errors (no opponent's noise in it)
    graded = {}
    for name, sd in (('untrained', untrained_sd), ('trained', state['weights'])):
      for side_, key in ((1, 'agent_first'), (-1, 'agent_second')):
        got = []
        play_vs_random_device(make_config(base), sd, side_, grade=got, grade_table=a.grade_table, grade_unroll=a.grade_unroll)
        graded.setdefault(name, {})[key] = got[0]
  if a.true_model:      # the same weights with a perfect model: the plain results' distance to these is the learned model's share
    true_rules, graded_true = {}, {}
    for name, sd in (('untrained', untrained_sd), ('trained', state['weights'])):
      for side_, key in ((1, 'agent_first'), (-1, 'agent_second')):
        got = [] if a.grade else None
        true_rules.setdefault(name, {})[key] = play_vs_random_device(make_config(base), sd, side_, grade=got, grade_table=a.grade_table,
                                                                     true_model=True)
        if a.grade:
          graded_true.setdefault(name, {})[key] = got[0]
  if a.gumbel:      # the same weights and simulations under the Gumbel search
    gumbel_res, graded_gumbel = {}, {}
    for name, sd in (('untrained', untrained_sd), ('trained', state['weights'])):
      for side_, key in ((1, 'agent_first'), (-1, 'agent_second')):
        got = [] if a.grade else None
        gumbel_res.setdefault(name, {})[key] = play_vs_random_device(make_config(base), sd, side_, grade=got, grade_table=a.grade_table,
                                                                     gumbel=True)
        if a.grade:
          graded_gumbel.setdefault(name, {})[key] = got[0]
  # the last checkpoint against the first kept one, from both seats (match.play_match); where the run kept a single
  # checkpoint, against the untrained network
  from model_based_rl_amd.match import play_match
  if len(kept) > 1:
    first = torch.load(kept[0], map_location='cpu', weights_only=False)
    opponent = 'checkpoint %d' % int(first['training_step'])
  else:
    first, opponent = {'weights': untrained_sd, 'training_step': 0}, 'untrained network'

  def side(st):
    import copy
    cfg = copy.copy(make_config(base))
    for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, random_opp=None,
                     human_opp=None).items():
      setattr(cfg, k, v)
    return {'config': cfg, 'weights': st['weights'], 'training_step': st['training_step']}
  _, vs_first = play_match(side(state), side(first), 256, list(range(256)), opening_plies=2, batch=256)
  out = {'recipe': ' '.join(base + extra), 'training_steps': int(state['training_step']), 'train_seconds': seconds,
         'selfplay_frames': thr['frames'], 'selfplay_games': thr['games'], 'learner': thr.get('learner'),
         'vs_random_512_games': {'untrained': {'agent_first (win, draw, loss)': before[1], 'agent_second': before[-1]},
                                 'trained': {'agent_first (win, draw, loss)': after[1], 'agent_second': after[-1]}},
         'match_last_vs_first': dict(vs_first, a='checkpoint %d' % int(state['training_step']), b=opponent, seeds=256,
                                     opening_plies=2)}
  if a.reanalyse_rows:      # what the actor logged per pass (actors._maybe_reanalyse): how much of the replay the passes rewrote
    from model_based_rl_amd.logger import read_metrics
    logged = [read_metrics(f) for f in glob.glob(os.path.join(saves, '**', 'metrics.csv'), recursive=True)]
    tag = lambda t: [v for m in logged for _, v in m.get('reanalyse/' + t, [])]
    out['reanalyse'] = {'passes': len(tag('rows')), 'rows': int(sum(tag('rows'))), 'seconds': float(sum(tag('seconds'))),
                        'mean_policy_l1_last': (tag('mean_policy_l1') or [None])[-1]}
  if a.opp_playouts:
    out['vs_%d_playout_search_512_games' % a.opp_playouts] = {
        name: {'agent_first (win, draw, loss)': r[1], 'agent_second': r[-1]} for name, r in vs_playouts.items()}
  if a.grade:
    out['graded_vs_random_512_games'] = graded
  if a.true_model:
    out['true_model_vs_random_512_games (win, draw, loss)'] = true_rules
    if a.grade:
      out['true_model_graded_vs_random_512_games'] = graded_true
  if a.gumbel:
    out['gumbel_vs_random_512_games (win, draw, loss)'] = gumbel_res
    if a.grade:
      out['gumbel_graded_vs_random_512_games'] = graded_gumbel
  if a.keep_checkpoint:
    torch.save({'weights': state['weights'], 'training_step': int(state['training_step'])}, a.keep_checkpoint)
  if a.match_against:
    other = torch.load(a.match_against, map_location='cpu', weights_only=False)
    _, vs_other = play_match(side(state), side(other), 256, list(range(256)), opening_plies=2, batch=256)
    out['match_last_vs_given'] = dict(vs_other, a='this run, checkpoint %d' % int(state['training_step']),
                                      b='%s, checkpoint %d' % (os.path.basename(a.match_against), int(other['training_step'])),
                                      seeds=256, opening_plies=2)
  print(json.dumps(out))
  if a.out:
    json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
  main()
