"""Matches between two saved networks on the device games (TicTacToe, ConnectFour): checkpoint A against checkpoint B from
both seats, and the score.

Every seed is played twice, once per seating, in batches of up to --batch games of one seating.  A batch is one Match
(engine.Match, mz_match_*) over two engines, one per network, each with its own weights and num_simulations: every ply
is the mover's own initial inference, root preparation, search + walk (or the lookahead of --only_prior / --only_value)
and finalize, enqueued whole plies at a time; the host synchronises once per PLIES_PER_SYNC plies and touches no game.
Draws keep the evaluator's keys -- engines with seed 0 and env_id_offset = the batch's first seed, the walk under
MZ_RNG_EVAL and the Dirichlet noise keyed by the ply -- so a network against itself with no opening plays the games of
Evaluator.play_games(device_env=True).  The opening plies (--opening_plies) are uniform random legal moves keyed by the
game's seed alone (MZ_RNG_OPEN): both seatings of a seed start from the same position.

Per-side settings come from each state's config: num_simulations, temperature, only_prior, only_value,
use_exploration_noise, true_model (that side searches the true rules of the game, Engine.tm_search: the same checkpoint on
both sides with true_model (0, 1) prices its learned model in Elo), gumbel (that side searches with the Gumbel search,
Engine.gz_search, with its config's gumbel_* parameters).  One action is applied per ply, on FCNetwork checkpoints."""
import copy
import json
import math
import time

import numpy as np
import torch

from .engine import Engine, Match, flatten_weights
from .evaluate import _pack_draws, consecutive_seeds, decode_history
from .sides import MATCH_ENVS, Side, gumbel_params, per_side, refuse, refuse_match      # noqa: F401  (refuse_match: importable from here)

MAX_BATCH = 4096
PLIES_PER_SYNC = 8      # whole plies enqueued per host synchronisation (evaluate.MOVES_PER_SYNC)


def elo_difference(score):
  """400 log10(s / (1 - s)); None at s <= 0 or s >= 1, where it is not finite"""
  return None if not 0.0 < score < 1.0 else 400.0 * math.log10(score / (1.0 - score))


def score_summary(wins, draws, losses):
  """the score s = (W + D / 2) / N, the Elo difference and its 95 % interval from the trinomial standard error of s:
  sqrt((W (1 - s)^2 + D (1/2 - s)^2 + L s^2) / N) / sqrt(N); an end of the interval outside (0, 1) has no Elo (None)"""
  n = wins + draws + losses
  if n == 0:
    return dict(wins=0, draws=0, losses=0, games=0, score=None, score_se=None, elo=None, elo_interval=[None, None])
  s = (wins + 0.5 * draws) / n
  var = (wins * (1.0 - s) ** 2 + draws * (0.5 - s) ** 2 + losses * s ** 2) / n
  se = math.sqrt(var / n)
  return dict(wins=int(wins), draws=int(draws), losses=int(losses), games=int(n), score=s, score_se=se, elo=elo_difference(s),
              elo_interval=[elo_difference(s - 1.96 * se), elo_difference(s + 1.96 * se)])


class MatchGame(object):
  """A finished game of a match.  seating 0: net A moved first after the opening, 1: net B did.  result: for net A (+1 win,
  0 draw, -1 loss; a cut at max_steps is a draw).  Per net, index 0 = A and 1 = B, the means DeviceGame carries: pred_return,
  pred_value, mcts_value, search_depth, and searched (plies that net searched).  With keep_history the per-ply lists:
  history.actions / rewards / to_play / dones over every ply, nets (0 = A, 1 = B, -1 = an opening ply), and over the
  searched plies history.child_visits / root_values, pred_values, pred_rewards, search_depths, searched_by."""
  terminal = True
  history = None

  def __init__(self, seed, seating, result, length):
    self.seed, self.seating, self.result, self.step = int(seed), int(seating), int(result), int(length)


def summarize(games):
  """W / D / L of net A per seating and in total, score, Elo difference with its interval, mean game length"""
  out = {}
  for key, sel in (('total', games), ('a_first', [g for g in games if g.seating == 0]),
                   ('b_first', [g for g in games if g.seating == 1])):
    r = [g.result for g in sel]
    out[key] = score_summary(sum(x > 0 for x in r), sum(x == 0 for x in r), sum(x < 0 for x in r))
  out.update(out.pop('total'))
  out['mean_length'] = float(np.mean([g.step for g in games])) if games else None
  return out


def _side(cfg):
  """(mode, temperature, noise_on) of a config's Side"""
  return Side.of(cfg).plies_args


def _records(r, seeds, seating, opening, sides, keep_history):
  """Match.results() of one seating as MatchGame records; sides: the two nets' Sides"""
  colour_a = 1 if (seating == 0) == (opening % 2 == 0) else -1      # the player net A is: +1 moves first
  games = []
  for i, seed in enumerate(seeds):
    g = MatchGame(seed, seating, int(r['result'][i]) * colour_a, r['length'][i])
    nm = [max(int(r['n_searched'][k, i]), 1) for k in (0, 1)]
    g.searched = tuple(int(r['n_searched'][k, i]) for k in (0, 1))
    g.pred_return = tuple(float(r['sum_pred_reward'][k, i]) for k in (0, 1))
    g.pred_value = tuple(float(r['sum_pred_value'][k, i]) / nm[k] for k in (0, 1))
    g.mcts_value = tuple(float(r['sum_root_value'][k, i]) / nm[k] for k in (0, 1))
    g.search_depth = tuple(float(r['depth_mean'][k, i]) for k in (0, 1))
    if keep_history:
      g.nets = [int(x) for x in r['net'][i, :g.step]]
      g.searched_plies = [p for p in range(g.step) if g.nets[p] >= 0]
      g.searched_by = [g.nets[p] for p in g.searched_plies]
      decode_history(g, r, i, g.searched_plies, [sides[k] for k in g.searched_by], g.searched_plies)
    games.append(g)
  return games


def play_match(state_a, state_b, num_games, seeds=None, opening_plies=0, draws=None, keep_history=False, batch=None,
               device=None, stats=None, true_model=None, gumbel=None):
  """num_games seeds, each played in both seatings (2 * num_games games), up to `batch` games of one seating in lock-step.
  seeds: consecutive, one per game; None draws a base seed.  draws (parity runs): per seed a dict of given draws -- 'walk'
  [plies] uniforms and 'noise' [plies][A] Dirichlet draws, both indexed by the ply with the opening plies counted, and
  'opening' [k] indices into the legal actions of the opening positions -- used in both seatings.  Returns (games, summary):
  MatchGame records in the order (batch, seating, seed) and summarize(games).  stats: a dict that receives plies (game plies
  played), device_seconds and syncs.  true_model: (a, b), whether that side searches the true rules of the game instead
  of its learned model (Engine.tm_search; evaluate --true_model); None: each state's config.true_model.  gumbel: (a, b), whether that side
  searches with the Gumbel search instead of PUCT (Engine.gz_search; evaluate --gumbel) -- a true value takes the parameters
  of that side's config (gumbel_considered, gumbel_c_visit, gumbel_c_scale, gumbel_scale; their defaults where it has none), a
  dict gives Engine.set_gumbel's arguments; None: each state's config.gumbel."""
  ca, cb = state_a['config'], state_b['config']
  for name, given in (('true_model', true_model), ('gumbel', gumbel)):
    if given is not None and len(given) != 2:
      raise ValueError('play_match: %s takes one value per side, got %r' % (name, tuple(given)))
  sides = tuple(Side.of(c, None if true_model is None else bool(true_model[k]), None if gumbel is None else gumbel[k] or False)
                for k, c in enumerate((ca, cb)))
  refuse(ca, match=True, side=sides[0], other=cb)
  refuse(cb, match=True, side=sides[1])
  if not torch.cuda.is_available():
    raise RuntimeError('a match needs a HIP device (torch.cuda.is_available() is False); there is no CPU path.')
  device = torch.device(device if device is not None else 'cuda')
  max_steps = min(int(ca.max_steps), int(cb.max_steps))
  opening_plies = int(opening_plies)
  if not 0 <= opening_plies < max_steps:
    raise ValueError('play_match: opening_plies %d outside [0, max_steps = %d)' % (opening_plies, max_steps))
  batch = int(batch or getattr(ca, 'batch', None) or MAX_BATCH)
  seeds = consecutive_seeds(seeds, num_games, 'play_match takes consecutive seeds, one per game')
  weights = [flatten_weights(s['weights']) for s in (state_a, state_b)]
  A, rules = int(ca.action_space), [side.plies_args for side in sides]
  games, t_dev, syncs, plies = [], 0.0, 0, 0
  for lo in range(0, num_games, batch):
    sd = seeds[lo:lo + batch]
    B = len(sd)
    # the device RNG's key: (engine seed 0, env id = the game's seed, ply, step)
    engines = [Engine.from_config(c, B, device=device, seed=0, env_id_offset=sd[0]) for c in (ca, cb)]
    for e, w, side in zip(engines, weights, sides):
      e.set_weights(w)
      side.configure(e, ca.environment)
    match = Match(engines[0], engines[1], ca.environment, max_steps, keep_history)
    packed = None if draws is None else _pack_draws(draws[lo:lo + batch], B, A, 1, 'opening')
    for seating in (0, 1):
      match.reset(first_net=seating, opening_plies=opening_plies)
      if packed:
        match.set_draws(**packed)
      live, done = B, opening_plies
      t0 = time.perf_counter()
      live = match.plies(0, *zip(*rules))      # (the opening alone may end games)
      while live > 0 and done < match.log_cap:      # (every ply applies one action: at most cap plies)
        n = min(PLIES_PER_SYNC, match.log_cap - done)
        live = match.plies(n, *zip(*rules))
        syncs += 1
        done += n
      t_dev += time.perf_counter() - t0
      r = match.results()
      plies += int(r['length'].sum())
      games += _records(r, sd, seating, opening_plies, sides, keep_history)
    match.close()
    for e in engines:
      e.close()
  if stats is not None:
    stats.update(plies=plies, device_seconds=t_dev, syncs=syncs)
  return games, dict(summarize(games), true_model=[int(x.true_model) for x in sides], gumbel=[int(bool(x.gumbel)) for x in sides])


def match_states(args):
  """[(label, state)] of --saves_dir / --nets: one directory for every net, or one directory per net"""
  dirs, nets = list(args.saves_dir), list(args.nets)
  if len(nets) < 2:
    raise ValueError('--match needs at least two --nets (the same name twice plays a network against itself)')
  if len(dirs) == 1:
    dirs = dirs * len(nets)
  elif len(dirs) == 2 and len(nets) == 2:
    pass
  elif len(dirs) != len(nets):
    raise ValueError('--match takes one --saves_dir for all --nets, or one per net')
  out = []
  for i, (d, net) in enumerate(zip(dirs, nets)):
    state = torch.load(d + net, map_location=torch.device('cpu'), weights_only=False)
    label = 'net:%s' % state['training_step'] if len(set(dirs)) == 1 else 'path:%d, net:%s' % (i, state['training_step'])
    out.append((label, state))
  return out


# (a side's config attribute, the command-line list it is picked from, its type)
PER_SIDE = (('temperature', 'temperatures', float), ('only_prior', 'only_prior', int), ('only_value', 'only_value', int),
            ('use_exploration_noise', 'use_exploration_noise', int), ('true_model', 'true_model', int), ('gumbel', 'gumbel', int))


def side_state(state, args, side):
  """a checkpoint's state with side `side`'s settings of the command line in its config"""
  state = dict(state, config=copy.copy(state['config']))
  c = state['config']
  ns = per_side(args.num_simulations, side, strict=True)
  if ns is not None:
    c.num_simulations = int(ns)
  for name, flag, kind in PER_SIDE:
    setattr(c, name, kind(per_side(getattr(args, flag, [0]), side, strict=True)))
  c.gumbel_considered, c.gumbel_c_visit, c.gumbel_c_scale, c.gumbel_scale = gumbel_params(args)
  c.apply_mcts_actions = 1
  c.random_opp = c.human_opp = None
  c.batch = args.batch
  return state


def _side_label(label, cfg):
  return ', '.join([label] + Side.of(cfg).label_parts('temp:{:g}', lookahead_alone=False))


def main(args):
  """evaluate --match: every pair of --nets (round robin when more than two), the score table printed and written"""
  refuse(args, match=True)
  states = match_states(args)
  for _, s in states:
    refuse_match(s['config'], states[0][1]['config'])
  n = len(states)
  seeds = list(range(args.seed, args.seed + args.num_games)) if args.seed is not None else None
  pairs = []
  table = [[None] * n for _ in range(n)]
  labels = [label for label, _ in states]
  for i in range(n):
    for j in range(i + 1, n):
      sa, sb = side_state(states[i][1], args, 0), side_state(states[j][1], args, 1)
      la, lb = _side_label(labels[i], sa['config']), _side_label(labels[j], sb['config'])
      print("\n\033[92mMatch\033[0m ({}) against ({}): {} seeds, both seatings".format(la, lb, args.num_games))
      print("  A {}; B {}".format(Side.of(sa['config']).search_line(), Side.of(sb['config']).search_line()))
      stats = {}
      t0 = time.perf_counter()
      games, s = play_match(sa, sb, args.num_games, seeds, opening_plies=args.opening_plies, batch=args.batch, stats=stats)
      wall = time.perf_counter() - t0
      fmt = lambda v: 'n/a' if v is None else '%+.0f' % v
      for key, name in (('a_first', 'A moves first'), ('b_first', 'B moves first')):
        print("  {:14s} W {:5d}  D {:5d}  L {:5d}".format(name, s[key]['wins'], s[key]['draws'], s[key]['losses']))
      print("  {:14s} W {:5d}  D {:5d}  L {:5d}   score {:.3f}   Elo {} [{}, {}]   mean length {:.1f}".format(
          'total', s['wins'], s['draws'], s['losses'], s['score'], fmt(s['elo']), fmt(s['elo_interval'][0]),
          fmt(s['elo_interval'][1]), s['mean_length']))
      s.update(a=la, b=lb, a_index=i, b_index=j, plies_per_s=stats['plies'] / wall if wall > 0 else None)
      pairs.append(s)
      table[i][j], table[j][i] = s['score'], 1.0 - s['score']
  if n > 2:
    print("\nScores, row against column:")
    for i in range(n):
      print("  {:24s} ".format(labels[i]) + ' '.join('  -  ' if v is None else '%.3f' % v for v in table[i]))
  out = {'num_games': args.num_games, 'seed': args.seed, 'opening_plies': args.opening_plies, 'nets': labels, 'pairs': pairs,
         'cross_table': table}
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(out, f, indent=1)
  return out
