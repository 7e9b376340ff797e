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
from .envs import BOARD_ENVS as MATCH_ENVS
from .game import History

MAX_BATCH = 4096
PLIES_PER_SYNC = 8      # whole plies enqueued per host synchronisation (evaluate.MOVES_PER_SYNC)


def _all(x):
  return list(x) if isinstance(x, (list, tuple)) else [x]


def refuse_match(args_or_config, other=None):
  """one sentence per configuration --match leaves out (NotImplementedError, starting '--match: '); other: the second
  checkpoint's config, for what the two must share.  Host arithmetic only: no device is touched."""
  c = args_or_config
  env = getattr(c, 'environment', None)
  if env is not None and env not in MATCH_ENVS:
    raise NotImplementedError('--match: the environment %s is not a two-player device game; matches are played on %s.'
                              % (env, ' and '.join(MATCH_ENVS)))
  if any(int(x) != 1 for x in _all(getattr(c, 'apply_mcts_actions', 1))):
    raise NotImplementedError('--match: --apply_mcts_actions must be 1; a ply of a match applies exactly one action.')
  if getattr(c, 'norm_obs', False):
    raise NotImplementedError('--match: --norm_obs is not applied by the device games.')
  if getattr(c, 'random_opp', None):
    raise NotImplementedError('--match: --random_opp has no place in a match; both sides are networks (give --nets two names).')
  if getattr(c, 'human_opp', None):
    raise NotImplementedError('--match: --human_opp is an interactive tool; both sides of a match are networks.')
  if getattr(c, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise NotImplementedError('--match: the architecture %s has no device match path; FCNetwork checkpoints only.' % c.architecture)
  if other is not None:
    refuse_match(other)
    if getattr(c, 'environment', None) != getattr(other, 'environment', None):
      raise NotImplementedError('--match: the two checkpoints play a different environment (%s and %s).'
                                % (getattr(c, 'environment', None), getattr(other, 'environment', None)))
    if bool(getattr(c, 'no_support', False)) != bool(getattr(other, 'no_support', False)):
      raise NotImplementedError('--match: the two checkpoints differ in no_support; their value heads are not comparable.')
    for key in ('value_support', 'reward_support'):
      if tuple(getattr(c, key, (-15, 15))) != tuple(getattr(other, key, (-15, 15))):
        raise NotImplementedError('--match: the two checkpoints have different supports (%s %s and %s).'
                                  % (key, tuple(getattr(c, key, (-15, 15))), tuple(getattr(other, key, (-15, 15)))))


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
  only_prior, only_value = bool(getattr(cfg, 'only_prior', 0)), bool(getattr(cfg, 'only_value', 0))
  if only_prior and only_value:
    raise ValueError('only_prior and only_value exclude each other')
  return (1 if only_prior else 2 if only_value else 0, float(getattr(cfg, 'temperature', 0) or 0),
          bool(getattr(cfg, 'use_exploration_noise', 0)))


def _pack_draws(draws, B, A):
  """the per-game draw dicts as the dense arrays Match.set_draws uploads, padded with zeros past a game's own draws"""
  out = {}
  if any('walk' in d for d in draws):
    n = max(1, max(len(d.get('walk', ())) for d in draws))
    out['walk'] = np.zeros((B, n), np.float64)
    for i, d in enumerate(draws):
      w = np.asarray([np.asarray(x, np.float64).reshape(-1)[0] for x in d.get('walk', ())], np.float64)
      out['walk'][i, :len(w)] = w
  if any('noise' in d for d in draws):
    n = max(1, max(len(d.get('noise', ())) for d in draws))
    out['noise'] = np.zeros((B, n, A), np.float64)
    for i, d in enumerate(draws):
      for p, nz in enumerate(d.get('noise', ())):
        out['noise'][i, p] = np.asarray(nz, np.float64)
  if any(len(d.get('opening', ())) for d in draws):
    n = max(len(d.get('opening', ())) for d in draws)
    out['opening'] = np.zeros((B, n), np.int32)
    for i, d in enumerate(draws):
      o = np.asarray(d.get('opening', ()), np.int32).reshape(-1)
      out['opening'][i, :len(o)] = o
  return out


def _records(r, seeds, seating, opening, sides, sims, keep_history):
  """Match.results() of one seating as MatchGame records"""
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
      n = g.step
      h = g.history = History()
      h.actions = [int(x) for x in r['actions'][i, :n]]
      h.rewards = [float(x) for x in r['rewards'][i, :n]]
      h.to_play = [int(np.sign(x)) for x in r['mover'][i, :n]]
      h.steps = list(range(n))
      h.dones = [abs(int(x)) == 2 for x in r['mover'][i, :n]]      # (the rules' done: not the cut at max_steps)
      g.nets = [int(x) for x in r['net'][i, :n]]
      ply = [p for p in range(n) if g.nets[p] >= 0]
      g.searched_plies = ply
      g.searched_by = [g.nets[p] for p in ply]
      h.child_visits = [[float(x) for x in r['child_visits'][i, p]] for p in ply]
      h.root_values = [float(r['root_values'][i, p]) for p in ply]
      g.pred_values = [float(r['pred_values'][i, p]) for p in ply]
      g.pred_rewards = [float(r['pred_rewards'][i, p]) for p in ply]
      g.search_depths = [[0] if sides[g.nets[p]][0] == 1 else [1] if sides[g.nets[p]][0] == 2 else
                         [int(x) for x in r['depths'][i, p, :sims[g.nets[p]]]] for p in ply]
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
  from .evaluate import gumbel_params, refuse_gumbel, refuse_true_model
  ca, cb = state_a['config'], state_b['config']
  refuse_match(ca, cb)
  if true_model is None:
    true_model = (getattr(ca, 'true_model', 0), getattr(cb, 'true_model', 0))
  true_model = tuple(int(bool(x)) for x in true_model)
  if len(true_model) != 2:
    raise ValueError('play_match: true_model takes one value per side, got %r' % (true_model,))
  for c, t in zip((ca, cb), true_model):
    refuse_true_model(_with_true_model(c, t), match=True)
  if gumbel is None:
    gumbel = (getattr(ca, 'gumbel', 0), getattr(cb, 'gumbel', 0))
  if len(gumbel) != 2:
    raise ValueError('play_match: gumbel takes one value per side, got %r' % (gumbel,))
  gz = []
  for c, t, g in zip((ca, cb), true_model, gumbel):
    if not g:
      gz.append(None)
      continue
    m, cv, cs, sc = gumbel_params(c)
    kw = dict(dict(max_considered=m, c_visit=cv, c_scale=cs, gumbel_scale=sc), **(g if isinstance(g, dict) else {}))
    c1 = _with_true_model(c, t)
    c1.gumbel, c1.gumbel_considered, c1.gumbel_c_visit, c1.gumbel_c_scale, c1.gumbel_scale = (
        1, kw['max_considered'], kw['c_visit'], kw['c_scale'], kw['gumbel_scale'])
    refuse_gumbel(c1, match=True)
    gz.append(kw)
  if not torch.cuda.is_available():
    raise RuntimeError('a match needs a HIP device (torch.cuda.is_available() is False); there is no CPU path.')
  device = torch.device(device if device is not None else 'cuda')
  sides = (_side(ca), _side(cb))
  sims = (int(ca.num_simulations), int(cb.num_simulations))
  max_steps = min(int(ca.max_steps), int(cb.max_steps))
  opening_plies = int(opening_plies)
  if not 0 <= opening_plies < max_steps:
    raise ValueError('play_match: opening_plies %d outside [0, max_steps = %d)' % (opening_plies, max_steps))
  batch = int(batch or getattr(ca, 'batch', None) or MAX_BATCH)
  if seeds is None:
    base = int(np.random.randint(0, 2 ** 30))
    seeds = list(range(base, base + num_games))
  seeds = [int(s) for s in seeds]
  if len(seeds) != num_games or any(s != seeds[0] + i for i, s in enumerate(seeds)):
    raise ValueError('play_match takes consecutive seeds, one per game')
  weights = [flatten_weights(s['weights']) for s in (state_a, state_b)]
  A = int(ca.action_space)
  games, t_dev, syncs, plies = [], 0.0, 0, 0
  for lo in range(0, num_games, batch):
    sd = seeds[lo:lo + batch]
    B = len(sd)
    # the device RNG's key: (engine seed 0, env id = the game's seed, ply, step)
    engines = [Engine.from_config(c, B, device=device, seed=0, env_id_offset=sd[0]) for c in (ca, cb)]
    for e, w, t, g in zip(engines, weights, true_model, gz):
      e.set_weights(w)
      if t:
        e.set_true_model(ca.environment)
      if g:
        e.set_gumbel(True, **g)
    match = Match(engines[0], engines[1], ca.environment, max_steps, keep_history)
    packed = None if draws is None else _pack_draws(draws[lo:lo + batch], B, A)
    for seating in (0, 1):
      match.reset(first_net=seating, opening_plies=opening_plies)
      if packed:
        match.set_draws(**packed)
      live, done = B, opening_plies
      t0 = time.perf_counter()
      live = match.plies(0, *zip(*sides))      # (the opening alone may end games)
      while live > 0 and done < match.log_cap:      # (every ply applies one action: at most cap plies)
        n = min(PLIES_PER_SYNC, match.log_cap - done)
        live = match.plies(n, *zip(*sides))
        syncs += 1
        done += n
      t_dev += time.perf_counter() - t0
      r = match.results()
      plies += int(r['length'].sum())
      games += _records(r, sd, seating, opening_plies, sides, sims, keep_history)
    match.close()
    for e in engines:
      e.close()
  if stats is not None:
    stats.update(plies=plies, device_seconds=t_dev, syncs=syncs)
  return games, dict(summarize(games), true_model=list(true_model), gumbel=[int(bool(g)) for g in gz])


def _with_true_model(cfg, t):
  c = copy.copy(cfg)
  c.true_model = int(t)
  return c


def _pick(values, side):
  values = _all(values)
  if len(values) not in (1, 2):
    raise ValueError('--match takes per-side lists of length one (both sides) or two, got %r' % (values,))
  return values[side if len(values) == 2 else 0]


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


def side_state(state, args, side):
  """a checkpoint's state with side `side`'s settings of the command line in its config"""
  from .evaluate import gumbel_params
  state = dict(state, config=copy.copy(state['config']))
  c = state['config']
  ns = _pick(args.num_simulations, side)
  if ns is not None:
    c.num_simulations = int(ns)
  c.temperature = float(_pick(args.temperatures, side))
  c.only_prior, c.only_value = int(_pick(args.only_prior, side)), int(_pick(args.only_value, side))
  c.use_exploration_noise = int(_pick(args.use_exploration_noise, side))
  c.true_model = int(_pick(getattr(args, 'true_model', [0]), side))
  c.gumbel = int(_pick(getattr(args, 'gumbel', [0]), side))
  c.gumbel_considered, c.gumbel_c_visit, c.gumbel_c_scale, c.gumbel_scale = gumbel_params(args)
  c.apply_mcts_actions = 1
  c.random_opp = c.human_opp = None
  c.batch = args.batch
  return state


def _side_label(label, cfg):
  mode = 'only prior' if cfg.only_prior else 'only value' if cfg.only_value else 'sims:%d' % cfg.num_simulations
  return '%s, %s%s%s%s%s' % (label, mode, ', temp:%g' % cfg.temperature if cfg.temperature else '',
                             ', with noise' if cfg.use_exploration_noise else '',
                             ', true rules' if getattr(cfg, 'true_model', 0) else '',
                             ', gumbel' if getattr(cfg, 'gumbel', 0) else '')


def main(args):
  """evaluate --match: every pair of --nets (round robin when more than two), the score table printed and written"""
  from .evaluate import gumbel_line, gumbel_params, refuse_unsupported
  refuse_match(args)
  refuse_unsupported(args)
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
      print("  A {}; B {}".format(gumbel_line(sa['config']), gumbel_line(sb['config'])))
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
