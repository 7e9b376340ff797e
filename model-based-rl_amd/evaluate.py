"""Evaluation of saved networks: the reference's evaluate.py (Evaluator, get_label, state_generator, run, the summary), with
the games played in lock-step on the GPU instead of one at a time.

Per move and live game: initial inference, root expansion (+ Dirichlet noise with --use_exploration_noise), then either
the search and the walk that picks the actions to apply (mz_search + mz_eval_walk) or the one-step lookahead of
--only_prior / --only_value (mz_eval_lookahead); the host environments apply the actions exactly as evaluate.py:331-376 does.
Game i of a run uses seed + i (evaluate.py:476-479): its host draws (the random opponent, the Dirichlet noise) come from
np.random.RandomState(seed_i + 3) -- the numpy stream set_all_seeds(seed_i) leaves (utils.py:136-144) -- and its device draws
(select_action's uniforms) from the counter-based RNG keyed by seed_i, so a game's record does not depend on the batch it
was played in.

With --device_env the games themselves live on the device as well (Engine.eval_env_*: the device rules of TicTacToe,
ConnectFour and CartPole): the host enqueues whole moves in chunks and synchronises once per chunk, every draw comes from
the counter-based RNG keyed by the game's seed (or is given by the caller), and the games come back as DeviceGame records.
The host-environment path is the default.

With --match the nets play each other instead of being evaluated one by one (match.py): every pair of --nets, every seed
from both seats, on the device games.

What a configuration's move rule is (Side) and what each option refuses (refuse, the refuse_* names) is stated in sides.py.

FCNetwork checkpoints on host environments (envs.get_environment) only; the interactive tools of the reference (rendering,
GIFs, plots, human play, MCTS PNG dumps) are refused.  One departure from the reference's output: its '[Game done]' line after
every game (evaluate.py:376-379) is printed only with --verbose -- thousands of games are played per configuration here, and
the summary block carries the same numbers."""
import copy
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

from .config import CARTPOLE_TIME_LIMITS, get_evaluation_args
from .engine import Engine, flatten_weights
from .envs import DEVICE_ENVS, get_environment      # noqa: F401  (DEVICE_ENVS: read from here by callers)
from .game import History
from .sides import (Side, gumbel_params, refuse, refuse_device_env, refuse_gumbel, refuse_grade, refuse_grade_unroll,      # noqa: F401
                    refuse_opp_playouts, refuse_true_model, refuse_unsupported)      # (the per-option entry points: importable from here)

MAX_BATCH = 4096
MOVES_PER_SYNC = 8      # --device_env: whole moves enqueued per host synchronisation


class DeviceGame(object):
  """A finished game of the device-environment path: what the summary and the CLI read, from the device's accumulators.
  With keep_history also the per-move lists under the host path's names (history.actions / rewards / to_play / dones /
  steps / child_visits / root_values, pred_values, pred_rewards, search_depths) and n_actions."""
  terminal = True
  history = None

  def __init__(self, step, ret, pred_return, pred_value, mcts_value, search_depth):
    self.step, self.ret, self.pred_return = int(step), float(ret), float(pred_return)
    self.pred_value, self.mcts_value, self.search_depth = float(pred_value), float(mcts_value), float(search_depth)


def game_return(game):
  return game.ret if isinstance(game, DeviceGame) else sum(game.history.rewards)


class SummaryTools(object):

  def summary(self, games):
    """the six (mean, std) pairs print_summary prints (evaluate.py:79-104), as a dict"""
    if games and isinstance(games[0], DeviceGame):
      cols = (('length', 'step'), ('return', 'ret'), ('pred_return', 'pred_return'), ('pred_value', 'pred_value'),
              ('mcts_value', 'mcts_value'), ('search_depth', 'search_depth'))
      return {key: [float(np.mean([getattr(g, f) for g in games])), float(np.std([getattr(g, f) for g in games]))]
              for key, f in cols}
    lengths = [game.step for game in games]
    returns = [sum(game.history.rewards) for game in games]
    pred_returns = [sum(game.pred_rewards) for game in games]
    pred_values = [np.mean(game.pred_values) for game in games]
    root_values = [np.mean(game.history.root_values) for game in games]
    # (the reference's quirk, kept: max() of the per-move lists of search depths is the LEXICOGRAPHIC maximum list, and its
    # mean is taken -- not the deepest simulation)
    search_depths = [np.mean(max(game.search_depths)) for game in games]
    out = {}
    for key, vals in (('length', lengths), ('return', returns), ('pred_return', pred_returns), ('pred_value', pred_values),
                      ('mcts_value', root_values), ('search_depth', search_depths)):
      out[key] = [float(np.mean(vals)), float(np.std(vals))]
    return out

  def print_summary(self, games):
    s = self.summary(games)
    print("\n\033[92mEvaluation finished! - label: ({})\033[0m".format(self.config.label))
    print("Average length: {:.1f}({:.1f})".format(*s['length']))
    print("Average return: {:.1f}({:.1f})".format(*s['return']))
    print("Average predicted return: {:.1f}({:.1f})".format(*s['pred_return']))
    print("Average predicted value: {:.1f}({:.1f})".format(*s['pred_value']))
    print("Average mcts value: {:.1f}({:.1f})".format(*s['mcts_value']))
    print("Average search depth: {:.1f}({:.1f})\n".format(*s['search_depth']))
    return s


class Evaluator(SummaryTools):

  def __init__(self, state, device=None):
    self.config = state['config']
    self.state = state
    if getattr(self.config, 'architecture', 'FCNetwork') != 'FCNetwork':
      raise NotImplementedError('the evaluator runs FCNetwork checkpoints only (%s has no batched evaluation path here)'
                                % self.config.architecture)
    refuse(self.config, lenient=True)      # (play_games(device_env=True) may still name the device path)
    self.grade_report = None      # --grade: the report of the last play_games (solver.grade_games)
    self.grade_unroll_report = None      # --grade_unroll K: the model by unroll depth on the same games (solver.grade_unroll)
    if not torch.cuda.is_available():
      raise RuntimeError('the evaluator needs a HIP device (torch.cuda.is_available() is False); there is no CPU path.')
    self.device = torch.device(device if device is not None else 'cuda')
    self.batch = int(getattr(self.config, 'batch', None) or MAX_BATCH)
    self.weights = None
    self.host_seconds = 0.0
    self.device_seconds = 0.0      # --device_env: wall time inside Engine.eval_env_moves, and the synchronisations it made
    self.device_syncs = 0
    if getattr(self.config, 'norm_obs', False):
      self.obs_min = np.array(self.config.obs_range[::2], dtype=np.float32)
      self.obs_max = np.array(self.config.obs_range[1::2], dtype=np.float32)
      self.obs_range = self.obs_max - self.obs_min

  def load_network(self):
    self.weights = flatten_weights(self.state['weights'])
    self.state = None

  def play_game(self, environment, seed=None, draws=None):
    """one game (evaluate.py:242-385) on a one-tree engine; seed: the game's seed (run() passes it)"""
    return self.play_games(1, None if seed is None else [seed], environments=[environment],
                           draws=None if draws is None else [draws])[0]

  def play_games(self, num_games, seeds=None, environments=None, draws=None, device_env=False, keep_history=False,
                 start_states=None, true_model=False, gumbel=False):
    """num_games games, up to self.batch of them in lock-step per engine.  seeds: one per game, consecutive (seed + i); None
    draws a base seed.  draws (parity runs): per game a dict of recorded draws -- 'walk' [moves][M] uniforms, 'noise' [moves][A]
    Dirichlet draws at the legal positions, 'opp' the random opponent's choices (indices into the legal actions).
    device_env (or config.device_env): the games live on the device environments and come back as DeviceGame records, with
    keep_history (or config.keep_history) carrying the per-move lists; start_states [num_games][4]: CartPole's start states
    instead of the counter RNG's (device path only).  true_model (or config.true_model): the moves are searched on the true
    rules (Engine.tm_search; device path, TicTacToe / ConnectFour).  gumbel (or config.gumbel): the moves are searched with the
    Gumbel search (Engine.gz_search; device path; True: the config's gumbel_* parameters, else their defaults; or a dict of
    Engine.set_gumbel's arguments)."""
    device_env = bool(device_env or getattr(self.config, 'device_env', False))
    side = Side.of(self.config, true_model or None, gumbel or None)
    refuse(self.config, device_env=device_env, side=side)
    grade = bool(getattr(self.config, 'grade', False))
    keep_history = bool(keep_history or grade or getattr(self.config, 'keep_history', False))
    assert self.weights is not None, '.load_network() needs to be called before playing.'
    if device_env and environments is not None:
      raise ValueError('play_games: a device-environment run builds no host environment')
    if start_states is not None and not device_env:
      raise ValueError('play_games: start_states are the device path\'s; give the host path environments that hold them')
    seeds = consecutive_seeds(seeds, num_games, 'play_games takes consecutive seeds, one per game (evaluate.py:476-479)')
    games = []
    for lo in range(0, num_games, self.batch):
      hi = min(num_games, lo + self.batch)
      if device_env:
        games += self._play_batch_device(seeds[lo:hi], None if draws is None else draws[lo:hi],
                                         None if start_states is None else start_states[lo:hi], keep_history, side)
        continue
      envs = environments[lo:hi] if environments is not None else [get_environment(self.config) for _ in range(lo, hi)]
      games += self._play_batch(envs, seeds[lo:hi], None if draws is None else draws[lo:hi], side)
    if grade:
      self.grade_report = self.grade(games)
      if getattr(self.config, 'grade_unroll', None):
        self.grade_unroll_report = self.grade_unroll(games)
    return games

  def _graded(self, games, solve, weights=False):
    """a solver's report on the keep_history games, from an engine that lives as long as the call; solve(solver, engine,
    **the keyword arguments grade_games and grade_unroll share)"""
    from . import solver
    cfg = self.config
    t0 = time.perf_counter()
    opp = getattr(cfg, 'random_opp', None)
    eng = Engine.from_config(cfg, min(len(games), self.batch), device=self.device, seed=0)
    try:
      if weights:
        eng.set_weights(self.weights)
      report = solve(solver, eng,
                     max_empties=None if cfg.environment == 'TicTacToe' else int(getattr(cfg, 'grade_empties', solver.DEFAULT_EMPTIES)),
                     graded_seat=None if opp is None else -int(opp),
                     max_nodes=int(getattr(cfg, 'grade_nodes', solver.DEFAULT_NODES)),
                     table=bool(getattr(cfg, 'grade_table', False)))
    finally:
      eng.close()
    report['seconds'] = time.perf_counter() - t0
    return report

  def grade(self, games):
    """--grade: the keep_history games graded against the exact solver (solver.grade_games) -- the network's moves where
    --random_opp seats an opponent, both sides' otherwise; TicTacToe every position, ConnectFour those with at most
    config.grade_empties empty cells"""
    return self._graded(games, lambda solver, eng, **kw: solver.grade_games(games, self.config.environment, eng, **kw))

  def grade_unroll(self, games):
    """--grade_unroll K: the model unrolled K steps along the moves of the same keep_history games, against the real
    positions and the exact solver (solver.grade_unroll), in --grade's scope: the positions where the network is to move
    where --random_opp seats an opponent, both seats' otherwise; truth for TicTacToe everywhere, for ConnectFour at
    positions with at most config.grade_empties empty cells"""
    return self._graded(games, lambda solver, eng, **kw: solver.grade_unroll(games, self.config.environment, eng,
                                                                             int(self.config.grade_unroll), **kw), weights=True)

  def _play_batch_device(self, seeds, draws, start_states, keep_history, side=None):
    """_play_batch with the games on the device environments: whole moves are enqueued MOVES_PER_SYNC at a time
    (Engine.eval_env_moves: observe, initial inference, root, search + walk or lookahead, finalize, apply), and the host
    only reads the number of games still live after each chunk.  side: the move rule (default: the config's); whichever
    search it names, everything around the search is the same."""
    cfg = self.config
    side = side or Side.of(cfg)
    refuse(cfg, device_env=True, side=side)
    opp_playouts = int(getattr(cfg, 'opp_playouts', 0) or 0)
    B, A = len(seeds), int(cfg.action_space)
    two = bool(cfg.two_players)
    t_batch = time.perf_counter()
    # the device RNG's key: (engine seed 0, env id = the game's seed, move, step)
    eng = Engine.from_config(cfg, B, device=self.device, seed=0, env_id_offset=seeds[0])
    eng.set_weights(self.weights)
    side.configure(eng, cfg.environment)
    eng.eval_env_reset(cfg.environment, int(cfg.max_steps), CARTPOLE_TIME_LIMITS.get(cfg.environment, 0),
                       getattr(cfg, 'random_opp', None) if two else None, keep_history)
    if opp_playouts:
      eng.eval_env_set_opponent(opp_playouts)
    if draws is not None or start_states is not None:
      eng.eval_env_set_draws(start_states=None if start_states is None else np.ascontiguousarray(start_states, np.float64).reshape(B, 4),
                             **_pack_draws(draws, B, A, side.max_actions, 'opp', walk=side.mode == 0, noise=side.noise_on))
    live, moves, t_dev = B, 0, 0.0
    while live > 0 and moves < eng.eval_log_cap:      # (every move applies at least one action: at most cap moves)
      n = min(MOVES_PER_SYNC, eng.eval_log_cap - moves)
      t0 = time.perf_counter()
      live = eng.eval_env_moves(n, side.mode, side.max_actions, side.temperature, side.noise_on)
      t_dev += time.perf_counter() - t0
      self.device_syncs += 1
      moves += n
    r = eng.eval_env_results()
    eng.close()
    games = []
    for i in range(B):
      nm = max(int(r['n_moves'][i]), 1)
      g = DeviceGame(r['step'][i], r['sum_reward'][i], r['sum_pred_reward'][i], r['sum_pred_value'][i] / nm,
                     r['sum_root_value'][i] / nm, r['depth_mean'][i])
      g.seed = seeds[i]
      if keep_history:
        k = int(r['n_moves'][i])
        decode_history(g, r, i, range(k), [side] * k, range(g.step))
        g.n_actions = [int(x) for x in r['n_actions'][i, :k]]
      if getattr(cfg, 'verbose', False):
        msg = "\033[92m[Game done]\033[0m --> "
        msg += "length: {:.1f}, return: {:.1f}, pred return: {:.1f}, pred value: {:.1f}, mcts value: {:.1f}"
        print(msg.format(g.step, g.ret, g.pred_return, g.pred_value, g.mcts_value))
      games.append(g)
    self.device_seconds += t_dev
    self.host_seconds += time.perf_counter() - t_batch - t_dev
    return games

  def _play_batch(self, envs, seeds, draws, side=None):
    cfg = self.config
    side = side or Side.of(cfg)
    B, A = len(envs), int(cfg.action_space)
    O = int(np.prod(cfg.obs_space))
    only_prior, only_value, noise_on = side.mode == 1, side.mode == 2, side.noise_on
    two = bool(cfg.two_players)
    random_opp = getattr(cfg, 'random_opp', None)
    M, T = side.max_actions, side.temperature
    # the device RNG's key: (engine seed 0, env id = the game's seed, move, step)
    eng = Engine.from_config(cfg, B, device=self.device, seed=0, env_id_offset=seeds[0])
    eng.set_weights(self.weights)
    rngs = [np.random.RandomState(s + 3) for s in seeds]
    opp_pos = [0] * B
    games = []
    for env, s in zip(envs, seeds):
      env.seed(s)
      g = cfg.new_game(env)
      g.pred_values, g.pred_rewards, g.search_depths = [], [], []
      games.append(g)
    t_host = 0.0
    move = 0
    while True:
      th = time.perf_counter()
      live = [i for i in range(B) if not games[i].terminal]
      if not live:
        break
      obs = np.zeros((B, O), np.float32)
      legal = np.ones((B, A), np.uint8)
      legal_actions = [None] * B
      to_play = np.ones(B, np.int8)
      noise = np.zeros((B, A)) if noise_on else None
      uniform = np.zeros((B, M)) if draws is not None else None
      for i in live:
        g = games[i]
        ob = np.float32(g.get_observation(-1))
        if getattr(cfg, 'norm_obs', False):
          ob = (ob - self.obs_min) / self.obs_range
        obs[i] = np.asarray(ob, np.float32).reshape(-1)
        env = g.environment
        la = env.legal_actions() if hasattr(env, 'legal_actions') else np.arange(A)
        legal_actions[i] = la
        legal[i] = 0
        legal[i, np.asarray(la, np.int64)] = 1
        to_play[i] = g.to_play
        if noise_on:      # Node.add_exploration_noise (mcts.py:57-61): one Dirichlet draw over the legal actions
          nz = draws[i]['noise'][move] if draws is not None else rngs[i].dirichlet([cfg.root_dirichlet_alpha] * len(la))
          nz = np.asarray(nz, np.float64)
          noise[i, np.asarray(la, np.int64)] = nz[np.asarray(la, np.int64)] if draws is not None else nz
        if draws is not None and not (only_prior or only_value):
          w = np.asarray(draws[i]['walk'][move], np.float64)
          uniform[i, :len(w)] = w
      t_host += time.perf_counter() - th
      eng.initial_inference(obs)
      eng.root_prepare(to_play, legal, noise, device_rng=False)
      if only_prior or only_value:
        out = eng.eval_lookahead('only_prior' if only_prior else 'only_value')
        actions, preds = out['action'].reshape(B, 1), out['pred_reward'].reshape(B, 1)
        n_act = torch.ones(B, dtype=torch.int32)
        child_visits = out['child_visits']
        root_values = torch.zeros(B, dtype=torch.float64)
        depths = None
      else:
        eng.search()
        w = eng.eval_walk(M, T, uniform, move=move)
        fin = eng.finalize(0.0, np.full(B, 0.5), move=move)
        actions, preds, n_act, depths = w['actions'], w['pred_rewards'], w['n_actions'], w['path_lengths']
        child_visits, root_values = fin['child_visits'], fin['root_value']
      pred_value = eng.root_outputs()[0].cpu().numpy()
      actions, preds, n_act = actions.cpu().numpy(), preds.cpu().numpy(), n_act.cpu().numpy()
      child_visits, root_values = child_visits.cpu().numpy(), root_values.cpu().numpy()
      depths = None if depths is None else depths.cpu().numpy()
      th = time.perf_counter()
      for i in live:
        g = games[i]
        g.search_depths.append([0] if only_prior else [1] if only_value else [int(x) for x in depths[i]])
        g.pred_values.append(float(pred_value[i]))
        g.store_search_statistics([float(x) for x in child_visits[i]], float(root_values[i]))
        for j in range(int(n_act[i])):      # evaluate.py:331-374
          action, reward = int(actions[i, j]), float(preds[i, j])
          g.pred_rewards.append(reward)
          if two:
            if g.to_play == random_opp:
              if draws is not None:
                action = int(legal_actions[i][draws[i]['opp'][opp_pos[i]]])
                opp_pos[i] += 1
              else:
                action = int(rngs[i].choice(legal_actions[i]))
            to_play_i = g.to_play
          g.apply(action)
          if g.terminal or g.step >= cfg.max_steps:
            g.environment.was_real_done = True
            g.terminal = True
            if two and to_play_i == random_opp:
              g.history.rewards[-1] *= -1
            break
        if getattr(cfg, 'verbose', False) and g.terminal:
          msg = "\033[92m[Game done]\033[0m --> "
          msg += "length: {:.1f}, return: {:.1f}, pred return: {:.1f}, pred value: {:.1f}, mcts value: {:.1f}"
          print(msg.format(g.step, np.sum(g.history.rewards), np.sum(g.pred_rewards), np.mean(g.pred_values),
                           np.mean(g.history.root_values)))
      t_host += time.perf_counter() - th
      move += 1
    eng.close()
    self.host_seconds += t_host
    for g in games:
      g.history.observations = []
      g.environment = None
    return games


def _with(cfg, **kv):
  """a shallow copy of a config with some attributes set"""
  c = copy.copy(cfg)
  for k, v in kv.items():
    setattr(c, k, v)
  return c


def consecutive_seeds(seeds, num_games, refusal):
  """one seed per game as ints, consecutive (seed + i; ValueError(refusal) otherwise); None draws a base seed"""
  if seeds is None:
    base = int(np.random.randint(0, 2 ** 30))
    seeds = range(base, base + num_games)
  seeds = [int(s) for s in seeds]
  if len(seeds) != num_games or any(s != seeds[0] + i for i, s in enumerate(seeds)):
    raise ValueError(refusal)
  return seeds


def decode_history(g, r, i, searched, sides, predicted):
  """the keep_history logs of game i (Engine.eval_env_results, Match.results) as g's per-move lists.  Over its g.step
  actions history.actions / rewards / steps, and from the doubled `mover` log (+-1: who moved, +-2: and the rules ended the
  game there -- not the cut at max_steps) history.to_play / dones.  Over `searched`, the log indices of the searched moves,
  history.child_visits / root_values, pred_values and search_depths (sides: the Side that searched each); pred_rewards at
  the indices `predicted`."""
  n = g.step
  h = g.history = History()
  h.actions = [int(x) for x in r['actions'][i, :n]]
  h.rewards = [float(x) for x in r['rewards'][i, :n]]
  h.to_play = [int(np.sign(x)) for x in r['mover'][i, :n]]
  h.steps = list(range(n))
  h.dones = [abs(int(x)) == 2 for x in r['mover'][i, :n]]
  h.child_visits = [[float(x) for x in r['child_visits'][i, p]] for p in searched]
  h.root_values = [float(r['root_values'][i, p]) for p in searched]
  g.pred_values = [float(r['pred_values'][i, p]) for p in searched]
  g.pred_rewards = [float(r['pred_rewards'][i, p]) for p in predicted]
  g.search_depths = [side.depths(r['depths'][i, p]) for p, side in zip(searched, sides)]


def _pack_draws(draws, B, A, width, third, walk=True, noise=True):
  """the per-game draw dicts of play_games / play_match as the dense arrays Engine.eval_env_set_draws / Match.set_draws
  upload: walk [B][moves][width], noise [B][moves][A] and `third` ('opp' or 'opening') [B][n], each padded with zeros past a
  game's own draws; walk / noise: whether the side reads them"""
  out = {}
  if draws is None:
    return out
  if walk and any('walk' in d for d in draws):
    out['walk'] = np.zeros((B, max(1, max(len(d.get('walk', ())) for d in draws)), width), np.float64)
    for i, d in enumerate(draws):
      for m, w in enumerate(d.get('walk', ())):
        w = np.asarray(w, np.float64).reshape(-1)[:width]
        out['walk'][i, m, :len(w)] = w
  if noise and any('noise' in d for d in draws):
    out['noise'] = np.zeros((B, max(1, max(len(d.get('noise', ())) for d in draws)), A), np.float64)
    for i, d in enumerate(draws):
      for m, nz in enumerate(d.get('noise', ())):
        out['noise'][i, m] = np.asarray(nz, np.float64)
  if any(len(d.get(third, ())) for d in draws):
    out[third] = np.zeros((B, max(len(d.get(third, ())) for d in draws)), np.int32)
    for i, d in enumerate(draws):
      o = np.asarray(d.get(third, ()), np.int32).reshape(-1)
      out[third][i, :len(o)] = o
  return out


def get_label(state, detailed=False, path_idx=None):
  label_parts = ['net:{}'.format(state['training_step'])]
  if detailed:
    if path_idx is not None:
      label_parts.append('path:{}'.format(path_idx))
    label_parts += Side.of(state['config']).label_parts()
  return ', '.join(label_parts)


# what state_generator copies from the command line into every state's config as it stands
COPIED = ('render', 'save_mcts', 'save_mcts_after_step', 'save_gif_as', 'sleep', 'random_opp', 'human_opp', 'verbose', 'batch',
          'device_env', 'keep_history', 'opp_playouts', 'grade', 'grade_empties', 'grade_nodes', 'grade_table', 'grade_unroll')


def state_generator(args):
  """evaluate.py:406-439: one state per (checkpoint, temperature, simulations, only_prior, only_value, noise, mcts actions,
  true_model, gumbel), only_prior together with only_value excluded"""
  lists = (args.temperatures, args.num_simulations, args.only_prior, args.only_value, args.use_exploration_noise,
           args.apply_mcts_actions, getattr(args, 'true_model', [0]), getattr(args, 'gumbel', [0]))
  for path_idx, saves_dir in enumerate(args.saves_dir):
    for net in args.nets:
      meta_state = torch.load(saves_dir + net, map_location=torch.device('cpu'), weights_only=False)
      for temperature, num_simulations, only_prior, only_value, noise, apply_mcts_actions, true_model, gumbel in itertools.product(*lists):
        if only_prior and only_value:
          continue
        state = copy.deepcopy(meta_state)
        c = state['config']
        c.saves_dir = saves_dir
        if num_simulations is not None:
          c.num_simulations = num_simulations
        c.temperature, c.only_prior, c.only_value, c.use_exploration_noise = temperature, only_prior, only_value, noise
        c.apply_mcts_actions, c.true_model, c.gumbel = apply_mcts_actions, int(true_model), int(gumbel)
        c.gumbel_considered, c.gumbel_c_visit, c.gumbel_c_scale, c.gumbel_scale = gumbel_params(args)
        for name in COPIED:
          setattr(c, name, getattr(args, name))
        c.label = get_label(state, args.detailed_label, path_idx)
        c.use_gpu = True
        yield state


def run(evaluator, seed=None):
  """evaluate.py:441-452: one game with its own seed"""
  environment = get_environment(evaluator.config)
  return evaluator.play_game(environment, seed=seed)


def main(argv=None):
  args = get_evaluation_args(argv)
  if args.match:      # checkpoint against checkpoint (match.py); implies the device path
    from . import match
    return match.main(args)
  refuse(args)
  evaluators = [Evaluator(state) for state in state_generator(args)]
  print("\n\033[92mStarting a {} episode evaluation of {} configurations\033[0m...".format(args.num_games, len(evaluators)))
  seeds = list(range(args.seed, args.num_games + args.seed)) if args.seed is not None else None
  results = []
  for evaluator in evaluators:
    print("\n\033[92mEvaluating... - label: ({}) on {}\033[0m".format(evaluator.config.label, evaluator.device))
    evaluator.load_network()
    t0 = time.perf_counter()
    games = evaluator.play_games(args.num_games, seeds)
    wall = time.perf_counter() - t0
    s = evaluator.print_summary(games)
    s['label'] = evaluator.config.label
    s['num_games'] = len(games)
    side = Side.of(evaluator.config)
    s['true_model'], s['gumbel'] = int(side.true_model), int(bool(side.gumbel))
    if side.gumbel:
      s['gumbel_params'] = dict(side.gumbel)
    if args.device_env:
      print("Search below the root: {}\n".format('the true rules of the game (--true_model)' if side.true_model else 'the learned model'))
      print(side.search_line() + "\n")
    if evaluator.config.two_players and args.random_opp is not None:
      returns = np.array([game_return(g) for g in games])
      s['wins'], s['draws'], s['losses'] = int((returns > 0).sum()), int((returns == 0).sum()), int((returns < 0).sum())
      s['opp_playouts'] = int(args.opp_playouts)
      opponent = '{}-playout search'.format(args.opp_playouts) if args.opp_playouts else 'a random opponent'
      print("Against {} (the agent moves {}): wins {} draws {} losses {}\n".format(
          opponent, 'second' if args.random_opp == 1 else 'first', s['wins'], s['draws'], s['losses']))
    if evaluator.grade_report is not None:
      from . import solver
      s['grade'] = evaluator.grade_report
      print(solver.format_report(evaluator.grade_report, evaluator.config.label))
      if evaluator.grade_unroll_report is not None:
        s['grade'] = dict(evaluator.grade_report, unroll=evaluator.grade_unroll_report)
        print(solver.format_unroll(evaluator.grade_unroll_report, evaluator.config.label))
    s['games_per_s'] = len(games) / wall
    s['host_share'] = evaluator.host_seconds / wall
    results.append(s)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump({'num_games': args.num_games, 'seed': args.seed, 'configurations': results}, f, indent=1)
  return results


if __name__ == '__main__':
  main(sys.argv[1:])
