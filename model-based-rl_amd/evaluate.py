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

FCNetwork checkpoints on host environments (envs.get_environment) only; the interactive tools of the reference (rendering,
GIFs, plots, human play, MCTS PNG dumps) are refused.  One departure from the reference's output: its '[Game done]' line after
every game (evaluate.py:376-379) is printed only with --verbose -- thousands of games are played per configuration here, and
the summary block carries the same numbers."""
import copy
import json
import os
import sys
import time

import numpy as np
import torch

from .config import CARTPOLE_TIME_LIMITS, get_evaluation_args
from .engine import Engine, flatten_weights
from .envs import BOARD_ENVS, DEVICE_ENVS, get_environment
from .game import History

MAX_BATCH = 4096
MOVES_PER_SYNC = 8      # --device_env: whole moves enqueued per host synchronisation

REFUSED = (
    ('render', 'rendering is an interactive tool and is not part of this evaluator (no display on the GPU machines).'),
    ('save_gif_as', 'saving GIFs needs rendered frames, which this evaluator does not produce.'),
    ('save_mcts', 'MCTS PNG dumps (pydot) are an interactive tool and are not part of this evaluator.'),
    ('human_opp', 'human play is an interactive tool and is not part of this evaluator; use --random_opp.'),
    ('plot_summary', 'plots are an interactive tool and are not part of this evaluator; use --out for a JSON summary.'),
)


def refuse_unsupported(args_or_config):
  """one sentence per interactive flag the evaluator leaves out (NotImplementedError)"""
  for name, why in REFUSED:
    if getattr(args_or_config, name, None):
      raise NotImplementedError('--%s: %s' % (name, why))


def refuse_device_env(args_or_config):
  """one sentence per configuration --device_env leaves out (NotImplementedError); nothing to refuse without the flag"""
  c = args_or_config
  if not getattr(c, 'device_env', False):
    return
  env = getattr(c, 'environment', None)
  if env is not None and env not in DEVICE_ENVS:
    raise NotImplementedError('--device_env: %s has no device form; the device environments are %s.' % (env, ', '.join(DEVICE_ENVS)))
  if getattr(c, 'norm_obs', False):
    raise NotImplementedError('--device_env: --norm_obs is not applied by the device environments; use the host path.')
  m = getattr(c, 'apply_mcts_actions', 1)
  if env == 'ConnectFour' and any(int(x) != 1 for x in (m if isinstance(m, (list, tuple)) else [m])):
    raise NotImplementedError('--device_env: ConnectFour takes --apply_mcts_actions 1 only; below the root the walk offers full '
                              'columns, which the host class refuses and a device game cannot.')


PLAYOUT_ENVS = BOARD_ENVS


def refuse_opp_playouts(args_or_config, match=False):
  """one sentence per configuration --opp_playouts (the playout-search opponent of the device games) leaves out
  (NotImplementedError); nothing to refuse at 0"""
  c = args_or_config
  n = int(getattr(c, 'opp_playouts', 0) or 0)
  if n == 0:
    return
  if match:
    raise NotImplementedError('--opp_playouts: --match plays two networks against each other and seats no playout opponent.')
  if n < 64 or n > 65536 or n % 64:
    raise NotImplementedError('--opp_playouts: the budget is a multiple of 64 in 64 to 65536 playouts per move, got %d.' % n)
  if not getattr(c, 'device_env', False):
    raise NotImplementedError('--opp_playouts: the playout opponent is planned on the device and needs --device_env.')
  if getattr(c, 'random_opp', None) is None:
    raise NotImplementedError('--opp_playouts: --random_opp names the seat the playout opponent takes and is missing.')
  env = getattr(c, 'environment', None)
  if env is not None and env not in PLAYOUT_ENVS:
    raise NotImplementedError('--opp_playouts: %s has no playout opponent; it plays %s.' % (env, ' and '.join(PLAYOUT_ENVS)))
  m = getattr(c, 'apply_mcts_actions', 1)
  if any(int(x) != 1 for x in (m if isinstance(m, (list, tuple)) else [m])):
    raise NotImplementedError('--opp_playouts: the playout opponent answers every move and takes --apply_mcts_actions 1 only.')


GRADE_ENVS = BOARD_ENVS


def refuse_grade(args_or_config, match=False):
  """one sentence per configuration --grade (moves graded against the exact solver, solver.py) leaves out
  (NotImplementedError, starting '--grade: '); nothing to refuse without the flag, but --grade_table, which only chooses
  the grading's search (a sentence starting '--grade_table: ')"""
  c = args_or_config
  if not getattr(c, 'grade', False):
    if getattr(c, 'grade_table', False):
      raise NotImplementedError('--grade_table: it chooses the search that --grade solves with and grades nothing without --grade.')
    return
  if match:
    raise NotImplementedError('--grade: the games of --match are not graded; grade each network with evaluate --device_env --grade.')
  if not getattr(c, 'device_env', False):
    raise NotImplementedError('--grade: the graded games are the device environments\' and need --device_env.')
  env = getattr(c, 'environment', None)
  if env is not None and env not in GRADE_ENVS:
    raise NotImplementedError('--grade: %s has no exact solver; it solves %s.' % (env, ' and '.join(GRADE_ENVS)))
  m = getattr(c, 'apply_mcts_actions', 1)
  if any(int(x) != 1 for x in (m if isinstance(m, (list, tuple)) else [m])):
    raise NotImplementedError('--grade: a graded decision is one searched move and takes --apply_mcts_actions 1 only.')


def refuse_grade_unroll(args_or_config):
  """one sentence per configuration --grade_unroll K (the model by unroll depth, solver.grade_unroll) leaves out
  (NotImplementedError, starting '--grade_unroll: '); nothing to refuse without the flag.  What --grade refuses stays
  refused by --grade's own sentence (refuse_grade runs first).  --no_support checkpoints are served: the unroll goes through
  mz_initial_inference and mz_recurrent_inference, which read the heads' single outputs."""
  c = args_or_config
  K = getattr(c, 'grade_unroll', None)
  if K is None or K is False:
    return
  if not getattr(c, 'grade', False):
    raise NotImplementedError('--grade_unroll: it unrolls the model along the games --grade keeps and does nothing without --grade.')
  if int(K) < 1 or int(K) > Engine.UNROLL_MAX_K:
    raise NotImplementedError('--grade_unroll: the depth is 1 to %d dynamics steps, got %d.' % (Engine.UNROLL_MAX_K, int(K)))


TRUE_MODEL_ENVS = BOARD_ENVS


def refuse_true_model(args_or_config, match=False):
  """one sentence per configuration --true_model (the search on the true rules of the device games, Engine.tm_search) leaves
  out (NotImplementedError, starting '--true_model: '); nothing to refuse while every value is 0.  The lists of the command
  line are read per side with --match (one value: both sides) and as alternatives without it."""
  c = args_or_config
  alls = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]
  tm = [int(x or 0) for x in alls(getattr(c, 'true_model', 0))]
  if not any(tm):
    return
  if any(x not in (0, 1) for x in tm):
    raise NotImplementedError('--true_model: the values are 0 (the learned model) and 1 (the true rules), got %r.' % (tm,))
  if not match and not getattr(c, 'device_env', False):
    raise NotImplementedError('--true_model: the true-rules search reads the device games\' positions and needs --device_env (or --match).')
  env = getattr(c, 'environment', None)
  if env is not None and env not in TRUE_MODEL_ENVS:
    raise NotImplementedError('--true_model: %s has no true-rules search; it searches %s.' % (env, ' and '.join(TRUE_MODEL_ENVS)))
  if any(int(x) != 1 for x in alls(getattr(c, 'apply_mcts_actions', 1))):
    raise NotImplementedError('--true_model: a move of the true-rules search applies one action and takes --apply_mcts_actions 1 only.')
  prior, value = [int(x or 0) for x in alls(getattr(c, 'only_prior', 0))], [int(x or 0) for x in alls(getattr(c, 'only_value', 0))]
  pick = lambda v, k: v[k if len(v) == 2 else 0]
  sides = range(2) if match else [0]
  if any(pick(tm, k) and ((pick(prior, k) or pick(value, k)) if match else (any(prior) or any(value))) for k in sides):
    raise NotImplementedError('--true_model: --only_prior / --only_value run no search; a side takes one of them or the true-rules search.')
  if getattr(c, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise NotImplementedError('--true_model: the architecture %s has no engine path; FCNetwork checkpoints only.' % c.architecture)


GUMBEL_DEFAULTS = dict(gumbel_considered=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0, gumbel_scale=0.0)


def gumbel_params(args_or_config):
  """(max_considered, c_visit, c_scale, gumbel_scale) of a command line or a config, the defaults where it has none"""
  g = lambda k: getattr(args_or_config, k, None)
  return tuple(type(v)(v if g(k) is None else g(k)) for k, v in GUMBEL_DEFAULTS.items())


def refuse_gumbel(args_or_config, match=False):
  """one sentence per configuration --gumbel (the Gumbel MuZero search, Engine.gz_search) leaves out (NotImplementedError,
  starting '--gumbel: '); nothing to refuse while every value is 0.  The lists of the command line are read per side with
  --match (one value: both sides) and as alternatives without it."""
  c = args_or_config
  alls = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]
  gz = [int(x or 0) for x in alls(getattr(c, 'gumbel', 0))]
  if not any(gz):
    return
  if any(x not in (0, 1) for x in gz):
    raise NotImplementedError('--gumbel: the values are 0 (PUCT) and 1 (the Gumbel search), got %r.' % (gz,))
  if not match and not getattr(c, 'device_env', False):
    raise NotImplementedError('--gumbel: the Gumbel search is served by the device games\' move loop and needs --device_env (or --match).')
  if any(int(x) != 1 for x in alls(getattr(c, 'apply_mcts_actions', 1))):
    raise NotImplementedError('--gumbel: a move of the Gumbel search applies one action and takes --apply_mcts_actions 1 only.')
  pick = lambda v, k: v[k if len(v) == 2 else 0]
  on_side = lambda v: any(pick(gz, k) and pick(v, k) for k in range(2)) if match else any(v)
  if on_side([int(x or 0) for x in alls(getattr(c, 'use_exploration_noise', 0))]):
    raise NotImplementedError('--gumbel: the Gumbel draw replaces the exploration noise at the root; a side takes --use_exploration_noise or the Gumbel search (--gumbel_scale is its stochastic setting).')
  temps = getattr(c, 'temperatures', None)
  temps = [float(x or 0) for x in alls(getattr(c, 'temperature', 0) if temps is None else temps)]
  if on_side([t != 0 for t in temps]):
    raise NotImplementedError('--gumbel: the move is chosen by the rule of the search, not sampled from the visits; a side takes temperature 0 (--gumbel_scale is the stochastic setting).')
  prior, value = [int(x or 0) for x in alls(getattr(c, 'only_prior', 0))], [int(x or 0) for x in alls(getattr(c, 'only_value', 0))]
  if on_side(prior) or on_side(value):
    raise NotImplementedError('--gumbel: --only_prior / --only_value run no search; a side takes one of them or the Gumbel search.')
  if on_side([int(x or 0) for x in alls(getattr(c, 'true_model', 0))]):
    raise NotImplementedError('--gumbel: an engine searches the true rules or with the Gumbel search; a side takes --true_model or --gumbel.')
  if getattr(c, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise NotImplementedError('--gumbel: the architecture %s has no engine path; FCNetwork checkpoints only.' % c.architecture)
  m, cv, cs, sc = gumbel_params(c)
  if m < 2:
    raise NotImplementedError('--gumbel: --gumbel_considered must be at least 2, got %d.' % m)
  if not cv >= 0:
    raise NotImplementedError('--gumbel: --gumbel_c_visit must not be negative, got %g.' % cv)
  if not cs > 0:
    raise NotImplementedError('--gumbel: --gumbel_c_scale must be positive, got %g.' % cs)
  if not sc >= 0:
    raise NotImplementedError('--gumbel: --gumbel_scale must not be negative, got %g.' % sc)


def gumbel_line(config):
  """the printed line that names a configuration's search"""
  if not getattr(config, 'gumbel', 0):
    return 'Search: PUCT'
  return 'Search: Gumbel, m = %d, c_visit = %g, c_scale = %g, gumbel_scale = %g' % gumbel_params(config)


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
    refuse_unsupported(self.config)
    refuse_device_env(self.config)
    refuse_opp_playouts(_with(self.config, device_env=True))      # (play_games(device_env=True) may still name the device path)
    refuse_grade(_with(self.config, device_env=True))
    refuse_grade_unroll(self.config)
    refuse_true_model(_with(self.config, device_env=True))
    refuse_gumbel(_with(self.config, device_env=True))
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
    true_model = bool(true_model or getattr(self.config, 'true_model', 0))
    refuse_true_model(_with(self.config, device_env=device_env, true_model=int(true_model)))
    gumbel = gumbel or bool(getattr(self.config, 'gumbel', 0))
    if gumbel:
      m, cv, cs, sc = gumbel_params(self.config)
      given = gumbel if isinstance(gumbel, dict) else {}
      gumbel = dict(dict(max_considered=m, c_visit=cv, c_scale=cs, gumbel_scale=sc), **given)
      refuse_gumbel(_with(self.config, device_env=device_env, gumbel=1, true_model=int(true_model), gumbel_considered=gumbel['max_considered'],
                          gumbel_c_visit=gumbel['c_visit'], gumbel_c_scale=gumbel['c_scale'], gumbel_scale=gumbel['gumbel_scale']))
    grade = bool(getattr(self.config, 'grade', False))
    keep_history = bool(keep_history or grade or getattr(self.config, 'keep_history', False))
    refuse_opp_playouts(_with(self.config, device_env=device_env))
    refuse_grade(_with(self.config, device_env=device_env))
    refuse_grade_unroll(self.config)
    assert self.weights is not None, '.load_network() needs to be called before playing.'
    if device_env and environments is not None:
      raise ValueError('play_games: a device-environment run builds no host environment')
    if start_states is not None and not device_env:
      raise ValueError('play_games: start_states are the device path\'s; give the host path environments that hold them')
    if seeds is None:
      base = int(np.random.randint(0, 2 ** 30))
      seeds = list(range(base, base + num_games))
    seeds = [int(s) for s in seeds]
    if len(seeds) != num_games or any(s != seeds[0] + i for i, s in enumerate(seeds)):
      raise ValueError('play_games takes consecutive seeds, one per game (evaluate.py:476-479)')
    games = []
    for lo in range(0, num_games, self.batch):
      hi = min(num_games, lo + self.batch)
      if device_env:
        games += self._play_batch_device(seeds[lo:hi], None if draws is None else draws[lo:hi],
                                         None if start_states is None else start_states[lo:hi], keep_history, true_model, gumbel)
        continue
      envs = environments[lo:hi] if environments is not None else [get_environment(self.config) for _ in range(lo, hi)]
      games += self._play_batch(envs, seeds[lo:hi], None if draws is None else draws[lo:hi])
    if grade:
      self.grade_report = self.grade(games)
      if getattr(self.config, 'grade_unroll', None):
        self.grade_unroll_report = self.grade_unroll(games)
    return games

  def grade(self, games):
    """--grade: the keep_history games graded against the exact solver (solver.grade_games) -- the network's moves where
    --random_opp seats an opponent, both sides' otherwise; TicTacToe every position, ConnectFour those with at most
    config.grade_empties empty cells"""
    from . import solver
    cfg = self.config
    t0 = time.perf_counter()
    opp = getattr(cfg, 'random_opp', None)
    eng = Engine.from_config(cfg, min(len(games), self.batch), device=self.device, seed=0)
    try:
      report = solver.grade_games(games, cfg.environment, eng,
                                  max_empties=None if cfg.environment == 'TicTacToe' else int(getattr(cfg, 'grade_empties', solver.DEFAULT_EMPTIES)),
                                  graded_seat=None if opp is None else -int(opp),
                                  max_nodes=int(getattr(cfg, 'grade_nodes', solver.DEFAULT_NODES)),
                                  table=bool(getattr(cfg, 'grade_table', False)))
    finally:
      eng.close()
    report['seconds'] = time.perf_counter() - t0
    return report

  def grade_unroll(self, games):
    """--grade_unroll K: the model unrolled K steps along the moves of the same keep_history games, against the real
    positions and the exact solver (solver.grade_unroll), in --grade's scope: the positions where the network is to move
    where --random_opp seats an opponent, both seats' otherwise; truth for TicTacToe everywhere, for ConnectFour at
    positions with at most config.grade_empties empty cells"""
    from . import solver
    cfg = self.config
    t0 = time.perf_counter()
    opp = getattr(cfg, 'random_opp', None)
    eng = Engine.from_config(cfg, min(len(games), self.batch), device=self.device, seed=0)
    try:
      eng.set_weights(self.weights)
      report = solver.grade_unroll(games, cfg.environment, eng, int(cfg.grade_unroll),
                                   max_empties=None if cfg.environment == 'TicTacToe' else int(getattr(cfg, 'grade_empties', solver.DEFAULT_EMPTIES)),
                                   graded_seat=None if opp is None else -int(opp),
                                   max_nodes=int(getattr(cfg, 'grade_nodes', solver.DEFAULT_NODES)),
                                   table=bool(getattr(cfg, 'grade_table', False)))
    finally:
      eng.close()
    report['seconds'] = time.perf_counter() - t0
    return report

  def _play_batch_device(self, seeds, draws, start_states, keep_history, true_model=False, gumbel=None):
    """_play_batch with the games on the device environments: whole moves are enqueued MOVES_PER_SYNC at a time
    (Engine.eval_env_moves: observe, initial inference, root, search + walk or lookahead, finalize, apply), and the host
    only reads the number of games still live after each chunk.  true_model: the engine searches the games' real positions
    (Engine.set_true_model); gumbel: Engine.set_gumbel's arguments, the engine searches with the Gumbel search; everything
    around the search is the same."""
    cfg = self.config
    refuse_device_env(_with(cfg, device_env=True))
    refuse_opp_playouts(_with(cfg, device_env=True))
    opp_playouts = int(getattr(cfg, 'opp_playouts', 0) or 0)
    B, A = len(seeds), int(cfg.action_space)
    only_prior, only_value = bool(getattr(cfg, 'only_prior', 0)), bool(getattr(cfg, 'only_value', 0))
    mode = 1 if only_prior else 2 if only_value else 0
    noise_on = bool(getattr(cfg, 'use_exploration_noise', 0))
    two = bool(cfg.two_players)
    M = int(getattr(cfg, 'apply_mcts_actions', 1))
    if M <= 0:
      M = int(cfg.num_simulations) + 1
    T = float(getattr(cfg, 'temperature', 0) or 0)
    t_batch = time.perf_counter()
    # the device RNG's key: (engine seed 0, env id = the game's seed, move, step)
    eng = Engine.from_config(cfg, B, device=self.device, seed=0, env_id_offset=seeds[0])
    eng.set_weights(self.weights)
    if true_model:
      eng.set_true_model(cfg.environment)
    if gumbel:
      eng.set_gumbel(True, **gumbel)
    eng.eval_env_reset(cfg.environment, int(cfg.max_steps), CARTPOLE_TIME_LIMITS.get(cfg.environment, 0),
                       getattr(cfg, 'random_opp', None) if two else None, keep_history)
    if opp_playouts:
      eng.eval_env_set_opponent(opp_playouts)
    if draws is not None or start_states is not None:
      eng.eval_env_set_draws(**_pack_draws(draws, B, A, M, mode, noise_on, start_states))
    live, moves, t_dev = B, 0, 0.0
    while live > 0 and moves < eng.eval_log_cap:      # (every move applies at least one action: at most cap moves)
      n = min(MOVES_PER_SYNC, eng.eval_log_cap - moves)
      t0 = time.perf_counter()
      live = eng.eval_env_moves(n, mode, M, T, noise_on)
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
        n, k = g.step, int(r['n_moves'][i])
        h = g.history = History()
        h.actions = [int(x) for x in r['actions'][i, :n]]
        h.rewards = [float(x) for x in r['rewards'][i, :n]]
        h.to_play = [int(np.sign(x)) for x in r['mover'][i, :n]]
        h.steps = list(range(n))
        h.dones = [abs(int(x)) == 2 for x in r['mover'][i, :n]]      # (env.step's done: not the cut at max_steps)
        h.child_visits = [[float(x) for x in row] for row in r['child_visits'][i, :k]]
        h.root_values = [float(x) for x in r['root_values'][i, :k]]
        g.pred_values = [float(x) for x in r['pred_values'][i, :k]]
        g.pred_rewards = [float(x) for x in r['pred_rewards'][i, :n]]
        g.n_actions = [int(x) for x in r['n_actions'][i, :k]]
        g.search_depths = [[0] if only_prior else [1] if only_value else [int(x) for x in row] for row in r['depths'][i, :k]]
      if getattr(cfg, 'verbose', False):
        msg = "\033[92m[Game done]\033[0m --> "
        msg += "length: {:.1f}, return: {:.1f}, pred return: {:.1f}, pred value: {:.1f}, mcts value: {:.1f}"
        print(msg.format(g.step, g.ret, g.pred_return, g.pred_value, g.mcts_value))
      games.append(g)
    self.device_seconds += t_dev
    self.host_seconds += time.perf_counter() - t_batch - t_dev
    return games

  def _play_batch(self, envs, seeds, draws):
    cfg = self.config
    B, A = len(envs), int(cfg.action_space)
    O = int(np.prod(cfg.obs_space))
    only_prior, only_value = bool(getattr(cfg, 'only_prior', 0)), bool(getattr(cfg, 'only_value', 0))
    noise_on = bool(getattr(cfg, 'use_exploration_noise', 0))
    two = bool(cfg.two_players)
    random_opp = getattr(cfg, 'random_opp', None)
    M = int(getattr(cfg, 'apply_mcts_actions', 1))
    if M <= 0:        # (the reference's loop then runs until an unexpanded node: at most num_simulations + 1 actions)
      M = int(cfg.num_simulations) + 1
    T = float(getattr(cfg, 'temperature', 0) or 0)
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


def _pack_draws(draws, B, A, M, mode, noise_on, start_states):
  """the per-game draw dicts of play_games as the dense arrays Engine.eval_env_set_draws uploads: walk [B][moves][M], noise
  [B][moves][A], opp [B][n], each padded with zeros past a game's own draws"""
  out = dict(start_states=None if start_states is None else np.ascontiguousarray(start_states, np.float64).reshape(B, 4))
  if draws is None:
    return out
  if mode == 0 and any('walk' in d for d in draws):
    mv = max(1, max(len(d['walk']) for d in draws))
    walk = np.zeros((B, mv, M), np.float64)
    for i, d in enumerate(draws):
      for m, w in enumerate(d['walk']):
        w = np.asarray(w, np.float64).reshape(-1)[:M]
        walk[i, m, :len(w)] = w
    out['walk'] = walk
  if noise_on and any('noise' in d for d in draws):
    mv = max(1, max(len(d['noise']) for d in draws))
    noise = np.zeros((B, mv, A), np.float64)
    for i, d in enumerate(draws):
      for m, nz in enumerate(d['noise']):
        noise[i, m] = np.asarray(nz, np.float64)
    out['noise'] = noise
  if any(len(d.get('opp', ())) for d in draws):
    n = max(len(d.get('opp', ())) for d in draws)
    opp = np.zeros((B, n), np.int32)
    for i, d in enumerate(draws):
      o = np.asarray(d.get('opp', ()), np.int32).reshape(-1)
      opp[i, :len(o)] = o
    out['opp'] = opp
  return out


def get_label(state, detailed=False, path_idx=None):
  label_parts = ['net:{}'.format(state['training_step'])]
  if detailed:
    if path_idx is not None:
      label_parts.append('path:{}'.format(path_idx))
    if state['config'].only_value:
      label_parts.append('only value')
    elif state['config'].only_prior:
      label_parts.append('only prior')
    else:
      label_parts.append('sims:{}'.format(state['config'].num_simulations))
      if state['config'].apply_mcts_actions > 1:
        label_parts.append('mcts-actions:{}'.format(state['config'].apply_mcts_actions))
      if state['config'].temperature:
        label_parts.append('temp:{}'.format(state['config'].temperature))
      if state['config'].use_exploration_noise:
        label_parts.append('with noise')
      if getattr(state['config'], 'true_model', 0):
        label_parts.append('true rules')
      if getattr(state['config'], 'gumbel', 0):
        label_parts.append('gumbel')
  return ', '.join(label_parts)


def state_generator(args):
  """evaluate.py:406-439: one state per (checkpoint, temperature, simulations, only_prior, only_value, noise, mcts actions),
  only_prior together with only_value excluded"""
  for path_idx, saves_dir in enumerate(args.saves_dir):
    for net in args.nets:
      meta_state = torch.load(saves_dir + net, map_location=torch.device('cpu'), weights_only=False)
      for temperature in args.temperatures:
        for num_simulations in args.num_simulations:
          for only_prior in args.only_prior:
            for only_value in args.only_value:
              for use_exploration_noise in args.use_exploration_noise:
                for apply_mcts_actions, true_model, gumbel in ((m, t, g) for m in args.apply_mcts_actions for t in getattr(args, 'true_model', [0])
                                                               for g in getattr(args, 'gumbel', [0])):
                  if not (only_prior and only_value):
                    state = copy.deepcopy(meta_state)
                    c = state['config']
                    c.saves_dir = saves_dir
                    if num_simulations is not None:
                      c.num_simulations = num_simulations
                    c.temperature = temperature
                    c.only_value = only_value
                    c.only_prior = only_prior
                    c.use_exploration_noise = use_exploration_noise
                    c.apply_mcts_actions = apply_mcts_actions
                    c.true_model = int(true_model)
                    c.gumbel = int(gumbel)
                    c.gumbel_considered, c.gumbel_c_visit, c.gumbel_c_scale, c.gumbel_scale = gumbel_params(args)
                    c.render = args.render
                    c.save_mcts = args.save_mcts
                    c.save_mcts_after_step = args.save_mcts_after_step
                    c.save_gif_as = args.save_gif_as
                    c.sleep = args.sleep
                    c.random_opp = args.random_opp
                    c.human_opp = args.human_opp
                    c.label = get_label(state, args.detailed_label, path_idx)
                    c.use_gpu = True
                    c.verbose = args.verbose
                    c.batch = args.batch
                    c.device_env = args.device_env
                    c.keep_history = args.keep_history
                    c.opp_playouts = args.opp_playouts
                    c.grade, c.grade_empties, c.grade_nodes = args.grade, args.grade_empties, args.grade_nodes
                    c.grade_table = args.grade_table
                    c.grade_unroll = args.grade_unroll
                    yield state


def run(evaluator, seed=None):
  """evaluate.py:441-452: one game with its own seed"""
  environment = get_environment(evaluator.config)
  return evaluator.play_game(environment, seed=seed)


def main(argv=None):
  args = get_evaluation_args(argv)
  refuse_opp_playouts(args, match=args.match)
  refuse_grade(args, match=args.match)
  refuse_grade_unroll(args)
  refuse_true_model(args, match=args.match)
  refuse_gumbel(args, match=args.match)
  if args.match:      # checkpoint against checkpoint (match.py); implies the device path
    from . import match
    return match.main(args)
  refuse_unsupported(args)
  refuse_device_env(args)
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
    s['true_model'] = int(getattr(evaluator.config, 'true_model', 0))
    if args.device_env:
      print("Search below the root: {}\n".format('the true rules of the game (--true_model)' if s['true_model'] else 'the learned model'))
    s['gumbel'] = int(getattr(evaluator.config, 'gumbel', 0))
    if s['gumbel']:
      s['gumbel_params'] = dict(zip(('max_considered', 'c_visit', 'c_scale', 'gumbel_scale'), gumbel_params(evaluator.config)))
    if args.device_env:
      print(gumbel_line(evaluator.config) + "\n")
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
