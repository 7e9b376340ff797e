"""Board-symmetry augmentation of training batches (--symmetry; DESIGN s7e): the numpy restatement of csrc/mz_symmetry.hip.h.

A TicTacToe position has 8 equivalent images (four quarter turns, each with or without a mirror), a Connect Four position 2
(itself and its left-right mirror); the image of a game is a legal game with the same rewards and values.  With --symmetry
every sample of a training batch is replaced by the image under an element drawn per (seed, update, sample): the observation's
cells, the K unrolled actions and the K + 1 policy targets move together.  The native learner step does it on the device
(mz_fcl_set_symmetry, one launch ahead of the step); the graphed-PyTorch and eager steps apply `apply_batch` below to the host
batch before upload, with the same seed and update number -- all three train on the same images, bit for bit (a permutation has
no rounding).

Kinds are mz_game_kind's: 1 TicTacToe (cell 3 * row + col, action = cell; g = 4 f + q: q quarter turns (r, c) -> (c, 2 - r),
then, if f, (r, c) -> (r, 2 - c)), 3 Connect Four (cell 7 * row + col, action = column; g = 1: col -> 6 - col)."""
import numpy as np

from .envs import ACTIONS, BOARD_KINDS as KIND_OF_ENV, CELLS

TICTACTOE, CONNECT_FOUR = KIND_OF_ENV['TicTacToe'], KIND_OF_ENV['ConnectFour']
RNG_SYM = 10      # MZ_RNG_SYM (csrc/mz_rng.h)
ELEMENTS = {TICTACTOE: 8, CONNECT_FOUR: 2}


def _ttt_cell(g, cell):
  r, c = divmod(cell, 3)
  for _ in range(g & 3):
    r, c = c, 2 - r
  if g >> 2:
    c = 2 - c
  return 3 * r + c


def cell_perm(kind):
  """p[g][c] = p_g(c): where cell c of the position lies in its image"""
  if kind == TICTACTOE:
    return np.array([[_ttt_cell(g, c) for c in range(9)] for g in range(8)], np.int64)
  return np.array([[7 * (c // 7) + (6 - c % 7 if g else c % 7) for c in range(42)] for g in range(2)], np.int64)


def action_perm(kind):
  """a[g][x] = a_g(x): the action of the image that does what action x does in the position"""
  if kind == TICTACTOE:
    return cell_perm(kind)
  return np.array([[6 - x if g else x for x in range(7)] for g in range(2)], np.int64)


def philox_x(seed, c0, c1, c2, c3):
  """word x of Philox4x32-10 (mz_philox, csrc/mz_rng.h) for arrays of counters"""
  seed = int(seed) & 0xFFFFFFFFFFFFFFFF
  M = np.uint64(0xFFFFFFFF)
  c0, c1, c2, c3 = [np.broadcast_to(np.asarray(c, np.uint64) & M, np.broadcast(c0, c1, c2, c3).shape).copy() for c in (c0, c1, c2, c3)]
  k0, k1 = seed & 0xFFFFFFFF, seed >> 32
  for _ in range(10):
    p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M
    k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
  return c0


def draw(kind, seed, update, batch):
  """the element of every sample of update `update`: philox(seed, update, b, 0, MZ_RNG_SYM << 24).x & (n - 1)"""
  x = philox_x(seed, int(update) & 0xFFFFFFFF, np.arange(batch), 0, RNG_SYM << 24)
  return (x & np.uint64(ELEMENTS[kind] - 1)).astype(np.int32)


def apply_batch(host, kind, seed, update):
  """-> (the host batch with obs / act / t_pol replaced by transformed copies, the elements [batch] int32).  `host` is the dict
  of arrays the learner's step consumes (obs [bs][cells], act [bs][K], t_pol [bs][K + 1][A], ...); it is not written."""
  obs, act, pol = host['obs'], host['act'], host['t_pol']
  bs = obs.shape[0]
  O, A = CELLS[kind], ACTIONS[kind]
  assert obs.shape == (bs, O) and act.ndim == 2 and pol.shape == (bs, act.shape[1] + 1, A), (obs.shape, act.shape, pol.shape)
  g = draw(kind, seed, update, bs)
  p, a = cell_perm(kind)[g], action_perm(kind)[g]      # [bs][O], [bs][A]
  rows = np.arange(bs)[:, None]
  obs2 = np.empty_like(obs)
  obs2[rows, p] = obs                                   # obs'[p_g(c)] = obs[c]
  inside = (act >= 0) & (act < A)                       # (a value that is no action of the game stays what it is)
  act2 = np.where(inside, a[rows, np.clip(act, 0, A - 1)], act).astype(act.dtype)
  pol2 = np.empty_like(pol)
  pol2[rows[:, :, None], np.arange(pol.shape[1])[None, :, None], a[:, None, :]] = pol      # pol'[k][a_g(x)] = pol[k][x]
  return dict(host, obs=obs2, act=np.ascontiguousarray(act2), t_pol=pol2), g


def kind_of(config):
  """the mz_game_kind of the configuration's environment for the symmetry tables, 0 where it has none"""
  return KIND_OF_ENV.get(getattr(config, 'environment', None), 0)


def seed_of(config):
  """the draw's seed: the run's seed, 0 without one"""
  seed = getattr(config, 'seed', None)
  return (int(seed) if seed is not None else 0) & 0xFFFFFFFFFFFFFFFF


def refuse_symmetry(config):
  """--symmetry on a configuration it does not cover: one NotImplementedError sentence, before any device is touched"""
  if not getattr(config, 'symmetry', False):
    return
  env = getattr(config, 'environment', None)
  kind = kind_of(config)
  if not kind:
    raise NotImplementedError('--symmetry: the symmetry tables exist for TicTacToe and ConnectFour, not for %s.' % env)
  if getattr(config, 'norm_obs', False):
    raise NotImplementedError('--symmetry: --norm_obs scales every cell by its own range, which the images of a position do not share.')
  if getattr(config, 'obs_u8', False):
    raise NotImplementedError('--symmetry: byte observations are not covered, the cells of %s are float32.' % env)
  obs_space = tuple(getattr(config, 'obs_space', (CELLS[kind],)))
  arch = getattr(config, 'architecture', 'FCNetwork')
  if arch != 'FCNetwork':
    raise NotImplementedError('--symmetry: --architecture %s takes image observations, the tables permute the flat board of the FCNetwork.' % arch)
  if len(obs_space) != 1:
    raise NotImplementedError('--symmetry: observations of shape %s are not covered, only the flat boards of the FCNetwork (2-D batches).' % (obs_space,))
  stack = int(getattr(config, 'stack_obs', 1) or 1)
  if stack > 1:
    raise NotImplementedError('--symmetry: --stack_obs %d is not covered, the tables permute the %d cells of one %s board.' % (stack, CELLS[kind], env))
  if int(obs_space[0]) != CELLS[kind]:
    raise NotImplementedError('--symmetry: observations of %d values are not covered, the tables permute the %d cells of one %s board.'
                              % (int(obs_space[0]), CELLS[kind], env))
