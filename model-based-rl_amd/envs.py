"""Environments that exist without gym.  TicTacToe follows the reference's custom environment
(custom_environments/tic_tac_toe.py:5-76: gym-0.x API, observation = turn * board, reward 1 for the
winning move, draw after nine moves).  CartPole is the classic-control task the reference reaches through gym.make
('CartPole-v1' / 'CartPole-v0'); gym is not installed, so the class below IS its definition and the device environment
(csrc/mz_games.h, mz_cartpole_step) follows it bit for bit.  Every other reference environment (Box2D, ALE) is
unavailable; its SHAPE is served by the on-device synthetic env (csrc/mz_selfplay.hip.h).  ConnectFour is not among the
reference's environments: the class below is its definition, a second two-player board game next to TicTacToe with the
same conventions, and the device environment (csrc/mz_games.h, mz_c4_step) follows it move for move."""
from types import SimpleNamespace

import numpy as np

from .config import CARTPOLE_TIME_LIMITS

_LINES = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 3, 6], [1, 4, 7], [2, 5, 8], [0, 4, 8], [2, 4, 6]])


class TicTacToe(object):

  def __init__(self):
    self.action_space = SimpleNamespace(n=9)
    self.observation_space = np.zeros(9, dtype=np.int32)
    self.reset()

  def seed(self, seed):
    return

  def reset(self):
    self.board = np.zeros(9, dtype=np.int32)
    self.turn = 1
    self._elapsed_steps = 0
    return self.board.copy()

  def legal_actions(self):
    return np.flatnonzero(self.board == 0)

  def step(self, action):
    self.board[action] = self.turn
    sums = self.board[_LINES].sum(axis=1)
    touched = (_LINES == action).any(axis=1)
    won = bool(np.any(np.abs(sums[touched]) == 3))
    done = won or self._elapsed_steps == 8
    result = None
    if won:
      result = 'player 1 wins' if self.turn == 1 else 'player 2 wins'
    elif done:
      result = 'draw'
    self._elapsed_steps += 1
    self.turn = -self.turn
    return self.turn * self.board.copy(), int(won), done, {'result': result}


class ConnectFour(object):
  """Connect Four on the standard board of 6 rows and 7 columns, with TicTacToe's conventions (gym-0.x API, observation =
  turn * board for the player about to move, reward 1 to the mover for the winning move).  board[7 * row + col], row 0 at
  the bottom: 0 empty, +1 / -1 the two players' stones.  An action is a column; the stone lands on its lowest empty cell."""
  ROWS, COLS = 6, 7
  _DIRECTIONS = ((1, 0), (0, 1), (1, 1), (1, -1))      # (d row, d col): vertical, horizontal, rising and falling diagonal

  def __init__(self):
    self.action_space = SimpleNamespace(n=7)
    self.observation_space = np.zeros(42, dtype=np.int32)
    self.reset()

  def seed(self, seed):
    return

  def reset(self):
    self.board = np.zeros(42, dtype=np.int32)
    self.turn = 1
    self._elapsed_steps = 0
    return self.board.copy()

  def set_position(self, board42, turn):
    """place a position (it need not be reachable): the step count is the number of stones"""
    self.board = np.array(board42, dtype=np.int32).reshape(42).copy()
    self.turn = int(turn)
    self._elapsed_steps = int(np.count_nonzero(self.board))

  def legal_actions(self):
    return np.flatnonzero(self.board[35:42] == 0)

  def _run(self, row, col, drow, dcol):
    """stones of the mover's colour next to (row, col) along (drow, dcol), not counting (row, col) itself"""
    n, r, c = 0, row + drow, col + dcol
    while 0 <= r < 6 and 0 <= c < 7 and self.board[7 * r + c] == self.turn:
      n, r, c = n + 1, r + drow, c + dcol
    return n

  def step(self, action):
    col = int(action)
    if not 0 <= col < 7 or self.board[35 + col] != 0:
      raise ValueError('column %d is full or does not exist' % col)
    row = int(np.flatnonzero(self.board[col::7] == 0)[0])
    self.board[7 * row + col] = self.turn
    won = any(self._run(row, col, dr, dc) + self._run(row, col, -dr, -dc) >= 3 for dr, dc in self._DIRECTIONS)
    done = won or not np.any(self.board == 0)
    result = None
    if won:
      result = 'player 1 wins' if self.turn == 1 else 'player 2 wins'
    elif done:
      result = 'draw'
    self._elapsed_steps += 1
    self.turn = -self.turn
    return self.turn * self.board.copy(), int(won), bool(done), {'result': result}


# sin / cos of the pole angle as fixed Taylor polynomials in z = theta * theta, Horner from the highest term down with plain
# float64 multiplies and adds: the device runs the very same IEEE operations (csrc/mz_games.h), where its libm and
# the host's differ in the last place -- and the pole, an unstable system, grows such a difference by ~e^0.09 per step.
# Within 1.2e-16 of math.sin / math.cos on [-0.8, 0.8]; the state is reset before |theta| passes 0.27.
_SIN_C = (1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0,
          -1.0 / 1307674368000.0)
_COS_C = (1.0, -1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0,
          -1.0 / 87178291200.0, 1.0 / 20922789888000.0)


def sin_p(t):
  t = float(t)
  z = t * t
  r = _SIN_C[7]
  for k in range(6, -1, -1):
    r = r * z + _SIN_C[k]
  return t * r


def cos_p(t):
  t = float(t)
  z = t * t
  r = _COS_C[8]
  for k in range(7, -1, -1):
    r = r * z + _COS_C[k]
  return r


class CartPole(object):
  """Cart and pole of Barto, Sutton & Anderson with gym's constants, Euler integration, reward 1 per step, termination
  at |x| > 2.4 or |theta| > 12 degrees, and gym's TimeLimit folded in (done at max_episode_steps; the reference does
  not tell truncation from termination, game.py:87-91).  gym-0.x API.  The state is four Python floats (float64)."""
  GRAVITY, MASS_CART, MASS_POLE, TOTAL_MASS = 9.8, 1.0, 0.1, 1.1
  LENGTH, POLEMASS_LENGTH, FORCE_MAG, TAU = 0.5, 0.05, 10.0, 0.02
  THETA_THRESHOLD = 12 * 2 * 3.141592653589793 / 360
  X_THRESHOLD = 2.4

  def __init__(self, max_episode_steps=500):
    self.action_space = SimpleNamespace(n=2)
    self.observation_space = np.zeros(4, dtype=np.float32)
    self.max_episode_steps = int(max_episode_steps)
    self.rng = np.random.RandomState()
    self.reset()

  def seed(self, seed):
    self.rng = np.random.RandomState(seed)

  def set_state(self, state4):
    self.state = tuple(float(v) for v in state4)

  def _obs(self):
    return np.array(self.state, dtype=np.float32)

  def reset(self):
    self.state = tuple(float(v) for v in self.rng.uniform(-0.05, 0.05, size=4))
    self._elapsed_steps = 0
    return self._obs()

  def legal_actions(self):
    return range(2)

  def step(self, action):
    x, x_dot, theta, theta_dot = self.state
    g, M, m_pole, l, pml, tau = self.GRAVITY, self.TOTAL_MASS, self.MASS_POLE, self.LENGTH, self.POLEMASS_LENGTH, self.TAU
    f = self.FORCE_MAG if int(action) == 1 else -self.FORCE_MAG
    c, s = cos_p(theta), sin_p(theta)
    temp = (f + pml * theta_dot * theta_dot * s) / M
    tha = (g * s - c * temp) / (l * (4.0 / 3.0 - m_pole * c * c / M))
    xa = temp - pml * tha * c / M
    x = x + tau * x_dot
    x_dot = x_dot + tau * xa
    theta = theta + tau * theta_dot
    theta_dot = theta_dot + tau * tha
    self.state = (x, x_dot, theta, theta_dot)
    th = self.THETA_THRESHOLD
    done = bool(x < -self.X_THRESHOLD or x > self.X_THRESHOLD or theta < -th or theta > th)
    self._elapsed_steps += 1
    if self._elapsed_steps >= self.max_episode_steps:
      done = True
    return self._obs(), 1.0, done, {}


# ---- the device games: the one table of them on the Python side (csrc/mz_games.h, mz_game_info, is the device's).
# --environment name -> (kind, obs_dim, actions, cells of the board or 0, two_players); every other table and list of
# games in the package is a view of this one.
DEVICE_GAMES = {
    'TicTacToe': (1, 9, 9, 9, True),
    'ConnectFour': (3, 42, 7, 42, True),
    'CartPole-v0': (2, 4, 2, 0, False),
    'CartPole-v1': (2, 4, 2, 0, False),
}
DEVICE_ENVS = tuple(DEVICE_GAMES)
KIND_OF_ENV = {name: g[0] for name, g in DEVICE_GAMES.items()}
# the two-player board games: what matches, the playout opponent, the solvers and the symmetry tables cover
BOARD_KINDS = {name: g[0] for name, g in DEVICE_GAMES.items() if g[3]}
BOARD_ENVS = tuple(BOARD_KINDS)
CELLS = {g[0]: g[3] for g in DEVICE_GAMES.values() if g[3]}
ACTIONS = {g[0]: g[2] for g in DEVICE_GAMES.values() if g[3]}
# the self-play loop's own spellings (Engine.selfplay_set_env); 0 is its synthetic environment
SELFPLAY_KINDS = dict({'synthetic': 0}, **{short: KIND_OF_ENV[name] for short, name in
                                           (('tictactoe', 'TicTacToe'), ('cartpole', 'CartPole-v1'), ('connect_four', 'ConnectFour'))})


def get_environment(config):
  if config.environment == 'TicTacToe':
    return TicTacToe()
  if config.environment == 'ConnectFour':
    return ConnectFour()
  if config.environment in CARTPOLE_TIME_LIMITS:
    return CartPole(CARTPOLE_TIME_LIMITS[config.environment])
  raise NotImplementedError('%s needs gym/ALE/Box2D, which are not installed; the GPU actor serves its shape with '
                            'the synthetic on-device environment' % config.environment)
