"""envs.ConnectFour, the definition the device environment follows (mz_selfplay_set_env kind 3): 2,000 random games against
an independent checker that scans all 69 four-cell windows of the whole board after every move, six placed positions with
one legal column each (tests/c4_positions.py), and the configuration."""
import numpy as np
import pytest

from tests.c4_positions import POSITIONS, WINS, lines_of

GAMES, SEED = 2000, 4


def test_random_games_against_a_window_scan():
  from model_based_rl_amd.envs import ConnectFour
  rng = np.random.RandomState(SEED)
  env = ConnectFour()
  assert env.action_space.n == 7 and env.observation_space.shape == (42,)
  env.seed(123)      # a no-op
  directions, full_columns, results = set(), 0, {'player 1 wins': 0, 'player 2 wins': 0, 'draw': 0}
  for g in range(GAMES):
    obs = env.reset()
    assert obs.shape == (42,) and not obs.any() and env.turn == 1 and env._elapsed_steps == 0
    grid = np.zeros((6, 7), np.int64)      # the checker's own board, [row][col], row 0 at the bottom
    mover, moves = 1, 0
    while True:
      heights = (grid != 0).sum(0)
      legal = [c for c in range(7) if heights[c] < 6]
      assert list(env.legal_actions()) == legal and env.turn == mover and env._elapsed_steps == moves
      assert np.array_equal(env.board, grid.reshape(42)) and env.board.dtype == np.int32
      full = [c for c in range(7) if heights[c] == 6]
      if full:
        full_columns += 1
        before = env.board.copy()
        with pytest.raises(ValueError):
          env.step(full[0])
        assert np.array_equal(env.board, before) and env.turn == mover and env._elapsed_steps == moves
      col = int(legal[rng.randint(len(legal))])
      grid[heights[col], col] = mover      # the landing cell: the lowest empty one
      obs, reward, done, info = env.step(col)
      moves += 1
      made = lines_of(grid.reshape(42), mover)
      assert not lines_of(grid.reshape(42), -mover)
      won = bool(made)
      directions.update(made)
      assert np.array_equal(env.board, grid.reshape(42)), (g, moves, 'landing cell')
      assert reward == int(won) and isinstance(reward, int) and done == (won or moves == 42) and isinstance(done, bool)
      assert np.array_equal(obs, -mover * grid.reshape(42))      # the observation of the player about to move
      want = ('player 1 wins' if mover == 1 else 'player 2 wins') if won else ('draw' if done else None)
      assert info == {'result': want}
      assert env.turn == -mover and env._elapsed_steps == moves
      mover = -mover
      if done:
        results[want] += 1
        break
  print('results', results, 'positions with a full column', full_columns, 'directions', sorted(directions))
  # conditions on the inputs: every direction of a line occurs, and full columns occur
  assert directions == set(WINS) and full_columns >= 1 and all(v >= 1 for v in results.values())


@pytest.mark.parametrize('kind,turn,col,board', POSITIONS, ids=[p[0] for p in POSITIONS])
def test_placed_positions(kind, turn, col, board):
  from model_based_rl_amd.envs import ConnectFour
  assert not lines_of(board, 1) and not lines_of(board, -1)      # no line before the move
  env = ConnectFour()
  env.set_position(board, turn)
  stones = int(np.count_nonzero(board))
  assert env._elapsed_steps == stones and env.turn == turn and list(env.legal_actions()) == [col]
  after = board.copy()
  after[7 * int(np.count_nonzero(board[col::7])) + col] = turn
  made = lines_of(after, turn)
  assert made == ([kind] if kind in WINS else [])      # the position is what its name says: that direction and no other
  assert (stones == 41) == (kind == 'draw')
  obs, reward, done, info = env.step(col)
  assert np.array_equal(env.board, after) and np.array_equal(obs, -turn * after)
  if kind in WINS:
    assert (reward, done, info['result']) == (1, True, 'player 1 wins' if turn == 1 else 'player 2 wins')
  elif kind == 'draw':
    assert (reward, done, info['result']) == (0, True, 'draw')
  else:
    assert (reward, done, info['result']) == (0, False, None)
  assert env._elapsed_steps == stones + 1 and env.turn == -turn


def test_configuration():
  from model_based_rl_amd.config import ENV_SHAPES, make_config
  from model_based_rl_amd.envs import ConnectFour, get_environment
  cfg = make_config(['--environment', 'ConnectFour', '--two_players'])
  assert cfg.action_space == 7 and tuple(cfg.obs_space) == (42,) and ENV_SHAPES['ConnectFour'] == (7, (42,))
  assert type(get_environment(cfg)) is ConnectFour
