"""envs.CartPole, the definition of CartPole-v1 / -v0 in this project (gym is not installed): its polynomials, one known
step, termination, rewards, the time limit, seeding, and the configuration entries.  No GPU."""
import math

import numpy as np
import pytest


def test_polynomials_against_libm():
  """sin_p / cos_p on 10^4 points of [-0.8, 0.8]: within 2.5e-16 of math.sin / math.cos (twice the 1.11e-16 measured on a
  400 001-point grid, for the off-grid points)"""
  from model_based_rl_amd.envs import cos_p, sin_p
  xs = np.random.RandomState(0).uniform(-0.8, 0.8, 10 ** 4)
  es = max(abs(sin_p(x) - math.sin(x)) for x in xs)
  ec = max(abs(cos_p(x) - math.cos(x)) for x in xs)
  print('max |sin_p - sin| %.3g, max |cos_p - cos| %.3g' % (es, ec))
  assert es <= 2.5e-16 and ec <= 2.5e-16


def test_known_step_from_the_zero_state():
  from model_based_rl_amd.envs import CartPole
  env = CartPole()
  env.set_state((0.0, 0.0, 0.0, 0.0))
  obs, reward, done, info = env.step(1)
  temp = 10.0 / 1.1
  tha = (9.8 * math.sin(0.0) - math.cos(0.0) * temp) / (0.5 * (4.0 / 3.0 - 0.1 / 1.1))
  xa = temp - 0.05 * tha / 1.1
  x, x_dot, theta, theta_dot = env.state
  assert x == 0.0 and theta == 0.0
  assert abs(x_dot - 0.02 * xa) <= 1e-12 and abs(x_dot - 10 / 1.1 * (1 + 0.05 / (1.1 * 0.5 * (4 / 3 - 0.1 / 1.1))) * 0.02) <= 1e-12
  assert abs(x_dot - 0.1951220) < 1e-7
  assert abs(theta_dot - 0.02 * tha) <= 1e-12 and abs(theta_dot + 0.2926829) < 1e-7
  assert reward == 1.0 and done is False
  assert obs.dtype == np.float32 and np.array_equal(obs, np.array(env.state, np.float32))
  assert env.action_space.n == 2 and env.observation_space.shape == (4,) and list(env.legal_actions()) == [0, 1]
  # the other action mirrors it
  env.set_state((0.0, 0.0, 0.0, 0.0))
  env.step(0)
  assert env.state == (0.0, -x_dot, 0.0, -theta_dot)


TH = 12 * 2 * math.pi / 360


@pytest.mark.parametrize('state,want', [
    ((2.4 - 1e-9, 0.0, 0.0, 0.0), False), ((2.4 + 1e-9, 0.0, 0.0, 0.0), True),
    ((-2.4 + 1e-9, 0.0, 0.0, 0.0), False), ((-2.4 - 1e-9, 0.0, 0.0, 0.0), True),
    ((0.0, 0.0, TH - 1e-9, 0.0), False), ((0.0, 0.0, TH + 1e-9, 0.0), True),
    ((0.0, 0.0, -TH + 1e-9, 0.0), False), ((0.0, 0.0, -TH - 1e-9, 0.0), True)])
def test_thresholds(state, want):
  """the state AFTER the step decides: with zero velocities x and theta stay where they were put"""
  from model_based_rl_amd.envs import CartPole
  env = CartPole()
  env.set_state(state)
  obs, reward, done, _ = env.step(1)
  assert env.state[0] == state[0] and env.state[2] == state[2]
  assert done is want and reward == 1.0      # reward 1 on every step, the terminating one included


@pytest.mark.parametrize('name,limit', [('CartPole-v1', 500), ('CartPole-v0', 200)])
def test_time_limit(name, limit):
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.envs import CartPole, get_environment
  env = get_environment(make_config(['--environment', name]))
  assert isinstance(env, CartPole) and env.max_episode_steps == limit
  env.seed(3)
  env.reset()
  for t in range(limit):
    if abs(env.state[2]) > 0.1:      # (drives the counter only)
      env.set_state((0.0, 0.0, 0.0, 0.0))
    assert env._elapsed_steps == t
    _, reward, done, _ = env.step(1 if env.state[2] > 0 else 0)
    assert reward == 1.0
    assert done == (t == limit - 1), t
  assert env._elapsed_steps == limit
  env.reset()
  assert env._elapsed_steps == 0


def test_seeded_reset():
  from model_based_rl_amd.envs import CartPole
  a, b = CartPole(), CartPole()
  a.seed(7); b.seed(7)
  for _ in range(3):
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob) and a.state == b.state
    assert all(-0.05 < v < 0.05 for v in a.state)
    assert oa.dtype == np.float32 and oa.shape == (4,)
  b.seed(8)
  assert not np.array_equal(a.reset(), b.reset())


def test_config_and_lookup():
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.envs import CartPole, get_environment
  cfg = make_config(['--environment', 'CartPole-v1', '--episode_length', '7'])
  assert cfg.action_space == 2 and tuple(cfg.obs_space) == (4,)
  assert cfg.episode_length == 500 and cfg.max_episode_steps == 500      # the time limit, not --episode_length
  assert isinstance(get_environment(cfg), CartPole)
  cfg0 = make_config(['--environment', 'CartPole-v0'])
  assert cfg0.episode_length == 200 and get_environment(cfg0).max_episode_steps == 200
  with pytest.raises(NotImplementedError):
    get_environment(make_config(['--environment', 'LunarLander-v2']))
