"""tests/dirichlet_py.py -- the float64 restatement the device's root noise is held to (tests/test_gpu_dirichlet.py) -- is
Dirichlet(alpha * 1_legal): N = 65,536 rows per (alpha, A, mask) against numpy's own sampler and the closed-form moments.
  KS       every marginal against numpy.random.RandomState.dirichlet, two-sample Kolmogorov-Smirnov: D below the distribution-free
           critical value sqrt(-ln(1e-6 / 2) / 2) * sqrt(2 / N) (a false alarm in 1e-6 comparisons)
  moments  E[x_i^k], k = 1..4, and E[x_i x_j] (j = i + 1 among the legal actions, cyclic) from math.lgamma, every sample mean
           within 5 standard errors, the standard error from the closed-form moment of order 2k
  independence  across environments, consecutive moves, move and move + 2^32: correlations within 5 / sqrt(N)
  acceptance    no draw comes near the 64 iterations the sampler allows
A masked row is Dirichlet over its legal actions and exactly 0 elsewhere; one mask with holes per (A), the same in every row."""
import functools
import math

import numpy as np
import pytest

from tests import dirichlet_py as dp

N = 65536
ALPHAS = [0.03, 0.25, 1.0, 1.5]
ACTIONS = [2, 4, 7, 18, 32]
SEED = (0x5EED1234 << 32) | 0x9ABCDEF1      # both key words in use
KS_CRIT = math.sqrt(-math.log(1e-6 / 2) / 2) * math.sqrt(2.0 / N)      # 2.69 * sqrt(2 / N) = 0.0149


def mask_of(A):
  """the legal actions of the masked case: density 0.6, at least one (A = 2: exactly one)"""
  m = np.random.RandomState(100 + A).uniform(size=A) < 0.6
  if A == 2:
    m = np.array([False, True])
  assert m.any() and not m.all()
  return m


@functools.lru_cache(maxsize=None)
def sample(alpha, A, masked):
  """(noise [N, A], largest iteration count, the legal mask [A]) -- computed once, shared, read-only"""
  m = mask_of(A) if masked else np.ones(A, bool)
  move = 1000 * A + int(100 * alpha)
  x, _, it = dp.dirichlet(alpha, SEED, 77, N, A, move, np.broadcast_to(m, (N, A)) if masked else None, with_iters=True)
  x.setflags(write=False)
  return x, int(it.max()), m


def ks_distance(a, b):
  """two-sample Kolmogorov-Smirnov distance, ties handled (both ECDFs at every pooled point).  Entries within 2^-50 of 1 count
  as 1 in both samples: at alpha = 0.03 and two legal actions a sixth of the mass lies in the last two float64 values up to 1,
  and which of the two a row lands on is decided by the last bit of the quotient -- numpy multiplies by 1 / sum, the
  restatement divides by the sum; 2 % of the rows differ by that bit alone.  Every other threshold is compared as it is."""
  a, b = np.sort(np.where(a > 1.0 - 2.0 ** -50, 1.0, a)), np.sort(np.where(b > 1.0 - 2.0 ** -50, 1.0, b))
  pts = np.concatenate([a, b])
  return float(np.abs(np.searchsorted(a, pts, side='right') / a.size - np.searchsorted(b, pts, side='right') / b.size).max())


def beta_moment(a, b, k):
  """E[x^k], x ~ Beta(a, b)"""
  return math.exp(math.lgamma(a + k) - math.lgamma(a) + math.lgamma(a + b) - math.lgamma(a + b + k))


CASES = [(al, A, mk) for al in ALPHAS for A in ACTIONS for mk in (False, True)]
IDS = ['alpha%g-A%d-%s' % (al, A, 'masked' if mk else 'all') for al, A, mk in CASES]


@pytest.mark.parametrize('alpha,A,masked', CASES, ids=IDS)
def test_marginals_against_numpy(alpha, A, masked):
  x, _, m = sample(alpha, A, masked)
  K = int(m.sum())
  assert np.all(x[:, ~m] == 0.0) and np.abs(x.sum(1) - 1.0).max() < 1e-12 and x.min() >= 0.0 and not np.isnan(x).any()
  if K == 1:
    assert np.all(x[:, m] == 1.0)
    return
  ref = np.random.RandomState(int(1000 * alpha) + A).dirichlet([float(np.float32(alpha))] * K, size=N)
  worst = max(ks_distance(x[:, a], ref[:, j]) for j, a in enumerate(np.flatnonzero(m)))
  print('alpha %g, A %d, %d legal: worst KS distance %.5f (critical %.5f)' % (alpha, A, K, worst, KS_CRIT))
  assert worst < KS_CRIT


@pytest.mark.parametrize('alpha,A,masked', CASES, ids=IDS)
def test_moments_against_the_closed_form(alpha, A, masked):
  x, _, m = sample(alpha, A, masked)
  K = int(m.sum())
  if K == 1:
    return
  a = float(np.float32(alpha))
  a0 = K * a
  worst = 0.0
  cols = np.flatnonzero(m)
  for k in (1, 2, 3, 4):
    mean, second = beta_moment(a, a0 - a, k), beta_moment(a, a0 - a, 2 * k)
    se = math.sqrt((second - mean * mean) / N)
    z = np.abs((x[:, cols] ** k).mean(0) - mean) / se
    worst = max(worst, float(z.max()))
    assert z.max() < 5.0, (k, int(cols[z.argmax()]), float(z.max()))
  # E[x_i x_j] = a^2 / (a0 (a0 + 1)); E[x_i^2 x_j^2] = (a (a + 1))^2 / (a0 (a0 + 1) (a0 + 2) (a0 + 3))
  mean = a * a / (a0 * (a0 + 1.0))
  second = (a * (a + 1.0)) ** 2 / (a0 * (a0 + 1.0) * (a0 + 2.0) * (a0 + 3.0))
  se = math.sqrt((second - mean * mean) / N)
  z = np.abs((x[:, cols] * x[:, np.roll(cols, -1)]).mean(0) - mean) / se
  worst = max(worst, float(z.max()))
  print('alpha %g, A %d, %d legal: worst moment deviation %.2f standard errors' % (alpha, A, K, worst))
  assert z.max() < 5.0, ('pair', int(cols[z.argmax()]), float(z.max()))


def test_acceptance_needs_few_iterations():
  worst = max(sample(al, A, mk)[1] for al, A, mk in CASES)
  print('most iterations of one draw: %d of %d' % (worst, dp.MAX_ITER))
  assert worst < dp.MAX_ITER


@pytest.mark.parametrize('alpha', [0.25, 1.5])
def test_draws_are_independent(alpha):
  A, move = 4, 12345
  draw = lambda env0, mv: dp.dirichlet(alpha, SEED, env0, N, A, mv)[0]
  base = draw(0, move)
  bound = 5.0 / math.sqrt(N)
  for what, other in (('the next environment', draw(1, move)), ('the next move', draw(0, move + 1)),
                      ('move + 2^32', draw(0, move + (1 << 32)))):
    assert not np.array_equal(base, other), what
    for i in range(A):
      for j in range(A):
        r = np.corrcoef(base[:, i], other[:, j])[0, 1]
        assert abs(r) < bound, (what, i, j, r)
  # (the next environment: rows 1.. of `base` are rows 0.. of that draw -- the key is the environment, not the row)
  assert np.array_equal(base[1:], draw(1, move)[:-1])


def test_gumbel_is_gumbel():
  """-ln(-ln u): the standard Gumbel law (CDF exp(-exp(-g))) by a one-sample KS test at the same false-alarm rate, distinct
  per (env, move, action), finite"""
  env, act = np.meshgrid(np.arange(100, 100 + N // 8), np.arange(8), indexing='ij')
  g = dp.gumbel(SEED, env, 7, act).reshape(-1)
  assert np.isfinite(g).all() and np.unique(g).size == g.size
  s = np.sort(g)
  cdf = np.exp(-np.exp(-s))
  n = s.size
  D = max(np.abs(cdf - np.arange(n) / n).max(), np.abs(cdf - np.arange(1, n + 1) / n).max())
  assert D < math.sqrt(-math.log(1e-6 / 2) / 2) / math.sqrt(n)
  assert not np.array_equal(g, dp.gumbel(SEED, env, 7 + (1 << 32), act).reshape(-1))
