"""The device-drawn root noise restated in float64 from the definition alone (the header comment of mz_gamma,
csrc/mz_selfplay.hip.h; k_gz_root, csrc/mz_gumbel.hip.h): its own vectorised Philox4x32-10, numpy's float64 libm.  Nothing of
the project is imported; tests/test_dirichlet_cpu.py shows that what is stated here is Dirichlet, tests/test_gpu_dirichlet.py
holds every device path to it.

  Gamma(alpha), Marsaglia-Tsang: alpha is rounded to float32 first; alpha' = alpha + 1 where alpha < 1; d = alpha' - 1/3,
  c = 1 / sqrt(9 d).  Iteration ctr = 0, 1, ... (at most 64; ctr advances on EVERY iteration) draws the Philox block of
  counter (env, (uint32)move, action | ctr << 8, 3 << 24 | (move >> 32 & 0xFFFFFF)) under the engine's seed:
    u1 = 1 - (x >> 8) / 2^24, u2 = (y >> 8) / 2^24, u = 1 - (z >> 8) / 2^24, the normal x = sqrt(-2 ln u1) cos(2 pi u2),
    v = (1 + c x)^3; the iteration is accepted when 1 + c x > 0 and ln u < x^2 / 2 + d - d v + d ln v: g = d v.
  alpha < 1: g *= U^(1 / alpha) with U = 1 - (x >> 8) / 2^24 of the block at ctr = 0xFFFFFF -- in the log domain here, so
  that nothing underflows.
  Dirichlet: the Gammas of the legal actions over their sum, 0 at the illegal ones.
  Gumbel: -ln(-ln u), u the 53-bit uniform of words (x, y) of counter (env, (uint32)move, move >> 32, 11 << 24 | action)."""
import numpy as np

RNG_DIRICHLET, RNG_GUMBEL = 3, 11
MAX_ITER = 64
_M = np.uint64(0xFFFFFFFF)
_S = np.uint64(32)


def philox(seed, c0, c1, c2, c3):
  """Philox4x32-10 keyed by the 64-bit seed on arrays of counter words (broadcast together); returns the four output words
  as uint64 arrays holding 32-bit values"""
  c = [np.asarray(x, np.uint64) & _M for x in np.broadcast_arrays(c0, c1, c2, c3)]
  k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c[0]
    p1 = np.uint64(0xCD9E8D57) * c[2]
    c = [(p1 >> _S) ^ c[1] ^ np.uint64(k0), p1 & _M, (p0 >> _S) ^ c[3] ^ np.uint64(k1), p0 & _M]
    k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
  return c


def _u24(w):
  return (w >> np.uint64(8)).astype(np.float64) / 16777216.0


def log_gamma(alpha, seed, env, move, action):
  """ln of the Gamma(alpha) draw of (env, move, action) -- env and action arrays of one shape, move one integer.  Returns
  (ln g, decision margin, iterations run), arrays of that shape.  The margin: the smallest, over the iterations run, of
  |1 + c x| and, where v > 0, |ln u - (x^2 / 2 + d - d v + d ln v)|."""
  env, action = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(action, np.uint64))
  shape = env.shape
  env, action = env.reshape(-1), action.reshape(-1)
  move = int(move)
  al = float(np.float32(alpha))
  aa = al + 1.0 if al < 1.0 else al
  d = aa - 1.0 / 3.0
  c = 1.0 / np.sqrt(9.0 * d)
  c1, c3 = move & 0xFFFFFFFF, (RNG_DIRICHLET << 24) | ((move >> 32) & 0xFFFFFF)
  n = env.size
  lg = np.full(n, np.log(d))              # no iteration accepted: g = d
  margin = np.full(n, np.inf)
  iters = np.zeros(n, np.int64)
  todo = np.arange(n)
  for ctr in range(MAX_ITER):
    if todo.size == 0:
      break
    r = philox(seed, env[todo], c1, action[todo] | np.uint64(ctr << 8), c3)
    u1, u2, u = 1.0 - _u24(r[0]), _u24(r[1]), 1.0 - _u24(r[2])
    x = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    w = 1.0 + c * x
    iters[todo] += 1
    m = np.abs(w)
    pos = w > 0.0
    v = np.where(pos, w, 1.0) ** 3
    gap = np.log(u) - (0.5 * x * x + d - d * v + d * np.log(v))
    m = np.where(pos, np.minimum(m, np.abs(gap)), m)
    margin[todo] = np.minimum(margin[todo], m)
    ok = pos & (gap < 0.0)
    lg[todo[ok]] = np.log(d * v[ok])
    todo = todo[~ok]
  if al < 1.0:
    r = philox(seed, env, c1, action | np.uint64(0xFFFFFF << 8), c3)
    lg = lg + np.log(1.0 - _u24(r[0])) / al
  return lg.reshape(shape), margin.reshape(shape), iters.reshape(shape)


def gamma(alpha, seed, env, move, action):
  """the Gamma(alpha) draw of (env, move, action), float64 (exp of log_gamma: tiny, not 0, where float32 underflows)"""
  return np.exp(log_gamma(alpha, seed, env, move, action)[0])


def dirichlet(alpha, seed, env0, B, A, move, legal=None, with_iters=False):
  """the root noise of environments env0 .. env0 + B - 1 at move `move`: (noise [B, A] float64, decision margin [B]).  legal
  [B, A] (nonzero = legal; every row needs a legal action) or None: illegal actions are zeroed before the sum; the margin of a
  row is the smallest one among its legal actions.  with_iters: also the largest iteration count of the row."""
  ok = np.ones((B, A), bool) if legal is None else np.asarray(legal).reshape(B, A) != 0
  assert ok.any(1).all()
  b, a = np.nonzero(ok)
  lg, mg, it = log_gamma(alpha, seed, env0 + b, move, a)
  L = np.full((B, A), -np.inf)
  L[b, a] = lg
  # the Gammas themselves over their sum, as the device and numpy form it (float64 holds them down to alpha = 0.03, where
  # the smallest is 2^-800; shifting every row to a largest Gamma of 1 would round the entries next to 1 on a coarser
  # grid than theirs, which a KS test at alpha = 0.03 sees).  A row whose sum underflows all the same is shifted.
  g = np.exp(L)
  tiny = g.sum(1) < 1e-300
  g[tiny] = np.exp(L[tiny] - L[tiny].max(1, keepdims=True))
  noise = g / g.sum(1, keepdims=True)
  margin = np.full((B, A), np.inf)
  margin[b, a] = mg
  if with_iters:
    iters = np.zeros((B, A), np.int64)
    iters[b, a] = it
    return noise, margin.min(1), iters.max(1)
  return noise, margin.min(1)


def gumbel(seed, env, move, action):
  """G of (env, move, action): -ln(-ln u), u from 53 bits"""
  move = int(move)
  r = philox(seed, np.asarray(env, np.uint64), move & 0xFFFFFFFF, (move >> 32) & 0xFFFFFFFF,
             np.uint64(RNG_GUMBEL << 24) | np.asarray(action, np.uint64))
  u = (((r[0] << _S) | r[1]) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
  u = np.where(u > 0.0, u, 2.0 ** -54)
  return -np.log(-np.log(u))
