"""A plain float64 FCNetwork for the support-shape tests (no test functions here).

The reference's FCNetwork in eval mode (networks.py:122-170) and Config.inverse_transform (config.py:27-33), with separate
value and reward supports, --no_target_transform and --no_support: every head is Linear -> ReLU -> Linear, the hidden
state is relu(LayerNorm(50)) with eps 1e-5, dynamics read [hidden | one-hot(action)], and a support head's scalar is the
softmax expectation over range(smin, smax + 1) followed by the inverse of h(x), all in float64."""
import numpy as np

H = 50


def inverse_h(x, dtype=np.float64):
  """the inverse of h(x) = sign(x)(sqrt(|x| + 1) - 1) + 0.001 x in the reference's operation order (config.py:31-32); in
  float32 its sqrt(...) - 1 cancellation makes the reference's own output a staircase"""
  x = np.asarray(x, dtype)
  c = lambda v: dtype(v)
  return np.sign(x) * (((np.sqrt(c(1) + c(4 * 0.001) * (np.abs(x) + c(1) + c(0.001))) - c(1)) / c(2 * 0.001)) ** 2 - c(1))


def support_to_scalar64(logits, smin, no_target_transform=False):
  """softmax expectation over the integer support starting at smin, then the inverse transform (config.py:27-33)"""
  z = np.asarray(logits, np.float64)
  p = np.exp(z - z.max(1, keepdims=True))
  p /= p.sum(1, keepdims=True)
  x = p @ np.arange(smin, smin + z.shape[1], dtype=np.float64)
  return x if no_target_transform else inverse_h(x)


def support_spread(logits, smin):
  """sum_i p_i |s_i - x| of the softmax over the support: logit errors e_i move the expectation x by
  sum_i p_i e_i (s_i - x) (to first order), at most max |e| times this"""
  z = np.asarray(logits, np.float64)
  p = np.exp(z - z.max(1, keepdims=True))
  p /= p.sum(1, keepdims=True)
  s = np.arange(smin, smin + z.shape[1], dtype=np.float64)
  return (p * np.abs(s - (p @ s)[:, None])).sum(1)


class FC64(object):

  def __init__(self, weights, O, A, value_support=(-15, 15), reward_support=(-15, 15), no_target_transform=False,
               no_support=False):
    self.w = {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, np.float64) for k, v in weights.items()}
    self.O, self.A = int(O), int(A)
    self.vmin, self.rmin = int(value_support[0]), int(reward_support[0])
    self.nt, self.ns = bool(no_target_transform), bool(no_support)
    sv = 1 if no_support else value_support[1] - value_support[0] + 1
    sr = 1 if no_support else reward_support[1] - reward_support[0] + 1
    assert self.w['value_head.value.weight'].shape == (sv, 512) and self.w['reward_head.reward.weight'].shape == (sr, 512)

  def _two(self, head, out, x):
    w = self.w
    y = np.maximum(x @ w[head + '.fc1.weight'].T + w[head + '.fc1.bias'], 0.0)
    return y @ w[head + '.' + out + '.weight'].T + w[head + '.' + out + '.bias']

  def _ln_relu(self, x):
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return np.maximum((x - mu) / np.sqrt(var + 1e-5) * self.w['LN.weight'] + self.w['LN.bias'], 0.0)

  def _scalar(self, out, smin):
    return out[:, 0].copy() if self.ns else support_to_scalar64(out, smin, self.nt)

  def representation(self, obs):
    return self._ln_relu(self._two('representation_head', 'out', np.asarray(obs, np.float64).reshape(len(obs), -1)))

  def prediction(self, hidden):
    """-> (value, policy logits)"""
    h = np.asarray(hidden, np.float64)
    return self._scalar(self._two('value_head', 'value', h), self.vmin), self._two('policy_head', 'policy', h)

  def _with_action(self, hidden, action):
    return np.concatenate([np.asarray(hidden, np.float64), np.eye(self.A)[np.asarray(action, np.int64).reshape(-1)]], 1)

  def dynamics(self, hidden, action):
    """-> (next hidden state, reward)"""
    x = self._with_action(hidden, action)
    return self._ln_relu(self._two('transition_head', 'out', x)), self._scalar(self._two('reward_head', 'reward', x), self.rmin)

  def value_spread(self, hidden):
    """support_spread of the value head's softmax"""
    return support_spread(self._two('value_head', 'value', np.asarray(hidden, np.float64)), self.vmin)

  def reward_spread(self, hidden, action):
    """support_spread of the reward head's softmax"""
    return support_spread(self._two('reward_head', 'reward', self._with_action(hidden, action)), self.rmin)

  def initial(self, obs):
    """-> (hidden, value, logits), the order of oracle.FCNet.initial"""
    h = self.representation(obs)
    v, lg = self.prediction(h)
    return h, v, lg

  def recurrent(self, hidden, action):
    """-> (hidden, reward, value, logits), the order of oracle.FCNet.recurrent"""
    h, r = self.dynamics(hidden, action)
    v, lg = self.prediction(h)
    return h, r, v, lg


def scalar_bound(want, support, transformed):
  """per-row bound on a float32 value / reward against the float64 reference: one float32 staircase step of the reference's
  own formula with the transform (tests/test_oracle_net.py:test_inverse_transform_large_values), else today's 1e-5 at 31 bins
  scaled with the largest support magnitude M = max(|smin|, |smax|)"""
  want = np.asarray(want, np.float64)
  if transformed:
    return 2e-4 * (1 + np.abs(want))
  return np.full_like(want, 1e-5 * max(1.0, max(abs(support[0]), abs(support[1])) / 15.0))
