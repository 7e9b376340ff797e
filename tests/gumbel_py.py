"""The Gumbel MuZero search (DESIGN s7h) restated in pure Python from the definition alone: Node objects with dict children
after the reference's mcts.py (the same expand / backpropagate / MinMaxStats, math.exp), the root rule (Gumbel-top-m with
sequential halving through seq), the rule below the root and the improved policy from completed Q-values.  Nothing of the
native code is imported.  Also the fake network every side of the tests evaluates: a function of (tree, parent slot, action)
through Philox words, on a coarse grid so that exact ties occur -- logits in eighths, values and rewards in sixteenths, the
given Gumbel draws in 1/64 -- so the device, the host twin and this restatement receive bit-identical float32 outputs."""
import math

import numpy as np

from tests.playout_py import philox

SIMS = 16
TREES = 12


def seq(m, n):
  """mctx's get_sequence_of_considered_visits(m, n)"""
  if m <= 1:
    return list(range(n))
  log2max = int(math.ceil(math.log2(m)))
  sequence, visits, k = [], [0] * m, m
  while len(sequence) < n:
    for _ in range(max(1, int(n / (log2max * k)))):
      sequence.extend(visits[:k])
      for i in range(k):
        visits[i] += 1
    k = max(2, k // 2)
  return sequence[:n]


# ---- the fake network
def fake_leaf(seed, tree, slot, action, A):
  """(value, reward, logits [A]) of the node reached from expansion slot `slot` of tree `tree` by `action`"""
  w = []
  for j in range(1 + (A + 1) // 4 + 1):
    w += philox(seed, tree, slot, action, j)
  value = np.float32(((w[0] >> 27) - 16) / 16.0)           # sixteenths in [-1, 1)
  reward = np.float32(((w[1] >> 28) - 8) / 16.0)           # sixteenths in [-0.5, 0.5)
  logits = np.array([((w[2 + a] >> 27) - 16) / 8.0 for a in range(A)], np.float32)      # eighths in [-2, 2)
  return value, reward, logits


def fake_root(seed, tree, A):
  """(value, logits [A], G [A]) of the root of tree `tree`; G on a grid of 1/64 in [-4, 4)"""
  value, _, logits = fake_leaf(seed, tree, 0xFFFF, 0, A)
  w = []
  for j in range((A + 3) // 4):
    w += philox(seed, tree, 0xFFFE, 0, j)
  return value, logits, np.array([((w[a] >> 23) - 256) / 64.0 for a in range(A)])


def fake_eval(seed, A):
  """eval_fn(sim, parent_slot [n], action [n]) -> (value [n], reward [n], logits [n, A]) on the fake network"""
  def f(sim, slot, act):
    outs = [fake_leaf(seed, b, int(slot[b]), int(act[b]), A) for b in range(len(slot))]
    return (np.array([o[0] for o in outs], np.float32), np.array([o[1] for o in outs], np.float32),
            np.stack([o[2] for o in outs]).astype(np.float32))
  return f


# ---- the search
class MinMaxStats(object):
  def __init__(self, lo=None, hi=None):
    self.minimum = float('inf') if lo is None else lo
    self.maximum = -float('inf') if hi is None else hi

  def update(self, value):
    self.minimum = min(self.minimum, value)
    self.maximum = max(self.maximum, value)

  def normalize(self, value):
    if self.maximum > self.minimum:
      return (value - self.minimum) / (self.maximum - self.minimum)
    elif self.maximum == self.minimum:
      return 1.0
    return value


class Node(object):
  def __init__(self, prior):
    self.visit_count, self.value_sum, self.reward, self.children, self.prior, self.to_play = 0, 0.0, 0.0, {}, prior, 1
    self.slot = None       # its expansion slot, once expanded
    self.vhat = None       # the raw network value at it, in its mover's view

  def expanded(self):
    return len(self.children) > 0

  def value(self):
    return 0 if self.visit_count == 0 else self.value_sum / self.visit_count

  def expand(self, logits, to_play, actions):
    self.to_play = to_play
    policy = {a: math.exp(float(logits[a])) for a in actions}
    policy_sum = sum(policy.values())
    for action, p in policy.items():
      self.children[action] = Node(p / policy_sum)


class Search(object):
  """one tree of A actions.  n: the engine's num_simulations (it fixes seq, however many simulations are run)"""

  def __init__(self, A, n, to_play, legal, root_value, root_logits, G=None, two_players=True, discount=0.997,
               known_bounds=(None, None), max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=0.0):
    self.A, self.n, self.two, self.discount = A, n, two_players, discount
    self.c_visit, self.c_scale = c_visit, c_scale
    self.min_max_stats = MinMaxStats(*known_bounds)
    self.root = Node(0)
    self.root.expand(root_logits, to_play, list(legal))
    self.root.vhat, self.root.slot = float(root_value), 0
    self.gl = {a: (gumbel_scale * float(G[a]) if gumbel_scale != 0 else 0.0) + float(root_logits[a]) for a in legal}
    self.seq = seq(min(max_considered, len(legal)), n)
    self.slots = [self.root]
    self.sims_done = 0
    self.paths, self.selected = [], []
    self.pending = None

  def q(self, child):
    value = child.value_sum / child.visit_count
    return child.reward + self.discount * (-value if self.two else value)

  def stats(self, node):
    """(pi' {a: .}, v_mix, sigma {a: .}, sum N) of an expanded node"""
    ch = node.children
    sum_n = sum(c.visit_count for c in ch.values())
    max_n = max(c.visit_count for c in ch.values())
    spq = sp = 0.0
    for a in sorted(ch):
      if ch[a].visit_count > 0:
        spq = spq + ch[a].prior * self.q(ch[a])
        sp = sp + ch[a].prior
    v_mix = (node.vhat + sum_n * spq / sp) / (1.0 + sum_n) if sum_n > 0 and sp > 0 else node.vhat
    cs = (self.c_visit + max_n) * self.c_scale
    sigma = {a: cs * self.min_max_stats.normalize(self.q(c) if c.visit_count > 0 else v_mix) for a, c in ch.items()}
    s_max = max(sigma.values())
    w = {a: ch[a].prior * math.exp(sigma[a] - s_max) for a in sorted(ch)}
    ws = 0.0
    for a in sorted(w):
      ws = ws + w[a]
    return {a: w[a] / ws for a in w}, v_mix, sigma, sum_n

  def root_choice(self, want):
    """arg-max of g + logit + sigma over the legal actions visited `want` times (None: the most visited's count)"""
    ch = self.root.children
    _, _, sigma, _ = self.stats(self.root)
    if want is None:
      want = max(c.visit_count for c in ch.values())
    cand = [a for a in ch if ch[a].visit_count == want] or list(ch)
    return max((self.gl[a] + sigma[a], a) for a in cand)[1]

  def select(self):
    """the descent of the next simulation -> (parent slot, action)"""
    node, path, to_play = self.root, [0], self.root.to_play
    parent = None
    while node.expanded():
      if node is self.root:
        action = self.root_choice(self.seq[self.sims_done])
      else:
        pi, _, _, sum_n = self.stats(node)
        action = max((pi[a] - node.children[a].visit_count / (1.0 + sum_n), a) for a in node.children)[1]
      parent = node
      path.append(1 + node.slot * self.A + action)
      node = node.children[action]
      to_play = -to_play if self.two else to_play
    self.pending = (parent, action, node, to_play, path)
    self.paths.append(path)
    self.selected.append((parent.slot, action))
    return parent.slot, action

  def expand_backup(self, value, reward, logits):
    parent, action, node, to_play, path = self.pending
    nodes = [self.root]
    for k in path[1:]:
      nodes.append(nodes[-1].children[(k - 1) % self.A])
    node.slot = len(self.slots)
    self.slots.append(node)
    node.reward = float(reward)
    node.vhat = float(value)
    node.expand(logits, to_play, list(range(self.A)))
    self.backpropagate(nodes, float(value), to_play)
    self.sims_done += 1

  def backpropagate(self, search_path, value, to_play):
    for idx, node in enumerate(reversed(search_path)):
      node.value_sum += value if node.to_play == to_play else -value
      node.visit_count += 1
      reward = (-node.reward if node.to_play == to_play else node.reward) if self.two else node.reward
      if idx < len(search_path) - 1:
        v = node.value_sum / node.visit_count
        self.min_max_stats.update(node.reward - self.discount * v if self.two else node.reward + self.discount * v)
      value = reward + self.discount * value

  def pick(self):
    """the end of the move -> (action, its child's reward, pi' [A], v_mix)"""
    action = self.root_choice(None)
    pi, v_mix, _, _ = self.stats(self.root)
    out = np.zeros(self.A)
    for a, p in pi.items():
      out[a] = p
    return action, self.root.children[action].reward, out, v_mix

  def arrays(self):
    """the tree in the engine's layout: node arrays [NN] (child a of slot e = node 1 + e * A + a), EX, v^ per slot"""
    A, S = self.A, self.n + 1
    NN = 1 + S * A
    d = dict(N=np.zeros(NN, np.int32), W=np.zeros(NN), P=np.zeros(NN), R=np.zeros(NN, np.float32), E=np.full(NN, -1, np.int32),
             TP=np.zeros(NN, np.int8), EX=np.zeros(NN, np.uint8), vhat=np.zeros(S, np.float32))

    def put(i, node):
      d['N'][i], d['W'][i], d['P'][i], d['R'][i], d['TP'][i], d['EX'][i] = (node.visit_count, node.value_sum, node.prior,
                                                                           node.reward, node.to_play, 1)
      d['E'][i] = -1 if node.slot is None else node.slot
    put(0, self.root)
    legal = 0
    for e, node in enumerate(self.slots):
      d['vhat'][e] = node.vhat
      for a, child in node.children.items():
        put(1 + e * A + a, child)
        if e == 0:
          legal |= 1 << a
    d['legal'] = legal
    d['minmax'] = np.array([self.min_max_stats.minimum, self.min_max_stats.maximum])
    d['sel_slot'] = np.array([s for s, _ in self.selected] + [0] * (self.n - len(self.selected)), np.int32)
    d['sel_action'] = np.array([a for _, a in self.selected] + [0] * (self.n - len(self.selected)), np.int32)
    d['plens'] = np.array([len(p) for p in self.paths] + [0] * (self.n - len(self.paths)), np.int32)
    d['paths'] = np.full((self.n, self.n + 2), -1, np.int32)
    for s, p in enumerate(self.paths):
      d['paths'][s, :len(p)] = p
    d['action'], d['pred_reward'], d['pi'], d['v_mix'] = self.pick()
    return d


# ---- the committed test sets: B = 12 trees, 16 simulations, roots with 1, 2 and 3 legal actions among them
SETS = {
    # name: (A, two_players, known_bounds, discount, seed of the fake network)
    'tictactoe': (9, True, (-1.0, 1.0), 0.997, 0x6B01),
    'connect_four': (7, True, (-1.0, 1.0), 0.997, 0x6B02),
    'single_player': (4, False, (None, None), 0.997, 0x6B03),
}


def case(name):
  """the roots of a test set: dict(A, two, bounds, discount, seed, to_play [B] int8, legal [B, A] uint8, root_value [B],
  root_logits [B, A] float32, G [B, A] float64)"""
  A, two, bounds, discount, seed = SETS[name]
  rng = np.random.RandomState(seed)
  legal = np.zeros((TREES, A), np.uint8)
  for b in range(TREES):
    k = b + 1 if b < 3 else int(rng.randint(3, A + 1))      # trees 0, 1, 2: one, two and three legal actions
    legal[b, rng.choice(A, k, replace=False)] = 1
  to_play = np.array([1 if not two or b % 2 == 0 else -1 for b in range(TREES)], np.int8)
  roots = [fake_root(seed, b, A) for b in range(TREES)]
  return dict(A=A, two=two, bounds=bounds, discount=discount, seed=seed, to_play=to_play, legal=legal,
              root_value=np.array([r[0] for r in roots], np.float32), root_logits=np.stack([r[1] for r in roots]).astype(np.float32),
              G=np.stack([r[2] for r in roots]))


def search_batch(c, gumbel_scale, sims=SIMS, num_simulations=None, **kw):
  """the trees of case c in lock-step on the fake network; returns the stacked arrays of Search.arrays"""
  trees = [Search(c['A'], sims, int(c['to_play'][b]), [a for a in range(c['A']) if c['legal'][b, a]], c['root_value'][b],
                  c['root_logits'][b], c['G'][b], two_players=c['two'], discount=c['discount'], known_bounds=c['bounds'],
                  gumbel_scale=gumbel_scale, **kw) for b in range(TREES)]
  for _ in range(sims if num_simulations is None else num_simulations):
    for b, t in enumerate(trees):
      slot, action = t.select()
      t.expand_backup(*fake_leaf(c['seed'], b, slot, action, c['A']))
  per = [t.arrays() for t in trees]
  return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


TREE_FIELDS = ('N', 'W', 'P', 'R', 'E', 'TP')
