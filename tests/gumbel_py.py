"""The Gumbel MuZero search (DESIGN s7h) restated in pure Python from the definition alone: Node objects with dict children
after the reference's mcts.py (the same expand / backpropagate / MinMaxStats, math.exp), the root rule (Gumbel-top-m with
sequential halving through seq), the rule below the root and the improved policy from completed Q-values.  Nothing of the
native code is imported.  Also the fake network every side of the tests evaluates: a function of (tree, parent slot, action)
through Philox words, on a coarse grid so that exact ties occur -- logits in eighths, values and rewards in sixteenths, the
given Gumbel draws in 1/64 -- so the device, the host twin and this restatement receive bit-identical float32 outputs.  Last
the table of committed test sets (SETS: per set its shape, seed, simulations, trees and search parameters) and the hand-built
roots (HAND) for the guarded branches: priors that underflow to 0, and exact ties across every child of every node."""
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


# ---- the committed test sets.  Trees 0, 1, 2 have one, two and three legal actions (as many as A allows)
SEED_CANDIDATES = tuple(range(0x6C01, 0x6C09))
SETS = {
    # name: (A, two_players, known_bounds, discount, seed of the fake network, simulations, trees, the search's parameters)
    'tictactoe': (9, True, (-1.0, 1.0), 0.997, 0x6B01, SIMS, TREES, {}),
    'connect_four': (7, True, (-1.0, 1.0), 0.997, 0x6B02, SIMS, TREES, {}),
    'single_player': (4, False, (None, None), 0.997, 0x6B03, SIMS, TREES, {}),
    # The sets below reach what the three above do not: the lane groups G = 4 with idle lanes (A = 2) and G = 32 (A = 17 .. 32),
    # max_considered below the number of legal actions, other simulation counts, c_visit / c_scale and discount 1.  Each seed
    # is the first of SEED_CANDIDATES for which the host twin's min_gap is >= 1e-9 at gumbel_scale 1 and 0 and the set reaches
    # its cases (tests/test_gumbel_cpu.py: test_the_margin_condition, test_the_sets_reach_the_cases_that_can_go_wrong, and
    # test_the_seeds_are_the_first_that_hold).  (c_visit + simulations) * c_scale <= 100 in every one of them.
    'a2_s8': (2, False, (None, None), 0.997, 0x6C01, 8, TREES, {}),
    'a18_s30': (18, False, (None, None), 0.997, 0x6C01, 30, TREES, {}),
    'a18_s30_m4': (18, False, (None, None), 0.997, 0x6C01, 30, TREES, dict(max_considered=4)),
    'a32_s50': (32, False, (None, None), 0.997, 0x6C01, 50, TREES, {}),
    'a32_two_m8': (32, True, (-1.0, 1.0), 1.0, 0x6C01, 16, TREES, dict(max_considered=8, c_scale=0.1)),
    'a9_s30_m4': (9, True, (-1.0, 1.0), 1.0, 0x6C01, 30, TREES, dict(max_considered=4)),
    'a7_s50_cv0': (7, True, (-1.0, 1.0), 1.0, 0x6C01, 50, TREES, dict(c_visit=0.0, c_scale=2.0)),
    'a13_s33_m5': (13, False, (-2.0, 2.0), 0.9, 0x6C01, 33, TREES, dict(max_considered=5)),
    'a18_b70_s8': (18, False, (None, None), 0.997, 0x6C01, 8, 70, {}),
}
NEW_SETS = tuple(n for n in SETS if n not in ('tictactoe', 'connect_four', 'single_player'))


def group_width(A):
  """the lanes per tree of the device kernels (the engine's shape table): 4, 8, 16 or 32"""
  return 4 if A <= 4 else 8 if A <= 8 else 16 if A <= 16 else 32


def case(name, seed=None):
  """the roots of a test set: dict(A, two, bounds, discount, seed, sims, trees, kw, to_play [B] int8, legal [B, A] uint8,
  root_value [B], root_logits [B, A] float32, G [B, A] float64).  seed: another fake-network seed than the committed one.
  A hand-built root (HAND) has its own outputs under 'eval' instead of the fake network's."""
  if name in HAND:
    return HAND[name]()
  A, two, bounds, discount, seed0, sims, trees, kw = SETS[name]
  seed = seed0 if seed is None else seed
  rng = np.random.RandomState(seed)
  legal = np.zeros((trees, A), np.uint8)
  for b in range(trees):
    k = min(b + 1, A) if b < 3 else int(rng.randint(min(3, A), A + 1))      # trees 0, 1, 2: one, two and three legal actions
    legal[b, rng.choice(A, k, replace=False)] = 1
  if A == 32:
    legal[3] = 1                                                             # every bit of the mask, 31 included
  to_play = np.array([1 if not two or b % 2 == 0 else -1 for b in range(trees)], np.int8)
  roots = [fake_root(seed, b, A) for b in range(trees)]
  return dict(A=A, two=two, bounds=bounds, discount=discount, seed=seed, sims=sims, trees=trees, kw=dict(kw), to_play=to_play,
              legal=legal, root_value=np.array([r[0] for r in roots], np.float32),
              root_logits=np.stack([r[1] for r in roots]).astype(np.float32), G=np.stack([r[2] for r in roots]))


def net(c):
  """eval_fn(sim, parent_slot [n], action [n]) of case c: its own outputs (a hand-built root), or the fake network"""
  return c['eval'] if 'eval' in c else fake_eval(c['seed'], c['A'])


def considered(c):
  """m [B] of the roots of case c: min(max_considered, legal actions)"""
  return np.minimum(c['kw'].get('max_considered', 16), c['legal'].sum(1).astype(np.int64))


def search_batch(c, gumbel_scale, sims=None, num_simulations=None, **kw):
  """the trees of case c in lock-step on its network; returns the stacked arrays of Search.arrays"""
  sims = c['sims'] if sims is None else sims
  kw = dict(c['kw'], **kw)
  n = c['trees']
  trees = [Search(c['A'], sims, int(c['to_play'][b]), [a for a in range(c['A']) if c['legal'][b, a]], c['root_value'][b],
                  c['root_logits'][b], c['G'][b], two_players=c['two'], discount=c['discount'], known_bounds=c['bounds'],
                  gumbel_scale=gumbel_scale, **kw) for b in range(n)]
  f = net(c)
  for s in range(sims if num_simulations is None else num_simulations):
    sel = [t.select() for t in trees]
    v, r, lg = f(s, np.array([x[0] for x in sel], np.int32), np.array([x[1] for x in sel], np.int32))
    for b, t in enumerate(trees):
      t.expand_backup(v[b], r[b], lg[b])
  per = [t.arrays() for t in trees]
  return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


# ---- hand-built roots: the outputs are a plain function of (parent slot, action), the same float32 values for every side
def _hand(A, two, bounds, discount, sims, legal, root_value, root_logits, G, ev):
  legal = np.asarray(legal, np.uint8)
  n = len(legal)
  return dict(A=A, two=two, bounds=bounds, discount=discount, seed=0, sims=sims, trees=n, kw={}, legal=legal,
              to_play=np.array([1 if not two or b % 2 == 0 else -1 for b in range(n)], np.int8),
              root_value=np.asarray(root_value, np.float32), root_logits=np.asarray(root_logits, np.float32),
              G=np.asarray(G, np.float64), eval=ev)


UNDERFLOW = ((5, 17), (17, 0), (0, 16), (9, 3))      # per tree: (the action with logit 0, the action with G = 900)


def underflow():
  """A = 18, every action legal (tree 3: ten of them): one logit is 0, the others are -800, so every prior but one is
  exp(-800) = 0 in float64; G is 900 on one of the -800 actions, which the first simulation therefore visits.  From then
  until the logit-0 action has its visit the root has sum N > 0 and sp == 0: v_mix is v^.  On a grid, as the fake network."""
  A, n = 18, len(UNDERFLOW)
  logits, G, legal = np.full((n, A), -800.0, np.float32), np.zeros((n, A)), np.ones((n, A), np.uint8)
  for b, (one, up) in enumerate(UNDERFLOW):
    logits[b, one], G[b, up] = 0.0, 900.0
  legal[3, [1, 2, 4, 5, 6, 7, 8, 10]] = 0

  def ev(sim, slot, act):
    slot, act = np.asarray(slot, np.int64), np.asarray(act, np.int64)
    v = (((slot * 7 + act * 3 + np.arange(len(slot))) % 16) - 8) / 16.0
    r = (((slot + act * 5) % 8) - 4) / 16.0
    lg = (((act[:, None] * 5 + slot[:, None] + 3 * np.arange(A)[None, :]) % 17) - 8) / 8.0
    return v.astype(np.float32), r.astype(np.float32), lg.astype(np.float32)
  return _hand(A, False, (None, None), 0.997, 24, legal, [0.25, -0.5, 0.125, 0.0625], logits, G, ev)


def _ties(A, two, bounds, discount):
  """every logit, value, reward and G is 0: every arg-max, at the root and below it, is an exact tie across all the
  existing children.  Tree 0: every action legal; tree 1: the largest is not; tree 2: actions 0, 1 and A - 2 alone"""
  legal = np.ones((3, A), np.uint8)
  legal[1, A - 1] = 0
  legal[2] = 0
  legal[2, [0, 1, A - 2]] = 1
  z = lambda sim, slot, act: (np.zeros(len(slot), np.float32), np.zeros(len(slot), np.float32), np.zeros((len(slot), A), np.float32))
  return _hand(A, two, bounds, discount, 20, legal, np.zeros(3), np.zeros((3, A)), np.zeros((3, A)), z)


HAND = {
    'underflow': underflow,
    'ties18': lambda: _ties(18, False, (None, None), 0.997),
    'ties32': lambda: _ties(32, True, (-1.0, 1.0), 1.0),
}
HAND_RUNS = (('underflow', 1.0), ('ties18', 1.0), ('ties18', 0.0), ('ties32', 1.0), ('ties32', 0.0))      # (root, gumbel_scale)


TREE_FIELDS = ('N', 'W', 'P', 'R', 'E', 'TP')
