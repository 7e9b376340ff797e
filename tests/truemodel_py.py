"""The true-rules search (DESIGN s7g) restated in pure Python from the definition alone: Node objects with dict children after
the reference's mcts.py (the same select_child / ucb_score / backpropagate, math.exp / math.log / math.sqrt), on the rules
of tests/playout_py.py.  Nothing of the native code is imported.  Also the fake network every side of the tests evaluates:
a deterministic function of the observation's integer cells alone, so the device, the host twin and this restatement
receive bit-identical float32 outputs whatever the batch."""
import math

import numpy as np

from tests import playout_py

FAKE_SEED = 0x7E57C0DE
_FAKE_CACHE = {}


def fake_outputs(cells, A):
  """(value, logits[A]) of the observation with integer cells in {-1, 0, +1}: Philox words keyed by the base-3 code of the
  cells.  value = (odd integer) / 2^23, strictly inside (-1, 1); logits on a grid of 64 levels of 1/16 in [-2, 2), so that
  about a tenth of the positions have an exact tie for the largest logit.  All exact in float32."""
  code = 0
  for c in reversed(cells):
    code = code * 3 + (int(c) + 1)
  key = (code, A)
  out = _FAKE_CACHE.get(key)
  if out is None:
    words = []
    for j in range(3):
      words += playout_py.philox(FAKE_SEED, code & 0xFFFFFFFF, (code >> 32) & 0xFFFFFFFF, (code >> 64) & 0xFFFFFFFF, j)
    value = np.float32((2 * ((words[0] >> 9) - (1 << 22)) + 1) / float(1 << 23))
    logits = np.array([((words[1 + a] >> 26) - 32) / 16.0 for a in range(A)], np.float32)
    out = _FAKE_CACHE[key] = (value, logits)
  return out


def fake_network(obs, A):
  """the fake network on a batch of observations [n, O] -> (value [n] float32, logits [n, A] float32)"""
  obs = np.asarray(obs)
  assert np.all(obs == np.rint(obs)) and np.all(np.abs(obs) <= 1)
  outs = [fake_outputs(row.astype(np.int64).tolist(), A) for row in obs]
  return np.array([o[0] for o in outs], np.float32), np.stack([o[1] for o in outs]).astype(np.float32)


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
    self.visit_count, self.value_sum, self.reward, self.children, self.prior, self.to_play = 0, 0, 0, {}, prior, 1
    self.slot = None                                       # its expansion slot, once it has one
    self.board = self.mover = self.step = None             # its position, once it has its slot
    self.finished = False

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
  """one tree.  kind 1 / 3; board: the game's cells as a list (9 / 42), turn +1 / -1, step: plies played."""

  def __init__(self, kind, board, turn, step, root_logits, noise=None, discount=0.997, pb_c_base=19652, pb_c_init=1.25,
               init_value_score=0.0, frac=0.25, known_bounds=(None, None)):
    self.kind, self.A = kind, (9 if kind == 1 else 7)
    self.discount, self.pb_c_base, self.pb_c_init, self.init_value_score = discount, pb_c_base, pb_c_init, init_value_score
    self.min_max_stats = MinMaxStats(*known_bounds)
    self.root = Node(0)
    self.root.board, self.root.mover, self.root.step, self.root.slot = list(board), turn, step, 0
    self.root.expand(root_logits, turn, playout_py.legal_actions(kind, board))
    if noise is not None:
      for a, child in self.root.children.items():
        child.prior = child.prior * (1 - frac) + float(noise[a]) * frac
    self.slots = [self.root]
    self.leaf_depth = []
    self.pending = None

  def ucb_score(self, parent, child):
    pb_c = math.log((parent.visit_count + self.pb_c_base + 1) / self.pb_c_base) + self.pb_c_init
    pb_c *= math.sqrt(parent.visit_count) / (child.visit_count + 1)
    prior_score = pb_c * child.prior
    if child.visit_count > 0:
      value_score = self.min_max_stats.normalize(child.reward + self.discount * -child.value())
    else:
      value_score = self.init_value_score
    return prior_score + value_score

  def select_child(self, node):
    if node.visit_count == 0:
      _, action = max((child.prior, action) for action, child in node.children.items())
    else:
      _, action = max((self.ucb_score(node, child), action) for action, child in node.children.items())
    return action, node.children[action]

  def select(self):
    """the descent; returns the leaf's observation (integer cells in the mover's view; zeros for a finished leaf)"""
    node, path, to_play, action = self.root, [self.root], self.root.to_play, None
    while node.expanded():
      action, node = self.select_child(node)
      path.append(node)
      to_play *= -1
    self.leaf_depth.append(len(path) - 1)
    O = 9 if self.kind == 1 else 42
    if node.slot is not None:      # a finished node that has its slot (or a root without a legal action): a revisit
      self.pending = (path, to_play, None)
      return [0] * O
    parent = path[-2]
    bd = list(parent.board)
    end = playout_py.play(self.kind, bd, parent.mover, action)
    leaf = dict(board=bd, mover=-parent.mover, step=parent.step + 1, reward=1.0 if end == 1 else 0.0, finished=end != 0)
    self.pending = (path, to_play, leaf)
    return [0] * O if leaf['finished'] else [leaf['mover'] * c for c in bd]

  def expand_backup(self, value, logits):
    path, to_play, leaf = self.pending
    node = path[-1]
    if leaf is not None:
      node.board, node.mover, node.step, node.finished = leaf['board'], leaf['mover'], leaf['step'], leaf['finished']
      node.reward = leaf['reward']
      node.slot = len(self.slots)
      self.slots.append(node)
      node.to_play = to_play
      if not node.finished:
        node.expand(logits, to_play, playout_py.legal_actions(self.kind, node.board))
    self.backpropagate(path, 0.0 if node.finished else float(value), to_play)

  def backpropagate(self, search_path, value, to_play):
    for idx, node in enumerate(reversed(search_path)):
      node.value_sum += value if node.to_play == to_play else -value
      node.visit_count += 1
      reward = -node.reward if node.to_play == to_play else node.reward
      if idx < len(search_path) - 1:
        self.min_max_stats.update(node.reward - self.discount * node.value())
      value = reward + self.discount * value

  def arrays(self, sims):
    """the tree in the engine's layout: node arrays [NN] (child a of slot e = node 1 + e * A + a), EX, and the slots' side state"""
    A, S = self.A, sims + 1
    NN = 1 + S * A
    d = dict(N=np.zeros(NN, np.int32), W=np.zeros(NN), P=np.zeros(NN), R=np.zeros(NN, np.float32), E=np.full(NN, -1, np.int32),
             TP=np.zeros(NN, np.int8), EX=np.zeros(NN, np.uint8), boards=np.zeros((S, 42), np.int8), mover=np.zeros(S, np.int8),
             step=np.zeros(S, np.int32), mask=np.zeros(S, np.uint32), finished=np.zeros(S, np.uint8))

    def put(i, node):
      d['N'][i], d['W'][i], d['P'][i], d['R'][i], d['TP'][i], d['EX'][i] = (node.visit_count, node.value_sum, node.prior,
                                                                           node.reward, node.to_play, 1)
      d['E'][i] = -1 if node.slot is None else node.slot
    put(0, self.root)
    for e, node in enumerate(self.slots):
      d['boards'][e, :len(node.board)] = node.board
      d['mover'][e], d['step'][e], d['finished'][e] = node.mover, node.step, node.finished
      for a, child in node.children.items():
        d['mask'][e] |= np.uint32(1 << a)
        put(1 + e * A + a, child)
    d['nexp'] = len(self.slots)
    d['legal'] = int(d['mask'][0])
    d['minmax'] = np.array([self.min_max_stats.minimum, self.min_max_stats.maximum])
    d['leaf_depth'] = np.array(self.leaf_depth + [0] * (sims - len(self.leaf_depth)), np.int32)
    return d


def search_batch(kind, boards, turn, step, root_logits, sims, noise=None, num_simulations=None, **kw):
  """n trees in lock-step, the fake network on every leaf; returns the stacked arrays of Search.arrays"""
  A = 9 if kind == 1 else 7
  cells = 9 if kind == 1 else 42
  trees = [Search(kind, [int(c) for c in boards[i][:cells]], int(turn[i]), int(step[i]), root_logits[i],
                  None if noise is None else noise[i], **kw) for i in range(len(boards))]
  for _ in range(sims if num_simulations is None else num_simulations):
    for t in trees:
      value, logits = fake_outputs(t.select(), A)
      t.expand_backup(value, logits)
  per = [t.arrays(sims) for t in trees]
  return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


def random_positions(kind, n, seed, min_plies=0, max_plies=7, max_empty=None):
  """n random unfinished positions with a legal action: boards [n, 42] int8, turn [n] int8, step [n] int32.  Random legal
  moves from the empty board, restarted when the game ends; max_empty: keep only positions with at most that many empty cells."""
  rng = np.random.RandomState(seed)
  cells = 9 if kind == 1 else 42
  boards, turns, steps = [], [], []
  while len(boards) < n:
    plies = int(rng.randint(min_plies, max_plies + 1))
    bd, mover, ok = [0] * cells, 1, True
    for _ in range(plies):
      acts = playout_py.legal_actions(kind, bd)
      if playout_py.play(kind, bd, mover, acts[rng.randint(len(acts))]):
        ok = False
        break
      mover = -mover
    if not ok or (max_empty is not None and bd.count(0) > max_empty):
      continue
    boards.append(bd + [0] * (42 - cells)); turns.append(mover); steps.append(plies)
  return np.array(boards, np.int8), np.array(turns, np.int8), np.array(steps, np.int32)


SIMS = 30


def case_positions(kind):
  """the positions the CPU and the GPU tests share: TicTacToe, 256 random positions 0 - 7 plies deep; Connect Four, 128 random
  positions with at most 10 empty cells plus the six boards of tests/c4_positions.py (one legal column each).  Returns
  boards [n, 42], turn [n], step [n], the fake network's root logits [n, A] and a Dirichlet draw [n, A] (zero where illegal)."""
  if kind == 1:
    bd, tn, st = random_positions(1, 256, 11, 0, 7)
  else:
    from tests.c4_positions import POSITIONS
    bd, tn, st = random_positions(3, 128, 12, 30, 41, max_empty=10)
    forced = np.array([b for _, _, _, b in POSITIONS], np.int8)
    bd = np.concatenate([bd, forced])
    tn = np.concatenate([tn, np.array([t for _, t, _, _ in POSITIONS], np.int8)])
    st = np.concatenate([st, (forced != 0).sum(1).astype(np.int32)])
  A, O = (9, 9) if kind == 1 else (7, 42)
  _, logits = fake_network(bd[:, :O].astype(np.int64) * tn[:, None].astype(np.int64), A)
  rng = np.random.RandomState(100 + kind)
  noise = np.zeros((len(bd), A))
  for i in range(len(bd)):
    la = playout_py.legal_actions(kind, bd[i].tolist())
    noise[i, la] = rng.dirichlet([0.25] * len(la))
  return bd, tn, st, logits, noise


TREE_FIELDS = ('N', 'W', 'P', 'R', 'E', 'TP')
SLOT_FIELDS = ('boards', 'mover', 'step', 'mask', 'finished')
