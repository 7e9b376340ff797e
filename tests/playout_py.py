"""The playout-search opponent (DESIGN s7d) restated in pure Python from the definition alone: its own Philox4x32-10, its own
rules on lists, math.log for the table of logarithms.  Nothing of the native code is imported; tests/test_playout_cpu.py
holds the host hook (mz_playout_plan_host) to it exactly, and tests/test_gpu_playout.py holds the device to the hook."""
import math

RNG_PLAYOUT = 9
M32 = 0xFFFFFFFF


def philox(seed, c0, c1, c2, c3):
  """Philox4x32-10 keyed by the 64-bit seed; returns the four output words"""
  k0, k1 = seed & M32, (seed >> 32) & M32
  for _ in range(10):
    p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
    c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
    k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
  return c0, c1, c2, c3


# ---- the rules, on lists.  TicTacToe: 9 cells, 3 * row + col.  Connect Four: 42 cells, 7 * row + col, row 0 at the bottom.
TTT_LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]


def legal_actions(kind, board):
  if kind == 1:
    return [a for a in range(9) if board[a] == 0]
  return [c for c in range(7) if board[35 + c] == 0]


def play(kind, board, mover, action):
  """the mover's stone goes on the board (in place); returns 1 the mover wins, 2 the game ends drawn, 0 it goes on"""
  if kind == 1:
    board[action] = mover
    if any(action in line and all(board[k] == mover for k in line) for line in TTT_LINES):
      return 1
    return 2 if all(c != 0 for c in board[:9]) else 0      # the ninth move ends the game
  row = next(r for r in range(6) if board[7 * r + action] == 0)
  board[7 * row + action] = mover
  for dr, dc in ((1, 0), (0, 1), (1, 1), (1, -1)):
    n = 1
    for sg in (1, -1):
      r, c = row + sg * dr, action + sg * dc
      while 0 <= r < 6 and 0 <= c < 7 and board[7 * r + c] == mover:
        n, r, c = n + 1, r + sg * dr, c + sg * dc
    if n >= 4:
      return 1
  return 2 if all(board[35 + c] != 0 for c in range(7)) else 0      # a full top row ends it


def playout(kind, board, mover, first, seed, env, move, iteration, lane):
  """lane `lane` of a fresh node: `first` by the node's mover, then uniformly random legal moves.  Returns (result 2 / 1 / 0
  for the node's mover: win / draw / loss, end flag of `first` itself)"""
  bd = list(board)
  end = play(kind, bd, mover, first)
  if end:
    return (2 if end == 1 else 1), end
  turn, p, r = mover, 0, None
  while True:
    turn = -turn
    if p % 16 == 0:
      r = philox(seed, env, move, iteration, (RNG_PLAYOUT << 24) | (lane << 4) | (p // 16))
    byte = (r[(p % 16) // 4] >> (8 * (p % 4))) & 255
    acts = legal_actions(kind, bd)
    e = play(kind, bd, turn, acts[(byte * len(acts)) >> 8])
    p += 1
    if e == 1:
      return (2 if turn == mover else 0), 0
    if e == 2:
      return 1, 0


class Node(object):
  def __init__(self, A):
    self.n, self.w, self.kid, self.end = [0] * A, [0] * A, [-1] * A, [0] * A


def plan(kind, board, turn, playouts, seed, env, move):
  """one move: (action, visits[A], wins[A]) of the root after playouts / 64 iterations"""
  A = 9 if kind == 1 else 7
  assert playouts % 64 == 0 and 64 <= playouts <= 65536
  iters = playouts // 64
  LN = [0.0] + [math.log(64.0 * v) for v in range(1, iters + 1)]
  nodes = [Node(A)]

  def evaluate(node, bd, mover, it):
    L = legal_actions(kind, bd)
    total = 0
    for lane in range(64):
      a = L[lane % len(L)]
      res, end = playout(kind, bd, mover, a, seed, env, move, it, lane)
      node.n[a] += 1
      node.w[a] += res
      if end:
        node.end[a] = end
      total += res
    return total

  for it in range(iters):
    bd, mover, node, path = list(board), turn, nodes[0], []
    if it == 0:
      evaluate(node, bd, mover, it)
      continue
    while True:
      V = sum(node.n) // 64
      best, best_score = None, None
      for a in legal_actions(kind, bd):
        score = float(node.w[a]) / (2.0 * float(node.n[a])) + math.sqrt(2.0 * LN[V] / float(node.n[a]))
        if best is None or score > best_score:
          best, best_score = a, score
      a = best
      path.append((node, a))
      if node.end[a]:
        v = 128 if node.end[a] == 1 else 64
        break
      play(kind, bd, mover, a)
      mover = -mover
      if node.kid[a] < 0:
        node.kid[a] = len(nodes)
        nodes.append(Node(A))
        v = 128 - evaluate(nodes[-1], bd, mover, it)
        break
      node = nodes[node.kid[a]]
    for nd, a in reversed(path):
      nd.n[a] += 64
      nd.w[a] += v
      v = 128 - v
  root = nodes[0]
  action = max(range(A), key=lambda a: (root.n[a], root.w[a], -a))
  return action, list(root.n), list(root.w)
