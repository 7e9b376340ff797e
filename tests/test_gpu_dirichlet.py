"""Every device path that draws the root's Dirichlet noise, and the Gumbel root's G, against the float64 restatement of
tests/dirichlet_py.py (shown to be Dirichlet by tests/test_dirichlet_cpu.py).

The comparison rule, the same everywhere.  The device evaluates Marsaglia-Tsang in float32 on the hardware's log2 / exp2 / cos /
sqrt, so an iteration may be accepted there and rejected in float64 when its decision is within float32 rounding of a tie.  The
restatement returns that distance per row (the decision margin):
  rows with a margin >= 1e-4   every entry of the device's noise within 1.6e-5 absolute of the restatement -- 16 x the 1.0e-6 a
                               numpy float32 evaluation of the same formulas (exact libm) deviates by on such rows; a wrong key
                               word, mask, counter or lane moves entries by about 1e-1
  the other rows               left out of the value comparison only; at most 1 % of a case's rows
  every row                    sums to 1 within 1e-12, no negative entry, no NaN, exactly 0 at the illegal actions
Paths: (a) k_dirichlet through Engine.root_prepare(device_rng=True); (b) the fused root of the synthetic environment, one case
per lane-group shape, across the move counter's high word, in the launch-per-step form; (c) the masked branches of the game
kernels (TicTacToe, Connect Four) and CartPole, whole moves and launch-per-step; (d) the Gumbel root's G within 1e-12.

Measured on an MI355X over all cases: worst deviation 1.78e-6 (alpha 0.03, A 7, k_dirichlet; at alpha >= 0.25 at most 3.5e-7),
most rows left out 0.77 % (A 32), Gumbel 4.4e-16 (DESIGN s5).  Before mz_gamma carried the boost's exponent past float32, 34 of the
4096 two-action rows of one move at alpha 0.03 came out (0.5, 0.5)."""
import numpy as np
import pytest

from tests import dirichlet_py as dp
from tests.parity_util import random_weights

pytestmark = pytest.mark.gpu

TOL, MARGIN, CAP = 1.6e-5, 1e-4, 0.01
SEED = (0x0BADC0DE << 32) | 0x5EEDF00D      # both key words in use
MOVES = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 55 + 3]


class Tally(object):
  """the rows of one case: every row's invariants at once, the value comparison on the rows above the margin, the cap at the end"""

  def __init__(self, name):
    self.name, self.rows, self.left_out, self.worst = name, 0, 0, 0.0

  def add(self, dev, alpha, env0, move, legal=None):
    B, A = dev.shape
    ok = np.ones((B, A), bool) if legal is None else np.asarray(legal).reshape(B, A) != 0
    ref, margin = dp.dirichlet(alpha, SEED, env0, B, A, move, ok)
    at = (self.name, 'move', move)
    assert not np.isnan(dev).any(), at
    assert dev.min() >= 0.0 and np.all(dev[~ok] == 0.0), at
    assert np.abs(dev.sum(1) - 1.0).max() <= 1e-12, (at, float(np.abs(dev.sum(1) - 1.0).max()))
    wide = margin >= MARGIN
    err = np.abs(dev - ref).max(1)
    self.rows += B
    self.left_out += int((~wide).sum())
    if wide.any():
      self.worst = max(self.worst, float(err[wide].max()))
    bad = np.flatnonzero(wide & (err > TOL))
    assert bad.size == 0, (at, '%d of %d rows off' % (bad.size, B), 'first: row', int(bad[0]), dev[bad[0]].tolist(), ref[bad[0]].tolist(),
                           'legal', int(ok[bad[0]].sum()))

  def close(self):
    print('%s: %d rows, %d below the margin (%.2f %%), worst deviation %.3g' % (self.name, self.rows, self.left_out,
                                                                                100.0 * self.left_out / self.rows, self.worst))
    assert self.left_out <= CAP * self.rows, (self.name, self.left_out, self.rows)


def masks(B, A, seed):
  """density 0.6, at least one legal action per row; rows 0, 16, .. exactly one legal action, rows 1, 17, .. exactly two"""
  rng = np.random.RandomState(seed)
  m = rng.uniform(size=(B, A)) < 0.6
  for b in range(B):
    k = 1 if b % 16 == 0 else 2 if b % 16 == 1 else 0
    if k or not m[b].any():
      m[b] = False
      m[b, rng.permutation(A)[:max(k, 1)]] = True
  return m.astype(np.uint8)


# ---- (a) k_dirichlet through root_prepare
PREPARE = [(A, alpha, (4096, 130)[(i + j) % 2], (0, 1000)[(i + j // 2) % 2])
           for i, A in enumerate([2, 4, 7, 9, 18, 32]) for j, alpha in enumerate([0.03, 0.25, 1.0, 1.5])]


def prepare_plan(A, alpha, B, env0):
  """the draws of one case as (move, legal or None): every move unmasked and masked"""
  return [(m, lg) for k, m in enumerate(MOVES) for lg in (None, masks(B, A, 1000 * A + k))]


@pytest.mark.parametrize('A,alpha,B,env0', PREPARE, ids=['A%d-alpha%g-B%d-env%d' % c for c in PREPARE])
def test_root_prepare_draw(A, alpha, B, env0):
  """alpha = 0.03 with two legal actions (A = 2 unmasked; the two-legal rows of every mask) is where a float32 boost U^(1/alpha)
  underflows in every legal action of a row, and the row came out uniform instead of nearly one-hot"""
  from model_based_rl_amd.engine import Engine, H
  eng = Engine(B, 4, A, 2, seed=SEED, env_id_offset=env0, root_dirichlet_alpha=alpha)
  eng.root_load(np.zeros(B, np.float32), np.zeros((B, A), np.float32), np.zeros((B, H), np.float32))
  t = Tally('root_prepare A %d alpha %g B %d env0 %d' % (A, alpha, B, env0))
  for move, legal in prepare_plan(A, alpha, B, env0):
    eng.root_prepare(None, legal, None, device_rng=True, move=move)
    t.add(eng.export_tree()['noise'], alpha, env0, move, legal)
  eng.close()
  t.close()


# ---- (b) the fused root on the synthetic environment: (A, lanes per group, alpha, first move, launch-per-step)
FUSED = [(4, 4, 0.25, 0, False), (6, 8, 0.03, 0, False), (10, 16, 1.0, 0, False), (16, 16, 1.5, 0, False), (18, 32, 0.25, 0, False),
         (32, 32, 0.03, 0, False), (6, 8, 0.25, 2 ** 32 - 3, False), (4, 4, 0.03, 0, True)]
FUSED_B, FUSED_ENV0, FUSED_STEPS = 130, 1000, 6


@pytest.mark.parametrize('A,G,alpha,base,no_persist', FUSED,
                         ids=['A%d-G%d-alpha%g-from%d%s' % (c[:4] + ('-launch_per_step' if c[4] else '',)) for c in FUSED])
def test_fused_root_draw(A, G, alpha, base, no_persist, monkeypatch):
  import torch
  from model_based_rl_amd.engine import Engine
  if no_persist:
    monkeypatch.setenv('MZ_NO_PERSIST', '1')
  B, env0 = FUSED_B, FUSED_ENV0
  eng = Engine(B, 8, A, 4, seed=SEED, env_id_offset=env0, root_dirichlet_alpha=alpha)
  eng.set_weights(random_weights(8, A, 3))
  assert eng.search_kernel_info()['G'] == G and eng.selfplay_moves_per_launch() == (0 if no_persist else 16)
  eng.selfplay_noise_log(True)
  eng.selfplay_export_trees(True)
  eng.selfplay_reset(5, 1.0)
  if base:
    eng.selfplay_set_moves(base)
  eng.selfplay_steps(FUSED_STEPS)
  _, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == FUSED_STEPS
  t = Tally('fused root A %d G %d alpha %g from move %d%s' % (A, G, alpha, base, ' launch-per-step' if no_persist else ''))
  last = base + FUSED_STEPS - 1
  for m in range(base, last + 1):
    if m >> 32 == 0:      # (the log is read by the low word of the counter; past it the last move's draw, from the tree)
      t.add(eng.selfplay_noise(m), alpha, env0, m)
  if last >> 32:
    t.add(eng.export_tree()['noise'], alpha, env0, last)
  else:
    assert np.array_equal(eng.export_tree()['noise'], eng.selfplay_noise(last))
  eng.close()
  t.close()


# ---- (c) the game kernels
GAME_B, GAME_ENV0, GAME_MOVES = 130, 1000, 16
GAMES = {'tictactoe': dict(O=9, A=9, sims=30, T=9, two=True), 'connect_four': dict(O=42, A=7, sims=8, T=42, two=True),
         'cartpole': dict(O=4, A=2, sims=8, T=12, two=False)}


def c4_board(cols):
  """a position whose columns `cols` (no two adjacent) are full, the colours alternating from the bottom: no line of four"""
  bd = np.zeros(42, np.int8)
  for c in cols:
    bd[7 * np.arange(6) + c] = [1, -1, 1, -1, 1, -1]
  return bd


C4_PLACED = {1: (0, 3, 6), 2: (1, 5), 3: (2, 4)}      # environment index mod 4 -> its full columns at move 0


def game_engine(kind, alpha):
  from model_based_rl_amd.engine import Engine
  g = GAMES[kind]
  kw = dict(two_players=True, known_bounds=(-1.0, 1.0), discount=1.0) if g['two'] else {}
  eng = Engine(GAME_B, g['O'], g['A'], g['sims'], seed=SEED, env_id_offset=GAME_ENV0, root_dirichlet_alpha=alpha, **kw)
  eng.selfplay_set_env(kind)
  eng.set_weights(random_weights(g['O'], g['A'], 2))
  eng.selfplay_noise_log(True)
  eng.selfplay_export_trees(True)
  eng.selfplay_reset(g['T'], 1.0)
  if kind == 'connect_four':
    for b in range(GAME_B):
      if b % 4 in C4_PLACED:      # (an even number of stones, as many of each colour: player 1 is to move)
        eng.selfplay_set_board_state(b, c4_board(C4_PLACED[b % 4]), 1)
  return eng


def game_legal(kind, rec):
  """the legal mask of the records' pre-step observations [B, O]"""
  if kind == 'tictactoe':
    return (rec[:, :9] == 0).astype(np.uint8)      # the empty cells
  if kind == 'connect_four':
    return (rec[:, 35:42] == 0).astype(np.uint8)      # the columns whose top cell is empty
  return None


@pytest.mark.parametrize('kind,alpha', [('tictactoe', 0.03), ('tictactoe', 1.0), ('connect_four', 0.25), ('connect_four', 1.5),
                                        ('cartpole', 0.03), ('cartpole', 0.25)])
def test_game_kernels_draw(kind, alpha):
  """16 whole moves in one launch: the draw of every move from the noise log, the masks from the records"""
  import torch
  eng = game_engine(kind, alpha)
  assert eng.selfplay_moves_per_launch() == 16
  eng.selfplay_steps(GAME_MOVES)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == GAME_MOVES
  rec = buf[:n].numpy().copy()
  t = Tally('%s alpha %g whole moves' % (kind, alpha))
  few = 0
  for m in range(GAME_MOVES):
    legal = game_legal(kind, rec[m])
    if m == 0 and kind == 'connect_four':
      assert sorted(set(legal.sum(1).tolist())) == [4, 5, 7]      # masks with holes from the first move on
    if legal is not None:
      few += int((legal.sum(1) <= 2).sum())
    t.add(eng.selfplay_noise(m), alpha, GAME_ENV0, m, legal)
  assert np.array_equal(eng.export_tree()['noise'], eng.selfplay_noise(GAME_MOVES - 1))
  eng.close()
  t.close()
  if kind == 'tictactoe':
    assert few > 0      # (positions with one or two empty cells were among them)


@pytest.mark.parametrize('kind,alpha', [('tictactoe', 0.03), ('connect_four', 0.25)])
def test_game_launch_per_step_draw(kind, alpha, monkeypatch):
  """the launch-per-step form (k_dirichlet on the environment's own mask and move counter): 16 moves one launch each, the draw
  of each read from the exported tree"""
  import torch
  monkeypatch.setenv('MZ_NO_PERSIST', '1')
  eng = game_engine(kind, alpha)
  assert eng.selfplay_moves_per_launch() == 0
  t = Tally('%s alpha %g launch-per-step' % (kind, alpha))
  for m in range(GAME_MOVES):
    eng.selfplay_steps(1)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == 1
    t.add(eng.export_tree()['noise'], alpha, GAME_ENV0, m, game_legal(kind, buf[0].numpy()))
  eng.close()
  t.close()


# ---- (d) the Gumbel root
@pytest.mark.parametrize('A', [7, 9])
def test_gumbel_root_draw(A):
  """G = -ln(-ln u) in float64 on the device: two logarithms of <= 1 ulp each are about 4e-14 at |G| <= 40; the bound leaves 25 x"""
  from model_based_rl_amd.engine import Engine, H
  B, env0 = 130, 100
  eng = Engine(B, 4, A, 2, seed=SEED, env_id_offset=env0)
  eng.root_load(np.zeros(B, np.float32), np.zeros((B, A), np.float32), np.zeros((B, H), np.float32))
  env, act = np.meshgrid(env0 + np.arange(B), np.arange(A), indexing='ij')
  for scale in (1.0, 0.0):
    eng.set_gumbel(True, gumbel_scale=scale)
    for move in (7, 2 ** 32 + 7):
      eng.root_prepare(None, masks(B, A, A))
      eng.gz_root(None, move=move)
      G = eng.gz_export()['G']
      if scale:
        ref = dp.gumbel(SEED, env, move, act)
        print('Gumbel A %d move %d: worst deviation %.3g' % (A, move, np.abs(G - ref).max()))
        assert np.abs(G - ref).max() <= 1e-12, (A, move)
      else:
        assert np.all(G == 0.0)
  eng.close()
