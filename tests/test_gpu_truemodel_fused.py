"""All simulations of a true-rules search in one launch (mz_tm_search_fused, k_tm_search; csrc/mz_truemodel.hip.h; DESIGN s7k)
against the two-launch loop of mz_tm_search: two engines with the same weights and the same roots, one searched by either, are
EQUAL -- every array of export_tree, every array of tm_export, and, where a descent is pending after the call, the leaves'
observations and their finished flags.  B = 40 roots (Bp = 48: three workgroups, the last with eight real rows) unless said
otherwise; TicTacToe at 12 simulations over roots with at most three empty cells among them (finished leaves and revisits are
certain), Connect Four at 30 over the empty board, the placed positions of tests/c4_positions.py and boards with full columns."""
import functools

import numpy as np
import pytest

from tests import truemodel_py as tp
from tests.eval_device_util import weights

pytestmark = pytest.mark.gpu
B = 40


@functools.lru_cache(maxsize=None)
def roots(kind, n=B):
  """boards [n, 42] int8, turn [n] int8, step [n] int32, legal [n, A] uint8, a Dirichlet draw [n, A] (zero where illegal)"""
  A = 9 if kind == 1 else 7
  late = 2 * n // 5      # (16 of 40) roots late in the game: at most three empty cells / boards with full columns
  if kind == 1:
    parts = [tp.random_positions(1, n - late, 21, 0, 7), tp.random_positions(1, late, 22, 6, 8, max_empty=3)]
  else:
    from tests.c4_positions import POSITIONS
    forced = np.array([b for _, _, _, b in POSITIONS], np.int8)
    placed = (forced, np.array([t for _, t, _, _ in POSITIONS], np.int8), (forced != 0).sum(1).astype(np.int32))
    empty = (np.zeros((2, 42), np.int8), np.ones(2, np.int8), np.zeros(2, np.int32))
    parts = [empty, placed, tp.random_positions(3, late, 23, 30, 41, max_empty=10), tp.random_positions(3, n - 8 - late, 24, 0, 24)]
  bd, tn, st = [np.concatenate([p[i] for p in parts])[:n] for i in range(3)]
  assert len(bd) == n
  masks = [tp.playout_py.legal_actions(kind, b.tolist()) for b in bd]
  legal = np.zeros((n, A), np.uint8)
  rng = np.random.RandomState(300 + kind)
  noise = np.zeros((n, A))
  for i, la in enumerate(masks):
    legal[i, la] = 1
    noise[i, la] = rng.dirichlet([0.25] * len(la))
  if kind == 1:
    assert ((bd[:, :9] == 0).sum(1) <= 3).sum() >= late
  else:
    assert (legal.sum(1) < 7).sum() >= late and (legal.sum(1) == 1).sum() >= 6 and not bd[0].any()
  return bd, tn, st, legal, noise


def searched(kind, n, pool, chunks, fused):
  """an engine whose trees hold `pool` simulations, rooted at roots(kind, n), searched in calls of `chunks` simulations by
  tm_search_fused or tm_search -> (every exported array, [(obs, finished) after every call that leaves a descent pending])"""
  from model_based_rl_amd.engine import Engine
  A, O = (9, 9) if kind == 1 else (7, 42)
  bd, tn, st, legal, noise = roots(kind, n)
  eng = Engine(n, O, A, pool, two_players=True)
  eng.set_true_model(kind)
  eng.set_weights(weights(O, A, 5))
  eng.initial_inference((bd[:, :O].astype(np.int32) * tn[:, None]).astype(np.float32))
  eng.root_prepare(tn, legal, noise)
  eng.tm_root(bd, tn, st)
  leaves, done = [], 0
  for c in chunks:
    (eng.tm_search_fused if fused else eng.tm_search)(c)
    done += c
    if done < pool:
      obs, fin = eng.tm_select()      # (a descent is pending: this copies tm.obs and leaf_fin out, nothing is launched)
      leaves.append((obs.cpu().numpy(), fin.cpu().numpy()))
  d = {'tree.' + k: v for k, v in eng.export_tree().items()}
  d.update({'tm.' + k: v for k, v in eng.tm_export().items()})
  d['root_value'], d['root_logits'] = [x.cpu().numpy() for x in eng.root_outputs()[:2]]
  eng.close()
  return d, leaves


def assert_equal(got, want):
  (gd, gl), (wd, wl) = got, want
  assert sorted(gd) == sorted(wd)
  for k in wd:
    assert np.array_equal(gd[k], wd[k]), (k, np.argwhere(np.asarray(gd[k]) != np.asarray(wd[k]))[:4].tolist())
  assert len(gl) == len(wl)
  for (go, gf), (wo, wf) in zip(gl, wl):
    assert np.array_equal(go, wo) and np.array_equal(gf, wf)


@pytest.mark.parametrize('kind,sims', [(1, 12), (3, 30)], ids=['tictactoe12', 'connect_four30'])
def test_fused_equals_the_two_launch_loop(kind, sims):
  """the pool used up by the call (its last simulation makes no descent), and a pool of four more (a descent is pending
  afterwards: the leaves' observations and flags are compared too)"""
  for pool in (sims, sims + 4):
    loop = searched(kind, B, pool, [sims], False)
    fused = searched(kind, B, pool, [sims], True)
    assert_equal(fused, loop)
    d, leaves = loop
    assert (d['tree.N'][:, 0] == sims).all() and len(leaves) == (pool > sims)
    if kind == 1 and pool == sims:      # the case exercises what it is for: finished leaves, and visits that expanded nothing
      fin = d['tm.finished'].astype(bool) & (np.arange(sims + 1)[None, :] < d['tm.nexp'][:, None])
      assert fin.any(1).sum() >= 16 and (d['tm.nexp'] < sims + 1).sum() >= 16


def test_split_call_equals_one_call():
  """5 then 7 simulations (sims_done > 0 at entry, a descent pending between them) against 12 at once, and against the loop"""
  whole = searched(1, B, 12, [12], True)
  split = searched(1, B, 12, [5, 7], True)
  loop = searched(1, B, 12, [5, 7], False)
  assert_equal(split, loop)
  assert len(split[1]) == 1
  assert_equal((split[0], []), (whole[0], []))


@pytest.mark.parametrize('kind,sims', [(1, 12), (3, 30)], ids=['tictactoe12', 'connect_four30'])
def test_aligned_batch(kind, sims):
  """B = 16: one workgroup, no padded row"""
  assert_equal(searched(kind, 16, sims, [sims], True), searched(kind, 16, sims, [sims], False))


def test_refusals():
  from model_based_rl_amd.engine import Engine
  bd, tn, st, legal, noise = roots(1)
  eng = Engine(B, 9, 9, 12, two_players=True)
  with pytest.raises(RuntimeError, match=r'mz_tm_search_fused: weights not set \(call mz_set_weights\)'):
    eng.tm_search_fused(1)
  eng.set_weights(weights(9, 9, 5))
  with pytest.raises(RuntimeError, match='mz_tm_search_fused: call mz_tm_root first'):      # (no true-rules search is set)
    eng.tm_search_fused(1)
  eng.set_true_model(1)
  eng.initial_inference((bd[:, :9].astype(np.int32) * tn[:, None]).astype(np.float32))
  eng.root_prepare(tn, legal, noise)
  with pytest.raises(RuntimeError, match='mz_tm_search_fused: call mz_tm_root first'):
    eng.tm_search_fused(1)
  eng.tm_root(bd, tn, st)
  for n in (0, 13):
    with pytest.raises(RuntimeError, match=r'mz_tm_search_fused: 0 \+ %d simulations exceed the pool sized for num_simulations = 12' % n):
      eng.tm_search_fused(n)
  eng.tm_search_fused(5)
  with pytest.raises(RuntimeError, match=r'mz_tm_search_fused: 5 \+ 8 simulations exceed the pool sized for num_simulations = 12'):
    eng.tm_search_fused(8)
  eng.tm_search_fused(7)
  with pytest.raises(RuntimeError, match=r'mz_tm_search_fused: 12 \+ 1 simulations exceed the pool sized for num_simulations = 12'):
    eng.tm_search_fused(1)
  eng.close()
