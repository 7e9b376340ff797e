"""Where the weight loads of the MFMA streams are issued and waited for (csrc/mz_fused.hip.h: the streamed fc1 steps issue
their four prefetch loads one behind each group of four MFMAs, behind ONE counted wait for their own pieces) changes no
arithmetic -- but a wrong wait count or ring position reads a register buffer before its load has landed, and shows as wrong
numbers only at some sizes.  Three checks at the small sizes where that shows first:

  root kernel (k_root, the body every whole-moves launch starts its moves with) against the float64 restatement tests/fc64.py,
      33 rows (two full workgroups + one with a single live row), first-stage step counts 1, 2, 3, 17, 32 (exactly one LDS
      chunk) and 33 (a second chunk of one step), every policy width class;
  whole-moves launch against root kernel + search kernel per move: records byte for byte, 33 environments, two launches of 3
      moves (the resident steps are reloaded and the ring restarted at every move), 1 / 2 / 5 simulations -- a wrong ring
      position at the entry or exit of the simulation loop shows at 1 and 2 first;
  one search through the fused kernel against the oracle's tree (the margin rule of tests/test_gpu_search.py), 33 trees x 5
      simulations, for the three tree placements.
Tolerances: those of tests/test_gpu_net.py for k_root (tests/test_oracle_net.py: 1e-5 on hidden state and logits; value:
every row within one step of the float32 staircase, 1.5e-4 (1 + |v|), and within 1e-5 on >= 97 % of the rows).  The second
half of the value rule is a statement about two FLOAT32 evaluations of Config.inverse_transform, which land on the same step of
its sqrt(...) - 1 cancellation in all but a few rows; a float64 evaluation has no staircase, so a correct float32 value lies up
to one step from it in most rows (measured: 28 of 33 rows beyond 1e-5 at O = 1, A = 2).  So the
value is held to the one-step bound against float64 and to the whole rule against the oracle's float32 network, as in
tests/test_gpu_net.py."""
import numpy as np
import pytest

from tests.fc64 import FC64
from tests.parity_util import env_switches, random_weights
from tests.test_oracle_net import TOL, scalar_close

pytestmark = pytest.mark.gpu
ROWS = 33


@pytest.mark.parametrize('A', [2, 4, 9, 18])
@pytest.mark.parametrize('O', [1, 8, 16, 128, 255, 257])
def test_root_vs_float64(O, A):
  from oracle import oracle as orc
  from model_based_rl_amd.engine import Engine
  from tests.test_gpu_net import _random_weights
  w = _random_weights(O, A, 11)
  obs = np.random.RandomState(5).standard_normal((ROWS, O)).astype(np.float32)
  eng = Engine(ROWS, O, A, 4)
  eng.set_weights(w)
  eng.initial_inference(obs)
  v, lg, h = [x.cpu().numpy() for x in eng.root_outputs()]
  eng.close()
  ho, vo, lgo = FC64(w, O, A).initial(obs)
  dh, dl, dv = np.abs(h - ho).max(), np.abs(lg - lgo).max(), np.abs(v - vo)
  print('O %d A %d: hidden %.2e logits %.2e value %.2e (%d rows beyond 1e-5)' % (O, A, dh, dl, dv.max(), (dv > TOL).sum()))
  assert h.shape == (ROWS, 50) and lg.shape == (ROWS, A)
  assert dh <= TOL and dl <= TOL, (dh, dl)
  assert np.all(dv <= 1.5e-4 * (1 + np.abs(vo))), dv.max()
  scalar_close(v, orc.FCNet(w, O, A).initial(obs)[1])


ENVS = {
    # name: (O, A, engine keywords, device environment, episode length, uint8 observations)
    'synthetic_A4': (8, 4, {}, None, 7, False),
    'synthetic_A6': (128, 6, {}, None, 7, True),          # the Pong-ram shapes: 17 first-stage steps in the launch's root
    'synthetic_A18': (8, 18, {}, None, 7, False),         # two policy tiles, 32 lanes per tree
    'tictactoe': (9, 9, dict(two_players=True, known_bounds=(-1.0, 1.0), discount=1.0), 'tictactoe', 9, False),
    'cartpole': (4, 2, {}, 'cartpole', 500, False),
}


def _records(name, sims, no_persist):
  import torch
  from model_based_rl_amd.engine import Engine
  O, A, kw, env, ep_len, u8 = ENVS[name]
  with env_switches(MZ_NO_PERSIST='1' if no_persist else None):
    eng = Engine(ROWS, O, A, sims, seed=77, **kw)
  if env:
    eng.selfplay_set_env(env)
  eng.set_weights(random_weights(O, A, 1))
  if u8:
    eng.selfplay_set_obs(uint8_obs=True, obs_min=[0.0], obs_range=[255.0])
  mpl = eng.selfplay_moves_per_launch()
  eng.selfplay_reset(ep_len, 1.0)
  recs = []
  for _ in range(2):
    eng.selfplay_steps(3)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == 3
    recs.append(buf[:n].numpy().copy())
  eng.close()
  return np.concatenate(recs, 0), mpl


# (the device TicTacToe plays whole moves on its compact-placement kernel only: 30 simulations select it, at 1 / 2 / 5 the
# trees fit LDS whole and both engines below play the launch-per-step form)
@pytest.mark.parametrize('name,sims', [(n, s) for n in sorted(ENVS) for s in (1, 2, 5)] + [('tictactoe', 30)])
def test_whole_moves_launch_vs_two_kernels_per_move(name, sims):
  whole, mpl = _records(name, sims, False)
  split, mpl0 = _records(name, sims, True)
  assert mpl0 == 0, mpl0
  # (TicTacToe at 1 / 2 / 5 simulations: no whole-moves kernel is selected, the two engines run the same launches)
  assert mpl == (0 if name == 'tictactoe' and sims != 30 else 16), mpl
  assert whole.shape == split.shape and whole.shape[:2] == (6, ROWS)
  assert np.array_equal(whole.view(np.int32), split.view(np.int32)), np.flatnonzero(np.any(whole.view(np.int32) != split.view(np.int32), axis=(1, 2)))


PLACEMENTS = {
    # LT: (switches at mz_create, A, the engine's simulation count -- the placement follows the tree size at that count)
    0: ({'MZ_NO_LDS_TREES': '1'}, 4, 30),
    1: ({}, 4, 30),
    2: ({}, 6, 50),
}


@pytest.mark.parametrize('lt', [0, 1, 2])
def test_fused_search_vs_oracle_tree(lt):
  from oracle import oracle as orc
  from model_based_rl_amd.engine import Engine
  from tests.test_gpu_search import check_against_oracle, random_weights as search_weights
  sw, A, cfg_sims = PLACEMENTS[lt]
  O, sims = 8, 5
  w = search_weights(O, A, 11)
  rng = np.random.RandomState(0)
  obs = rng.standard_normal((ROWS, O)).astype(np.float32)
  noise = rng.dirichlet([0.25] * A, size=ROWS)
  tp = np.ones(ROWS, np.int8)
  with env_switches(**sw):
    eng = Engine(ROWS, O, A, cfg_sims)
  eng.set_weights(w)
  info = eng.search_kernel_info()
  assert info['kind'] == 'fused' and info['lt'] == lt, info
  eng.initial_inference(obs)
  eng.root_prepare(tp, None, noise)
  eng.search(sims)
  u = rng.uniform(size=ROWS)
  out = {k: v.cpu().numpy() for k, v in eng.finalize(np.ones(ROWS), u).items()}
  ex = eng.export_tree(hidden=True)
  eng.close()
  t = orc.Trees(orc.tree_cfg(A, sims), ROWS)
  hpool, v0 = t.search_fc(orc.FCNet(w, O, A), obs, tp, None, noise, 0.25)
  action, cv, rv, vc = t.finalize(np.ones(ROWS), u)
  ref = dict(action=action, child_visits=cv, root_value=rv, visit_counts=vc, hpool=hpool, v0=v0, tree=t.export(), margin=t.margin())
  # the engine's trees have room for cfg_sims simulations: the nodes and hidden-state slots 5 simulations can reach come first
  NN = 1 + (sims + 1) * A
  for k in ('N', 'E', 'TP'):
    ex[k] = ex[k][:, :NN]
  ex['hidden'] = ex['hidden'][:, :ref['hpool'].shape[1]]
  check_against_oracle(out, ex, ref, 'LT %d, %d trees x %d simulations' % (lt, ROWS, sims))
