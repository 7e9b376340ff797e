"""The action table of the A <= 4 row of k_search_fused (csrc/mz_fused.hip.h, mz_fused_atab): the one-hot columns and the
bias of the dynamics fc1 are no longer multiplied -- W[:, 50 + a] + b is read per tree into the accumulator tiles before the
first of 13 k-steps.  What can go wrong: a table entry packed from the wrong feature or action, a lane reading another
column's action, a counted LDS wait that lets an MFMA start before its tile has arrived, a ring position that is off by the
step that went away, and the table's place in the dynamic LDS (in front of the pb_c table and the trees).

33 trees everywhere: two full workgroups and one with a single live row, so workgroups see mixed actions, all-equal
actions (a legal mask of one action at the root) and dead columns.

  network outputs of every simulation against the float64 network of tests/fc64.py (the sim_io log and the exported tree,
      as tests/test_gpu_supports.py does it, with its bounds): A = 2, 3, 4 at 1, 2 and 5 simulations -- a wrong ring position
      after the shortened fc1 shows at 1 and 2 first;
  bit equality inside the row: whole-moves launch vs launch per move (A = 4 and the CartPole game kernel, two launches of 3
      moves, records byte for byte), whole trees in LDS vs trees in the pool, and the compact placement -- whose table reads
      come from global memory -- vs trees in the pool at the same simulation count (exported trees, hidden states and the
      sim_io log byte for byte);
  placement: with the table counted, A = 4 at 30 simulations and CartPole at 62 still keep whole trees in LDS and play 16
      moves per launch; A = 4 holds whole trees up to 34 simulations (92,944 + 16,640 of 110,080 bytes; 35: 112,208).
"""
import numpy as np
import pytest

from tests.fc64 import FC64
from tests.parity_util import env_switches
from tests.test_gpu_supports import Errors, check_simulations, engine, slots_of, weights, O

pytestmark = pytest.mark.gpu
ROWS = 33
VS = RS = (-15, 15)
LT1_MAX_SIMS_A4 = 34      # (module docstring)


def _search(A, sims, run_sims=None, switches=None, mask=None, seed=5):
  """one search of 33 trees; -> (float64 network, exported tree with hidden states, sim_io log [B, sims + 1, 2 + A], info)"""
  rng = np.random.RandomState(seed)
  w = weights(VS, RS, A, False, seed=9)
  eng = engine(ROWS, VS, RS, A, False, sims=sims, switches=switches)
  eng.set_weights(w)
  info = eng.search_kernel_info()
  obs = (rng.standard_normal((ROWS, O)) * 2).astype(np.float32)
  noise = rng.dirichlet([0.25] * A, size=ROWS)
  legal = None
  if mask is not None:
    legal = np.zeros((ROWS, A), np.uint8)
    legal[:, mask] = 1
  log = eng.sim_io('log', keep_moves=1)
  eng.initial_inference(obs)
  eng.root_prepare(None, legal, noise)
  eng.search(run_sims)
  t = eng.export_tree(hidden=True)
  io = log[0].cpu().numpy().copy()
  eng.sim_io('off')
  eng.close()
  return FC64(w, O, A, VS, RS, False), obs, t, io, info


@pytest.mark.parametrize('sims', [1, 2, 5])
@pytest.mark.parametrize('A', [2, 3, 4])
def test_every_simulation_vs_float64(A, sims):
  ref, obs, t, io, info = _search(A, sims)
  assert info['kind'] == 'fused' and info['lt'] == 1 and info['G'] == 4, info
  err = Errors('A %d, %d simulations' % (A, sims), VS, RS, False)
  err.exact('root hidden', t['hidden'][:, 0], ref.initial(obs)[0])
  check_simulations(err, ref, t, io, A, sims, VS, RS)
  err.report()
  if A == 4 and sims == 5:      # all four actions are present among the simulations (and mixed inside the workgroups)
    _, _, act = slots_of(t, A, sims)
    assert set(np.unique(act)) == {0, 1, 2, 3}
    assert all(len(np.unique(act[16 * g:16 * g + 16, 0])) > 1 for g in range(2))


@pytest.mark.parametrize('sims', [1, 2])
@pytest.mark.parametrize('a', [0, 3])
def test_one_action_per_workgroup_vs_float64(a, sims):
  """a legal mask of one action at the root: in the first simulation every tree of every workgroup holds that action (all
  lanes read the same table row: a broadcast)"""
  A = 4
  ref, obs, t, io, info = _search(A, sims, mask=a)
  assert info['kind'] == 'fused' and info['lt'] == 1, info
  _, parent, act = slots_of(t, A, sims)
  assert np.all(act[:, 0] == a) and np.all(parent[:, 0] == 0)
  err = Errors('A 4, only action %d legal, %d simulations' % (a, sims), VS, RS, False)
  check_simulations(err, ref, t, io, A, sims, VS, RS)
  err.report()


def _same_bytes(x, y, what):
  assert x.shape == y.shape and x.dtype == y.dtype, what
  assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what


@pytest.mark.parametrize('A,sims,lt', [(4, 30, 1), (2, 62, 1), (4, LT1_MAX_SIMS_A4, 1), (4, LT1_MAX_SIMS_A4 + 1, 2), (3, 62, 2)])
def test_lds_placements_vs_pool_trees_bitwise(A, sims, lt):
  """LT 1 reads the table from LDS in front of whole trees, LT 2 from global memory, the pool placement (MZ_NO_LDS_TREES)
  from LDS in front of the pb_c table alone: the same values in the same order, so trees, hidden states and logged network
  outputs agree byte for byte.  The placements are those the fit gives with the table counted."""
  run = min(sims, 8)
  _, _, t, io, info = _search(A, sims, run_sims=run)
  assert info['kind'] == 'fused' and info['lt'] == lt, info
  _, _, t0, io0, info0 = _search(A, sims, run_sims=run, switches={'MZ_NO_LDS_TREES': '1'})
  assert info0['kind'] == 'fused' and info0['lt'] == 0, info0
  for k in ('N', 'W', 'P', 'R', 'E', 'TP', 'hidden', 'minmax'):
    _same_bytes(t[k], t0[k], (A, sims, k))
  _same_bytes(io, io0, (A, sims, 'sim_io'))
  assert np.all((t['E'] > 0).sum(1) == run)


@pytest.mark.parametrize('name', ['synthetic_A4', 'cartpole'])
def test_whole_moves_vs_launch_per_move_bitwise(name):
  """two launches of 3 moves, 5 simulations: the table is loaded once per launch and survives the root of every move"""
  from tests.test_gpu_stream_placement import _records
  whole, mpl = _records(name, 5, False)
  split, mpl0 = _records(name, 5, True)
  assert (mpl, mpl0) == (16, 0)
  _same_bytes(whole, split, name)


@pytest.mark.parametrize('A,sims,env', [(4, 30, None), (2, 62, 'cartpole')])
def test_placement_keeps_whole_trees_and_whole_moves(A, sims, env):
  from model_based_rl_amd.engine import Engine
  from tests.parity_util import random_weights
  obs_dim = 4 if env else 8
  eng = Engine(ROWS, obs_dim, A, sims, seed=1)
  if env:
    eng.selfplay_set_env(env)
  eng.set_weights(random_weights(obs_dim, A, 1))
  info = eng.search_kernel_info()
  mpl = eng.selfplay_moves_per_launch()
  eng.close()
  assert info['kind'] == 'fused' and info['lt'] == 1 and info['ks1'] == 14, info
  assert mpl == 16, mpl
