"""The weight streams' gather tables on the device, and the one launch sequence behind both weight entries (csrc/mz_pack.inc, mz_engine.hip):
every table an engine holds equals mz_pack_host's for its shape, and mz_set_weights and mz_set_weights_async leave the same scale and the
same search behind for the same weights.  16 environments, 2 simulations; action counts 2 (action table), 6, 9 with the split-f16 stream,
21 (two policy tiles); observation widths 4 and 27.

A split-f16 engine's mz_set_weights_async hands over to mz_set_weights (its float16 range check reads back), so at A = 9 the second
weight set is the same entry a second time: what that case adds is the device's idx_h2 and one search on the stream that the shared
launch sequence's k_pack_weights_h2 branch packed, twice with the same result.  The two entries proper are compared at A = 2, 6, 21."""
import ctypes as C

import numpy as np
import pytest

from tests.pack_util import pack_host
from tests.parity_util import random_weights

pytestmark = pytest.mark.gpu
B, SIMS = 16, 2


def _tables(eng, p):
  from model_based_rl_amd import _abi
  out = []
  for which, n in ((0, p['n_packed']), (1, p['n_packed']), (2, p['n_packed_h2'])):
    if not n:
      out.append(None)
      continue
    t = np.full(n, -7, np.int32)
    _abi.check(eng.lib.mz_pack_indices(eng._h, which, t.ctypes.data, C.c_size_t(n)), 'mz_pack_indices')
    out.append(t)
  return out


def _search_outputs(eng, w, sync, obs, noise):
  eng.set_weights(w, sync=sync)
  scale = eng.weight_scale().copy()
  eng.initial_inference(obs)
  eng.root_prepare(None, None, noise)
  eng.search()
  t = eng.export_tree(hidden=True)
  return scale, {k: np.ascontiguousarray(np.asarray(v)).copy() for k, v in t.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize('A,O,split', [(2, 4, False), (6, 27, False), (9, 4, True), (21, 27, False)])
def test_device_tables_and_both_weight_entries(A, O, split):
  from model_based_rl_amd.engine import Engine
  eng = Engine(B, O, A, SIMS, seed=3, split_f16=split)
  try:
    _, p, want = pack_host(eng.lib, O, A, 31, 31, int(split))
    assert p['n_flat'] == eng.num_weights
    got = _tables(eng, p)
    for name, g, w_ in zip(('idx', 'idx2', 'idx_h2'), got, want):
      assert (g is None) == (w_ is None) and (g is None or np.array_equal(g, w_)), (A, O, name)
    assert (got[2] is not None) == split
    info = eng.search_kernel_info()
    assert info['kind'] == ('split_f16' if split else 'fused'), info
    rng = np.random.RandomState(11)
    w = random_weights(O, A, seed=4)
    obs = rng.standard_normal((B, O)).astype(np.float32)
    noise = rng.dirichlet([0.25] * A, size=B)
    scale_s, tree_s = _search_outputs(eng, w, True, obs, noise)      # mz_set_weights
    # mz_set_weights_async (host weights, the host's scale decision); with split: mz_set_weights again, see above
    scale_a, tree_a = _search_outputs(eng, w, False, obs, noise)
    assert scale_s[3] == 1.0 and np.array_equal(scale_s.view(np.uint32), scale_a.view(np.uint32)), (scale_s, scale_a)
    assert sorted(tree_s) == sorted(tree_a) and 'N' in tree_s and 'hidden' in tree_s
    for k in tree_s:
      assert np.array_equal(tree_s[k].view(np.uint8), tree_a[k].view(np.uint8)), (A, O, k)
    assert np.all((tree_s['E'] > 0).sum(1) == SIMS)      # (both searches ran: every tree expanded one node per simulation)
  finally:
    eng.close()
