"""SURVEY.md s8 row f1 (replay sampling + n-step targets) inside the driver's GPU record: the host-side parity tests of
tests/test_replay_native.py need no GPU, so the `-m "not gpu"` run is where they normally execute; these wrappers run the
same checks under the gpu marker, so that GPUTEST_rNN re-confirms them on the GPU box's host (where the replay actually
runs beside the device loop) -- plus the parallel ingest against one thread there."""
import os

import pytest

from tests import test_replay_native as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('path', T.FILES, ids=[os.path.basename(f)[:-4] for f in T.FILES])
def test_sample_batch_matches_reference_on_the_gpu_host(path):
  T.test_sample_batch_matches_reference(path)


@pytest.mark.parametrize('path', T.FILES, ids=[os.path.basename(f)[:-4] for f in T.FILES])
def test_save_history_matches_reference_on_the_gpu_host(path):
  T.test_save_history_matches_reference(path)


def test_parallel_ingest_is_bit_identical_on_the_gpu_host():
  T.test_parallel_ingest_is_bit_identical_to_one_thread(40, 500, 3000)


def test_packed_byte_observations_in_ram_records():
  """The -ram- shapes with their 128 byte observations PACKED in the experience record (mz_selfplay_set_obs uint8_obs = 2: four
  bytes per float slot, 48 instead of 144 floats per Pong-ram record) against the unpacked records of the same run: every field
  equal, the observations byte for byte; and a replay with obs_u8 fed the packed chunk samples the batch a plain replay fed the
  unpacked chunk samples (game.py:93-96: History keeps the raw observation; the learner gets float32 back)."""
  import types
  import numpy as np
  import torch
  from oracle import oracle as orc
  from model_based_rl_amd.engine import Engine, records_view
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  B, O, A, sims, moves = 256, 128, 6, 50, 24
  w = orc.load_weights(np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g1_net_pong.npz')))
  out = {}
  for packed in (False, True):
    eng = Engine(B, O, A, sims, seed=99)
    eng.set_weights(w)
    eng.selfplay_set_obs(uint8_obs=True, obs_min=[0.0], obs_range=[255.0], packed=packed)
    eng.selfplay_reset(7, 1.0, stagger=True)
    assert eng.rec_floats == (O // 4 if packed else O) + A + 10
    eng.selfplay_steps(moves)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == moves and buf.shape[-1] == eng.rec_floats
    out[packed] = buf[:n].numpy().copy()
    eng.close()
  a, b = records_view(out[False], O, A), records_view(out[True], O, A, obs_u8=True)
  assert b['obs'].dtype == np.uint8 and np.array_equal(a['obs'], b['obs'].astype(np.float32))
  for k in ('child_visits', 'root_value', 'error', 'reward', 'action', 'done', 'step', 'env_id', 'episode'):
    assert np.array_equal(a[k], b[k]), k
  cfg = dict(batch_size=32, epsilon=0.01, alpha=1.0, beta=1.0, obs_space=(O,), action_space=A, window_size=1 << 15, window_step=None,
             num_unroll_steps=5, td_steps=10, max_history_length=500, discount=0.997, seed=0)
  ra, rb = PrioritizedReplay(types.SimpleNamespace(**cfg)), PrioritizedReplay(types.SimpleNamespace(obs_u8=True, **cfg))
  ra.ingest_records(out[False], moves, B)
  rb.ingest_records(out[True], moves, B)
  assert ra.size() == rb.size() > 0 and ra.tree.total_priority == rb.tree.total_priority
  import random
  random.seed(5); np.random.seed(5)
  (oa, aa, (ta, va, pa)), ia, wa = ra.sample_batch()
  random.seed(5); np.random.seed(5)
  (ob, ab, (tb, vb, pb)), ib, wb = rb.sample_batch()
  assert ia == ib and np.array_equal(oa, ob) and aa == ab and np.array_equal(ta, tb) and np.array_equal(va, vb) and np.array_equal(pa, pb)
  assert np.array_equal(wa, wb) and oa.dtype == np.float32


def test_stand_alone_end_of_move_kernel_with_packed_bytes(monkeypatch):
  """k_env_step_record -- the end of a synthetic move when the search runs as separate kernels (MZ_NO_FUSED) -- with byte
  observations packed in the record and unpacked: one ragged workgroup (B = 17), 8 simulations, O = 5 (a last slot of one
  byte), 5 moves of episodes of 3 steps, so that every environment ends a game and starts the next.  Every field of every
  record against its definition: step / episode / done / env id by the episode arithmetic, observation and reward from
  mz_synth_obs, the packed record's fields equal to the unpacked one's; and the last move's search statistics against the
  tree the search left in the pool (visit shares, root value, error against the initial inference's value)."""
  import numpy as np
  import torch
  import types
  from model_based_rl_amd.engine import Engine, flatten_weights, records_view
  from model_based_rl_amd.networks import FCNetwork
  B, O, A, sims, T, moves = 17, 5, 4, 8, 3, 5
  monkeypatch.setenv('MZ_NO_FUSED', '1')
  torch.manual_seed(4)
  w = flatten_weights(FCNetwork(O, A, torch.device('cpu'), types.SimpleNamespace()).state_dict())
  out = {}
  for packed in (False, True):
    eng = Engine(B, O, A, sims, seed=31, env_id_offset=5)
    eng.set_weights(w)
    assert eng.search_kernel_info()['kind'] == 'standalone' and eng.selfplay_moves_per_launch() == 0
    eng.selfplay_set_obs(uint8_obs=True, obs_min=[0.0], obs_range=[255.0], packed=packed)
    eng.selfplay_export_trees(True)
    eng.selfplay_reset(T, 1.0, stagger=False)
    assert eng.rec_floats == (2 if packed else O) + A + 10
    eng.selfplay_steps(moves)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == moves
    rec = buf[:n].numpy().copy()
    v = records_view(rec, O, A, obs_u8=packed)
    m = np.arange(moves)[:, None]
    assert np.array_equal(v['step'], np.broadcast_to(m % T, (moves, B))) and np.array_equal(v['episode'], np.broadcast_to(m // T, (moves, B)))
    assert np.array_equal(v['done'], np.broadcast_to(m % T == T - 1, (moves, B))) and np.all(v['to_play'] == 1)
    assert np.array_equal(v['env_id'], np.broadcast_to(5 + np.arange(B), (moves, B)))
    for mm in range(moves):
      for b in range(B):
        obs, rew = eng.synth_obs(5 + b, mm // T, mm % T)
        assert np.array_equal(v['obs'][mm, b].astype(np.float32), obs) and v['reward'][mm, b] == np.float32(rew), (mm, b)
    if packed:
      assert not rec[..., :2].copy().view(np.uint8)[..., O:].any()      # the last slot's three spare bytes
    t = eng.export_tree()
    N, W = t['N'][:, 1:1 + A].astype(np.float64), t['W']
    assert np.all(t['N'][:, 0] == sims)
    assert np.array_equal(v['child_visits'][-1], (N / N.sum(1, keepdims=True)).astype(np.float32))
    assert np.array_equal(v['root_value'][-1], W[:, 0] / t['N'][:, 0])
    v0 = eng.root_outputs()[0].cpu().numpy().astype(np.float64)
    assert np.array_equal(v['error'][-1], v['root_value'][-1] - v0)
    assert np.all(np.take_along_axis(v['child_visits'], v['action'][..., None].astype(np.int64), -1) > 0)
    out[packed] = v
    eng.close()
  for k in out[False]:
    assert np.array_equal(np.asarray(out[False][k], np.float64 if k == 'obs' else None), np.asarray(out[True][k], np.float64 if k == 'obs' else None)), k
