"""Reanalyse with the Gumbel search (mz_reanalyse_gumbel, csrc/mz_reanalyse.hip.h, Engine.reanalyse_gumbel, reanalyse.Reanalyser
under --reanalyse_gumbel; DESIGN s7j):
  exact       scale 0: fresh == the step-by-step path (initial_inference / root_prepare / gz_root / gz_search / gz_pick, finalize
              for the mean value) on the same engine bit for bit, both value kinds, on the positions of tests/test_gpu_reanalyse.py
              (both movers, occupied cells, full columns; legal masks from the host environments); pi' is 0 at illegal actions and
              sums to 1; guard rows and `rows` untouched; pi' is not the visit shares and v_mix is not the mean value
  keyed       scale 1: a one-chunk engine (B = 128) equals the step-by-step path with gz_root(None, move=draw_key), the three-chunk
              engine (B = 48) equals that bit for bit, the same key repeats, another key does not
  refusals    every sentence, and the engine works afterwards
  untouched   Engine.reanalyse after reanalyse_gumbel and set_gumbel(False) == an engine that never saw the Gumbel search
  end to end  Gumbel self-play through an Actor under W0 into a replay, a Gumbel-mode Reanalyser under W1: the replay's policy
              targets and values are the W1 search's, a second pass with the same key changes nothing
  wiring      the actor makes a Gumbel-mode Reanalyser after a weight pull and hands it the training step as the key
Shapes: those of tests/test_gpu_reanalyse.py -- B = 48, 2 * 48 + 17 = 113 rows, 5 guard rows."""
import functools
import os

import numpy as np
import pytest

import tests.test_gpu_reanalyse as base
from tests.eval_device_util import weights

pytestmark = pytest.mark.gpu

B, N_ROWS, GUARD, PATTERN = base.B, base.N_ROWS, base.GUARD, base.PATTERN
SIMS = {'synthetic': 8, 'tictactoe': 8, 'cartpole': 8, 'connect_four': 16}      # TicTacToe: A > n, zero-visit phase; Connect Four: m = 7, halving runs
QUIET = dict(max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=0.0)
NOISY = dict(QUIET, gumbel_scale=1.0)
KEY = (3 << 32) | 7      # (both words of the key are in use)


def make_engine(name, batch=B):
  from model_based_rl_amd.engine import Engine
  kind, O, A, two = base.SHAPES[name]
  eng = Engine(batch, O, A, SIMS[name], two_players=two, known_bounds=(-1, 1) if two else (None, None), discount=1.0 if two else 0.997, seed=3)
  eng.set_weights(weights(O, A, 7))
  return eng


def stepwise(eng, obs, to_play, legal, sims, move=0):
  """the step-by-step Gumbel search of the rows, chunk by chunk of the engine's B -> (pi' [n, A] float64, v_mix [n], mean value [n])"""
  n, O = obs.shape
  A, Bn = legal.shape[1], eng.B
  pi, vmix, mean = np.zeros((n, A), np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64)
  for at in range(0, n, Bn):
    m = min(Bn, n - at)
    o, tp, lg = np.zeros((Bn, O), np.float32), np.ones(Bn, np.int8), np.ones((Bn, A), np.uint8)
    o[:m], tp[:m], lg[:m] = obs[at:at + m], to_play[at:at + m], legal[at:at + m]
    eng.initial_inference(o)
    eng.root_prepare(tp, lg, None, device_rng=False)
    eng.gz_root(None, move=move)
    eng.gz_search(sims)
    _, _, p, v = eng.gz_pick()
    pi[at:at + m], vmix[at:at + m] = p.cpu().numpy()[:m], v.cpu().numpy()[:m]
    mean[at:at + m] = eng.finalize(0.0, np.zeros(Bn))['root_value'].cpu().numpy()[:m]
  return pi, vmix, mean


def run_gumbel(eng, rows, kind, sims, A, value='mean', draw_key=0):
  import torch
  pr = torch.from_numpy(rows.copy()).pin_memory()
  fresh = torch.full((N_ROWS + GUARD, A + 2), float(PATTERN), dtype=torch.float32).pin_memory()
  eng.reanalyse_gumbel(pr, fresh, N_ROWS, kind, sims, value=value, draw_key=draw_key)
  return pr.numpy(), fresh.numpy()


def split(fresh, A):
  return fresh[:N_ROWS, :A], np.ascontiguousarray(fresh[:N_ROWS, A:]).view(np.float64)[:, 0]


@functools.lru_cache(maxsize=None)
def case(name):
  """one engine per shape with the Gumbel search at scale 0, the rows, the PUCT pass of the engine before it saw the Gumbel
  search, and the step-by-step results (computed once, left unchanged)"""
  import torch
  kind, O, A, two = base.SHAPES[name]
  rng = np.random.RandomState(len(name))
  obs, to_play, legal = base.positions(name, rng)
  rows = base.rows_of(obs, to_play, A, rng)
  eng = make_engine(name)
  _, puct = base.run_reanalyse(eng, rows, kind, SIMS[name], A)
  eng.set_gumbel(True, **QUIET)
  ref = stepwise(eng, obs, to_play, legal, SIMS[name])
  torch.cuda.synchronize()
  return eng, obs, rows, legal, to_play, puct.copy(), ref


@pytest.mark.parametrize('value', ['mean', 'vmix'])
@pytest.mark.parametrize('name', sorted(SIMS))
def test_fresh_equals_the_step_by_step_path_bit_for_bit(name, value):
  kind, O, A, two = base.SHAPES[name]
  eng, obs, rows, legal, to_play, puct, (pi, vmix, mean) = case(name)
  if two:      # both movers, occupied cells / full columns among the rows
    assert (to_play == 1).any() and (to_play == -1).any() and (legal == 0).any() and (kind != 3 or (legal.sum(1) == 1).sum() >= 12)
  after, fresh = run_gumbel(eng, rows, kind, SIMS[name], A, value)
  got_pi, got_v = split(fresh, A)
  want_v = vmix if value == 'vmix' else mean
  assert np.array_equal(got_pi.view(np.uint32), pi.astype(np.float32).view(np.uint32))
  assert np.array_equal(got_v.view(np.uint64), want_v.view(np.uint64))
  # 0 at every illegal action, a distribution over the rest (A float32 roundings of at most half an ulp of 1 each)
  assert np.all(got_pi[legal == 0] == 0.0) and np.all(got_pi >= 0.0)
  assert np.all(np.abs(got_pi.astype(np.float64).sum(1) - 1.0) <= A * 2.0 ** -24)
  # the guard rows behind row n_rows keep their pattern, and the rows themselves are only read
  assert np.all(fresh[N_ROWS:] == PATTERN)
  assert np.array_equal(after.view(np.uint32), rows.view(np.uint32))
  # able to fail for the right reason: pi' is not the visit shares of the same number of simulations, v_mix not the mean value
  puct_cv, _ = split(puct, A)
  several = legal.sum(1) > 1      # (a position with one legal action has one policy)
  assert (np.any(got_pi != puct_cv, axis=1) & several).sum() > several.sum() // 2
  assert (vmix != mean).sum() > N_ROWS // 2
  assert len(np.unique(got_v)) > N_ROWS // 4      # (searched, not a constant)


@pytest.mark.parametrize('name', ['tictactoe', 'connect_four'])
def test_draws_are_keyed_by_the_row_not_the_batch(name):
  import torch
  kind, O, A, two = base.SHAPES[name]
  _, obs, rows, legal, to_play, _, quiet_ref = case(name)
  one = make_engine(name, batch=128)      # the whole pass is one chunk: tree index == row index
  one.set_gumbel(True, **NOISY)
  pi, vmix, mean = stepwise(one, obs, to_play, legal, SIMS[name], move=KEY)
  torch.cuda.synchronize()
  assert not np.array_equal(pi, quiet_ref[0])      # (the noise did something)
  _, fresh_one = run_gumbel(one, rows, kind, SIMS[name], A, 'mean', KEY)
  one.close()
  got_pi, got_v = split(fresh_one, A)
  assert np.array_equal(got_pi.view(np.uint32), pi.astype(np.float32).view(np.uint32))
  assert np.array_equal(got_v.view(np.uint64), mean.view(np.uint64))
  three = make_engine(name)               # three chunks of 48: the key is the row's index in the pass
  three.set_gumbel(True, **NOISY)
  _, fresh_three = run_gumbel(three, rows, kind, SIMS[name], A, 'mean', KEY)
  assert np.array_equal(fresh_three.view(np.uint32), fresh_one.view(np.uint32))
  _, again = run_gumbel(three, rows, kind, SIMS[name], A, 'mean', KEY)
  assert np.array_equal(again.view(np.uint32), fresh_three.view(np.uint32))
  _, other = run_gumbel(three, rows, kind, SIMS[name], A, 'mean', KEY + 1)
  three.close()
  changed = np.any(other[:N_ROWS].view(np.uint32) != fresh_three[:N_ROWS].view(np.uint32), axis=1)
  assert changed.sum() > 0
  assert np.all(other[:N_ROWS, :A][legal == 0] == 0.0) and np.all(other[N_ROWS:] == PATTERN)


def test_refusals():
  import torch
  from model_based_rl_amd.engine import Engine
  O, A = 9, 9
  eng = Engine(B, O, A, 8, two_players=True, seed=1)
  rows = torch.zeros(B, O + A + 10, dtype=torch.float32).pin_memory()
  fresh = torch.zeros(B, A + 2, dtype=torch.float32).pin_memory()
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: weights not set'):
    eng.reanalyse_gumbel(rows, fresh, B, 1)
  eng.set_weights(weights(O, A, 7))
  with pytest.raises(RuntimeError, match=r'mz_reanalyse_gumbel: no Gumbel search is set on this engine \(call mz_set_gumbel first\)'):
    eng.reanalyse_gumbel(rows, fresh, B, 1)
  eng.set_gumbel(True, **QUIET)
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: rec_floats'):
    eng.reanalyse_gumbel(torch.zeros(B, O + A + 9, dtype=torch.float32).pin_memory(), fresh, B, 1)
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: kind must be'):
    eng.reanalyse_gumbel(rows, fresh, B, 4)
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: Connect Four needs'):
    eng.reanalyse_gumbel(rows, fresh, B, 3)
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: CartPole needs'):
    eng.reanalyse_gumbel(rows, fresh, B, 'cartpole')
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: n_rows must be'):
    eng.reanalyse_gumbel(rows, fresh, -1, 1)
  for sims in (0, 9):
    with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: num_simulations must be in 1 .. 8'):
      eng.reanalyse_gumbel(rows, fresh, B, 1, num_simulations=sims)
  with pytest.raises(ValueError, match='reanalyse_gumbel: rows must be a contiguous pinned'):
    eng.reanalyse_gumbel(torch.zeros(B, O + A + 10), fresh, B, 1)
  with pytest.raises(ValueError, match="reanalyse_gumbel: value is 'mean' or 'vmix'"):
    eng.reanalyse_gumbel(rows, fresh, B, 1, value='median')
  rc = eng.lib.mz_reanalyse_gumbel(eng._h, 1, rows.data_ptr(), O + A + 10, B, fresh.data_ptr(), 8, 2, 0, eng.stream)      # (the C sentence itself)
  assert rc != 0 and eng.lib.mz_last_error().decode().startswith('mz_reanalyse_gumbel: value_kind 2')
  eng.set_gumbel(False)
  with pytest.raises(RuntimeError, match='mz_reanalyse_gumbel: no Gumbel search is set'):
    eng.reanalyse_gumbel(rows, fresh, B, 1)
  eng.set_gumbel(True, **QUIET)
  eng.reanalyse_gumbel(rows, fresh, 0, 1)                       # nothing to do is not an error
  eng.reanalyse_gumbel(rows, fresh, B, 'tictactoe')            # and the engine still works after the refusals
  assert np.allclose(fresh.numpy()[:, :A].sum(1), 1.0, atol=1e-6)
  eng.reanalyse_gumbel(rows, fresh, B, 'tictactoe', num_simulations=3)      # fewer simulations than the pool: a descent stays pending,
  eng.gz_search(2)                                                          # which the stepwise search may take up
  eng.reanalyse(rows, fresh, B, 'tictactoe')
  assert np.allclose(fresh.numpy()[:, :A].sum(1), 1.0, atol=1e-6)
  eng.close()


def test_the_puct_pass_is_untouched():
  name = 'tictactoe'
  kind, O, A, two = base.SHAPES[name]
  eng, obs, rows, legal, to_play, puct, _ = case(name)
  try:
    eng.set_gumbel(True, **NOISY)
    run_gumbel(eng, rows, kind, SIMS[name], A, 'vmix', KEY)
    eng.set_gumbel(False)
    _, fresh = base.run_reanalyse(eng, rows, kind, SIMS[name], A)
  finally:
    eng.set_gumbel(True, **QUIET)      # (the shared engine as case() leaves it)
  assert np.array_equal(fresh.view(np.uint32), puct.view(np.uint32))


def test_end_to_end_targets_are_the_new_networks_improved_policy(tmp_path):
  """16 Gumbel self-play moves of 48 TicTacToe environments at 8 simulations under W0, through an Actor built as train builds
  it, into a replay; one Gumbel-mode Reanalyser pass over the whole replay under W1: the stored policy targets and values, and
  the policy targets sample_batch returns, are the step-by-step W1 Gumbel search of those observations"""
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.reanalyse import Reanalyser, refuse_reanalyse, refuse_reanalyse_gumbel
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.selfplay_search import refuse_selfplay_gumbel
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = base.ttt_config(tmp_path, '--selfplay_gumbel', '--selfplay_gumbel_value', 'vmix', '--reanalyse_rows', '4096', '--reanalyse_gumbel',
                        '--weight_sync_frequency', '1000')      # (no pull inside the 16 moves: the actor itself runs no pass here)
  for refuse in (refuse_reanalyse, refuse_reanalyse_gumbel, refuse_selfplay_gumbel):
    refuse(cfg)
  O, A = 9, 9
  w0, w1 = weights(O, A, 7), weights(O, A, 8)
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  storage.store_weights(w0, 0)
  actor = Actor(0, cfg, storage, replay)
  actor.launch(max_moves=16)
  assert actor.engine.selfplay_gumbel and actor.reanalyser is None and actor.reanalyse_runs == 0
  assert replay.size() > 200
  stale = replay.reanalyse_pick(4096)
  stale_rows = stale['rows'].copy()
  replay.reanalyse_release(stale['ticket'])
  assert np.any((stale_rows[:, O:O + A] * 8) % 1 != 0), 'the stored policies are pi\', not visit shares of 8 simulations'
  re = Reanalyser(cfg, replay, max_rows=4096)
  assert re.B == B and re.gumbel and re.gumbel_value == 'vmix' and re.engine.gumbel
  re.set_weights(w1)
  out = re.run(4096, draw_key=5)
  assert out['rows'] >= replay.size() and out['slices'] > 0 and out['skipped_slices'] == 0 and not out['busy']
  assert out['mean_policy_l1'] > 0 and out['mean_abs_value_change'] > 0 and out['seconds'] > 0
  # the step-by-step W1 search: another engine of the same configuration, the Gumbel search at the Reanalyser's scale 0
  eng = Engine.from_config(cfg, B)
  eng.set_weights(w1)
  eng.set_gumbel(True, **QUIET)

  def w1_search(obs):
    lg = (obs == 0).astype(np.uint8)
    # the mover: the stones on the board are the mover's +1 and the other's -1; player +1 moves on an even number of stones
    tp = np.where((obs != 0).sum(1) % 2 == 0, 1, -1).astype(np.int8)
    pi, vmix, _ = stepwise(eng, np.ascontiguousarray(obs, np.float32), tp, lg, 8)
    return pi.astype(np.float32), vmix
  now = replay.reanalyse_pick(4096)
  replay.reanalyse_release(now['ticket'])
  assert now['n_rows'] == stale['n_rows'] == out['rows']
  rows = now['rows'][:now['n_rows']]
  want_pi, want_v = w1_search(rows[:, :O])
  assert np.array_equal(rows[:, O:O + A].view(np.uint32), want_pi.view(np.uint32))
  assert np.array_equal(np.ascontiguousarray(rows[:, O + A:O + A + 2]).view(np.uint64)[:, 0], want_v.view(np.uint64))
  assert np.array_equal(rows[:, :O], stale_rows[:now['n_rows'], :O])
  assert np.array_equal(rows[:, O + A + 2:].view(np.uint32), stale_rows[:now['n_rows'], O + A + 2:].view(np.uint32))
  batch, _ = replay.sample_batch_arrays()      # (position 0 of the unroll is the sampled step itself)
  want_pol, _ = w1_search(batch['obs'].reshape(-1, O))
  assert np.array_equal(batch['t_pol'][:, 0].view(np.uint32), want_pol.view(np.uint32))
  # a second pass with the same weights and the same key changes nothing
  again = re.run(4096, draw_key=5)
  assert again['rows'] == out['rows'] and again['mean_abs_value_change'] == 0 and again['mean_policy_l1'] == 0
  re.close(); eng.close(); actor.close(); actor.engine.close()


def test_the_actor_hands_the_training_step_to_a_gumbel_reanalyser(tmp_path, monkeypatch):
  import torch
  from model_based_rl_amd import reanalyse
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  calls = []
  real = reanalyse.Reanalyser

  class Recording(real):
    def run(self, *a, **k):
      calls.append((self.gumbel, self.engine.gumbel if self.gumbel else False, a, dict(k)))
      return real.run(self, *a, **k)
  monkeypatch.setattr(reanalyse, 'Reanalyser', Recording)
  for gumbel in (True, False):
    del calls[:]
    extra = ['--selfplay_gumbel', '--reanalyse_gumbel'] if gumbel else []
    cfg = base.ttt_config(tmp_path / str(gumbel), '--reanalyse_rows', '2048', '--reanalyse_every', '1', '--weight_sync_frequency', '16', *extra)
    storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
    storage.store_weights(weights(9, 9, 7), 5)            # (training step 5: past a multiple of --reanalyse_every at every pull)
    actor = Actor(0, cfg, storage, replay)
    actor.launch(max_moves=32)
    assert actor.reanalyse_runs >= 1 and len(calls) == actor.reanalyse_runs and actor.last_reanalyse['rows'] > 0
    if gumbel:
      assert all(c == (True, True, (2048,), {'draw_key': 5}) for c in calls), calls
      assert actor.reanalyser.gumbel_value == 'mean'
      picked = replay.reanalyse_pick(2048)
      replay.reanalyse_release(picked['ticket'])
      pol = picked['rows'][:picked['n_rows'], 9:18]
      assert np.any((pol * 8) % 1 != 0) and np.abs(pol.sum(1) - 1).max() <= 1e-6      # pi' everywhere, no visit shares mixed in
    else:      # as before: a PUCT pass, called as it was
      assert all(c == (False, False, (2048,), {}) for c in calls), calls
      assert not getattr(actor.reanalyser.engine, 'gumbel', False)
    actor.reanalyser.close()
    actor.close(); actor.engine.close()
    torch.cuda.synchronize()
