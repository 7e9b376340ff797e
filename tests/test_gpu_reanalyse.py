"""MuZero Reanalyse on the device (csrc/mz_reanalyse.hip.h, Engine.reanalyse, reanalyse.Reanalyser):
  exact       fresh == the step-by-step path (initial_inference / root_prepare / search / finalize on the same engine) bit for
              bit, on positions with occupied cells and full columns and both movers; legal masks of the step-by-step side come
              from the host environments; child_visits is 0 at illegal actions and sums to 1; guard rows and `rows` untouched
  end to end  self-play into a replay under W0, Reanalyser.run under W1: sample_batch's policy targets are the W1 search's, and
              a second pass changes nothing
  refusals    wrong rec_floats, kind / shape mismatch, weights not set
  train       with --reanalyse_rows 0 no Reanalyser is ever made; with it, the actor runs a pass after a weight pull
Shapes: B = 48 (three 16-tree workgroups, not a multiple of the 128-thread block), 2 * 48 + 17 rows (a partial last chunk)."""
import functools
import os

import numpy as np
import pytest

from tests.eval_device_util import ENV_FLAGS, weights

pytestmark = pytest.mark.gpu

B, N_ROWS, GUARD, SIMS = 48, 2 * 48 + 17, 5, 30
#        name: (kind, obs_dim, action_space, two_players)
SHAPES = {'synthetic': (0, 8, 4, False), 'tictactoe': (1, 9, 9, True), 'connect_four': (3, 42, 7, True), 'cartpole': (2, 4, 2, False)}
PATTERN = np.float32(-12345.5)


def positions(name, rng):
  """N_ROWS stored positions of the shape: (obs [n, O] float32, to_play [n] int8, legal [n, A] uint8 from the host environments)"""
  from model_based_rl_amd import envs
  from tests.c4_positions import POSITIONS
  kind, O, A, two = SHAPES[name]
  obs, to_play, legal = np.zeros((N_ROWS, O), np.float32), np.ones(N_ROWS, np.int8), np.ones((N_ROWS, A), np.uint8)
  if kind in (0, 2):
    obs[:] = rng.uniform(-1, 1, size=obs.shape)
    return obs, to_play, legal
  i = 0
  if kind == 3:                                               # six full columns, seen by either mover
    for _, turn, _, board in POSITIONS:
      for t in (turn, -turn):
        e = envs.ConnectFour()
        e.reset()
        e.board, e.turn = np.array(board, np.int32), t
        obs[i], to_play[i], legal[i] = t * e.board, t, 0
        legal[i, e.legal_actions()] = 1
        i += 1
  while i < N_ROWS:                                           # random games from the start: cells and columns fill up
    e = envs.TicTacToe() if kind == 1 else envs.ConnectFour()
    e.reset()
    done = False
    while not done and i < N_ROWS:
      acts = np.asarray(e.legal_actions())
      obs[i], to_play[i], legal[i] = e.turn * np.asarray(e.board).reshape(-1), e.turn, 0
      legal[i, acts] = 1
      i += 1
      _, _, done, _ = e.step(int(rng.choice(acts)))
  return obs, to_play, legal


def rows_of(obs, to_play, A, rng):
  """record rows as the replay stores them: the observation, stale statistics, and the mover in bit 1 of the flags word"""
  n, O = obs.shape
  rows = rng.uniform(-1, 1, size=(n, O + A + 10)).astype(np.float32)      # (every field the kernel must not read is noise)
  rows[:, :O] = obs
  ints = rows[:, O + A + 5:].view(np.int32)
  ints[:, 1] = rng.randint(0, 2, n) | np.where(to_play < 0, 2, 0)           # bit 0 (done) is noise too
  return rows


@functools.lru_cache(maxsize=None)
def case(name):
  """one engine per shape, the rows, and the step-by-step results per simulation count (computed once, left unchanged)"""
  import torch
  from model_based_rl_amd.engine import Engine
  kind, O, A, two = SHAPES[name]
  rng = np.random.RandomState(len(name))
  obs, to_play, legal = positions(name, rng)
  rows = rows_of(obs, to_play, A, rng)
  eng = Engine(B, O, A, SIMS, two_players=two, known_bounds=(-1, 1) if two else (None, None), discount=1.0 if two else 0.997, seed=3)
  eng.set_weights(weights(O, A, 7))
  ref = {}
  for sims in (1, 5, 30):
    cv, rv = np.zeros((N_ROWS, A), np.float64), np.zeros(N_ROWS, np.float64)
    for at in range(0, N_ROWS, B):
      n = min(B, N_ROWS - at)
      o, tp, lg = np.zeros((B, O), np.float32), np.ones(B, np.int8), np.ones((B, A), np.uint8)
      o[:n], tp[:n], lg[:n] = obs[at:at + n], to_play[at:at + n], legal[at:at + n]
      eng.initial_inference(o)
      eng.root_prepare(tp, lg, None, device_rng=False)
      eng.search(sims)
      out = eng.finalize(0.0, np.zeros(B))
      cv[at:at + n], rv[at:at + n] = out['child_visits'].cpu().numpy()[:n], out['root_value'].cpu().numpy()[:n]
    ref[sims] = (cv, rv)
  torch.cuda.synchronize()
  return eng, rows, legal, to_play, ref


def run_reanalyse(eng, rows, kind, sims, A):
  import torch
  pr = torch.from_numpy(rows.copy()).pin_memory()
  fresh = torch.full((N_ROWS + GUARD, A + 2), float(PATTERN), dtype=torch.float32).pin_memory()
  eng.reanalyse(pr, fresh, N_ROWS, kind, sims)
  return pr.numpy(), fresh.numpy()


@pytest.mark.parametrize('sims', [1, 5, 30])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_fresh_equals_the_step_by_step_path_bit_for_bit(name, sims):
  kind, O, A, two = SHAPES[name]
  eng, rows, legal, to_play, ref = case(name)
  if two:      # both movers, occupied cells / full columns among the rows
    assert (to_play == 1).any() and (to_play == -1).any() and (legal == 0).any() and (kind != 3 or (legal.sum(1) == 1).sum() >= 12)
  after, fresh = run_reanalyse(eng, rows, kind, sims, A)
  cv, rv = ref[sims]
  got_cv = fresh[:N_ROWS, :A]
  got_rv = np.ascontiguousarray(fresh[:N_ROWS, A:]).view(np.float64)[:, 0]
  assert np.array_equal(got_cv.view(np.uint32), cv.astype(np.float32).view(np.uint32))
  assert np.array_equal(got_rv.view(np.uint64), rv.view(np.uint64))
  # 0 at every illegal action, a distribution over the rest (A float32 roundings of at most half an ulp of 1 each)
  assert np.all(got_cv[legal == 0] == 0.0) and np.all(got_cv >= 0.0)
  assert np.all(np.abs(got_cv.astype(np.float64).sum(1) - 1.0) <= A * 2.0 ** -24)
  # the guard rows behind row n_rows keep their pattern, and the rows themselves are only read
  assert np.all(fresh[N_ROWS:] == PATTERN)
  assert np.array_equal(after.view(np.uint32), rows.view(np.uint32))
  if sims > 1:
    assert len(np.unique(got_rv)) > N_ROWS // 4      # (searched, not a constant)


def test_refusals():
  import torch
  from model_based_rl_amd.engine import Engine
  O, A = 9, 9
  eng = Engine(B, O, A, 8, two_players=True, seed=1)
  rows = torch.zeros(B, O + A + 10, dtype=torch.float32).pin_memory()
  fresh = torch.zeros(B, A + 2, dtype=torch.float32).pin_memory()
  with pytest.raises(RuntimeError, match='weights not set'):
    eng.reanalyse(rows, fresh, B, 1)
  eng.set_weights(weights(O, A, 7))
  with pytest.raises(RuntimeError, match='rec_floats'):
    eng.reanalyse(torch.zeros(B, O + A + 9, dtype=torch.float32).pin_memory(), fresh, B, 1)
  with pytest.raises(RuntimeError, match='kind must be'):
    eng.reanalyse(rows, fresh, B, 4)
  with pytest.raises(RuntimeError, match='Connect Four needs'):
    eng.reanalyse(rows, fresh, B, 3)
  with pytest.raises(RuntimeError, match='CartPole needs'):
    eng.reanalyse(rows, fresh, B, 'cartpole')
  with pytest.raises(RuntimeError, match='n_rows must be'):
    eng.reanalyse(rows, fresh, -1, 1)
  with pytest.raises(RuntimeError, match='num_simulations'):
    eng.reanalyse(rows, fresh, B, 1, num_simulations=9)
  with pytest.raises(ValueError, match='pinned'):
    eng.reanalyse(torch.zeros(B, O + A + 10), fresh, B, 1)
  eng.reanalyse(rows, fresh, 0, 1)                       # nothing to do is not an error
  eng.reanalyse(rows, fresh, B, 'tictactoe')            # and the engine still works after the refusals
  assert np.allclose(fresh.numpy()[:, :A].sum(1), 1.0, atol=1e-6)
  eng.close()


def ttt_config(tmp_path, *extra):
  from model_based_rl_amd.config import make_config
  return make_config(ENV_FLAGS['TicTacToe'] + ['--num_envs', str(B), '--num_simulations', '8', '--seed', '5', '--window_size', '4096',
                                               '--batch_size', '64', '--td_steps', '3', '--max_history_length', '8',
                                               '--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'r'] + list(extra))


def test_end_to_end_targets_are_the_new_networks(tmp_path):
  """16 self-play moves of 48 TicTacToe environments under W0 into a replay, one Reanalyser pass over the whole replay under
  W1: the policy targets sample_batch returns at the sampled steps are the step-by-step W1 search of those observations"""
  import torch
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.reanalyse import Reanalyser
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  cfg = ttt_config(tmp_path)
  O, A = 9, 9
  w0, w1 = weights(O, A, 7), weights(O, A, 8)
  replay = PrioritizedReplay(cfg)
  eng = Engine.from_config(cfg, B)
  eng.set_weights(w0)
  eng.selfplay_set_env('tictactoe')
  eng.selfplay_reset(9, 1.0)
  eng.selfplay_steps(16)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == 16
  replay.ingest_records(buf[:n].numpy().copy(), n, B)
  assert replay.size() > 200
  stale = replay.reanalyse_pick(4096)
  stale_rows = stale['rows'].copy()
  replay.reanalyse_release(stale['ticket'])
  re = Reanalyser(cfg, replay, max_rows=4096)
  assert re.B == B and re.engine is not eng
  re.set_weights(w1)
  out = re.run(4096)
  assert out['rows'] >= replay.size() and out['slices'] > 0 and out['skipped_slices'] == 0
  assert out['mean_policy_l1'] > 0 and out['mean_abs_value_change'] > 0 and out['seconds'] > 0
  batch, _ = replay.sample_batch_arrays()
  # the step-by-step W1 search of the sampled observations (position 0 of the unroll is the sampled step itself)
  eng.set_weights(w1)
  obs = batch['obs'].reshape(-1, O)
  want = np.zeros((len(obs), A), np.float32)
  for at in range(0, len(obs), B):
    m = min(B, len(obs) - at)
    o, tp, lg = np.zeros((B, O), np.float32), np.ones(B, np.int8), np.ones((B, A), np.uint8)
    o[:m] = obs[at:at + m]
    lg[:m] = obs[at:at + m] == 0
    # the mover: the stones on the board are the mover's +1 and the other's -1; player +1 moves on an even number of stones
    tp[:m] = np.where((obs[at:at + m] != 0).sum(1) % 2 == 0, 1, -1)
    eng.initial_inference(o)
    eng.root_prepare(tp, lg, None, device_rng=False)
    eng.search()
    want[at:at + m] = eng.finalize(0.0, np.zeros(B))['child_visits'].cpu().numpy()[:m].astype(np.float32)
  assert np.array_equal(batch['t_pol'][:, 0].view(np.uint32), want.view(np.uint32))
  now = replay.reanalyse_pick(4096)
  replay.reanalyse_release(now['ticket'])
  assert now['n_rows'] == stale['n_rows'] == out['rows']
  assert np.array_equal(now['rows'][:, :O], stale_rows[:, :O]) and np.array_equal(now['rows'][:, O + A + 2:].view(np.uint32), stale_rows[:, O + A + 2:].view(np.uint32))
  assert not np.array_equal(now['rows'][:, O:O + A + 2], stale_rows[:, O:O + A + 2])
  # a second pass with the same weights changes nothing
  again = re.run(4096)
  assert again['rows'] == out['rows'] and again['mean_abs_value_change'] == 0 and again['mean_policy_l1'] == 0
  assert not out['busy'] and not again['busy']
  # a second Reanalyser on the same replay (several actors share one): while the first one's ticket is out its pass is skipped,
  # not failed, and nothing is written; afterwards it runs
  other = Reanalyser(cfg, replay, max_rows=4096)
  other.set_weights(w0)
  held = replay.reanalyse_pick(4096)
  skipped = other.run(4096)
  assert skipped['busy'] and skipped['rows'] == 0 and skipped['slices'] == 0
  assert replay.reanalyse_write(held['ticket'], re.fresh[:held['n_rows']])['rows'] == held['n_rows']      # (the holder is unharmed)
  back = other.run(4096)
  assert not back['busy'] and back['rows'] == out['rows'] and back['mean_policy_l1'] > 0
  other.close(); re.close(); eng.close()


def test_train_creates_a_reanalyser_only_when_asked(tmp_path, monkeypatch):
  import torch
  from model_based_rl_amd import reanalyse
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.logger import read_metrics
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  made = []
  real = reanalyse.Reanalyser

  class Counting(real):
    def __init__(self, *a, **k):
      made.append(1)
      real.__init__(self, *a, **k)
  monkeypatch.setattr(reanalyse, 'Reanalyser', Counting)
  runs = {}
  for rows in (0, 2048):
    cfg = ttt_config(tmp_path / str(rows), '--reanalyse_rows', str(rows), '--reanalyse_every', '1', '--weight_sync_frequency', '16')
    storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
    storage.store_weights(weights(9, 9, 7), 5)            # (training step 5: past a multiple of --reanalyse_every at every pull)
    actor = Actor(0, cfg, storage, replay)
    actor.launch(max_moves=32)
    runs[rows] = (actor.reanalyse_runs, len(made), replay.get_throughput())
    if rows:
      assert actor.reanalyser is not None and actor.last_reanalyse['rows'] > 0 and actor.reanalyse_skipped == 0
      # another actor's pass holds the shared replay's ticket at the next pull: this actor leaves its pass out and plays on
      held = replay.reanalyse_pick(64)
      assert held['ticket']
      storage.store_weights(weights(9, 9, 8), 9)
      actor.launch(max_moves=16)
      assert actor.reanalyse_skipped == 1 and actor.reanalyse_runs == runs[rows][0] and actor.last_reanalyse['busy']
      assert actor.move_counter == 48 and actor.training_step == 9
      replay.reanalyse_release(held['ticket'])
      m = read_metrics(os.path.join(actor.dirs['worker'], 'metrics.csv'))
      assert len(m['reanalyse/rows']) == actor.reanalyse_runs and 'reanalyse/mean_policy_l1' in m
      actor.reanalyser.close()
    else:
      assert actor.reanalyser is None
    actor.close(); actor.engine.close()
    torch.cuda.synchronize()
  assert runs[0][:2] == (0, 0) and runs[2048][0] >= 1 and runs[2048][1] == 1
  assert runs[0][2] == runs[2048][2]                      # the same games reached the replay either way


def test_train_main_with_the_flag_off_makes_no_reanalyser(tmp_path, monkeypatch):
  """the whole driver: train.main with --reanalyse_rows 0 (spelled out, and left to its default) plays and ingests, and no
  Reanalyser is ever constructed"""
  from model_based_rl_amd import reanalyse, train
  made = []
  real = reanalyse.Reanalyser

  class Counting(real):
    def __init__(self, *a, **k):
      made.append(1)
      real.__init__(self, *a, **k)
  monkeypatch.setattr(reanalyse, 'Reanalyser', Counting)
  base = ENV_FLAGS['TicTacToe'] + ['--num_envs', str(B), '--num_simulations', '8', '--seed', '5', '--window_size', '4096',
                                   '--weight_sync_frequency', '16', '--selfplay_only', '--max_moves', '32']
  got = []
  for i, extra in enumerate((['--reanalyse_rows', '0'], [])):
    thr = train.main(base + extra + ['--runs_dir', str(tmp_path / ('runs%d' % i)), '--run_tag', 'r'])
    assert thr['frames'] > 0 and thr['games'] > 0
    got.append((thr['frames'], thr['games']))
  assert made == [] and got[0] == got[1]
