"""Self-play on the device board games searched on the true rules (mz_selfplay_set_true_model; csrc/mz_truemodel.hip.h; DESIGN
s7k).  The records of the device loop against a second engine driven move by move from Python over the host games of envs.py --
initial_inference, root_prepare with the device's Dirichlet draw, tm_root, tm_search, finalize: the same kernels on the same
inputs under the same RNG keys, so the int32 views of whole records are EQUAL --, with the move's simulations in one launch and in
the two-launch loop; the captured graph against direct launches; a game's records in two batches; the mode switched off; the actor
and the learner; one engine through all three modes of the loop (DESIGN s7l); the refusals.  B = 40 environments (three 16-tree workgroups, the last one padded), random FCNetwork weights."""
import functools
import os

import numpy as np
import pytest

from tests.parity_util import random_weights

pytestmark = pytest.mark.gpu
B, SEED = 40, 123
TWO = dict(two_players=True, known_bounds=(-1.0, 1.0), discount=1.0)
# game -> (selfplay_set_env's name, true-model kind, O, A, weight seed, simulations, moves, selfplay_reset's episode_len)
GAMES = {'tictactoe': ('tictactoe', 1, 9, 9, 3, 12, 20, 9),             # 20 moves: every environment finishes two games
         'connect_four': ('connect_four', 3, 42, 7, 2, 16, 48, 42)}


def make_engine(game, batch=B, env_id_offset=0, mode=True, fused=True):
  from model_based_rl_amd.engine import Engine
  name, kind, O, A, wseed, sims, _, _ = GAMES[game]
  eng = Engine(batch, O, A, sims, seed=SEED, env_id_offset=env_id_offset, **TWO)
  eng.set_weights(random_weights(O, A, wseed))
  eng.selfplay_set_env(name)
  if mode:
    eng.set_true_model(kind)
    eng.selfplay_set_true_model(True, fused=fused)
  return eng


def play_ring(eng, moves, episode_len, chunk=16):
  """`moves` moves through the device ring in launches of at most `chunk` (selfplay_steps: the hipGraph path) -> records"""
  import torch
  eng.selfplay_reset(episode_len, 1.0)
  recs = []
  for done in range(0, moves, chunk):
    k = min(chunk, moves - done)
    eng.selfplay_steps(k)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == k
    recs.append(buf[:n].numpy().copy())
  return np.concatenate(recs, 0)


def play_direct(eng, moves, episode_len):
  """`moves` moves straight into a pinned buffer (selfplay_steps_into: direct launches, no graph) -> records"""
  import torch
  eng.selfplay_reset(episode_len, 1.0)
  out = torch.zeros(moves, eng.B, eng.rec_floats, dtype=torch.float32).pin_memory()
  eng.selfplay_steps_into(out, moves)
  torch.cuda.synchronize()
  return out.numpy().copy()


@functools.lru_cache(maxsize=None)
def twin_records(game):
  """the expected records: a second engine of the same weights and seed drives host games move by move and every record is
  assembled here.  Returns (records [moves, B, rec] float32, games finished per environment)."""
  from model_based_rl_amd import envs
  name, kind, O, A, wseed, sims, moves, _ = GAMES[game]
  eng = make_engine(game, mode=False)
  eng.set_true_model(kind)
  hosts = [envs.TicTacToe() if game == 'tictactoe' else envs.ConnectFour() for _ in range(B)]
  rec = np.zeros((moves, B, O + A + 10), np.float32)
  episode, finished = np.zeros(B, np.int64), np.zeros(B, np.int64)
  for m in range(moves):
    turn = np.array([h.turn for h in hosts], np.int8)
    obs = np.stack([(h.turn * h.board).astype(np.float32) for h in hosts])
    boards = np.zeros((B, 42), np.int8)
    legal = np.zeros((B, A), np.uint8)
    for b, h in enumerate(hosts):
      legal[b, h.legal_actions()] = 1
      boards[b, :O] = np.asarray(h.board).reshape(-1)
    steps = np.array([h._elapsed_steps for h in hosts], np.int32)
    eng.initial_inference(obs)
    eng.root_prepare(turn, legal, None, device_rng=True, move=m)
    eng.tm_root(boards, turn, steps)
    eng.tm_search(sims)
    fin = {k: v.cpu().numpy() for k, v in eng.finalize(1.0, None, move=m).items()}
    ints = rec[m].view(np.int32)
    rec[m, :, :O] = obs
    rec[m, :, O:O + A] = fin['child_visits'].astype(np.float32)
    rec[m, :, O + A:O + A + 2] = np.ascontiguousarray(fin['root_value']).view(np.float32).reshape(B, 2)
    rec[m, :, O + A + 2:O + A + 4] = np.ascontiguousarray(fin['error']).view(np.float32).reshape(B, 2)
    for b, h in enumerate(hosts):
      a = int(fin['action'][b])
      assert legal[b, a], (m, b, 'the action is legal')
      _, reward, done, _ = h.step(a)
      rec[m, b, O + A + 4] = np.float32(reward)
      ints[b, O + A + 5:] = (a, int(done) | (2 if turn[b] < 0 else 0), steps[b], b, episode[b])
      if done:
        episode[b] += 1
        finished[b] += 1
        h.reset()
  eng.close()
  return rec, finished


@pytest.mark.parametrize('game', ['tictactoe', 'connect_four'])
def test_records_equal_a_python_driven_loop(game):
  from model_based_rl_amd.engine import records_view
  name, kind, O, A, wseed, sims, moves, episode_len = GAMES[game]
  want, finished = twin_records(game)
  got = {}
  for fused in (True, False):
    eng = make_engine(game, fused=fused)
    assert eng.selfplay_moves_per_launch() == 0
    got[fused] = play_ring(eng, moves, episode_len)
    eng.close()
    same = got[fused].view(np.int32) == want.view(np.int32)
    assert np.array_equal(got[fused].view(np.int32), want.view(np.int32)), (fused, 'first difference (move, env, slot)', np.argwhere(~same)[:4].tolist())
  assert np.array_equal(got[True].view(np.int32), got[False].view(np.int32))
  rv = records_view(got[True], O, A)
  legal = (rv['obs'] == 0) if game == 'tictactoe' else (rv['obs'][..., 35:42] == 0)
  assert np.all(rv['child_visits'][~legal] == 0) and np.abs(rv['child_visits'] * sims - np.rint(rv['child_visits'] * sims)).max() < 1e-5, 'visit shares over the legal actions'
  print('%s: %d moves, %d..%d games finished per environment' % (game, moves, finished.min(), finished.max()))
  assert finished.min() >= (2 if game == 'tictactoe' else 1)      # the reset path ran in every environment
  assert set(np.unique(rv['to_play'])) == {-1, 1}


def test_graph_and_direct_forms_agree():
  """two graph launches of 16 moves (the second a replay of the captured graph) against 32 direct launches on a fresh engine: a
  draw or a position frozen into the graph would repeat move 0's"""
  from model_based_rl_amd.engine import records_view
  a = make_engine('tictactoe')
  ring = play_ring(a, 32, 9)
  a.close()
  b = make_engine('tictactoe')
  direct = play_direct(b, 32, 9)
  b.close()
  assert np.array_equal(ring.view(np.int32), direct.view(np.int32))
  rv = records_view(ring, 9, 9)
  assert rv['done'].sum(0).min() >= 3 and not np.array_equal(ring[:16].view(np.int32), ring[16:].view(np.int32))


def test_batch_independence():
  full = make_engine('tictactoe', batch=32)
  a = play_ring(full, 20, 9)
  full.close()
  part = make_engine('tictactoe', batch=16, env_id_offset=16)
  b = play_ring(part, 20, 9)
  part.close()
  assert a.shape[1] == 32 and b.shape[1] == 16
  assert np.array_equal(a[:, 16:32].view(np.int32), b.view(np.int32))
  assert not np.array_equal(a[:, 0:16, 9:18], b[:, :, 9:18])      # (other environments draw other noise)


@pytest.mark.parametrize('game', ['tictactoe', 'connect_four'])
def test_mode_off_is_the_parents_form(game):
  episode_len = GAMES[game][7]
  plain = make_engine(game, mode=False)
  mpl = plain.selfplay_moves_per_launch()
  want = play_ring(plain, 16, episode_len)
  plain.close()
  eng = make_engine(game)
  assert eng.selfplay_moves_per_launch() == 0
  on = play_ring(eng, 16, episode_len)
  eng.selfplay_set_true_model(False)
  assert eng.selfplay_moves_per_launch() == mpl
  got = play_ring(eng, 16, episode_len)
  eng.close()
  assert np.array_equal(got.view(np.int32), want.view(np.int32))
  assert not np.array_equal(on.view(np.int32), want.view(np.int32))      # (and the mode did something)


def test_actor_and_learner(tmp_path):
  """an Actor built as train builds it plays 32 moves of 64 TicTacToe environments into the replay; 21 updates of the native
  learner step give finite losses and a lower policy loss.

  Lower on WHAT: the loss an update logs is mean(w * loss) over its own prioritized batch, w the batch's importance weights
  normalised by their maximum (Learner._finish_step).  Two updates' logged figures therefore differ by their batches' weight
  scale before they differ by anything the network learned: measured on an MI355X, the logged policy loss of this run swings
  between 0.31 and 2.06 from one update to the next (0.514 at the first, 1.236 at the 21st), and the same run WITHOUT
  --selfplay_true_model swings between 0.52 and 2.10, so last-against-first of that series is a coin toss about the sampler on
  either path.  The policy loss is compared where the batch does not change: one batch drawn from the replay before the updates,
  every sample weighted 1, put through the learner's own loss (Learner._device_step_fc: the K-step unroll and the soft
  cross-entropy of the update, no optimiser step) before the 21 updates and after them.  Strictly lower, no tolerance."""
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import records_view
  from model_based_rl_amd.learners import Learner, _GraphedUpdate
  from model_based_rl_amd.logger import read_metrics
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  from model_based_rl_amd.train import refuse_selfplay_true_model
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--known_bounds', '-1', '1', '--discount', '1', '--td_steps', '10',
                     '--num_envs', '64', '--num_simulations', '12', '--selfplay_true_model', '--seed', '5', '--window_size', '16384',
                     '--batch_size', '128', '--stored_before_train', '256', '--training_steps', '21', '--learner_log_frequency', '1',
                     '--send_weights_frequency', '1000', '--save_state_frequency', '1000000', '--use_gpu_for', 'actors', 'learner',
                     '--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'r', '--actor_log_frequency', '1'])
  refuse_selfplay_true_model(cfg, 1)
  torch.manual_seed(0)
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  learner = Learner(cfg, storage, replay)
  learner.send_weights()
  actor = Actor(0, cfg, storage, replay)
  assert not actor.host_env
  seen = []
  actor.record_tap = lambda v: seen.append(v.copy())
  actor.launch(max_moves=32)
  assert actor.engine.selfplay_true_model and actor.engine.true_model == 1 and actor.engine.selfplay_moves_per_launch() == 0
  rv = records_view(np.concatenate(seen, 0), 9, 9)
  assert rv['done'].shape == (32, 64) and actor.games_played == int(rv['done'].sum()) > 64
  assert np.all(rv['child_visits'][rv['obs'] != 0] == 0) and np.abs(rv['child_visits'] * 12 - np.rint(rv['child_visits'] * 12)).max() < 1e-5
  host, _ = replay.sample_batch_arrays()      # the fixed batch: 128 stored positions with their unrolled targets
  root = np.asarray(host['t_pol'])[:, 0]
  assert np.abs(root.sum(-1) - 1).max() <= 1e-6 and np.all(root[np.asarray(host['obs']).reshape(128, 9) != 0] == 0)
  fixed = {k: torch.from_numpy(np.ascontiguousarray(host[k])).to(learner.device) for k in _GraphedUpdate.ORDER}
  fixed['act'], fixed['w'] = fixed['act'].to(torch.int64), torch.ones_like(fixed['w'])

  def fixed_batch_losses():
    _, reward, value, policy = learner._device_step_fc(*[fixed[k] for k in _GraphedUpdate.ORDER])
    return {k: float(v.detach().mean()) for k, v in (('reward', reward), ('value', value), ('policy', policy))}
  before = fixed_batch_losses()
  learner.launch(max_steps=21)
  assert learner.training_step == 21 and learner._native is not None
  after = fixed_batch_losses()
  m = read_metrics(os.path.join(learner.dirs['worker'], 'metrics.csv'))
  policy = [v for _, v in m['loss/policy']]
  print('policy loss logged per update', ['%.4f' % v for v in policy])
  print('the fixed batch before', before, 'and after the 21 updates', after)
  assert len(policy) == 21
  for k in ('reward', 'value', 'policy'):
    assert np.all(np.isfinite([v for _, v in m['loss/' + k]])), k
    assert np.isfinite(before[k]) and np.isfinite(after[k]), k
  actor.close(); actor.engine.close()
  assert after['policy'] < before['policy']


def test_one_engine_through_the_modes():
  """One TicTacToe engine of 16 environments (one workgroup's trees) at 30 simulations goes PUCT -> Gumbel -> off -> true rules (one
  launch per move) -> off -> Gumbel, its ring drained between the switches, and plays 4 moves of fresh games in each: every
  segment's records EQUAL those of an engine that was only ever in that mode and was given the same move counter (what keys the
  draws).  While the true rules are on, switching the Gumbel mode off succeeds and leaves them on."""
  import torch
  from model_based_rl_amd.engine import Engine
  gumbel = dict(max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=1.0)

  def engine():
    eng = Engine(16, 9, 9, 30, seed=SEED, **TWO)
    eng.set_weights(random_weights(9, 9, 3))
    eng.selfplay_set_env('tictactoe')
    return eng

  def segment(eng, index):      # 4 moves of fresh games under the move counter of the index-th segment
    eng.selfplay_reset(9, 1.0)
    eng.selfplay_set_moves(4 * index)
    eng.selfplay_steps(4)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == 4
    return buf[:n].numpy().copy().view(np.int32)

  def to_gumbel(eng):
    eng.set_gumbel(True, **gumbel)
    eng.selfplay_set_gumbel(True)

  def to_true_rules(eng):
    eng.set_true_model(1)
    eng.selfplay_set_true_model(True)

  def gumbel_off(eng):
    eng.selfplay_set_gumbel(False)
    eng.set_gumbel(False)      # (an engine takes the Gumbel search or the true-rules search)

  def true_rules_off(eng):
    eng.selfplay_set_true_model(False)
    eng.set_true_model(0)

  # (the switch before the segment, the mode it plays in)
  walk = ((None, 'puct'), (to_gumbel, 'gumbel'), (gumbel_off, 'puct'), (to_true_rules, 'true_rules'),
          (lambda eng: eng.selfplay_set_gumbel(False), 'true_rules'),      # off of the mode that is not on: the true rules stay
          (true_rules_off, 'puct'), (to_gumbel, 'gumbel'))
  eng = engine()
  whole_moves = eng.selfplay_moves_per_launch()
  got = []
  for index, (switch, mode) in enumerate(walk):
    if switch:
      switch(eng)
    assert eng.selfplay_search == mode and (eng.selfplay_gumbel, eng.selfplay_true_model) == (mode == 'gumbel', mode == 'true_rules')
    assert eng.selfplay_moves_per_launch() == (whole_moves if mode == 'puct' else 0)
    got.append(segment(eng, index))
  eng.close()
  for mode, enter in (('puct', None), ('gumbel', to_gumbel), ('true_rules', to_true_rules)):
    only = engine()
    if enter:
      enter(only)
    for index, (_, m) in enumerate(walk):
      want = segment(only, index)
      same = np.array_equal(got[index], want)
      assert same == (m == mode), (mode, index, m)      # (and at one counter the three modes leave different records)
    only.close()


def test_engine_refusals():
  import torch
  from model_based_rl_amd.engine import Engine
  eng = Engine(B, 9, 9, 12, seed=SEED, **TWO)
  eng.set_weights(random_weights(9, 9, 3))
  eng.set_true_model(1)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_true_model: the true-rules self-play runs on the device board games; set one first'):
    eng.selfplay_set_true_model(True)
  eng.set_true_model(0)
  eng.selfplay_set_env('tictactoe')
  with pytest.raises(RuntimeError, match=r'mz_selfplay_set_true_model: the true-rules search of the environment\'s game is not set on this engine \(call mz_set_true_model 1 first\)'):
    eng.selfplay_set_true_model(True)
  eng.set_gumbel(True, max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=1.0)
  eng.selfplay_set_gumbel(True)
  with pytest.raises(RuntimeError, match=r'mz_selfplay_set_true_model: the self-play moves are searched with the Gumbel search \(mz_selfplay_set_gumbel 0 first\)'):
    eng.selfplay_set_true_model(True)
  eng.selfplay_set_gumbel(False)
  eng.set_gumbel(False)
  eng.set_true_model(1)
  eng.selfplay_reset(9, 1.0)
  eng.selfplay_set_draws(uniform=np.full(B, 0.5))
  with pytest.raises(RuntimeError, match=r'mz_selfplay_set_true_model: host-given draws are set \(mz_selfplay_set_draws\)'):
    eng.selfplay_set_true_model(True)
  eng.selfplay_set_draws()
  eng.sim_io('log', keep_moves=1)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_true_model: mz_sim_io instruments the fused search kernels'):
    eng.selfplay_set_true_model(True)
  eng.sim_io('off')
  eng.selfplay_steps(2)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_true_model: 2 moves wait in the device ring; drain them first'):
    eng.selfplay_set_true_model(True)
  eng.selfplay_drain()
  torch.cuda.synchronize()
  eng.selfplay_set_true_model(True, fused=False)
  eng.selfplay_set_true_model(True)      # (from the loop to the one-launch form while on)
  # the neighbouring entries while the mode is on
  with pytest.raises(RuntimeError, match=r'mz_set_true_model: the self-play loop searches the true rules of the current game on this engine \(mz_selfplay_set_true_model 0 first\)'):
    eng.set_true_model(0)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_draws: the self-play moves are searched on the true rules'):
    eng.selfplay_set_draws(uniform=np.full(B, 0.5))
  with pytest.raises(RuntimeError, match='mz_selfplay_set_env: the self-play moves are searched on the true rules'):
    eng.selfplay_set_env('synthetic')
  with pytest.raises(RuntimeError, match='mz_selfplay_set_gumbel: the self-play moves are searched on the true rules'):
    eng.selfplay_set_gumbel(True)
  with pytest.raises(RuntimeError, match='mz_sim_io: the self-play moves are searched on the true rules'):
    eng.sim_io('log', keep_moves=1)
  with pytest.raises(RuntimeError, match='mz_selfplay_steps_timed: the moves are searched on the true rules'):
    eng.selfplay_steps_timed(1)
  eng.selfplay_steps(1)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_true_model: 1 moves wait in the device ring; drain them first'):
    eng.selfplay_set_true_model(False)
  eng.selfplay_drain()
  torch.cuda.synchronize()
  eng.selfplay_set_true_model(False)
  eng.set_true_model(0)
  eng.close()
