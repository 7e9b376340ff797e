"""Self-play on the device games searched with the Gumbel search (mz_selfplay_set_gumbel; csrc/mz_gumbel_selfplay.hip.h; DESIGN
s7i).  The records of the device loop against a second engine driven move by move from Python over the host games of envs.py --
the same kernels on the same inputs under the same RNG key, so the int32 views of whole records are EQUAL --; the captured graph
against direct launches; a game's records in two batches; the mode switched off; the actor and the learner on pi' targets; the
refusals.  B = 40 environments (three 16-tree workgroups, the last one padded), random FCNetwork weights."""
import os

import numpy as np
import pytest

from tests.parity_util import random_weights

pytestmark = pytest.mark.gpu
B, SEED = 40, 123
GUMBEL = dict(max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=1.0)
TWO = dict(two_players=True, known_bounds=(-1.0, 1.0), discount=1.0)
# game -> (selfplay_set_env's name, O, A, engine arguments, weight seed, simulations, moves, selfplay_reset's episode_len)
GAMES = {'tictactoe': ('tictactoe', 9, 9, TWO, 3, 8, 20, 9),            # A = 9 > 8 simulations: halving stays in its zero-visit phase
         'connect_four': ('connect_four', 42, 7, TWO, 2, 16, 48, 42),   # m = 7: halving runs
         'cartpole': ('cartpole', 4, 2, {}, 1, 8, 32, 12)}              # m = 2; the time limit of 12 resets beside termination


def make_engine(game, batch=B, env_id_offset=0, gumbel=True, value='mean'):
  from model_based_rl_amd.engine import Engine
  name, O, A, kw, wseed, sims, _, _ = GAMES[game]
  eng = Engine(batch, O, A, sims, seed=SEED, env_id_offset=env_id_offset, **kw)
  eng.set_weights(random_weights(O, A, wseed))
  eng.selfplay_set_env(name)
  if gumbel:
    eng.set_gumbel(True, **GUMBEL)
    eng.selfplay_set_gumbel(True, value)
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


def host_games(game, eng, episode_len):
  from model_based_rl_amd import envs
  if game == 'cartpole':
    hosts = [envs.CartPole(episode_len) for _ in range(eng.B)]
    for b, h in enumerate(hosts):
      h.reset()
      h.set_state(eng.cartpole_reset_state(b, 0))
    return hosts
  return [envs.TicTacToe() if game == 'tictactoe' else envs.ConnectFour() for _ in range(eng.B)]


def twin_records(game, moves, value):
  """the expected records: a second engine of the same weights and seed drives host games move by move -- initial_inference on
  the host observation, root_prepare without noise, gz_root(move), gz_search, gz_pick, finalize -- and every record is assembled
  here.  Returns (records [moves, B, rec] float32, games finished per environment, ends by the time limit alone)."""
  name, O, A, kw, wseed, sims, _, episode_len = GAMES[game]
  eng = make_engine(game, gumbel=False)
  eng.set_gumbel(True, **GUMBEL)
  hosts = host_games(game, eng, episode_len)
  cart = game == 'cartpole'
  rec = np.zeros((moves, B, O + A + 10), np.float32)
  episode, finished, by_limit = np.zeros(B, np.int64), np.zeros(B, np.int64), 0
  for m in range(moves):
    if cart:
      obs = np.stack([h._obs() for h in hosts])
      turn = np.ones(B, np.int64)
      legal = np.ones((B, A), bool)
      eng.initial_inference(obs)
      eng.root_prepare(None, None, None, device_rng=False)
    else:
      turn = np.array([h.turn for h in hosts], np.int64)
      obs = np.stack([(h.turn * h.board).astype(np.float32) for h in hosts])
      legal = np.zeros((B, A), bool)
      for b, h in enumerate(hosts):
        legal[b, h.legal_actions()] = True
      eng.initial_inference(obs)
      eng.root_prepare(turn.astype(np.int8), legal.astype(np.uint8), None, device_rng=False)
    v0 = eng.root_outputs()[0].cpu().numpy().astype(np.float64)
    eng.gz_root(None, move=m)
    eng.gz_search(sims)
    action, _, pi, vmix = [x.cpu().numpy() for x in eng.gz_pick()]
    fin = eng.finalize(0.0, np.full(B, 0.5), move=m)
    root_value = vmix if value == 'vmix' else fin['root_value'].cpu().numpy()
    error = root_value - v0
    if value == 'mean':
      assert np.array_equal(error, fin['error'].cpu().numpy())
    ints = rec[m].view(np.int32)
    rec[m, :, :O] = obs
    rec[m, :, O:O + A] = pi.astype(np.float32)
    rec[m, :, O + A:O + A + 2] = np.ascontiguousarray(root_value).view(np.float32).reshape(B, 2)
    rec[m, :, O + A + 2:O + A + 4] = np.ascontiguousarray(error).view(np.float32).reshape(B, 2)
    for b, h in enumerate(hosts):
      assert legal[b, action[b]], (m, b, 'the pick is a legal action')
      step = h._elapsed_steps
      _, reward, done, _ = h.step(int(action[b]))
      rec[m, b, O + A + 4] = np.float32(reward)
      ints[b, O + A + 5:] = (action[b], int(done) | (2 if turn[b] < 0 else 0), step, b, episode[b])
      if done:
        if cart:
          x, _, th, _ = h.state
          by_limit += int(abs(x) <= h.X_THRESHOLD and abs(th) <= h.THETA_THRESHOLD)
        episode[b] += 1
        finished[b] += 1
        h.reset()
        if cart:
          h.set_state(eng.cartpole_reset_state(b, int(episode[b])))
  eng.close()
  return rec, finished, by_limit


CASES = [('tictactoe', 'mean'), ('tictactoe', 'vmix'), ('connect_four', 'mean'), ('cartpole', 'mean')]


@pytest.mark.parametrize('game,value', CASES)
def test_records_equal_a_python_driven_loop(game, value):
  from model_based_rl_amd.engine import records_view
  name, O, A, kw, wseed, sims, moves, episode_len = GAMES[game]
  eng = make_engine(game, value=value)
  assert eng.selfplay_moves_per_launch() == 0
  rec = play_ring(eng, moves, episode_len)
  eng.close()
  want, finished, by_limit = twin_records(game, moves, value)
  rv = records_view(rec, O, A)
  pi = rv['child_visits']
  legal = {'tictactoe': lambda o: o == 0, 'connect_four': lambda o: o[..., 35:42] == 0, 'cartpole': lambda o: np.ones(o.shape[:-1] + (A,), bool)}[game](rv['obs'])
  assert np.all(pi[~legal] == 0), 'pi\' is exactly 0 on illegal actions'
  assert np.all(pi >= 0) and np.abs(pi.sum(-1, dtype=np.float32) - np.float32(1)).max() <= 1e-6, np.abs(pi.sum(-1, dtype=np.float32) - 1).max()
  assert np.all(np.take_along_axis(legal, rv['action'][..., None].astype(np.int64), -1)), 'the action is legal'
  same = rec.view(np.int32) == want.view(np.int32)
  assert np.array_equal(rec.view(np.int32), want.view(np.int32)), ('first difference (move, env, slot)', np.argwhere(~same)[:4].tolist())
  print('%s %s: %d moves, %d..%d games finished per environment, %d ends by the time limit'
        % (game, value, moves, finished.min(), finished.max(), by_limit))
  assert finished.min() >= (2 if game == 'tictactoe' else 1)      # the reset path ran in every environment
  if game == 'cartpole':
    assert by_limit >= 1 and by_limit < finished.sum()             # both the time limit and termination reset
  if game != 'cartpole':
    assert set(np.unique(rv['to_play'])) == {-1, 1}
  if value == 'vmix':      # (and the setting did something: v_mix is not the mean value)
    mean_run, _, _ = twin_records(game, 2, 'mean')
    assert not np.array_equal(mean_run.view(np.int32), want[:2].view(np.int32))


def test_graph_and_direct_forms_agree():
  """two graph launches of 16 moves (the second a replay of the captured graph) against 32 direct launches on a fresh engine: a
  draw frozen into the graph would repeat move 0's noise"""
  from model_based_rl_amd.engine import records_view
  a = make_engine('tictactoe')
  ring = play_ring(a, 32, 9)
  a.close()
  b = make_engine('tictactoe')
  direct = play_direct(b, 32, 9)
  b.close()
  assert np.array_equal(ring.view(np.int32), direct.view(np.int32))
  rv = records_view(ring, 9, 9)
  fresh = (rv['step'][0] == 0) & (rv['step'][16] == 0)      # empty boards at move 0 and at move 16: the same observation, other noise
  assert fresh.sum() == 0 or not np.array_equal(rv['child_visits'][0][fresh], rv['child_visits'][16][fresh])


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


@pytest.mark.parametrize('game', ['tictactoe', 'cartpole'])
def test_mode_off_is_the_parents_form(game):
  episode_len = GAMES[game][7]
  plain = make_engine(game, gumbel=False)
  mpl = plain.selfplay_moves_per_launch()
  want = play_ring(plain, 16, episode_len)
  plain.close()
  eng = make_engine(game)
  assert eng.selfplay_moves_per_launch() == 0
  if game == 'cartpole':      # (this shape and weight set play whole moves, tests/test_gpu_cartpole.py: the plan really comes back)
    assert mpl == 16
  play_ring(eng, 16, episode_len)
  eng.selfplay_set_gumbel(False)
  assert eng.selfplay_moves_per_launch() == mpl
  got = play_ring(eng, 16, episode_len)
  eng.close()
  assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_actor_and_learner_on_improved_policy_targets(tmp_path):
  """an Actor built as train builds it plays 32 moves of 64 TicTacToe environments into the replay; a sampled batch's policy
  targets are pi'; 1 + 20 updates of the native learner step give finite losses and a lower policy loss"""
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import records_view
  from model_based_rl_amd.learners import Learner
  from model_based_rl_amd.logger import read_metrics
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  from model_based_rl_amd.train import refuse_selfplay_gumbel
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--known_bounds', '-1', '1', '--discount', '1', '--td_steps', '10',
                     '--num_envs', '64', '--num_simulations', '8', '--selfplay_gumbel', '--seed', '5', '--window_size', '16384',
                     '--batch_size', '128', '--stored_before_train', '256', '--training_steps', '21', '--learner_log_frequency', '1',
                     '--send_weights_frequency', '1000', '--save_state_frequency', '1000000', '--use_gpu_for', 'actors', 'learner',
                     '--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'r', '--actor_log_frequency', '1'])
  refuse_selfplay_gumbel(cfg, 1)
  torch.manual_seed(0)
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  learner = Learner(cfg, storage, replay)
  learner.send_weights()
  actor = Actor(0, cfg, storage, replay)
  assert not actor.host_env
  seen = []
  actor.record_tap = lambda v: seen.append(v.copy())
  actor.launch(max_moves=32)
  assert actor.engine.selfplay_gumbel and actor.engine.selfplay_moves_per_launch() == 0
  rv = records_view(np.concatenate(seen, 0), 9, 9)
  assert rv['done'].shape == (32, 64) and actor.games_played == int(rv['done'].sum()) > 64
  assert np.all(rv['child_visits'][rv['obs'] != 0] == 0) and np.abs(rv['child_visits'].sum(-1) - 1).max() <= 1e-6
  assert np.any((rv['child_visits'] * 8) % 1 != 0), 'the policy slots are not visit shares of 8 simulations'
  host, _ = replay.sample_batch_arrays()
  obs, t_pol = np.asarray(host['obs']).reshape(128, 9), np.asarray(host['t_pol'])
  root = t_pol[:, 0]
  assert np.abs(root.sum(-1) - 1).max() <= 1e-6 and np.all(root[obs != 0] == 0), 'the root policy target is pi\' of the row\'s position'
  sums = t_pol.sum(-1)      # (unroll steps past the end of a game carry the replay's own filler: a distribution or nothing)
  assert np.all((np.abs(sums - 1) <= 1e-6) | (sums == 0))
  learner.launch(max_steps=21)
  assert learner.training_step == 21 and learner._native is not None
  m = read_metrics(os.path.join(learner.dirs['worker'], 'metrics.csv'))
  policy = [v for _, v in m['loss/policy']]
  print('policy loss per update', ['%.4f' % v for v in policy])
  assert len(policy) == 21
  for k in ('reward', 'value', 'policy'):
    assert np.all(np.isfinite([v for _, v in m['loss/' + k]])), k
  assert policy[-1] < policy[0]
  actor.close(); actor.engine.close()


def test_engine_refusals():
  import torch
  from model_based_rl_amd.engine import Engine
  eng = Engine(B, 9, 9, 8, seed=SEED, **TWO)
  eng.set_weights(random_weights(9, 9, 3))
  with pytest.raises(RuntimeError, match=r'mz_selfplay_set_gumbel: no Gumbel search is set on this engine \(call mz_set_gumbel first\)'):
    eng.selfplay_set_gumbel(True)
  eng.set_gumbel(True, **GUMBEL)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_gumbel: the Gumbel self-play runs on the device games; set one first'):
    eng.selfplay_set_gumbel(True)
  with pytest.raises(ValueError, match="value is 'mean' or 'vmix'"):
    eng.selfplay_set_gumbel(True, 'median')
  eng.selfplay_set_env('tictactoe')
  eng.selfplay_reset(9, 1.0)
  eng.selfplay_set_draws(uniform=np.full(B, 0.5))
  with pytest.raises(RuntimeError, match=r'mz_selfplay_set_gumbel: host-given draws are set \(mz_selfplay_set_draws\)'):
    eng.selfplay_set_gumbel(True)
  eng.selfplay_set_draws()
  eng.sim_io('log', keep_moves=1)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_gumbel: mz_sim_io instruments the fused search kernels'):
    eng.selfplay_set_gumbel(True)
  eng.sim_io('off')
  eng.selfplay_steps(2)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_gumbel: 2 moves wait in the device ring; drain them first'):
    eng.selfplay_set_gumbel(True)
  eng.selfplay_drain()
  torch.cuda.synchronize()
  eng.selfplay_set_gumbel(True)
  # the neighbouring entries while the mode is on
  with pytest.raises(RuntimeError, match=r'mz_set_gumbel: the self-play loop searches with the Gumbel search on this engine \(mz_selfplay_set_gumbel 0 first\)'):
    eng.set_gumbel(False)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_draws: the self-play moves are searched with the Gumbel search'):
    eng.selfplay_set_draws(uniform=np.full(B, 0.5))
  with pytest.raises(RuntimeError, match='mz_selfplay_set_env: the self-play moves are searched with the Gumbel search'):
    eng.selfplay_set_env('synthetic')
  with pytest.raises(RuntimeError, match='mz_sim_io: the self-play moves are searched with the Gumbel search'):
    eng.sim_io('log', keep_moves=1)
  with pytest.raises(RuntimeError, match='mz_selfplay_steps_timed: the moves are searched with the Gumbel search'):
    eng.selfplay_steps_timed(1)
  eng.selfplay_steps(1)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_gumbel: 1 moves wait in the device ring; drain them first'):
    eng.selfplay_set_gumbel(False)
  eng.selfplay_drain()
  torch.cuda.synchronize()
  eng.selfplay_set_gumbel(False)
  eng.set_gumbel(False)      # ... and off again in the other order
  eng.close()
