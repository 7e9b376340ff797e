"""The device CartPole environment (mz_selfplay_set_env kind 2; csrc/mz_selfplay.hip.h) against its definition, the host
class envs.CartPole: bit for bit in the whole-moves launch (k_search_fused<14,1,4,1,..,SP,HEAD,GAME>, the state in LDS across
the 16 moves of a launch), in the launch-per-step form, with split-f16; the trees of the new instantiation against the oracle's
tree; the refusals; the actor and the evaluator on it.  B = 40 environments (three workgroups, the last one padded), 8
simulations, random FCNetwork weights everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.parity_util import env_switches, philox_action_uniform, random_weights, replay_move

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, O, A, SIMS, SEED = 40, 4, 2, 8, 77


def make_engine(split=False, no_persist=False):
  from model_based_rl_amd.engine import Engine
  with env_switches(MZ_NO_PERSIST='1' if no_persist else None):
    eng = Engine(B, O, A, SIMS, seed=SEED, split_f16=split)
  eng.selfplay_set_env('cartpole')
  eng.set_weights(random_weights(O, A, 1))
  return eng


def play(eng, launches, episode_len, chunk=16, states=None):
  """launches x chunk moves; returns (records [moves, B, rec] float32, final states [B, 4] float64)"""
  import torch
  eng.selfplay_reset(episode_len, 1.0)
  for env, st in (states or {}).items():
    eng.selfplay_set_env_state(env, st)
  recs = []
  for _ in range(launches):
    eng.selfplay_steps(chunk)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == chunk
    recs.append(buf[:n].numpy().copy())
  return np.concatenate(recs, 0), eng.selfplay_env_state()


def host_check(eng, rec, final, episode_len, states=None):
  """every environment's records against a host CartPole started from cartpole_reset_state(env, episode) at every episode
  start (or from `states`, where the test placed the first one) and driven by the records' actions: float32 observation BITS,
  reward, done flag, step and episode index at every move, and the float64 states at the end, exactly.
  Returns per environment the lengths of its finished episodes and whether an episode ended by the time limit alone."""
  from model_based_rl_amd.engine import records_view
  from model_based_rl_amd.envs import CartPole
  rv = records_view(rec, O, A)
  M = rec.shape[0]
  lengths, by_limit = [], 0
  for b in range(B):
    host = CartPole(episode_len)
    ep = 0
    host.reset()
    host.set_state((states or {}).get(b, eng.cartpole_reset_state(b, 0)))
    mine = []
    for m in range(M):
      assert np.array_equal(rv['obs'][m, b].view(np.int32), host._obs().view(np.int32)), (b, m, 'observation')
      assert rv['step'][m, b] == host._elapsed_steps and rv['episode'][m, b] == ep and rv['env_id'][m, b] == b, (b, m)
      _, reward, done, _ = host.step(int(rv['action'][m, b]))
      assert rv['reward'][m, b] == np.float32(reward) == 1.0 and bool(rv['done'][m, b]) == done, (b, m, 'reward / done')
      assert rv['to_play'][m, b] == 1
      if done:
        x, _, th, _ = host.state
        inside = abs(x) <= CartPole.X_THRESHOLD and abs(th) <= CartPole.THETA_THRESHOLD
        assert not inside or host._elapsed_steps == episode_len      # done inside the thresholds: only by the time limit
        by_limit += int(inside and rv['step'][m, b] == episode_len - 1)
        mine.append(host._elapsed_steps)
        ep += 1
        host.reset()
        host.set_state(eng.cartpole_reset_state(b, ep))
    assert np.array_equal(np.array(host.state).view(np.int64), final[b].view(np.int64)), (b, 'final state')
    lengths.append(mine)
  return lengths, by_limit


@pytest.fixture(scope='module')
def whole_moves_run():
  """64 moves as four whole-moves launches, episode_len 500 (shared, read-only)"""
  eng = make_engine()
  info, mpl = eng.search_kernel_info(), eng.selfplay_moves_per_launch()
  rec, final = play(eng, 4, 500)
  yield eng, rec, final, info, mpl
  eng.close()


def test_device_equals_host_bit_for_bit(whole_moves_run):
  eng, rec, final, info, mpl = whole_moves_run
  assert info == dict(kind='fused', lt=1, ks1=14, G=4) and mpl == 16, (info, mpl)
  lengths, _ = host_check(eng, rec, final, 500)
  finished = sum(1 for l in lengths if l)
  twice = sum(1 for l in lengths if len(l) >= 2)
  print('%d of %d environments finished an episode in 64 moves, %d finished two; mean length %.1f'
        % (finished, B, twice, np.mean([x for l in lengths for x in l])))
  assert finished >= 0.9 * B and twice >= 1


def test_reset_states_are_uniform_draws_of_env_and_episode(whole_moves_run):
  """cartpole_reset_state names every episode's start for the comparison above, so it is checked on its own: every
  component in [-0.05, 0.05), the four of a state different, a state a function of (env, episode) and of nothing else,
  different for every (env, episode), and spread like a uniform draw (mean 0 +- 5 standard errors, both halves of the range
  reached).  4000 states: standard error of a component's mean 0.1 / sqrt(12 * 4000) = 4.6e-4."""
  eng = whole_moves_run[0]
  st = np.array([[eng.cartpole_reset_state(e, k) for k in range(40)] for e in range(100)])
  assert st.shape == (100, 40, 4) and st.dtype == np.float64
  assert np.all(st >= -0.05) and np.all(st < 0.05)
  assert len(np.unique(st)) == st.size                      # no two components equal: the four differ, and so does every (env, episode)
  assert np.array_equal(st[7, 3], eng.cartpole_reset_state(7, 3)) and not np.array_equal(st[7, 3], st[3, 7])
  flat = st.reshape(-1, 4)
  assert np.all(np.abs(flat.mean(0)) < 5 * 0.1 / np.sqrt(12 * flat.shape[0]))
  assert np.all(flat.min(0) < -0.045) and np.all(flat.max(0) > 0.045)


def test_time_limit_inside_the_launch():
  eng = make_engine()
  assert eng.selfplay_moves_per_launch() == 16
  rec, final = play(eng, 4, 12)
  lengths, by_limit = host_check(eng, rec, final, 12)
  eng.close()
  assert max(x for l in lengths for x in l) <= 12
  print('%d episodes ended by the time limit alone (step index 11, state inside the thresholds)' % by_limit)
  assert by_limit >= 1


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_cartpole import make_engine, play
eng = make_engine(no_persist=True)      # (env_switches clears the MZ_* switches it is not given)
assert eng.selfplay_moves_per_launch() == 0, eng.selfplay_moves_per_launch()
rec, final = play(eng, 3, 500)
np.save(sys.argv[1], rec)
print('CHILD OK')
'''


def test_launch_per_step_form_gives_the_same_records(whole_moves_run, tmp_path):
  """MZ_NO_PERSIST=1 (read at mz_create; a fresh child process): observe, root, Dirichlet, tree root, search and
  k_cartpole_step_record as separate kernels produce the records of the whole-moves launch byte for byte over 48 moves"""
  eng, rec, final, info, mpl = whole_moves_run
  assert mpl == 16
  env = dict(os.environ)
  env['MZ_NO_PERSIST'] = '1'
  out = str(tmp_path / 'rec.npy')
  r = subprocess.run([sys.executable, '-c', CHILD % ROOT, out], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
  assert r.returncode == 0 and 'CHILD OK' in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
  other = np.load(out)
  assert other.shape == (48,) + rec.shape[1:]
  assert np.array_equal(other.view(np.int32), rec[:48].view(np.int32))


def test_trees_of_the_new_instantiation_vs_oracle():
  """16 moves of the 40 trees of the single-player game kernel replayed through the oracle's tree on the launch's own
  logged network outputs, Dirichlet draws and select_action uniforms: actions, visit distributions, visit counts (the
  exported trees of the last move) and root values exact, as in tests/test_gpu_fused_exact.py"""
  import torch
  from oracle import oracle as orc
  from model_based_rl_amd.engine import records_view
  eng = make_engine()
  assert eng.selfplay_moves_per_launch() == 16
  eng.selfplay_noise_log(True)
  eng.selfplay_export_trees(True)
  eng.selfplay_reset(500, 1.0)
  log = eng.sim_io('log', keep_moves=16)
  eng.selfplay_steps(16)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == 16
  rv = records_view(buf[:n].numpy().copy(), O, A)
  io_all = log.cpu().numpy()
  tree = eng.export_tree()
  cfg = orc.tree_cfg(A, SIMS)
  for m in range(16):
    noise = eng.selfplay_noise(m)
    u = philox_action_uniform(SEED, np.arange(B), m)
    ref = replay_move(cfg, B, A, SIMS, io_all[m], noise, 0.25, np.ones(B, np.int8), None, 1.0, u, want_tree=(m == 15))
    assert np.array_equal(rv['action'][m], ref['action']), (m, 'action')
    assert np.array_equal(rv['child_visits'][m], ref['child_visits'].astype(np.float32)), (m, 'visit distribution')
    vc = ref['visit_counts'].astype(np.float64)
    assert np.all(vc.sum(1) == SIMS) and np.array_equal(rv['child_visits'][m], (vc / vc.sum(1, keepdims=True)).astype(np.float32)), (m, 'visit counts')
    assert np.array_equal(rv['root_value'][m], ref['root_value']), (m, 'root value')
    assert np.array_equal(rv['error'][m], ref['root_value'] - ref['v0'].astype(np.float64)), (m, 'error')
    if ref['tree'] is not None:
      eo = ref['tree']
      EX = eo['EX'].astype(bool)
      assert np.array_equal(tree['EX'].astype(bool), EX)
      for k in ('N', 'E', 'TP', 'W'):
        assert np.array_equal(tree[k][EX], eo[k][EX]), k
      assert np.array_equal(tree['N'][:, 1:1 + A], ref['visit_counts'])      # the root's children
      assert np.array_equal(tree['R'].astype(np.float64)[EX], eo['R'][EX])
      assert np.array_equal(tree['minmax'], eo['minmax'])
      assert np.array_equal(tree['noise'], noise)
  eng.sim_io('off')
  eng.close()


def test_threshold_crossing_inside_a_launch():
  eng = make_engine()
  states = {0: (0.0, 0.0, 0.2, 1.0), 1: (2.39, 1.0, 0.0, 0.0)}
  rec, final = play(eng, 1, 500, states=states)
  from model_based_rl_amd.engine import records_view
  rv = records_view(rec, O, A)
  for b in (0, 1):
    assert np.array_equal(rv['obs'][0, b], np.array(states[b], np.float32))
    assert rv['done'][0, b] == 1 and rv['step'][0, b] == 0 and rv['episode'][0, b] == 0
    assert rv['episode'][1, b] == 1 and rv['step'][1, b] == 0
    assert np.array_equal(rv['obs'][1, b], eng.cartpole_reset_state(b, 1).astype(np.float32))
  assert rv['done'][0, 2:].sum() == 0
  host_check(eng, rec, final, 500, states=states)
  eng.close()


def test_refusals():
  from model_based_rl_amd.engine import Engine
  for kw, O_ in ((dict(), 8), (dict(two_players=True), 4)):
    eng = Engine(B, O_, A, SIMS, **kw)
    with pytest.raises(RuntimeError, match='CartPole needs obs_dim 4, action_space 2 and a single player'):
      eng.selfplay_set_env('cartpole')
    eng.close()
  eng = Engine(B, O, A, SIMS)
  eng.selfplay_set_env('cartpole')
  with pytest.raises(RuntimeError, match='CartPole environment has neither byte observations nor --norm_obs'):
    eng.selfplay_set_obs(obs_min=[0.0], obs_range=[1.0])
  with pytest.raises(RuntimeError, match='CartPole environment has neither byte observations nor --norm_obs'):
    eng.selfplay_set_obs(uint8_obs=True)
  with pytest.raises(RuntimeError, match='packed byte observations are for the synthetic -ram- environments'):
    eng.selfplay_set_obs(uint8_obs=True, packed=True)
  eng.close()
  eng = Engine(B, O, A, SIMS)      # ... and in the other order
  eng.selfplay_set_obs(obs_min=[0.0], obs_range=[1.0])
  with pytest.raises(RuntimeError, match='CartPole environment has neither byte observations nor --norm_obs'):
    eng.selfplay_set_env('cartpole')
  eng.close()


def test_actor_on_the_device_environment(tmp_path):
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.engine import records_view
  from model_based_rl_amd.envs import CartPole
  from model_based_rl_amd.logger import read_metrics
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = make_config(['--environment', 'CartPole-v1', '--num_envs', '64', '--num_simulations', str(SIMS), '--seed', '5',
                     '--window_size', '16384', '--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'r', '--actor_log_frequency', '1'])
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  storage.store_weights({k: torch.from_numpy(v) for k, v in random_weights(O, A, 1).items()}, 1)
  actor = Actor(0, cfg, storage, replay)
  assert not actor.host_env
  seen = []
  actor.record_tap = lambda v: seen.append(v.copy())
  actor.launch(max_moves=96)
  assert actor.engine.selfplay_moves_per_launch() == 16
  rec = np.concatenate(seen, 0)
  rv = records_view(rec, O, A)
  thr = replay.get_throughput()
  assert thr['frames'] > 0 and thr['games'] > 0 and actor.games_played == int(rv['done'].sum()) > 0
  # every finished game's return equals its length: reward 1 per step (the logged points average the games of a move)
  m = read_metrics(os.path.join(actor.dirs['worker'], 'metrics.csv'))
  assert len(m['games/return']) > 0
  assert [v for _, v in m['games/return']] == [v for _, v in m['games/length']]
  for b in range(64):
    ends = np.flatnonzero(rv['done'][:, b])
    start = 0
    for e in ends:
      assert rv['reward'][start:e + 1, b].sum() == e + 1 - start == rv['step'][e, b] + 1
      start = e + 1
  # the first finished game of environment 0 replays on the host class exactly
  end = int(np.flatnonzero(rv['done'][:, 0])[0])
  host = CartPole(500)
  host.reset()
  host.set_state(actor.engine.cartpole_reset_state(0, 0))
  for t in range(end + 1):
    assert np.array_equal(rv['obs'][t, 0].view(np.int32), host._obs().view(np.int32)), t
    _, reward, done, _ = host.step(int(rv['action'][t, 0]))
    assert done == (t == end) and reward == rv['reward'][t, 0]
  actor.close(); actor.engine.close()


def test_evaluator_plays_the_host_class():
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  cfg = make_config(['--environment', 'CartPole-v1', '--num_simulations', str(SIMS), '--seed', '5'])
  cfg.temperature, cfg.only_prior, cfg.only_value, cfg.use_exploration_noise, cfg.apply_mcts_actions = 0, 0, 0, 0, 1
  cfg.label, cfg.random_opp, cfg.batch = 'random', None, 32
  weights = {k: torch.from_numpy(v) for k, v in random_weights(O, A, 1).items()}
  ev = Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  games = ev.play_games(32, list(range(100, 132)))
  s = ev.summary(games)
  assert s['return'][0] == s['length'][0] > 0 and s['return'][1] == s['length'][1]
  alone = ev.play_games(1, [105])[0]
  g5 = games[5]
  assert alone.history.actions == g5.history.actions and alone.history.rewards == g5.history.rewards
  assert alone.step == g5.step and alone.history.root_values == g5.history.root_values


def test_split_f16_plays_the_launch_per_step_form():
  eng = make_engine(split=True)
  assert eng.split_f16 and eng.selfplay_moves_per_launch() == 0
  rec, final = play(eng, 2, 500)
  host_check(eng, rec, final, 500)
  eng.close()
