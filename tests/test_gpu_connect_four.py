"""The device Connect Four environment (mz_selfplay_set_env kind 3; csrc/mz_selfplay.hip.h) against its definition, the host
class envs.ConnectFour: move for move in the two whole-moves instantiations (k_search_fused<15,1,8,LT,..,HEAD,GAME>: whole trees
at 8 simulations, the compact placement at 30), in the launch-per-step form, with split-f16; their trees against the
oracle's tree; placed positions; the refusals; the actor and the evaluator on it.  B = 40 environments (three workgroups,
the last one padded), random FCNetwork weights everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.c4_positions import POSITIONS, WINS
from tests.parity_util import env_switches, philox_action_uniform, random_weights, replay_move

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, O, A, SEED = 40, 42, 7, 91
PLACEMENT = {8: 1, 30: 2}      # simulations -> tree placement of the whole-moves kernel they select
KW = dict(two_players=True, known_bounds=(-1.0, 1.0), discount=1.0)
PLACED = {base + i: i for base in (0, 16) for i in range(6)}      # environment -> index into POSITIONS (two workgroups)


def make_engine(sims, split=False, no_persist=False):
  from model_based_rl_amd.engine import Engine
  with env_switches(MZ_NO_PERSIST='1' if no_persist else None):
    eng = Engine(B, O, A, sims, seed=SEED, split_f16=split, **KW)
  eng.selfplay_set_env('connect_four')
  eng.set_weights(random_weights(O, A, 2))
  return eng


def play(eng, launches, chunk=16, placed=None):
  """launches x chunk moves; returns (records [moves, B, rec] float32, board states [B, 44] int8 at the end)"""
  import torch
  eng.selfplay_reset(42, 1.0)
  for env, i in (placed or {}).items():
    eng.selfplay_set_board_state(env, POSITIONS[i][3], POSITIONS[i][1])
  recs = []
  for _ in range(launches):
    eng.selfplay_steps(chunk)
    buf, n = eng.selfplay_drain()
    torch.cuda.synchronize()
    assert n == chunk
    recs.append(buf[:n].numpy().copy())
  return np.concatenate(recs, 0), eng.selfplay_board_state()


def host_check(rec, final, placed=None):
  """every environment's records replayed through a host ConnectFour driven by the recorded actions: the observation's
  float32 bits, child_visits exactly 0 at full columns and the action legal, reward, done, the to_play flag, step, episode
  and env id at every move; the device's boards, turns and steps at the end.  Returns (games finished, moves by player 2)."""
  from model_based_rl_amd.engine import records_view
  from model_based_rl_amd.envs import ConnectFour
  rv = records_view(rec, O, A)
  M = rec.shape[0]
  games = second = 0
  for b in range(B):
    host = ConnectFour()
    if placed and b in placed:
      host.set_position(POSITIONS[placed[b]][3], POSITIONS[placed[b]][1])
    ep = 0
    for m in range(M):
      want = (host.turn * host.board).astype(np.float32)
      assert np.array_equal(rv['obs'][m, b].view(np.int32), want.view(np.int32)), (b, m, 'observation')
      legal = np.zeros(A, bool)
      legal[host.legal_actions()] = True
      cv, action = rv['child_visits'][m, b], int(rv['action'][m, b])
      assert np.all(cv[~legal] == 0) and legal[action] and cv[action] > 0, (b, m, 'legal moves')
      assert rv['to_play'][m, b] == host.turn, (b, m, 'to_play')
      assert rv['step'][m, b] == host._elapsed_steps and rv['episode'][m, b] == ep and rv['env_id'][m, b] == b, (b, m)
      second += int(host.turn == -1)
      _, reward, done, _ = host.step(action)
      assert rv['reward'][m, b] == np.float32(reward) and bool(rv['done'][m, b]) == done, (b, m, 'reward / done')
      if done:
        games += 1
        ep += 1
        host.reset()
    assert np.array_equal(final[b, :42], host.board.astype(np.int8)), (b, 'final board')
    assert final[b, 42] == host.turn and final[b, 43] == host._elapsed_steps, (b, 'final turn / step')
  return games, second


@pytest.fixture(scope='module', params=sorted(PLACEMENT))
def whole_moves_run(request):
  """48 moves as three whole-moves launches (shared, read-only)"""
  sims = request.param
  eng = make_engine(sims)
  info, mpl = eng.search_kernel_info(), eng.selfplay_moves_per_launch()
  rec, final = play(eng, 3)
  yield sims, eng, rec, final, info, mpl
  eng.close()


def test_device_equals_host_move_for_move(whole_moves_run):
  sims, eng, rec, final, info, mpl = whole_moves_run
  assert mpl == 16 and info == dict(kind='fused', lt=PLACEMENT[sims], ks1=15, G=8), (info, mpl)
  games, second = host_check(rec, final)
  print('%d simulations: %d games finished in 48 moves of %d environments, %d moves by player 2' % (sims, games, B, second))
  assert games >= B and second > 0      # (a game has at most 42 moves: every environment finishes one)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_connect_four import make_engine, play
eng = make_engine(int(sys.argv[2]), no_persist=True)      # (env_switches clears the MZ_* switches it is not given)
assert eng.selfplay_moves_per_launch() == 0, eng.selfplay_moves_per_launch()
rec, final = play(eng, 3)
np.save(sys.argv[1], rec)
print('CHILD OK')
'''


def test_launch_per_step_form_gives_the_same_records(whole_moves_run, tmp_path):
  """MZ_NO_PERSIST=1 (read at mz_create; a fresh child process): k_c4_observe, root, Dirichlet, tree root, search and
  k_c4_step_record as separate kernels produce the records of the whole-moves launch byte for byte over 48 moves"""
  sims, eng, rec, final, info, mpl = whole_moves_run
  assert mpl == 16
  env = dict(os.environ)
  env['MZ_NO_PERSIST'] = '1'
  out = str(tmp_path / 'rec.npy')
  r = subprocess.run([sys.executable, '-c', CHILD % ROOT, out, str(sims)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
  assert r.returncode == 0 and 'CHILD OK' in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
  other = np.load(out)
  assert other.shape == rec.shape
  assert np.array_equal(other.view(np.int32), rec.view(np.int32))


@pytest.mark.parametrize('sims', sorted(PLACEMENT))
def test_trees_of_the_new_instantiations_vs_oracle(sims):
  """16 moves of the 40 trees of each two-player game kernel replayed through the oracle's tree on the launch's own logged
  network outputs, Dirichlet draws, select_action uniforms, the recorded to_play and the legal masks: actions, visit
  distributions, visit counts and root values exact, and the exported trees of the last move (N, E, TP, W, R, minmax)"""
  import torch
  from oracle import oracle as orc
  from model_based_rl_amd.engine import records_view
  eng = make_engine(sims)
  assert eng.selfplay_moves_per_launch() == 16 and eng.search_kernel_info()['lt'] == PLACEMENT[sims]
  eng.selfplay_noise_log(True)
  eng.selfplay_export_trees(True)
  eng.selfplay_reset(42, 1.0)
  log = eng.sim_io('log', keep_moves=16)
  eng.selfplay_steps(16)
  buf, n = eng.selfplay_drain()
  torch.cuda.synchronize()
  assert n == 16
  rec = buf[:n].numpy().copy()
  rv = records_view(rec, O, A)
  io_all = log.cpu().numpy()
  tree = eng.export_tree()
  cfg = orc.tree_cfg(A, sims, two_players=True, known_bounds=(-1.0, 1.0), discount=1.0)
  for m in range(16):
    noise = eng.selfplay_noise(m)
    u = philox_action_uniform(SEED, np.arange(B), m)
    legal = (rec[m, :, 35:42] == 0).astype(np.uint8)      # the columns whose top cell is empty
    to_play = rv['to_play'][m].astype(np.int8)
    assert np.all((noise > 0) == (legal > 0))
    ref = replay_move(cfg, B, A, sims, io_all[m], noise, 0.25, to_play, legal, 1.0, u, want_tree=(m == 15))
    assert np.array_equal(rv['action'][m], ref['action']), (m, 'action')
    assert np.array_equal(rv['child_visits'][m], ref['child_visits'].astype(np.float32)), (m, 'visit distribution')
    vc = ref['visit_counts'].astype(np.float64)
    assert np.all(vc.sum(1) == sims) and np.array_equal(rv['child_visits'][m], (vc / vc.sum(1, keepdims=True)).astype(np.float32)), (m, 'visit counts')
    assert np.array_equal(rv['root_value'][m], ref['root_value']), (m, 'root value')
    assert np.array_equal(rv['error'][m], ref['root_value'] - ref['v0'].astype(np.float64)), (m, 'error')
    if ref['tree'] is not None:
      eo = ref['tree']
      EX = eo['EX'].astype(bool)
      assert np.array_equal(tree['EX'].astype(bool), EX)
      for k in ('N', 'E', 'TP', 'W'):
        assert np.array_equal(tree[k][EX], eo[k][EX]), k
      assert np.array_equal(tree['N'][:, 1:1 + A], ref['visit_counts'])      # the root's children
      assert np.array_equal(tree['TP'][:, 0], to_play)
      assert np.array_equal(tree['R'].astype(np.float64)[EX], eo['R'][EX])
      assert np.array_equal(tree['minmax'], eo['minmax'])
      assert np.array_equal(tree['noise'], noise)
  assert (rv['to_play'] == -1).any()
  eng.sim_io('off')
  eng.close()


@pytest.mark.parametrize('form', ['whole_moves', 'launch_per_step'])
@pytest.mark.parametrize('sims', sorted(PLACEMENT))
def test_placed_positions(sims, form):
  """the six positions with one legal column in environments 0-5 and 16-21 (two workgroups): the forced move and its
  verdict in move 0, a fresh game in move 1 of the terminal ones, and the host replay of all 16 moves"""
  from model_based_rl_amd.engine import records_view
  eng = make_engine(sims, no_persist=(form == 'launch_per_step'))
  assert eng.selfplay_moves_per_launch() == (16 if form == 'whole_moves' else 0)
  rec, final = play(eng, 1, placed=PLACED)
  eng.close()
  rv = records_view(rec, O, A)
  for b, i in PLACED.items():
    kind, turn, col, board = POSITIONS[i]
    assert np.array_equal(rv['obs'][0, b], (turn * board).astype(np.float32)), (b, kind)
    assert rv['action'][0, b] == col and rv['child_visits'][0, b, col] == 1.0, (b, kind)
    assert rv['to_play'][0, b] == turn and rv['step'][0, b] == np.count_nonzero(board) and rv['episode'][0, b] == 0, (b, kind)
    assert rv['reward'][0, b] == (1.0 if kind in WINS else 0.0) and rv['done'][0, b] == int(kind != 'plain'), (b, kind)
    if kind != 'plain':      # a new game: an empty board, player 1 to move, step 0, the next episode
      assert not rv['obs'][1, b].any() and rv['to_play'][1, b] == 1 and rv['step'][1, b] == 0 and rv['episode'][1, b] == 1, (b, kind)
    else:
      assert rv['to_play'][1, b] == -turn and rv['step'][1, b] == np.count_nonzero(board) + 1 and rv['episode'][1, b] == 0
  host_check(rec, final, placed=PLACED)


def test_refusals():
  from model_based_rl_amd.engine import Engine
  needs = 'Connect Four needs obs_dim 42, action_space 7 and two_players'
  neither = 'Connect Four environment has neither byte observations nor --norm_obs'
  for O_, A_, kw in ((9, 9, KW), (42, 6, KW), (42, 7, {})):      # other shapes, a single player
    eng = Engine(B, O_, A_, 8, **kw)
    with pytest.raises(RuntimeError, match=needs):
      eng.selfplay_set_env('connect_four')
    eng.close()
  eng = Engine(B, O, A, 8, **KW)
  eng.selfplay_set_env('connect_four')
  with pytest.raises(RuntimeError, match=neither):
    eng.selfplay_set_obs(obs_min=[0.0], obs_range=[1.0])
  with pytest.raises(RuntimeError, match=neither):
    eng.selfplay_set_obs(uint8_obs=True)
  with pytest.raises(RuntimeError, match='packed byte observations are for the synthetic -ram- environments'):
    eng.selfplay_set_obs(uint8_obs=True, packed=True)
  eng.selfplay_reset(42, 1.0)
  with pytest.raises(RuntimeError, match='mz_selfplay_set_draws: only for the TicTacToe environment'):
    eng.selfplay_set_draws(uniform=np.zeros(B))
  eng.close()
  for kw, sentence in ((dict(obs_min=[0.0], obs_range=[1.0]), neither), (dict(uint8_obs=True), neither),      # ... and in the other order
                       (dict(uint8_obs=True, packed=True), 'packed byte observations are for the synthetic -ram- environments')):
    eng = Engine(B, O, A, 8, **KW)
    eng.selfplay_set_obs(**kw)
    with pytest.raises(RuntimeError, match=sentence):
      eng.selfplay_set_env('connect_four')
    eng.close()
  # the two debug calls: any other kind is refused
  eng = Engine(B, 9, 9, 8, **KW)
  eng.selfplay_set_env('tictactoe')
  eng.selfplay_reset(9, 1.0)
  with pytest.raises(RuntimeError, match='mz_selfplay_board_state: the Connect Four environment is not set up'):
    eng.selfplay_board_state()
  with pytest.raises(RuntimeError, match='mz_selfplay_set_board_state: the Connect Four environment is not set up'):
    eng.selfplay_set_board_state(0, np.zeros(42, np.int8), 1)
  eng.close()
  eng = Engine(B, O, A, 8, **KW)      # (the synthetic environment)
  eng.selfplay_reset(42, 1.0)
  with pytest.raises(RuntimeError, match='mz_selfplay_board_state: the Connect Four environment is not set up'):
    eng.selfplay_board_state()
  eng.close()


def _actor(tmp_path, num_envs):
  import torch
  from model_based_rl_amd.actors import Actor
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.replay_buffer import PrioritizedReplay
  from model_based_rl_amd.shared_storage import SharedStorage
  cfg = make_config(['--environment', 'ConnectFour', '--two_players', '--known_bounds', '-1', '1', '--discount', '1',
                     '--num_envs', str(num_envs), '--num_simulations', '8', '--seed', '5', '--window_size', '16384',
                     '--runs_dir', str(tmp_path / 'runs'), '--run_tag', 'r', '--actor_log_frequency', '1'])
  storage, replay = SharedStorage(cfg), PrioritizedReplay(cfg)
  storage.store_weights({k: torch.from_numpy(v) for k, v in random_weights(O, A, 2).items()}, 1)
  return Actor(0, cfg, storage, replay), replay


def test_actor_on_the_device_environment(tmp_path):
  """a pool of 64 environments plays one chunk of 16 moves on the device: the frames reach the replay, the finished games
  are counted, both movers appear among the records"""
  from model_based_rl_amd.engine import records_view
  actor, replay = _actor(tmp_path, 64)
  assert not actor.host_env
  seen = []
  actor.record_tap = lambda v: seen.append(v.copy())
  actor.launch(max_moves=16)
  assert actor.engine.selfplay_moves_per_launch() == 16
  rv = records_view(np.concatenate(seen, 0), O, A)
  assert rv['done'].shape == (16, 64)
  thr = replay.get_throughput()
  print('throughput', thr, 'games', actor.games_played)
  assert thr['frames'] > 0 and actor.games_played == int(rv['done'].sum()) == thr['games']
  assert set(np.unique(rv['to_play'])) == {-1, 1}
  # (every game starts at the empty board with player 1: the movers alternate until a game ends)
  assert np.all(rv['to_play'][0] == 1) and np.all(rv['to_play'][1] == -1)
  actor.close(); actor.engine.close()


def test_actor_plays_one_game_on_the_host_class(tmp_path):
  from model_based_rl_amd.logger import read_metrics
  actor, replay = _actor(tmp_path, 1)
  assert actor.host_env
  actor.launch(max_moves=1)      # (the host loop plays whole games: one)
  assert actor.games_played == 1 and 7 <= actor.move_counter <= 42
  m = read_metrics(os.path.join(actor.dirs['worker'], 'metrics.csv'))
  assert [v for _, v in m['games/length']] == [actor.move_counter]
  actor.close(); actor.engine.close()


def test_evaluator_plays_the_host_class_against_the_random_opponent():
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.evaluate import Evaluator
  cfg = make_config(['--environment', 'ConnectFour', '--two_players', '--known_bounds', '-1', '1', '--discount', '1',
                     '--num_simulations', '8', '--seed', '5'])
  for k, v in dict(temperature=0, only_prior=0, only_value=0, use_exploration_noise=0, apply_mcts_actions=1, render=False,
                   save_mcts=False, save_gif_as='', random_opp=-1, human_opp=None, label='random', verbose=False, batch=8).items():
    setattr(cfg, k, v)
  weights = {k: torch.from_numpy(v) for k, v in random_weights(O, A, 2).items()}
  ev = Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  games = ev.play_games(8, list(range(100, 108)))
  returns = np.array([sum(g.history.rewards) for g in games])
  wins, draws, losses = int((returns > 0).sum()), int((returns == 0).sum()), int((returns < 0).sum())
  assert wins + draws + losses == 8 == len(games)
  assert all(7 <= g.step <= 42 for g in games), [g.step for g in games]


def test_split_f16_plays_the_launch_per_step_form():
  """(selfplay_moves_per_launch reports 0 for the form with one launch per step of a move.)  32 moves pass the host replay;
  they are not compared with the float32 records"""
  eng = make_engine(8, split=True)
  assert eng.split_f16 and eng.selfplay_moves_per_launch() == 0 and eng.search_kernel_info()['kind'] == 'split_f16'
  rec, final = play(eng, 2)
  eng.close()
  host_check(rec, final)
