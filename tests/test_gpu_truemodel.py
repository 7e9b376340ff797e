"""The true-rules search on the device (DESIGN s7g; csrc/mz_truemodel.hip.h):
  1  the stepwise device loop (tm_root, tm_select, the fake network on the read-back observations, tm_expand_backup) against
     the host twin on the CPU test's positions.  The bar is tests/test_gpu_tree.py's: every field exact except the priors P,
     within 8 ulp (device exp() against glibc's, at most 9 terms in a normaliser); the leaves' observations exact after
     every simulation; tm_expand_backup_select gives the tree of the pair bit for bit
  2  tm_search against the stepwise loop on the same engine and weights: identical in every field, P included, and the
     move's own root value and logits survive it
  3  play_games(device_env=True, true_model=True) against a loop that drives an engine move by move from Python on the host
     rules, log by log; the same call without the flag plays the plain search's games
  4  matches: a net against itself with true_model (1, 1) plays test 3's games; with (0, 1) every ply is its mover's own
     kind of search, in both seatings
  5  --grade on true-rules games returns a report with the keys of the plain one"""
import functools

import numpy as np
import pytest

from tests import truemodel_py as tp
from tests.eval_device_util import eval_state, record, weights

pytestmark = pytest.mark.gpu

SIMS = tp.SIMS


def ulp_diff(a, b):
  a = np.ascontiguousarray(a, np.float64).view(np.int64)
  b = np.ascontiguousarray(b, np.float64).view(np.int64)
  return np.abs(a - b)


def _legal_bytes(mask, A):
  return ((np.asarray(mask, np.uint32)[:, None] >> np.arange(A)) & 1).astype(np.uint8)


def _engine(kind, n, sims=SIMS):
  from model_based_rl_amd.engine import Engine
  A, O = (9, 9) if kind == 1 else (7, 42)
  eng = Engine(n, O, A, sims, two_players=True)
  eng.set_true_model(kind)
  return eng


def _export(eng):
  d = eng.export_tree()
  d.pop('EX')
  d.update(eng.tm_export())
  return d


@functools.lru_cache(maxsize=None)
def _host(kind, with_noise):
  """the host twin on the shared positions, and the observations it evaluated per simulation"""
  from model_based_rl_amd.engine import mz_config, tm_search_host
  A, O = (9, 9) if kind == 1 else (7, 42)
  bd, tn, st, lg, noise = tp.case_positions(kind)
  seen = []

  def net(obs):
    seen.append(obs.copy())
    return tp.fake_network(obs, A)
  host = tm_search_host(mz_config(len(bd), O, A, SIMS, two_players=True), kind, bd, tn, st, lg, net, noise=noise if with_noise else None)
  return host, seen


def _stepwise(kind, with_noise, fused, check_obs=None):
  """the device loop on injected outputs; fused: tm_expand_backup_select instead of the pair"""
  A = 9 if kind == 1 else 7
  bd, tn, st, lg, noise = tp.case_positions(kind)
  n = len(bd)
  eng = _engine(kind, n)
  legal = np.array([sum(1 << a for a in tp.playout_py.legal_actions(kind, b.tolist())) for b in bd], np.uint32)
  eng.root_load(np.zeros(n, np.float32), lg)
  eng.root_prepare(tn, _legal_bytes(legal, A), noise if with_noise else None)
  eng.tm_root(bd, tn, st)
  out = eng.tm_select()
  for s in range(SIMS):
    obs, fin = out[0].cpu().numpy(), out[1].cpu().numpy()
    if check_obs is not None:
      assert np.array_equal(obs, check_obs[s]), ('leaf observations', s)
      assert np.array_equal(fin != 0, ~obs.any(1))      # (a finished leaf, and only it, has the zero observation)
    v, l = tp.fake_network(obs, A)
    if fused:
      out = eng.tm_expand_backup_select(v, l, last=s == SIMS - 1)
    else:
      eng.tm_expand_backup(v, l)
      out = eng.tm_select() if s + 1 < SIMS else None
  d = _export(eng)
  eng.close()
  return d


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
@pytest.mark.parametrize('with_noise', [False, True], ids=['plain', 'noise'])
def test_stepwise_loop_equals_the_host_twin(kind, with_noise):
  host, seen = _host(kind, with_noise)
  dev = _stepwise(kind, with_noise, False, check_obs=seen)
  assert np.array_equal(dev['EX'], host['EX'])
  ex = host['EX'] == 1
  for key in ('N', 'W', 'R', 'E', 'TP'):
    diff = np.argwhere((dev[key] != host[key]) & ex)
    assert len(diff) == 0, (key, diff[:5].tolist())
  assert ulp_diff(dev['P'][ex], host['P'][ex]).max() <= 8, 'P'
  assert np.array_equal(dev['legal'], host['legal']) and np.array_equal(dev['minmax'], host['minmax'])
  assert np.array_equal(dev['nexp'], host['nexp'])
  taken = np.arange(SIMS + 1)[None, :] < host['nexp'][:, None]
  for key in tp.SLOT_FIELDS:
    assert np.array_equal(dev[key][taken], host[key][taken]), key
  # the illegal children of every taken slot are marked as at the root
  A = 9 if kind == 1 else 7
  gone = np.repeat(taken, A, axis=1) & (host['EX'][:, 1:] == 0)
  assert not dev['TP'][:, 1:][gone].any() and not dev['P'][:, 1:][gone].any()
  fused = _stepwise(kind, with_noise, True)
  for key in tp.TREE_FIELDS:
    assert np.array_equal(fused[key][ex], dev[key][ex]), key      # bit for bit, P included
  for key in ('legal', 'minmax', 'nexp', 'EX'):
    assert np.array_equal(fused[key], dev[key]), key
  for key in tp.SLOT_FIELDS:
    assert np.array_equal(fused[key][taken], dev[key][taken]), key


@pytest.mark.parametrize('kind', [1, 3], ids=['tictactoe', 'connect_four'])
def test_tm_search_equals_the_stepwise_loop_on_the_engines_network(kind):
  A, O = (9, 9) if kind == 1 else (7, 42)
  bd, tn, st, _, noise = tp.case_positions(kind)
  n = len(bd)
  obs0 = (bd[:, :O].astype(np.int32) * tn[:, None]).astype(np.float32)
  legal = _legal_bytes([sum(1 << a for a in tp.playout_py.legal_actions(kind, b.tolist())) for b in bd], A)
  eng = _engine(kind, n)
  eng.set_weights(weights(O, A, 5))

  def root():
    eng.initial_inference(obs0)
    v, lg, _ = eng.root_outputs()
    v, lg = v.cpu().numpy().copy(), lg.cpu().numpy().copy()
    eng.root_prepare(tn, legal, noise)
    eng.tm_root(bd, tn, st)
    return v, lg
  v0, lg0 = root()
  eng.tm_search()
  v1, lg1, _ = eng.root_outputs()
  assert np.array_equal(v1.cpu().numpy(), v0) and np.array_equal(lg1.cpu().numpy(), lg0)      # the move's own root outputs stay
  whole = _export(eng)
  assert (whole['N'][:, 0] == SIMS).all()
  root()
  reached_finished = 0
  for s in range(SIMS):
    obs, fin = eng.tm_select()
    reached_finished += int(fin.sum())
    eng.initial_inference(obs)
    v, lg, _ = eng.root_outputs()
    eng.tm_expand_backup(v.clone(), lg.clone())
  step = _export(eng)
  eng.close()
  assert reached_finished > 0
  assert np.array_equal(whole['EX'], step['EX']) and np.array_equal(whole['nexp'], step['nexp'])
  ex = whole['EX'] == 1
  for key in tp.TREE_FIELDS:
    assert np.array_equal(whole[key][ex], step[key][ex]), key
  assert np.array_equal(whole['minmax'], step['minmax'])
  taken = np.arange(SIMS + 1)[None, :] < whole['nexp'][:, None]
  for key in tp.SLOT_FIELDS:
    assert np.array_equal(whole[key][taken], step[key][taken]), key


# ---- games
GAMES = {'TicTacToe': 64, 'ConnectFour': 32}
GSIMS, SEED0 = 16, 4000
LONGEST = {'TicTacToe': 9, 'ConnectFour': 42}


def _host_env(env):
  from model_based_rl_amd import envs
  e = envs.TicTacToe() if env == 'TicTacToe' else envs.ConnectFour()
  e.reset()
  return e


def _draws(env, n, A):
  rng = np.random.RandomState(77)
  return [dict(walk=[rng.uniform(size=1) for _ in range(LONGEST[env])], noise=[rng.dirichlet([0.25] * A) for _ in range(LONGEST[env])])
          for _ in range(n)]


def _state(env, **over):
  return eval_state(env, sims=GSIMS, temperature=0.5, use_exploration_noise=1, **over)


def _python_loop(env, state, seeds, draws, true_model):
  """the games driven move by move from Python on the host rules: per move one engine call sequence over every game (a
  finished game rides along with the zero observation and is not read)"""
  from model_based_rl_amd.engine import Engine
  cfg = state['config']
  B, A, O = len(seeds), int(cfg.action_space), int(np.prod(cfg.obs_space))
  eng = Engine.from_config(cfg, B, seed=0, env_id_offset=seeds[0])
  eng.set_weights(state['weights'])
  if true_model:
    eng.set_true_model(env)
  envs = [_host_env(env) for _ in range(B)]
  done = [False] * B
  logs = [dict(step=0, actions=[], rewards=[], to_play=[], dones=[], child_visits=[], root_values=[], pred_values=[], pred_rewards=[],
               search_depths=[]) for _ in range(B)]
  move = 0
  while not all(done):
    obs, legal, to_play = np.zeros((B, O), np.float32), np.ones((B, A), np.uint8), np.ones(B, np.int8)
    boards, turn, step = np.zeros((B, 42), np.int8), np.ones(B, np.int8), np.zeros(B, np.int32)
    noise, uniform = np.zeros((B, A)), np.zeros((B, 1))
    for i, e in enumerate(envs):
      boards[i, :len(e.board)], turn[i], step[i] = e.board, e.turn, logs[i]['step']
      if done[i]:
        continue
      obs[i] = (e.turn * e.board).astype(np.float32)
      legal[i] = 0
      legal[i, e.legal_actions()] = 1
      to_play[i] = e.turn
      noise[i] = np.asarray(draws[i]['noise'][move]) * legal[i]
      uniform[i] = draws[i]['walk'][move]
    eng.initial_inference(obs)
    eng.root_prepare(to_play, legal, noise)
    if true_model:
      eng.tm_root(boards, turn, step)
      eng.tm_search()
    else:
      eng.search()
    w = eng.eval_walk(1, 0.5, uniform, move=move)
    fin = eng.finalize(0.0, np.full(B, 0.5), move=move)
    pv = eng.root_outputs()[0].cpu().numpy()
    actions, preds, depths = w['actions'].cpu().numpy(), w['pred_rewards'].cpu().numpy(), w['path_lengths'].cpu().numpy()
    visits, rv = fin['child_visits'].cpu().numpy(), fin['root_value'].cpu().numpy()
    for i, e in enumerate(envs):
      if done[i]:
        continue
      L = logs[i]
      mover = e.turn
      _, reward, d, _ = e.step(int(actions[i, 0]))
      L['actions'].append(int(actions[i, 0])); L['rewards'].append(float(reward)); L['to_play'].append(int(mover)); L['dones'].append(bool(d))
      L['child_visits'].append([float(x) for x in visits[i]]); L['root_values'].append(float(rv[i])); L['pred_values'].append(float(pv[i]))
      L['pred_rewards'].append(float(preds[i, 0])); L['search_depths'].append([int(x) for x in depths[i]])
      L['step'] += 1
      done[i] = bool(d) or L['step'] >= cfg.max_steps
    move += 1
  eng.close()
  return logs


@functools.lru_cache(maxsize=None)
def _device_games(env, true_model):
  from model_based_rl_amd.evaluate import Evaluator
  state = _state(env)
  n = GAMES[env]
  seeds = list(range(SEED0, SEED0 + n))
  draws = _draws(env, n, int(state['config'].action_space))
  ev = Evaluator(state)
  ev.load_network()
  games = ev.play_games(n, seeds, draws=draws, device_env=True, keep_history=True, true_model=true_model)
  return state, seeds, draws, [record(g) for g in games]


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
@pytest.mark.parametrize('true_model', [True, False], ids=['true_rules', 'learned_model'])
def test_games_equal_the_python_driven_loop(env, true_model):
  state, seeds, draws, got = _device_games(env, true_model)
  want = _python_loop(env, state, seeds, draws, true_model)
  for i, (g, w) in enumerate(zip(got, want)):
    for key in w:
      assert g[key] == w[key], (env, seeds[i], key)
  assert len(set(g['step'] for g in got)) > 1
  if true_model:      # every predicted reward is the true one: 1 exactly where the move won, else 0
    assert all(g['pred_rewards'] == g['rewards'] and set(g['rewards']) <= {0.0, 1.0} for g in got)
    assert any(1.0 in g['rewards'] for g in got)
    # a revisit of a finished node expands nothing: some searches list fewer path lengths than simulations
    assert any(0 in d for g in got for d in g['search_depths'])
    assert all(all(x > 0 for x in d[:d.index(0)] if 0 in d) and not any(d[d.index(0):]) for g in got for d in g['search_depths'] if 0 in d)
  else:
    assert any(g['pred_rewards'] != g['rewards'] for g in got)
    assert got != _device_games(env, True)[3]


# ---- matches
def _search_rows(env, state, rows, true_model):
  """the rows (one searched position each) as one batch through a fresh engine: the plain search, or the true-rules one"""
  from model_based_rl_amd.engine import Engine
  cfg = state['config']
  n, A = len(rows), int(cfg.action_space)
  eng = Engine.from_config(cfg, n, seed=0, env_id_offset=0)
  eng.set_weights(state['weights'])
  cells = len(rows[0]['board'])
  boards = np.zeros((n, 42), np.int8)
  boards[:, :cells] = np.stack([r['board'] for r in rows])
  turn = np.array([r['turn'] for r in rows], np.int8)
  legal = np.stack([r['legal'] for r in rows])
  eng.initial_inference((boards[:, :cells].astype(np.int32) * turn[:, None]).astype(np.float32))
  eng.root_prepare(turn, legal, np.stack([r['noise'] for r in rows]) * legal)
  if true_model:
    eng.set_true_model(env)
    eng.tm_root(boards, turn, np.array([r['ply'] for r in rows], np.int32))
    eng.tm_search()
  else:
    eng.search()
  w = eng.eval_walk(1, 0.5, np.array([[r['walk']] for r in rows]))
  fin = eng.finalize(0.0, np.full(n, 0.5))
  out = dict(actions=w['actions'].cpu().numpy()[:, 0], preds=w['pred_rewards'].cpu().numpy()[:, 0], depths=w['path_lengths'].cpu().numpy(),
             visits=fin['child_visits'].cpu().numpy(), root_values=fin['root_value'].cpu().numpy(),
             pred_value=eng.root_outputs()[0].cpu().numpy())
  eng.close()
  return out


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_a_net_against_itself_on_the_true_rules_is_the_single_network_game(env):
  from model_based_rl_amd.match import play_match
  state, seeds, draws, single = _device_games(env, True)
  mdraws = [dict(walk=[float(w[0]) for w in d['walk']], noise=d['noise']) for d in draws]
  games, summary = play_match(state, state, len(seeds), seeds, draws=mdraws, keep_history=True, true_model=(1, 1))
  assert summary['true_model'] == [1, 1] and len(games) == 2 * len(seeds)
  for g in games:
    got, want = record(g), single[g.seed - SEED0]
    for key in want:
      assert got[key] == want[key], (env, g.seed, g.seating, key)


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_each_side_of_a_match_runs_its_own_kind_of_search(env):
  from model_based_rl_amd.match import play_match
  state, seeds, draws, _ = _device_games(env, True)
  n = 24
  mdraws = [dict(walk=[float(w[0]) for w in d['walk']], noise=d['noise']) for d in draws[:n]]
  games, summary = play_match(state, state, n, seeds[:n], draws=mdraws, keep_history=True, true_model=(0, 1))
  assert summary['true_model'] == [0, 1] and sorted(set(g.seating for g in games)) == [0, 1]
  rows = {0: [], 1: []}
  for g in games:
    e = _host_env(env)
    h = g.history
    for p, a in enumerate(h.actions):
      legal = np.zeros(int(state['config'].action_space), np.uint8)
      legal[e.legal_actions()] = 1
      assert g.nets[p] == (p + g.seating) % 2
      rows[g.nets[p]].append(dict(g=g, ply=p, board=e.board.astype(np.int8).copy(), turn=e.turn, legal=legal,
                                  noise=np.asarray(mdraws[g.seed - SEED0]['noise'][p]), walk=mdraws[g.seed - SEED0]['walk'][p]))
      e.step(a)
  network_rewards = 0
  for net in (0, 1):
    out = _search_rows(env, state, rows[net], true_model=bool(net))
    for i, r in enumerate(rows[net]):
      g, p = r['g'], r['ply']
      at = (env, g.seed, g.seating, p)
      assert g.history.actions[p] == int(out['actions'][i]), at
      assert g.pred_rewards[p] == float(out['preds'][i]), at
      assert g.history.child_visits[p] == [float(x) for x in out['visits'][i]], at
      assert g.history.root_values[p] == float(out['root_values'][i]) and g.pred_values[p] == float(out['pred_value'][i]), at
      assert g.search_depths[p] == [int(x) for x in out['depths'][i]], at
      if net == 1:
        assert g.pred_rewards[p] == g.history.rewards[p], at      # the true reward
      else:
        network_rewards += g.pred_rewards[p] not in (0.0, 1.0)
  assert network_rewards > 0


def test_grade_on_true_rules_games_reports_the_plain_keys():
  from model_based_rl_amd.evaluate import Evaluator
  reports = []
  for tm in (0, 1):
    state = eval_state('TicTacToe', sims=GSIMS, grade=True, grade_table=False, grade_empties=12, grade_nodes=4096, grade_unroll=None,
                       device_env=True, true_model=tm)
    ev = Evaluator(state)
    ev.load_network()
    ev.play_games(32, list(range(SEED0, SEED0 + 32)))
    reports.append(ev.grade_report)
  assert reports[1] is not None and sorted(reports[0]) == sorted(reports[1])


def test_engine_refusals():
  from model_based_rl_amd.engine import Engine
  eng = Engine(4, 9, 9, 4, two_players=True)
  with pytest.raises(RuntimeError, match='mz_set_true_model: kind must be 0'):
    eng.set_true_model(2)
  with pytest.raises(RuntimeError, match='mz_set_true_model: Connect Four needs obs_dim 42'):
    eng.set_true_model(3)
  with pytest.raises(RuntimeError, match='mz_tm_root: no true-rules search is set'):
    eng.tm_root(np.zeros((4, 42), np.int8), np.ones(4, np.int8), np.zeros(4, np.int32))
  eng.set_true_model(1)
  with pytest.raises(RuntimeError, match='mz_tm_root: call mz_root_prepare first'):
    eng.tm_root(np.zeros((4, 42), np.int8), np.ones(4, np.int8), np.zeros(4, np.int32))
  with pytest.raises(RuntimeError, match='mz_tm_select: call mz_tm_root first'):
    eng.tm_select()
  eng.set_weights(weights(9, 9, 5))
  # the games refuse what the search does not serve, one sentence each
  eng.eval_env_reset('TicTacToe', 9)
  for mode, M, why in ((0, 2, 'one action per move'), (1, 1, 'only_prior / only_value')):      # (the first call sizes the walk)
    with pytest.raises(RuntimeError, match='true_model: .*' + why):
      eng.eval_env_moves(1, mode, M)
  eng.close()
  c4 = Engine(4, 42, 7, 4, two_players=True)
  c4.set_weights(weights(42, 7, 5))
  c4.set_true_model(3)
  c4.set_true_model(0)      # off again: the plain search
  c4.eval_env_reset('ConnectFour', 42)
  assert c4.eval_env_moves(1) == 4
  c4.close()
