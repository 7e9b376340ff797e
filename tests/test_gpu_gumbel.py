"""The Gumbel search on the device (DESIGN s7h; csrc/mz_gumbel.hip.h), on the CPU test's sets (gp.SETS: the first three, B = 12
and 16 simulations, and those that reach the other lane groups, m < legal actions, other simulation counts and parameters,
and nine blocks of trees) and its hand-built roots (gp.HAND):
  1  the stepwise device loop (gz_root, gz_select, the fake network on the read-back (parent slot, action), gz_expand_backup)
     against the host twin: N, E, TP, R, W, nexp, MinMax, v^, the paths, parent slot / action after every descent and the
     chosen action equal; P within 8 ulp (device exp() against glibc's); pi' and v_mix within 1e-12.  The sets hold the
     margin condition of tests/test_gumbel_cpu.py, so no decision is allowed to differ.  gz_expand_backup_select gives the
     tree of the pair bit for bit.  The twin equals the float64 restatement on every one of them (tests/test_gumbel_cpu.py),
     so this holds the kernels to the restatement at
       G = 4   A = 4; A = 2 with two idle lanes (m = 1, 2)                      8, 16 simulations
       G = 8   A = 7                                                            16, 50 (c_visit 0, c_scale 2, discount 1)
       G = 16  A = 9, 13; m = 4, 5 of up to 13 legal                            16, 30, 33
       G = 32  A = 18 with 14 idle lanes, A = 32 (bit 31; a root with all 32);  8, 16, 30, 50; 12 trees (two blocks) and
               m = 16 of 17 .. 32 legal, m = 4, m = 8                            70 (nine blocks, the last ragged)
     Measured on an MI355X, the worst over gumbel_scale 1 and 0 (the test prints them):
       set            P ulp  |d pi'|   |d v_mix|      set            P ulp  |d pi'|   |d v_mix|
       tictactoe      2      2.2e-19   0              a32_two_m8     2      5.6e-17   0
       connect_four   2      1.3e-26   0              a9_s30_m4      2      4.3e-19   0
       single_player  2      5.6e-17   1.4e-17        a7_s50_cv0     2      1.7e-18   0
       a2_s8          2      2.7e-23   0              a13_s33_m5     2      1.7e-18   0
       a18_s30        2      1.4e-17   0              a18_b70_s8     2      2.8e-17   0
       a18_s30_m4     2      3.3e-24   0              underflow      0      0         0
       a32_s50        2      1.4e-17   0              ties18, ties32 0      0         0
     -- a rounding of pi' and of v_mix at the most, with (c_visit + max N) * c_scale up to 100: the bound of 1e-12 stays
  2  gz_search on the engine's own network against the stepwise loop through gather_hidden + recurrent_inference: bit for bit;
     also on 37 trees (three 16-row workgroups of the recurrent inference, the last ragged) at A = 18 and at A = 2
  3  device-drawn G: a game's draws and record do not depend on its batch; scale 0 draws nothing and is deterministic
  4  play_games(device_env=True, gumbel=...) against a loop that drives an engine move by move from Python, log by log; a
     match with gumbel (0, 1): every ply is its mover's own kind of search; with the mode off the records are the parent's
  5  --grade on Gumbel games reports the plain keys; the engine's refusals by their sentence"""
import functools

import numpy as np
import pytest

from tests import gumbel_py as gp
from tests.eval_device_util import eval_state, record, weights

pytestmark = pytest.mark.gpu

SIMS, B = gp.SIMS, gp.TREES


def ulp_diff(a, b):
  a = np.ascontiguousarray(a, np.float64).view(np.int64)
  b = np.ascontiguousarray(b, np.float64).view(np.int64)
  return np.abs(a - b)


def _engine(c, n=None, sims=None, **kw):
  from model_based_rl_amd.engine import Engine
  eng = Engine(c['trees'] if n is None else n, 4, c['A'], c['sims'] if sims is None else sims, two_players=c['two'],
               known_bounds=c['bounds'], discount=c['discount'], **kw)
  return eng


@functools.lru_cache(maxsize=None)
def _host(name, scale, num_simulations=None):
  from tests.test_gumbel_cpu import host_search
  return host_search(gp.case(name), scale, **({} if num_simulations is None else dict(num_simulations=num_simulations)))


def _export(eng):
  d = eng.export_tree()
  d.update(eng.gz_export())
  a, r, pi, vm = eng.gz_pick()
  d.update(action=a.cpu().numpy(), pred_reward=r.cpu().numpy(), pi=pi.cpu().numpy(), v_mix=vm.cpu().numpy())
  return d


def _stepwise(name, scale, fused, host=None, num_simulations=None):
  """the device loop on injected outputs; fused: gz_expand_backup_select instead of the pair.  host: the twin's record, the
  descents are compared with it as they are made.  The simulations, the trees and the parameters are the case's; the
  descents as read back are returned with the tree (sel_slot, sel_action, plens, paths, as the twin names them)"""
  c = gp.case(name)
  n, sims = c['trees'], c['sims']
  run = sims if num_simulations is None else num_simulations
  eng = _engine(c)
  eng.set_gumbel(True, gumbel_scale=scale, **c['kw'])
  eng.root_load(c['root_value'], c['root_logits'], np.zeros((n, 50), np.float32))
  eng.root_prepare(c['to_play'], c['legal'])
  eng.gz_root(c['G'] if scale else None)
  out = eng.gz_select()
  net = gp.net(c)
  rec = dict(sel_slot=np.zeros((n, sims), np.int32), sel_action=np.zeros((n, sims), np.int32), plens=np.zeros((n, sims), np.int32),
             paths=np.full((n, sims, sims + 2), -1, np.int32))
  for s in range(run):
    slot, act = out[0].cpu().numpy(), out[1].cpu().numpy()
    paths, lens = eng.last_paths()
    paths, lens = paths.cpu().numpy(), lens.cpu().numpy()
    rec['sel_slot'][:, s], rec['sel_action'][:, s], rec['plens'][:, s] = slot, act, lens
    for b in range(n):
      rec['paths'][b, s, :lens[b]] = paths[b, :lens[b]]
    if host is not None:
      assert np.array_equal(slot, host['sel_slot'][:, s]) and np.array_equal(act, host['sel_action'][:, s]), ('descent', s)
      assert np.array_equal(lens, host['plens'][:, s]), ('path lengths', s)
      for b in range(n):
        assert np.array_equal(paths[b, :lens[b]], host['paths'][b, s, :lens[b]]), ('path', s, b)
    v, r, lg = net(s, slot, act)
    hidden = np.zeros((n, 50), np.float32)
    if fused:
      out = eng.gz_expand_backup_select(v, r, lg, hidden, last=s == run - 1)
    else:
      eng.gz_expand_backup(v, r, lg, hidden)
      out = eng.gz_select() if s + 1 < run else None
  d = _export(eng)
  d.update(rec)
  eng.close()
  return d


def _loop_equals_the_host_twin(name, scale):
  """the bars of item 1 of the module docstring on one (set or hand-built root, gumbel_scale); returns the device's search"""
  host = _host(name, scale)
  assert host['min_gap'] >= 1e-9
  dev = _stepwise(name, scale, False, host=host)
  ex = dev['EX'] == 1
  for key in ('N', 'W', 'R', 'E', 'TP'):
    diff = np.argwhere((dev[key] != host[key]) & ex)
    assert len(diff) == 0, (key, diff[:5].tolist())
  c = gp.case(name)      # every simulation expands a node: the root, its legal children, every child of sims expanded nodes
  n, sims = c['trees'], c['sims']
  assert (dev['N'][:, 0] == sims).all() and ex.sum() == n * (1 + sims * c['A']) + c['legal'].sum()
  worst = (ulp_diff(dev['P'][ex], host['P'][ex]).max(), np.abs(dev['pi'] - host['pi']).max(), np.abs(dev['v_mix'] - host['v_mix']).max())
  print('gumbel %s scale %g (G = %d, %d trees, %d simulations): P %d ulp, |d pi\'| %.3g, |d v_mix| %.3g'
        % ((name, scale, gp.group_width(c['A']), n, sims) + worst))
  assert worst[0] <= 8, 'P'
  assert np.array_equal(dev['legal'], host['legal']) and np.array_equal(dev['minmax'], host['minmax'])
  assert np.array_equal(dev['vhat'], host['vhat'])
  if scale:
    assert np.array_equal(dev['G'], c['G'])
  else:
    assert not dev['G'].any()
  assert np.array_equal(dev['action'], host['action']) and np.array_equal(dev['pred_reward'], host['pred_reward'])
  assert worst[1] <= 1e-12 and worst[2] <= 1e-12
  assert (dev['sel_action'] < c['A']).all() and (dev['action'] < c['A']).all()      # (never an idle lane's)
  fused = _stepwise(name, scale, True)
  for key in gp.TREE_FIELDS + ('legal', 'minmax', 'vhat', 'G', 'EX', 'action', 'pred_reward', 'pi', 'v_mix', 'sel_slot', 'sel_action',
                               'plens', 'paths'):
    assert np.array_equal(fused[key], dev[key]), key      # bit for bit, P and pi' included
  return dev


@pytest.mark.parametrize('name', list(gp.SETS))
@pytest.mark.parametrize('scale', [1.0, 0.0], ids=['given_G', 'no_noise'])
def test_stepwise_loop_equals_the_host_twin(name, scale):
  _loop_equals_the_host_twin(name, scale)


@pytest.mark.parametrize('name,scale', gp.HAND_RUNS)
def test_stepwise_loop_equals_the_host_twin_on_the_hand_built_roots(name, scale):
  """the guarded branches (gp.underflow: sum N > 0 with sp == 0; gp._ties: every arg-max an exact tie of the whole group),
  by the bars of the sets and by the hand-made assertions of tests/test_gumbel_cpu.py on the device's own record"""
  from tests.test_gumbel_cpu import check_ties_break_to_the_largest_action, check_underflow_is_reached
  dev = _loop_equals_the_host_twin(name, scale)
  c = gp.case(name)
  if name == 'underflow':
    first = _stepwise(name, scale, False, host=_host(name, scale, 1), num_simulations=1)
    check_underflow_is_reached(first, dev, c)
  else:
    check_ties_break_to_the_largest_action(dev, c)
    assert np.array_equal(dev['sel_action'], gp.search_batch(c, scale)['sel_action'])


def _roots(A, n, seed):
  """n roots of A actions for the engine's own network: root 0 with one legal action, root 1 with all; G in 1/64"""
  rng = np.random.RandomState(seed)
  legal = np.zeros((n, A), np.uint8)
  for b in range(n):
    legal[b, rng.choice(A, 1 if b == 0 else A if b == 1 else int(rng.randint(1, A + 1)), replace=False)] = 1
  return dict(A=A, two=False, bounds=(None, None), discount=0.997, trees=n, legal=legal, to_play=np.ones(n, np.int8),
              G=rng.randint(-256, 256, (n, A)) / 64.0)


@pytest.mark.parametrize('name', list(gp.SETS)[:3] + ['b37_a18_s30', 'b37_a2_s8'])
def test_gz_search_equals_the_stepwise_loop_on_the_engines_network(name):
  """the three first sets' roots, and 37 trees -- three 16-row workgroups of the recurrent inference, the last one ragged -- of
  A = 18 (G = 32: five blocks of the tree kernels, the last ragged) with 30 simulations and of A = 2 (G = 4) with 8"""
  if name.startswith('b37'):
    c = _roots(18, 37, 0x6D01) if name == 'b37_a18_s30' else _roots(2, 37, 0x6D02)
    c['sims'] = 30 if name == 'b37_a18_s30' else 8
  else:
    c = gp.case(name)
  A, O, n, sims = c['A'], 4, c['trees'], c['sims']
  eng = _engine(c)
  eng.set_weights(weights(O, A, 5))
  eng.set_gumbel(True, gumbel_scale=1.0)
  obs = np.random.RandomState(3).uniform(-1, 1, (n, O)).astype(np.float32)

  def root():
    eng.initial_inference(obs)
    eng.root_prepare(c['to_play'], c['legal'])
    eng.gz_root(c['G'])
  root()
  eng.gz_search()
  whole = _export(eng)
  whole['hidden'] = eng.export_tree(hidden=True)['hidden']
  assert (whole['N'][:, 0] == sims).all()
  root()
  for s in range(sims):
    slot, act = eng.gz_select()
    ho, r, v, lg = eng.recurrent_inference(eng.gather_hidden(), act)
    eng.gz_expand_backup(v, r, lg, ho)
  step = _export(eng)
  step['hidden'] = eng.export_tree(hidden=True)['hidden']
  eng.close()
  for key in gp.TREE_FIELDS + ('legal', 'minmax', 'vhat', 'G', 'EX', 'action', 'pred_reward', 'pi', 'v_mix', 'hidden'):
    assert np.array_equal(whole[key], step[key]), key
  assert whole['vhat'][:, 1:].any() and (whole['pi'].sum(1) > 0.999).all()
  assert (whole['action'] < A).all() and (whole['pi'][c['legal'] == 0] == 0).all()


def test_device_drawn_gumbel_does_not_depend_on_the_batch():
  """the same game seeds in a batch of 12 at offset 100 and in a batch of 5 at offset 103: the same G and the same record"""
  c = gp.case('connect_four')
  A, O = c['A'], 4
  w = weights(O, A, 5)
  obs = np.random.RandomState(4).uniform(-1, 1, (B, O)).astype(np.float32)

  def run(lo, n, scale, move=7):
    eng = _engine(c, n=n, seed=0, env_id_offset=100 + lo)
    eng.set_weights(w)
    eng.set_gumbel(True, gumbel_scale=scale)
    eng.initial_inference(obs[lo:lo + n])
    eng.root_prepare(c['to_play'][lo:lo + n], c['legal'][lo:lo + n])
    eng.gz_root(None, move=move)
    eng.gz_search()
    d = _export(eng)
    eng.close()
    return d
  big, small = run(0, B, 1.0), run(3, 5, 1.0)
  assert big['G'].any() and len(np.unique(big['G'])) == big['G'].size
  assert np.isfinite(big['G']).all() and np.abs(big['G']).max() < 40
  for key in gp.TREE_FIELDS + ('G', 'vhat', 'action', 'pi', 'v_mix', 'minmax'):
    assert np.array_equal(big[key][3:8], small[key]), key
  assert not np.array_equal(run(0, B, 1.0, move=8)['G'], big['G'])      # the move is in the key
  plain, again = run(0, B, 0.0), run(0, B, 0.0, move=8)
  assert not plain['G'].any()
  for key in gp.TREE_FIELDS + ('action', 'pi', 'v_mix'):
    assert np.array_equal(plain[key], again[key]), key
  assert not np.array_equal(plain['N'], big['N'])      # (the draws matter)


# ---- games and matches: B = 8 games, 8 simulations
GAMES, GSIMS, SEED0 = 8, 8, 4100
GZ = dict(max_considered=4, c_visit=50.0, c_scale=1.0, gumbel_scale=1.0)


def _host_env(env):
  from model_based_rl_amd import envs
  e = envs.TicTacToe() if env == 'TicTacToe' else envs.ConnectFour()
  e.reset()
  return e


def _search_rows(state, rows, gumbel):
  """rows (one searched position each: its game, ply, board, turn, legal) through one engine shaped like the match's -- tree b
  is the game of seed SEED0 + b, one call per (seating, ply), so the device draws are keyed as the match keys them: the
  plain search at temperature 0, or the Gumbel one"""
  from model_based_rl_amd.engine import Engine
  cfg = state['config']
  A, O = int(cfg.action_space), int(np.prod(cfg.obs_space))
  eng = Engine.from_config(cfg, GAMES, seed=0, env_id_offset=SEED0)
  eng.set_weights(state['weights'])
  if gumbel:
    eng.set_gumbel(True, **gumbel)
  groups = {}
  for i, r in enumerate(rows):
    groups.setdefault((r['g'].seating, r['ply']), []).append(i)
  out = [None] * len(rows)
  for (_, ply), idx in sorted(groups.items()):
    obs, legal, to_play = np.zeros((GAMES, O), np.float32), np.ones((GAMES, A), np.uint8), np.ones(GAMES, np.int8)
    for i in idx:
      r, b = rows[i], rows[i]['g'].seed - SEED0
      obs[b], legal[b], to_play[b] = (r['board'].astype(np.int32) * r['turn']).astype(np.float32), r['legal'], r['turn']
    eng.initial_inference(obs)
    eng.root_prepare(to_play, legal)
    if gumbel:
      eng.gz_root(None, move=ply)
      eng.gz_search()
      a, pr, _, _ = eng.gz_pick()
      actions, preds = a.cpu().numpy(), pr.cpu().numpy()
      depths = eng.eval_walk(1, 0.0, np.zeros((GAMES, 1)))['path_lengths'].cpu().numpy()
    else:
      eng.search()
      w = eng.eval_walk(1, 0.0, None, move=ply)      # (a tie among the most visited is broken by the device draw the match uses)
      actions, preds, depths = w['actions'].cpu().numpy()[:, 0], w['pred_rewards'].cpu().numpy()[:, 0], w['path_lengths'].cpu().numpy()
    fin = eng.finalize(0.0, np.full(GAMES, 0.5), move=ply)
    visits, rv, pv = fin['child_visits'].cpu().numpy(), fin['root_value'].cpu().numpy(), eng.root_outputs()[0].cpu().numpy()
    for i in idx:
      b = rows[i]['g'].seed - SEED0
      out[i] = dict(action=int(actions[b]), pred=float(preds[b]), depths=[int(x) for x in depths[b]], visits=[float(x) for x in visits[b]],
                    root_value=float(rv[b]), pred_value=float(pv[b]))
  eng.close()
  return out


def _python_loop(env, state, seeds, gumbel):
  """the games driven move by move from Python on the host rules, every game in the batch the device path uses"""
  from model_based_rl_amd.engine import Engine
  cfg = state['config']
  n, A, O = len(seeds), int(cfg.action_space), int(np.prod(cfg.obs_space))
  eng = Engine.from_config(cfg, n, seed=0, env_id_offset=seeds[0])
  eng.set_weights(state['weights'])
  eng.set_gumbel(True, **gumbel)
  envs = [_host_env(env) for _ in range(n)]
  done = [False] * n
  logs = [dict(step=0, actions=[], rewards=[], to_play=[], dones=[], child_visits=[], root_values=[], pred_values=[], pred_rewards=[],
               search_depths=[]) for _ in range(n)]
  move = 0
  while not all(done):
    obs, legal, to_play = np.zeros((n, O), np.float32), np.ones((n, A), np.uint8), np.ones(n, np.int8)
    for i, e in enumerate(envs):
      if done[i]:
        continue
      obs[i] = (e.turn * e.board).astype(np.float32)
      legal[i] = 0
      legal[i, e.legal_actions()] = 1
      to_play[i] = e.turn
    eng.initial_inference(obs)
    eng.root_prepare(to_play, legal)
    eng.gz_root(None, move=move)
    eng.gz_search()
    a, pr, _, _ = eng.gz_pick()
    depths = eng.eval_walk(1, 0.0, np.zeros((n, 1)), move=move)['path_lengths'].cpu().numpy()
    fin = eng.finalize(0.0, np.full(n, 0.5), move=move)
    pv = eng.root_outputs()[0].cpu().numpy()
    actions, preds = a.cpu().numpy(), pr.cpu().numpy()
    visits, rv = fin['child_visits'].cpu().numpy(), fin['root_value'].cpu().numpy()
    for i, e in enumerate(envs):
      if done[i]:
        continue
      L = logs[i]
      mover = e.turn
      _, reward, d, _ = e.step(int(actions[i]))
      L['actions'].append(int(actions[i])); L['rewards'].append(float(reward)); L['to_play'].append(int(mover)); L['dones'].append(bool(d))
      L['child_visits'].append([float(x) for x in visits[i]]); L['root_values'].append(float(rv[i])); L['pred_values'].append(float(pv[i]))
      L['pred_rewards'].append(float(preds[i])); L['search_depths'].append([int(x) for x in depths[i]])
      L['step'] += 1
      done[i] = bool(d) or L['step'] >= cfg.max_steps
    move += 1
  eng.close()
  return logs


@functools.lru_cache(maxsize=None)
def _device_games(env, mode):
  """mode 'gumbel': play_games(gumbel=GZ); 'never': the flag never named; 'unset': an Evaluator whose config names gumbel 0"""
  from model_based_rl_amd.evaluate import Evaluator
  state = eval_state(env, sims=GSIMS, **(dict(gumbel=0) if mode == 'unset' else {}))
  seeds = list(range(SEED0, SEED0 + GAMES))
  ev = Evaluator(state)
  ev.load_network()
  kw = dict(gumbel=dict(GZ)) if mode == 'gumbel' else dict(gumbel=False) if mode == 'unset' else {}
  games = ev.play_games(GAMES, seeds, device_env=True, keep_history=True, **kw)
  return state, seeds, [record(g) for g in games]


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_games_equal_the_python_driven_loop(env):
  state, seeds, got = _device_games(env, 'gumbel')
  want = _python_loop(env, state, seeds, GZ)
  for i, (g, w) in enumerate(zip(got, want)):
    for key in w:
      assert g[key] == w[key], (env, seeds[i], key)
  assert all(all(x > 0 for x in d) for g in got for d in g['search_depths'])      # every simulation expands a node
  assert got != _device_games(env, 'never')[2]


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_the_mode_off_is_the_parent_behaviour(env):
  from model_based_rl_amd.match import play_match
  assert _device_games(env, 'never')[2] == _device_games(env, 'unset')[2]
  state, seeds, _ = _device_games(env, 'never')
  never, s0 = play_match(state, state, GAMES, seeds, keep_history=True)
  unset, s1 = play_match(state, state, GAMES, seeds, keep_history=True, gumbel=(0, 0))
  assert [record(g) for g in never] == [record(g) for g in unset]
  assert s0 == s1 and s0['gumbel'] == [0, 0]


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_each_side_of_a_match_runs_its_own_kind_of_search(env):
  from model_based_rl_amd.match import play_match
  state = eval_state(env, sims=GSIMS)
  seeds = list(range(SEED0, SEED0 + GAMES))
  games, summary = play_match(state, state, GAMES, seeds, keep_history=True, gumbel=(0, dict(GZ)))
  assert summary['gumbel'] == [0, 1] and sorted(set(g.seating for g in games)) == [0, 1]
  rows = {0: [], 1: []}
  for g in games:
    e = _host_env(env)
    for p, a in enumerate(g.history.actions):
      legal = np.zeros(int(state['config'].action_space), np.uint8)
      legal[e.legal_actions()] = 1
      assert g.nets[p] == (p + g.seating) % 2
      rows[g.nets[p]].append(dict(g=g, ply=p, board=e.board.astype(np.int8).copy(), turn=int(e.turn), legal=legal))
      e.step(a)
  for net in (0, 1):
    out = _search_rows(state, rows[net], GZ if net else None)
    for r, o in zip(rows[net], out):
      g, p = r['g'], r['ply']
      at = (env, g.seed, g.seating, p, net)
      assert g.history.actions[p] == o['action'], at
      assert g.pred_rewards[p] == o['pred'], at
      assert g.history.child_visits[p] == o['visits'], at
      assert g.history.root_values[p] == o['root_value'] and g.pred_values[p] == o['pred_value'], at
      assert g.search_depths[p] == o['depths'], at


def test_grade_on_gumbel_games_reports_the_plain_keys():
  from model_based_rl_amd.evaluate import Evaluator
  reports = []
  for gz in (0, 1):
    state = eval_state('TicTacToe', sims=GSIMS, grade=True, grade_table=False, grade_empties=12, grade_nodes=4096, grade_unroll=None,
                       device_env=True, gumbel=gz)
    ev = Evaluator(state)
    ev.load_network()
    ev.play_games(16, list(range(SEED0, SEED0 + 16)))
    reports.append(ev.grade_report)
  assert reports[1] is not None and sorted(reports[0]) == sorted(reports[1])


def test_cartpole_is_served():
  from model_based_rl_amd.evaluate import Evaluator
  state = eval_state('CartPole-v0', sims=GSIMS, max_steps=12)
  ev = Evaluator(state)
  ev.load_network()
  games = ev.play_games(4, [5, 6, 7, 8], device_env=True, keep_history=True, gumbel=True)
  assert all(1 <= g.step <= 12 and all(a in (0, 1) for a in g.history.actions) for g in games)


def test_engine_refusals():
  from model_based_rl_amd.engine import Engine
  eng = Engine(4, 9, 9, 4, two_players=True)
  with pytest.raises(RuntimeError, match='mz_gz_root: no Gumbel search is set'):
    eng.gz_root()
  for kw, why in ((dict(max_considered=1), 'max_considered must be >= 2'), (dict(c_visit=-1.0), 'c_visit must be >= 0'),
                  (dict(c_scale=0.0), 'c_scale must be > 0'), (dict(gumbel_scale=-1.0), 'gumbel_scale must be >= 0')):
    with pytest.raises(RuntimeError, match='mz_set_gumbel: ' + why):
      eng.set_gumbel(True, **kw)
  eng.set_true_model(1)
  with pytest.raises(RuntimeError, match='mz_set_gumbel: the true-rules search is set'):
    eng.set_gumbel(True)
  eng.set_true_model(0)
  eng.set_gumbel(True)
  with pytest.raises(RuntimeError, match='mz_set_true_model: the Gumbel search is set'):
    eng.set_true_model(1)
  with pytest.raises(RuntimeError, match='mz_gz_root: call mz_root_prepare first'):
    eng.gz_root()
  with pytest.raises(RuntimeError, match='mz_gz_select: call mz_gz_root first'):
    eng.gz_select()
  with pytest.raises(RuntimeError, match='mz_gz_pick: call mz_gz_root first'):
    eng.gz_pick()
  eng.root_load(np.zeros(4, np.float32), np.zeros((4, 9), np.float32), np.zeros((4, 50), np.float32))
  noise = np.full((4, 9), 1.0 / 9)
  eng.root_prepare(noise=noise)
  with pytest.raises(RuntimeError, match='mz_gz_root: this root was prepared with exploration noise'):
    eng.gz_root()
  eng.root_prepare()
  eng.gz_root()
  with pytest.raises(RuntimeError, match='mz_gz_pick: no simulation was run'):
    eng.gz_pick()
  z = np.zeros(4, np.float32)
  with pytest.raises(RuntimeError, match='mz_gz_search: weights not set'):
    eng.gz_search()
  for s in range(4):
    eng.gz_select()
    eng.gz_expand_backup(z, z, np.zeros((4, 9), np.float32), np.zeros((4, 50), np.float32))
  with pytest.raises(RuntimeError, match='mz_gz_expand_backup: call mz_gz_select first'):
    eng.gz_expand_backup(z, z, np.zeros((4, 9), np.float32))
  with pytest.raises(RuntimeError, match='mz_gz_select: all 4 simulations already done'):
    eng.gz_select()
  eng.set_weights(weights(9, 9, 5))
  # the games refuse what the search does not serve, one sentence each
  eng.eval_env_reset('TicTacToe', 9)
  for mode, M, noise_on, why in ((0, 2, False, 'one action per move'), (1, 1, False, 'only_prior / only_value'),
                                 (0, 1, True, 'replaces the exploration noise')):      # (the first call sizes the walk)
    with pytest.raises(RuntimeError, match='gumbel: .*' + why):
      eng.eval_env_moves(1, mode, M, 0.0, noise_on)
  eng.set_gumbel(False)      # off again: the plain search
  eng.eval_env_reset('TicTacToe', 9)
  assert eng.eval_env_moves(1) == 4
  eng.close()
