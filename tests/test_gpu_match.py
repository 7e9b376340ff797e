"""Matches between two networks on the device games (csrc/mz_match.hip.h, match.play_match).  Every comparison is exact.
  self      a network against itself is the single-network game of Evaluator.play_games(device_env=True), in both seatings
  mover     every searched ply is the mover's own search: the positions rebuilt on the host classes and run through a
            plain Engine of that net and simulation count give the logged visits, values, depths and action
  openings  the counter RNG's opening plies, the same in both seatings; a game an opening ply wins
  batches   a seed's record does not depend on the batch it was played in
  mixed     search against only_prior / only_value; the per-network accumulators against the logs
  cut       max_steps ends games as draws; live reaches 0; a second reset replays identically
  CLI       evaluate.main(--match), two nets and a round robin of three
Shapes: 8 and 5 simulations, 70 games (one partial 128-thread block) and 130 (two blocks); 16-row padding non-trivial."""
import functools
import json
import os

import numpy as np
import pytest

from tests.eval_device_util import eval_state, philox_uniform, record

pytestmark = pytest.mark.gpu

N, SEED0, SIMS_A, SIMS_B = 70, 2000, 8, 5
LONGEST = {'TicTacToe': 9, 'ConnectFour': 42}
MZ_RNG_OPEN = 8


def _host_env(env):
  from model_based_rl_amd import envs
  e = envs.TicTacToe() if env == 'TicTacToe' else envs.ConnectFour()
  e.reset()
  return e


def _states(env, over_a=None, over_b=None, **both):
  """networks A (weights seed 5, 8 simulations) and B (seed 6, 5 simulations)"""
  a = eval_state(env, sims=SIMS_A, wseed=5, **dict(both, **(over_a or {})))
  b = eval_state(env, sims=SIMS_B, wseed=6, **dict(both, **(over_b or {})))
  return a, b


def _given_draws(rng, env, n, A, opening):
  """every draw of n games: walk uniforms and Dirichlet draws per ply, opening indices below the fewest legal actions an
  opening position can have (nine cells less the stones; seven columns, none full within six plies)"""
  cap = LONGEST[env]
  nmin = [9 - p if env == 'TicTacToe' else 7 for p in range(opening)]
  return [dict(walk=[float(rng.uniform()) for _ in range(cap)], noise=[rng.dirichlet([0.25] * A) for _ in range(cap)],
               opening=[int(rng.randint(0, m)) for m in nmin]) for _ in range(n)]


def _mrecord(g):
  """everything a match record carries"""
  out = record(g)
  out.update(seed=g.seed, seating=g.seating, result=g.result, nets=list(g.nets), searched=g.searched, pred_return=g.pred_return,
             pred_value=g.pred_value, mcts_value=g.mcts_value, search_depth=g.search_depth)
  return out


def _replay(env, g, max_steps):
  """g's logged actions on the host class -> (the searched positions in ply order, the winner's colour or 0); the logged
  movers, rewards, dones and the game's length are the host class's"""
  e = _host_env(env)
  h = g.history
  positions, winner = [], 0
  assert g.step == len(h.actions) == len(h.rewards) == len(g.nets) <= max_steps
  for p, a in enumerate(h.actions):
    legal = [int(x) for x in e.legal_actions()]
    assert a in legal and h.to_play[p] == e.turn, (g.seed, p)
    if g.nets[p] >= 0:
      mask = np.zeros(len(e.board) if env == 'TicTacToe' else 7, np.uint8)
      mask[legal] = 1
      positions.append(dict(ply=p, net=g.nets[p], obs=(e.turn * e.board).astype(np.float32), legal=mask, to_play=e.turn))
    mover = e.turn
    _, reward, done, _ = e.step(a)
    assert h.rewards[p] == float(reward) and h.dones[p] == bool(done), (g.seed, p)
    if reward:
      winner = mover
    assert (bool(done) or p + 1 >= max_steps) == (p == g.step - 1), (g.seed, p)
  assert len(positions) == len(h.child_visits) == len(g.pred_values) == sum(g.searched)
  return positions, winner


def _colour_a(seating, opening):
  return 1 if (seating == 0) == (opening % 2 == 0) else -1


def _check_on_plain_engine(env, state, net, games, draws_by_seed, max_steps):
  """every position `net` moved in, as ONE batch through a plain Engine of that net: initial_inference, root_prepare,
  then search + eval_walk + finalize or eval_lookahead; against the logs"""
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.match import _side
  cfg = state['config']
  mode, T, noise_on = _side(cfg)
  rows = []
  for g in games:
    positions, _ = _replay(env, g, max_steps)
    for k, pos in enumerate(positions):
      if pos['net'] == net:
        rows.append((g, k, pos))
  n = len(rows)
  assert n > 0
  A = int(cfg.action_space)
  obs = np.stack([pos['obs'] for _, _, pos in rows])
  legal = np.stack([pos['legal'] for _, _, pos in rows])
  to_play = np.array([pos['to_play'] for _, _, pos in rows], np.int8)
  noise = None
  if noise_on:
    noise = np.stack([np.asarray(draws_by_seed[g.seed]['noise'][pos['ply']], np.float64) * pos['legal'] for g, _, pos in rows])
  uniform = np.array([[draws_by_seed[g.seed]['walk'][pos['ply']]] for g, _, pos in rows], np.float64)
  eng = Engine.from_config(cfg, n, seed=0, env_id_offset=0)
  eng.set_weights(state['weights'])
  eng.initial_inference(obs)
  eng.root_prepare(to_play, legal, noise, device_rng=False)
  pred_value = eng.root_outputs()[0].cpu().numpy()
  if mode == 0:
    eng.search()
    w = eng.eval_walk(1, T, uniform)
    fin = eng.finalize(0.0, np.full(n, 0.5))
    actions, preds = w['actions'].cpu().numpy()[:, 0], w['pred_rewards'].cpu().numpy()[:, 0]
    depths = w['path_lengths'].cpu().numpy()
    visits, root_values = fin['child_visits'].cpu().numpy(), fin['root_value'].cpu().numpy()
  else:
    out = eng.eval_lookahead(mode)
    actions, preds, visits = out['action'].cpu().numpy(), out['pred_reward'].cpu().numpy(), out['child_visits'].cpu().numpy()
    root_values = np.zeros(n)
    depths = np.full((n, 1), 0 if mode == 1 else 1)
  eng.close()
  for i, (g, k, pos) in enumerate(rows):
    at = (g.seed, g.seating, pos['ply'])
    assert g.history.actions[pos['ply']] == int(actions[i]), at
    assert g.history.child_visits[k] == [float(x) for x in visits[i]], at
    assert g.history.root_values[k] == float(root_values[i]), at
    assert g.pred_values[k] == float(pred_value[i]), at
    assert g.pred_rewards[k] == float(preds[i]), at
    assert g.search_depths[k] == [int(x) for x in depths[i]], at
  return n


def _check_results(env, games, summary, opening, max_steps):
  """results, lengths and the summary's W / D / L against the host replay"""
  counts = {1: 0, 0: 0, -1: 0}
  for g in games:
    _, winner = _replay(env, g, max_steps)
    assert g.result == winner * _colour_a(g.seating, opening), (g.seed, g.seating)
    counts[g.result] += 1
  assert (summary['wins'], summary['draws'], summary['losses']) == (counts[1], counts[0], counts[-1])
  assert summary['games'] == len(games) and summary['mean_length'] == float(np.mean([g.step for g in games]))
  for key, seating in (('a_first', 0), ('b_first', 1)):
    r = [g.result for g in games if g.seating == seating]
    assert (summary[key]['wins'], summary[key]['draws'], summary[key]['losses']) == (r.count(1), r.count(0), r.count(-1))


# ---- 1. a network against itself is the single-network game
SELF = {
    'search_t0': dict(),
    'search_t0_noise': dict(use_exploration_noise=1),
    'search_t05': dict(temperature=0.5),
    'search_t05_noise': dict(temperature=0.5, use_exploration_noise=1),
    'only_prior': dict(only_prior=1),
    'only_prior_noise': dict(only_prior=1, use_exploration_noise=1),
    'only_value': dict(only_value=1),
}


@pytest.mark.parametrize('name', sorted(SELF))
@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_a_network_against_itself_is_the_single_network_game(env, name):
  from model_based_rl_amd.evaluate import Evaluator
  from model_based_rl_amd.match import play_match
  state = eval_state(env, sims=SIMS_A, **SELF[name])
  seeds = list(range(SEED0, SEED0 + N))
  games, summary = play_match(state, state, N, seeds, keep_history=True)
  ev = Evaluator(state)
  ev.load_network()
  single = [record(g) for g in ev.play_games(N, seeds, device_env=True, keep_history=True)]
  assert len(games) == 2 * N and [g.seating for g in games] == [0] * N + [1] * N
  for g in games:
    want = single[g.seed - SEED0]
    got = record(g)
    for key in want:
      assert got[key] == want[key], (env, name, g.seed, g.seating, key)      # exact: the same launches with the same keys
    assert g.nets == [(p + g.seating) % 2 for p in range(g.step)]
  if 'noise' in name or 't05' in name:      # (drawn games differ: finished games sat beside live ones)
    assert len(set(g.step for g in games)) > 1
  assert summary['games'] == 2 * N


# ---- 2. each ply is the mover's own search
@functools.lru_cache(maxsize=None)
def _two_nets(env):
  from model_based_rl_amd.match import play_match
  a, b = _states(env, over_a=dict(temperature=0.0), over_b=dict(temperature=0.5), use_exploration_noise=1)
  A = int(a['config'].action_space)
  seeds = list(range(SEED0, SEED0 + N))
  draws = _given_draws(np.random.RandomState(11 + A), env, N, A, 2)
  games, summary = play_match(a, b, N, seeds, opening_plies=2, draws=draws, keep_history=True)
  return a, b, seeds, draws, games, summary


@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_each_ply_is_the_movers_own_search(env):
  a, b, seeds, draws, games, summary = _two_nets(env)
  by_seed = dict(zip(seeds, draws))
  max_steps = int(a['config'].max_steps)
  assert len(games) == 2 * N
  for g in games:      # the opening, then the two nets in turn, the seating's first
    assert g.nets[:2] == [-1, -1] and g.nets[2:] == [(p + g.seating) % 2 for p in range(g.step - 2)], (g.seed, g.seating)
    assert g.history.actions[:2] == [_nth_legal(env, g.history.actions[:p], by_seed[g.seed]['opening'][p]) for p in range(2)]
  na = _check_on_plain_engine(env, a, 0, games, by_seed, max_steps)
  nb = _check_on_plain_engine(env, b, 1, games, by_seed, max_steps)
  assert na + nb == sum(g.step - 2 for g in games) and na > N and nb > N
  assert all(len(d) == (SIMS_A if net == 0 else SIMS_B) for g in games for d, net in zip(g.search_depths, g.searched_by))
  _check_results(env, games, summary, 2, max_steps)
  assert len(set(g.result for g in games)) > 1      # (the two nets do not play alike)


def _nth_legal(env, actions_before, idx):
  e = _host_env(env)
  for a in actions_before:
    e.step(a)
  legal = [int(x) for x in e.legal_actions()]
  return legal[min(idx, len(legal) - 1)]


# ---- 3. openings
@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_openings_are_the_counter_rngs_and_alike_in_both_seatings(env):
  from model_based_rl_amd.match import play_match
  a, b = _states(env)
  seeds = list(range(SEED0, SEED0 + N))
  games, _ = play_match(a, b, N, seeds, opening_plies=3, keep_history=True)
  firsts = {}
  for g in games:
    e = _host_env(env)
    for p in range(3):
      legal = [int(x) for x in e.legal_actions()]
      u = philox_uniform(0, g.seed, p, MZ_RNG_OPEN)
      assert g.history.actions[p] == legal[min(int(np.floor(u * len(legal))), len(legal) - 1)], (g.seed, g.seating, p)
      e.step(g.history.actions[p])
    assert g.nets[:3] == [-1, -1, -1] and g.nets[3] == g.seating
    firsts.setdefault(g.seed, []).append(g.history.actions[:3])
  assert all(len(v) == 2 and v[0] == v[1] for v in firsts.values())
  assert len(set(str(v[0]) for v in firsts.values())) > N // 4      # (different seeds, different openings)


def test_an_opening_ply_that_wins_ends_the_game():
  from model_based_rl_amd.match import play_match
  a, b = _states('ConnectFour')
  seeds = list(range(SEED0, SEED0 + N))
  # even games: +1 stacks column 0 and wins with the seventh ply; odd games: nobody has won after seven plies
  draws = [dict(opening=[0, 1, 0, 1, 0, 1, 0] if i % 2 == 0 else [3, 3, 3, 3, 3, 3, 2]) for i in range(N)]
  games, summary = play_match(a, b, N, seeds, opening_plies=7, draws=draws, keep_history=True)
  for g in games:
    if (g.seed - SEED0) % 2 == 0:
      assert g.step == 7 and g.history.actions == [0, 1, 0, 1, 0, 1, 0] and g.nets == [-1] * 7
      assert g.history.dones == [False] * 6 + [True] and g.history.rewards[-1] == 1.0
      assert g.searched == (0, 0) and g.history.child_visits == []
      assert g.result == (-1 if g.seating == 0 else 1)      # (after seven plies the seating's first net is player -1)
    else:
      assert g.step > 7 and g.history.actions[:7] == [3, 3, 3, 3, 3, 3, 2] and g.nets[7] == g.seating
  _check_results('ConnectFour', games, summary, 7, 42)


# ---- 4. batch invariance
def test_a_seeds_record_does_not_depend_on_the_batch():
  from model_based_rl_amd.match import play_match
  a, b = _states('ConnectFour', temperature=0.5, use_exploration_noise=1)
  big, _ = play_match(a, b, 130, list(range(500, 630)), opening_plies=1, keep_history=True, batch=130)
  s = 500 + 127      # (games 127, 128, 129 of the large batch: the last thread of its first block and the second block)
  small, _ = play_match(a, b, 3, [s, s + 1, s + 2], opening_plies=1, keep_history=True, batch=3)
  want = {(g.seed, g.seating): _mrecord(g) for g in big}
  assert len(want) == 260 and len(small) == 6
  for g in small:
    assert _mrecord(g) == want[(g.seed, g.seating)], (g.seed, g.seating)
  assert len(set(str(g.history.actions) for g in big)) > 130      # (different seeds, different games)


# ---- 5. mixed sides
MIXED = {'prior': (dict(), dict(only_prior=1)), 'value': (dict(only_value=1), dict(temperature=0.5)),
         'prior_value': (dict(only_prior=1), dict(only_value=1))}


@pytest.mark.parametrize('name', sorted(MIXED))
@pytest.mark.parametrize('env', ['TicTacToe', 'ConnectFour'])
def test_mixed_sides_and_the_per_network_accumulators(env, name):
  from model_based_rl_amd.match import play_match
  a, b = _states(env, over_a=MIXED[name][0], over_b=MIXED[name][1], use_exploration_noise=1)
  A = int(a['config'].action_space)
  seeds = list(range(SEED0, SEED0 + N))
  draws = _given_draws(np.random.RandomState(3 + A), env, N, A, 1)
  games, summary = play_match(a, b, N, seeds, opening_plies=1, draws=draws, keep_history=True)
  by_seed = dict(zip(seeds, draws))
  max_steps = int(a['config'].max_steps)
  _check_on_plain_engine(env, a, 0, games, by_seed, max_steps)
  _check_on_plain_engine(env, b, 1, games, by_seed, max_steps)
  _check_results(env, games, summary, 1, max_steps)
  for g in games:      # the accumulators: float64 sums of the logs in ply order, per network
    for net in (0, 1):
      ks = [k for k, who in enumerate(g.searched_by) if who == net]
      assert g.searched[net] == len(ks)
      if not ks:
        continue
      pv = rv = pr = 0.0
      for k in ks:
        pv, rv, pr = pv + g.pred_values[k], rv + g.history.root_values[k], pr + g.pred_rewards[k]
      at = (g.seed, g.seating, net)
      assert g.pred_value[net] == pv / len(ks) and g.mcts_value[net] == rv / len(ks) and g.pred_return[net] == pr, at
      assert g.search_depth[net] == float(np.mean(max(g.search_depths[k] for k in ks))), at


# ---- 6. the cut
@pytest.mark.parametrize('env,max_steps', [('TicTacToe', 5), ('ConnectFour', 11)])
def test_the_cut_at_max_steps(env, max_steps):
  from model_based_rl_amd.engine import Engine, Match
  from model_based_rl_amd.match import play_match
  a, b = _states(env, max_steps=max_steps, temperature=0.5)
  seeds = list(range(SEED0, SEED0 + N))
  games, summary = play_match(a, b, N, seeds, keep_history=True)
  _check_results(env, games, summary, 0, max_steps)
  cut = [g for g in games if g.step == max_steps and not any(g.history.dones)]
  assert cut and all(g.result == 0 for g in cut) and max(g.step for g in games) == max_steps
  # games the rules ended keep their result (TicTacToe's earliest win is its fifth ply: on the cut, and still a win)
  decided = [g for g in games if g.history.dones[-1] and g.history.rewards[-1] == 1.0]
  assert all(g.result == (1 if g.history.to_play[-1] == _colour_a(g.seating, 0) else -1) for g in decided)
  print(env, 'cut', len(cut), 'decided', len(decided), 'of', len(games))
  if env == 'TicTacToe':
    assert decided
  # the handle itself: live reaches 0 with the last chunk, and a second reset replays identically
  engines = [Engine.from_config(s['config'], N, seed=0, env_id_offset=SEED0) for s in (a, b)]
  for e, s in zip(engines, (a, b)):
    e.set_weights(s['weights'])
  m = Match(engines[0], engines[1], env, max_steps, keep_history=True)
  assert m.log_cap == max_steps
  runs = []
  for _ in range(2):
    m.reset(first_net=0, opening_plies=0)
    live, done = N, 0
    while done < max_steps:
      n = min(8, max_steps - done)
      live = m.plies(n, (0, 0), (0.5, 0.5), (False, False))
      done += n
    assert live == 0
    runs.append(m.results())
    with pytest.raises(RuntimeError, match='draws are given before the first ply'):
      m.set_draws(walk=np.zeros((N, 1)))
  for key in runs[0]:
    assert np.array_equal(runs[0][key], runs[1][key]), key
  first = [g for g in games if g.seating == 0]
  assert [int(x) for x in runs[0]['length']] == [g.step for g in first]
  assert [int(x) for x in runs[0]['result']] == [g.result for g in first]      # (no opening, seating 0: A is player +1)
  # refusals of the handle
  with pytest.raises(RuntimeError, match='opening_plies'):
    m.reset(0, max_steps)
  m.close()
  one = Engine(N, engines[0].O, engines[0].A, SIMS_A, two_players=False, seed=0, env_id_offset=SEED0)
  other = Engine(N + 1, engines[0].O, engines[0].A, SIMS_A, two_players=True, seed=0, env_id_offset=SEED0)
  for args, word in (((engines[0], one, env), 'single-player'), ((engines[0], other, env), 'different numbers of games'),
                     ((engines[0], engines[1], 'CartPole-v0'), 'CartPole')):
    with pytest.raises(RuntimeError, match=word):
      Match(args[0], args[1], args[2], max_steps)
  for e in engines + [one, other]:
    e.close()


# ---- 7. CLI
def _checkpoints(tmp_path):
  import torch
  saves = tmp_path / 'runs' / 'TicTacToe' / 'g' / 'r' / 'saves'
  saves.mkdir(parents=True)
  for step, wseed in ((10, 5), (20, 6), (30, 7)):
    state = eval_state('TicTacToe', sims=SIMS_A, wseed=wseed)
    torch.save({'dirs': {}, 'config': state['config'], 'weights': state['weights'], 'optimizer': {}, 'training_step': step},
               str(saves / str(step)))
  return str(saves) + os.sep


def test_cli(tmp_path, capsys):
  from model_based_rl_amd import evaluate
  saves = _checkpoints(tmp_path)
  out = tmp_path / 'match.json'
  res = evaluate.main(['--match', '--saves_dir', saves, '--nets', '10', '20', '--num_games', '24', '--seed', '0', '--batch', '16',
                       '--opening_plies', '1', '--num_simulations', '8', '5', '--out', str(out)])
  js = json.load(open(str(out)))
  assert js['pairs'] == json.loads(json.dumps(res['pairs'])) and len(js['pairs']) == 1
  p = js['pairs'][0]
  assert p['wins'] + p['draws'] + p['losses'] == 48 == p['games']
  assert p['a_first']['games'] == p['b_first']['games'] == 24
  assert 'sims:8' in p['a'] and 'sims:5' in p['b'] and 'net:10' in p['a'] and 'net:20' in p['b']
  assert abs(p['score'] - (p['wins'] + 0.5 * p['draws']) / 48) < 1e-15
  assert 'score' in capsys.readouterr().out
  rr = evaluate.main(['--match', '--saves_dir', saves, '--nets', '10', '20', '30', '--num_games', '8', '--seed', '3', '--out', str(out)])
  js = json.load(open(str(out)))
  assert [(p['a_index'], p['b_index']) for p in js['pairs']] == [(0, 1), (0, 2), (1, 2)] and len(rr['pairs']) == 3
  assert all(p['games'] == 16 for p in js['pairs'])
  t = js['cross_table']
  assert len(t) == 3 and all(len(row) == 3 for row in t) and all(t[i][i] is None for i in range(3))
  assert all(abs(t[i][j] + t[j][i] - 1.0) < 1e-15 for i in range(3) for j in range(3) if i != j)
  assert 'row against column' in capsys.readouterr().out
