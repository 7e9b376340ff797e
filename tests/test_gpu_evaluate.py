"""The evaluator on the GPU (csrc/mz_eval.hip.h, model_based_rl_amd.evaluate):
  walk       mz_eval_walk against a numpy restatement of evaluate.py:314-326 over the exported trees (actions, n_actions
             exact, predicted rewards bit-identical) and its search depths against the stepwise descent's (mz_select)
  lookahead  mz_eval_lookahead's rows bit-identical to mz_recurrent_inference on the same rows; its choices, rewards and
             child visits as evaluate.py:278-304 computes them from those rows and the tree's priors
  batches    a game's record does not depend on the batch it was played in
  CLI        evaluate.main on a checkpoint in Learner.save_state's format"""
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 4096


def _weights(O, A, seed, no_support=False, scale_heads=3.0):
  import torch
  from model_based_rl_amd.networks import FCNetwork
  torch.manual_seed(seed)
  cfg = types.SimpleNamespace(value_support=(-15, 15), reward_support=(-15, 15), no_support=no_support,
                              no_target_transform=False)
  w = {k: v.numpy().copy() for k, v in FCNetwork(O, A, torch.device('cpu'), cfg).state_dict().items()}
  for k in w:
    if k.endswith('value.weight') or k.endswith('reward.weight'):
      w[k] = (w[k] * scale_heads).astype(np.float32)
  return w


def _roots(rng, n, A, two_players):
  legal = (rng.uniform(size=(n, A)) < 0.7).astype(np.uint8)
  legal[np.arange(n), rng.randint(0, A, size=n)] = 1
  to_play = (rng.randint(0, 2, size=n) * 2 - 1).astype(np.int8) if two_players else None
  noise = np.zeros((n, A))
  for i in range(n):
    idx = np.flatnonzero(legal[i])
    noise[i, idx] = rng.dirichlet([0.25] * len(idx))
  return legal, to_play, noise


def np_walk(ex, A, M, T, U):
  """evaluate.py:314-326 with Config.select_action (config.py:70-81) restated as mz_sample_index computes it, vectorised
  over the trees: children = the legal actions in ascending order at the root, range(A) below it"""
  N, E, R, legal = ex['N'], ex['E'], ex['R'], ex['legal']
  n, NN = N.shape
  rows = np.arange(n)
  node = np.zeros(n, np.int64)
  active = np.ones(n, bool)
  actions = np.full((n, M), -1, np.int32)
  rewards = np.zeros((n, M), np.float32)
  n_actions = np.zeros(n, np.int32)
  legal_bits = ((legal[:, None] >> np.arange(A)) & 1).astype(bool)
  for step in range(M):
    e = E[rows, node]
    active &= e >= 0
    if not active.any():
      break
    base = 1 + np.maximum(e, 0) * A
    kids = np.minimum(base[:, None] + np.arange(A), NN - 1)
    cnt = N[rows[:, None], kids].astype(np.float64)
    valid = np.where((node == 0)[:, None], legal_bits, True)
    nv = valid.sum(1)
    u = U[:, step]
    if T == 0:
      m = np.where(valid, cnt, -1.0).max(1)
      tie = valid & (cnt == m[:, None])
      nt = tie.sum(1)
      k = np.minimum((u * nt).astype(np.int64), nt - 1)
      pos = np.argmax(tie & (np.cumsum(tie, 1) == (k + 1)[:, None]), axis=1)
    else:
      with np.errstate(invalid='ignore', divide='ignore'):
        ex_ = 1 / T
        d = np.where(valid, cnt ** ex_ if ex_ != 1.0 else cnt, 0.0)
        s = d.sum(1)                                     # integers: exact in any order
        d = d / s[:, None]
        c = np.cumsum(d, 1)
        c = c / c[:, -1:]
        idx = (valid & (c <= u[:, None])).sum(1)           # searchsorted(side='right') over the legal entries
      idx = np.minimum(idx, nv - 1)
      pos = np.argmax(valid & (np.cumsum(valid, 1) == (idx + 1)[:, None]), axis=1)
    ch = base + pos
    sel = active & (nv > 0)
    actions[sel, step] = pos[sel]
    rewards[sel, step] = R[rows[sel], ch[sel]]
    n_actions[sel] += 1
    active = sel
    node = np.where(sel, ch, node)
  return actions, rewards, n_actions


SHAPES = [('lunar', 8, 4, 30, False), ('pong_ram', 128, 6, 50, False), ('a18', 128, 18, 30, False), ('tictactoe', 9, 9, 30, True)]


@pytest.mark.parametrize('name,O,A,sims,two', SHAPES, ids=[s[0] for s in SHAPES])
def test_walk_vs_numpy(name, O, A, sims, two):
  from model_based_rl_amd.engine import Engine
  rng = np.random.RandomState(A * 1000 + sims)
  eng = Engine(B, O, A, sims, two_players=two, known_bounds=(-1.0, 1.0) if two else (None, None), seed=11)
  eng.set_weights(_weights(O, A, seed=A))
  obs = rng.standard_normal((B, O)).astype(np.float32)
  legal, to_play, noise = _roots(rng, B, A, two)
  # (1) the stepwise loop: select's depth of every simulation (len(search_path) - 1)
  eng.initial_inference(obs)
  eng.root_prepare(to_play, legal, noise)
  depth = np.zeros((B, sims), np.int32)
  for s in range(sims):
    _, _, act, d = eng.select()
    depth[:, s] = d.cpu().numpy()
    ho, r, v, lg = eng.recurrent_inference(eng.gather_hidden(), act)
    eng.expand_backup(v, r, lg, ho)
  ex = eng.export_tree()
  for T in (0.0, 0.25, 1.0):
    for M in (1, 3, sims + 1):
      U = rng.uniform(size=(B, M))
      out = {k: v.cpu().numpy() for k, v in eng.eval_walk(M, T, U, move=7).items()}
      a_ref, r_ref, n_ref = np_walk(ex, A, M, T, U)
      assert np.array_equal(out['n_actions'], n_ref), (T, M)
      assert np.array_equal(out['actions'], a_ref), (T, M)
      assert np.array_equal(out['pred_rewards'].view(np.uint32), r_ref.view(np.uint32)), (T, M)
      assert np.array_equal(out['path_lengths'], depth + 1), (T, M)
      if M == sims + 1 and T == 0.0:
        assert out['n_actions'].max() >= 3          # (deep enough trees for the walk to mean something)
  # (2) after the fused search kernel (mz_search): the walk reads the pool it leaves; device uniforms are reproducible
  eng.initial_inference(obs)
  eng.root_prepare(to_play, legal, noise)
  eng.search()
  ex = eng.export_tree()
  U = rng.uniform(size=(B, 3))
  out = {k: v.cpu().numpy() for k, v in eng.eval_walk(3, 0.0, U).items()}
  a_ref, r_ref, n_ref = np_walk(ex, A, 3, 0.0, U)
  assert np.array_equal(out['actions'], a_ref) and np.array_equal(out['n_actions'], n_ref)
  assert np.array_equal(out['pred_rewards'].view(np.uint32), r_ref.view(np.uint32))
  pl = out['path_lengths']
  # every simulation adds one visit to each node of its path but the root: the visits below the root sum to sum(len - 1)
  assert pl.min() >= 2 and np.array_equal((ex['N'] * ex['EX'])[:, 1:].sum(1), pl.sum(1) - sims)
  dev1 = {k: v.cpu().numpy() for k, v in eng.eval_walk(sims + 1, 1.0, None, move=3).items()}
  dev2 = {k: v.cpu().numpy() for k, v in eng.eval_walk(sims + 1, 1.0, None, move=3).items()}
  dev3 = {k: v.cpu().numpy() for k, v in eng.eval_walk(sims + 1, 1.0, None, move=4).items()}
  assert all(np.array_equal(dev1[k], dev2[k]) for k in dev1)
  assert not np.array_equal(dev1['actions'], dev3['actions'])
  eng.close()


@pytest.mark.parametrize('nb', [4096, 4093])
@pytest.mark.parametrize('A', [4, 6, 9, 18])
@pytest.mark.parametrize('two', [False, True], ids=['one_player', 'two_players'])
@pytest.mark.parametrize('no_support', [False, True], ids=['support', 'no_support'])
def test_lookahead_vs_rows(nb, A, two, no_support):
  from model_based_rl_amd.engine import Engine
  O, discount = 16, 0.997
  rng = np.random.RandomState(nb + A + 2 * two + 4 * no_support)
  eng = Engine(nb, O, A, 5, two_players=two, no_support=no_support, discount=discount)
  eng.set_weights(_weights(O, A, seed=A + 1, no_support=no_support))
  obs = rng.standard_normal((nb, O)).astype(np.float32)
  legal, to_play, noise = _roots(rng, nb, A, two)
  eng.initial_inference(obs)
  eng.root_prepare(to_play, legal, noise)
  hidden = eng.root_outputs()[2]
  _, r, v, _ = eng.recurrent_inference(hidden.repeat_interleave(A, 0), np.tile(np.arange(A, dtype=np.int32), nb))
  r, v = r.cpu().numpy().reshape(nb, A), v.cpu().numpy().reshape(nb, A)
  lg = legal.astype(bool)
  # --only_value (evaluate.py:286-303)
  out = {k: x.cpu().numpy() for k, x in eng.eval_lookahead('only_value', rows=True).items()}
  assert np.array_equal(out['row_reward'].view(np.uint32), r.view(np.uint32))
  assert np.array_equal(out['row_value'].view(np.uint32), v.view(np.uint32))
  dv = np.float32(discount) * v
  q = r - dv if two else r + dv
  want = np.full(nb, -1)
  for i in range(nb):
    best = -np.inf
    for a in np.flatnonzero(lg[i]):
      if q[i, a] > best:
        best, want[i] = q[i, a], a
  assert np.array_equal(out['action'], want)
  assert np.array_equal(out['pred_reward'].view(np.uint32), r[np.arange(nb), want].view(np.uint32))
  assert np.array_equal(out['child_visits'], np.where(lg, 1.0 / lg.sum(1, keepdims=True), 0.0))
  # --only_prior (evaluate.py:278-284): the tree's float64 priors (noise mixed in), ties to the largest action
  P = eng.export_tree()['P'][:, 1:1 + A]
  want = np.array([max((P[i, a], a) for a in np.flatnonzero(lg[i]))[1] for i in range(nb)])
  out = {k: x.cpu().numpy() for k, x in eng.eval_lookahead('only_prior', rows=True).items()}
  assert np.array_equal(out['action'], want)
  assert np.array_equal(out['pred_reward'].view(np.uint32), r[np.arange(nb), want].view(np.uint32))
  assert np.array_equal(out['row_reward'], out['pred_reward'])
  assert np.array_equal(out['row_value'].view(np.uint32), v[np.arange(nb), want].view(np.uint32))
  assert np.array_equal(out['child_visits'], np.eye(A)[want])
  eng.close()


def _ttt_state(tmp=None, step=0, **over):
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--discount', '1', '--known_bounds', '-1', '1',
                     '--num_simulations', '30'])
  torch.manual_seed(3)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': step}
  for k, v in dict(temperature=0.5, only_prior=0, only_value=0, use_exploration_noise=1, apply_mcts_actions=1, render=False,
                   save_mcts=False, save_gif_as='', random_opp=-1, human_opp=None, label='t', verbose=False).items():
    setattr(cfg, k, v)
  for k, v in over.items():
    setattr(cfg, k, v)
  return state


def _record(g):
  h = g.history
  return (g.step, list(h.actions), list(h.rewards), [list(c) for c in h.child_visits], list(h.root_values), list(g.pred_values),
          list(g.pred_rewards), [list(d) for d in g.search_depths])


def test_batch_invariance():
  from model_based_rl_amd.envs import TicTacToe
  from model_based_rl_amd.evaluate import Evaluator
  seed = 100
  recs = {}
  for batch in (64, 16):
    state = _ttt_state()
    state['config'].batch = batch
    ev = Evaluator(state)
    ev.load_network()
    recs[batch] = [_record(g) for g in ev.play_games(64, list(range(seed, seed + 64)))]
  ev = Evaluator(_ttt_state())
  ev.load_network()
  alone = _record(ev.play_game(TicTacToe(), seed=seed + 5))
  assert recs[64] == recs[16]
  assert alone == recs[64][5]
  assert len(set(str(r[1]) for r in recs[64])) > 32          # (different seeds, different games)


def test_cli_on_a_checkpoint(tmp_path):
  import torch
  from model_based_rl_amd import evaluate
  state = _ttt_state(step=42)
  saves = tmp_path / 'runs' / 'TicTacToe' / 'g' / 'r' / 'saves'
  saves.mkdir(parents=True)
  torch.save({'dirs': {}, 'config': state['config'], 'weights': state['weights'], 'optimizer': {}, 'training_step': 42},
             str(saves / '42'))
  out = tmp_path / 'summary.json'
  res = evaluate.main(['--saves_dir', str(saves) + os.sep, '--nets', '42', '--num_games', '512', '--random_opp', '-1',
                       '--seed', '0', '--num_simulations', '10', '--only_value', '0', '1', '--detailed_label', '--out', str(out)])
  js = json.load(open(str(out)))
  assert len(js['configurations']) == 2 == len(res)
  assert sorted(c['label'] for c in js['configurations']) == ['net:42, path:0, only value', 'net:42, path:0, sims:10']
  for c in js['configurations']:
    assert c['num_games'] == 512 and c['wins'] + c['draws'] + c['losses'] == 512
    assert c['games_per_s'] > 0 and 0 < c['host_share'] < 1
    assert set(('length', 'return', 'pred_return', 'pred_value', 'mcts_value', 'search_depth')) <= set(c)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
G7 = sorted(f for f in os.listdir(GOLDEN) if f.startswith('g7_eval_'))
# one step of the float32 inverse-transform staircase the network scalars may differ by (README "Parity"), and the
# decision margin inside which such a difference may flip a choice (a score gap is a difference of such values)
STEP = lambda x: 1e-5 + 1.5e-4 * (1 + abs(x))
ALLOW = 3e-4


@pytest.mark.parametrize('name', G7, ids=[f[len('g7_eval_'):-4] for f in G7])
def test_reference_games(name):
  """the reference's own Evaluator.play_game (scripts/make_eval_goldens.py), replayed with its recorded draws: every move's
  child visits, search depths, applied actions, rewards and game ends exact; predicted values / rewards and root values
  within one staircase step.  A divergence is accepted only at a move whose recorded decision margin lies inside ALLOW --
  then the rest of that game is not compared, and the test says so."""
  import warnings
  import torch
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.envs import TicTacToe
  from model_based_rl_amd.evaluate import Evaluator
  g = np.load(os.path.join(GOLDEN, name))
  w = np.load(os.path.join(GOLDEN, str(g['weights_file'])))
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--known_bounds', '-1', '1', '--discount', '1',
                     '--num_simulations', str(int(g['num_simulations']))])
  ro = int(g['random_opp'])
  for k, v in dict(temperature=float(g['temperature']), only_prior=int(g['only_prior']), only_value=int(g['only_value']),
                   use_exploration_noise=int(g['use_exploration_noise']), apply_mcts_actions=int(g['apply_mcts_actions']),
                   random_opp=ro if ro else None, human_opp=None, render=False, save_mcts=False, save_gif_as='', label=name,
                   verbose=False).items():
    setattr(cfg, k, v)
  weights = {k[2:]: torch.from_numpy(w[k].copy()) for k in w.files if k.startswith('w.')}
  ev = Evaluator({'config': cfg, 'weights': weights, 'training_step': 0})
  ev.load_network()
  one_action = int(g['apply_mcts_actions']) == 1
  notes, compared, total = [], 0, 0
  for gi, seed in enumerate(g['seeds']):
    mv = np.flatnonzero(g['move_game'] == gi)
    av = np.flatnonzero(g['act_game'] == gi)
    total += len(mv)
    pad = 12           # (draws past the recorded game: only read after a divergence)
    draws = dict(walk=[g['walk_u'][m, :g['walk_n'][m]] for m in mv] + [np.full(g['walk_u'].shape[1], 0.5)] * pad,
                 noise=[g['noise'][m] for m in mv] + [np.full(9, 1 / 9.)] * pad,
                 opp=[int(x) for m in mv for x in g['opp'][m, :g['opp_n'][m]]] + [0] * 4 * pad)
    game = ev.play_game(TicTacToe(), seed=int(seed), draws=draws)
    h = game.history
    bad = None
    for j, m in enumerate(mv):
      same = (j < len(h.child_visits) and np.array_equal(np.asarray(h.child_visits[j]), g['child_visits'][m])
              and list(game.search_depths[j]) == list(g['search_depths'][m, :g['search_depths_n'][m]]))
      if same and one_action:
        same = j < len(h.actions) and h.actions[j] == g['action'][av[j]] and h.rewards[j] == g['reward'][av[j]]
      if not same:
        bad = j
        break
      assert abs(game.pred_values[j] - g['pred_value'][m]) <= STEP(g['pred_value'][m]), (name, gi, j)
      assert abs(h.root_values[j] - g['root_value'][m]) <= STEP(g['root_value'][m]), (name, gi, j)
      compared += 1
    if bad is None:
      assert list(h.actions) == list(g['action'][av]) and list(h.rewards) == list(g['reward'][av]), (name, gi)
      assert list(h.dones) == [bool(x) for x in g['done'][av]] and game.step == g['game_step'][gi], (name, gi)
      assert sum(h.rewards) == g['game_return'][gi]
      for a, b in zip(game.pred_rewards, g['pred_reward'][av]):
        assert abs(a - b) <= STEP(b), (name, gi, a, b)
    else:
      margin = g['margin'][mv[bad]]
      assert margin <= ALLOW, ('%s game %d diverges at move %d with decision margin %.3g > %.1g: a real difference'
                               % (name, gi, bad, margin, ALLOW))
      notes.append('game %d: move %d decided within the float32 allowance (margin %.2g), not compared further' % (gi, bad, margin))
  if notes:
    warnings.warn('%s: %s' % (name, '; '.join(notes)))
    print('%s: %d of %d moves compared; %s' % (name, compared, total, '; '.join(notes)))
  assert compared >= total // 2, (name, compared, total, notes)
