"""The Gumbel search without a GPU (DESIGN s7h):
  seq        the sequence of considered visits against two hand-listed ones and its invariants
  twin       mz_gz_search_host -- sequential C++ through the per-node body the kernels run -- equals the Python restatement
             of tests/gumbel_py.py: every integer field, W and R bit for bit (both use glibc on the same float32 network
             outputs), P, pi' and v_mix to 1e-12
             -- on the first three sets (A = 9, 7, 4; 16 simulations) and on those added to reach the lane groups G = 4 with
             idle lanes and G = 32, m < legal actions, 8 .. 50 simulations, other c_visit / c_scale, discount 1 and 70 trees
             (gp.SETS), each of which is asserted to reach what it is there for
  by hand    one root with three legal actions and four simulations, from the formulas; the guarded branches of mz_gz_node on
             roots built for them (gp.HAND): sum N > 0 with sp == 0, and exact ties across every child of every node
  margin     min_gap >= 1e-9 on every committed test set: a device / host difference of about 1e-13 (8 ulp of exp on values
             <= 1, a few roundings on scores below 2^7) cannot flip a decision the host takes with that margin, so the GPU
             tests demand equality with no allowance.  Exact ties have gap 0 and are allowed (they break to the largest action).
             Every set keeps (c_visit + simulations) * c_scale <= 100, so sigma <= 100 and g + logit + sigma < 2^7; on the
             underflow root the scores reach 100 + 74 and -800, where a rounding is 1.2e-13 at the most: the same argument
  seeds      a set's fake-network seed is the first of gp.SEED_CANDIDATES that holds the margin and reaches the set's cases
  refusals   one test per sentence of evaluate.refuse_gumbel, the flags, label and --out key on a stub engine"""
import json
import math
import types

import numpy as np
import pytest

from tests import gumbel_py as gp

SIMS = gp.SIMS


def _cfg(c):
  from model_based_rl_amd.engine import mz_config
  return mz_config(c['trees'], 4, c['A'], c['sims'], two_players=c['two'], known_bounds=c['bounds'], discount=c['discount'])


def host_search(c, scale, **kw):
  """the host twin on case c (a set of gp.SETS or a hand-built root): simulations, trees and parameters are the case's"""
  from model_based_rl_amd.engine import gz_search_host
  return gz_search_host(_cfg(c), c['root_value'], c['root_logits'], gp.net(c), to_play=c['to_play'],
                        legal=c['legal'], gumbel=c['G'] if scale else None, gumbel_scale=scale, **dict(c['kw'], **kw))


class _Searched(dict):
  """per (set or hand-built root, gumbel_scale): (the host twin's trees, the restatement's), searched when first asked for"""

  def __missing__(self, key):
    c = gp.case(key[0])
    self[key] = (host_search(c, key[1]), gp.search_batch(c, key[1]))
    return self[key]


@pytest.fixture(scope='module')
def searched():
  return _Searched()


def test_seq_against_the_hand_listed_sequences():
  from model_based_rl_amd.engine import gz_seq
  a = [0, 0, 0, 0, 1, 1, 2, 2]
  b = [0] * 7 + [1, 1, 1, 2, 2, 2, 3, 3, 3] + [4, 4, 5, 5, 6, 6, 7, 7, 8, 8] + [9, 9, 10, 10]
  assert gz_seq(4, 8).tolist() == a and gp.seq(4, 8) == a
  assert gz_seq(7, 30).tolist() == b and gp.seq(7, 30) == b


def test_seq_invariants():
  from model_based_rl_amd.engine import gz_seq
  for m in range(1, 33):      # every row of the device's table [A + 1][sims], A <= 32
    for n in range(1, 65):
      s = gz_seq(m, n).tolist()
      assert s == gp.seq(m, n), (m, n)
      assert len(s) == n
      assert s[:min(m, n)] == [0] * min(m, n)
      # replayed on m candidates: an entry c goes to a candidate that has c visits, so every candidate's counts never decrease
      visits = [0] * max(m, 1)
      for c in s:
        assert c in visits, (m, n, s)
        visits[visits.index(c)] += 1


@pytest.mark.parametrize('name', list(gp.SETS))
@pytest.mark.parametrize('scale', [1.0, 0.0], ids=['given_G', 'no_noise'])
def test_host_twin_equals_the_restatement(searched, name, scale):
  _twin_equals_the_restatement(searched[name, scale], gp.case(name))


def _twin_equals_the_restatement(pair, c):
  host, want = pair
  ex = want['EX'] == 1
  for key in ('N', 'E', 'TP', 'W', 'R'):
    diff = np.argwhere((host[key] != want[key]) & ex)
    assert len(diff) == 0, (key, diff[:5].tolist())
  assert np.abs(host['P'] - want['P'])[ex].max() <= 1e-12
  for key in ('legal', 'minmax', 'vhat', 'sel_slot', 'sel_action', 'paths', 'plens', 'action', 'pred_reward'):
    assert np.array_equal(host[key], np.asarray(want[key]).astype(host[key].dtype)), key
  assert np.abs(host['pi'] - want['pi']).max() <= 1e-12 and np.abs(host['v_mix'] - want['v_mix']).max() <= 1e-12
  assert np.all(host['pi'][c['legal'] == 0] == 0) and np.allclose(host['pi'].sum(1), 1, atol=1e-12)
  assert (host['N'][:, 0] == c['sims']).all()


@pytest.mark.parametrize('name', list(gp.SETS))
@pytest.mark.parametrize('scale', [1.0, 0.0], ids=['given_G', 'no_noise'])
def test_host_twin_reproduces_the_pinned_outputs(searched, name, scale):
  """Every output array of mz_gz_search_host on the committed sets, bit for bit, as the twin gave it before its tree code
  moved into csrc/mz_tree_host.h -- vhat, paths, plens and min_gap included.  The digests and the snippet that writes them:
  tests/golden/search_twins_sha256.json, test_truemodel_cpu.test_host_twin_reproduces_the_pinned_outputs."""
  import os
  from tests.test_truemodel_cpu import array_digests
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'search_twins_sha256.json')) as f:
    want = json.load(f)['gz/%s/%g' % (name, scale)]
  got = array_digests(searched[name, scale][0])
  assert sorted(got) == sorted(want)
  assert [k for k in sorted(got) if got[k] != want[k]] == []


@pytest.mark.parametrize('name', list(gp.SETS))
def test_the_sets_reach_the_cases_that_can_go_wrong(searched, name):
  c = gp.case(name)
  host, _ = searched[name, 1.0]
  plain, _ = searched[name, 0.0]
  assert _unreached(name, c, host, plain) == []


def _unreached(name, c, host, plain):
  """what set `name` (roots c, the twin's searches at gumbel_scale 1 and 0) does not reach of what it is there for"""
  A, no = c['A'], []
  nl = c['legal'].sum(1)
  if sorted(nl.tolist())[:3] != [min(k, A) for k in (1, 2, 3)] or nl[0] != 1:
    no.append('no roots with one, two and three legal actions')
  if host['plens'].max() < 4:
    no.append('no descent goes two levels below the root')
  if not ((plain['action'] != host['action']).any() or (plain['sel_action'] != host['sel_action']).any()):
    no.append('G changes nothing')
  binds = int((gp.considered(c) < nl).sum())      # roots where sequential halving starts from fewer than the legal actions
  if 'max_considered' in c['kw'] and binds < 4:
    no.append('max_considered binds on %d roots, fewer than 4' % binds)
  if name == 'a18_s30' and binds < 1:
    no.append('no root with more than 16 legal actions')
  if name == 'a2_s8' and sorted(set(gp.considered(c).tolist())) != [1, 2]:
    no.append('m = 1 and m = 2 do not both occur')
  if A == 32 and not (nl == 32).any():
    no.append('no root with 32 legal actions')
  if gp.group_width(A) == 32:
    for d in (host, plain):      # a descent or a pick in the upper half of the lane group, and of its last action
      taken = np.concatenate([d['sel_action'].ravel(), d['action'].ravel()])
      if not (taken >= 16).any():
        no.append('no descent or pick of an action >= 16')
      if not (taken == A - 1).any():
        no.append('no descent or pick of action A - 1')
  return no


def test_the_seeds_are_the_first_that_hold():
  """the seed rule of the sets added after the first three (gp.SETS): a set's seed is the first of gp.SEED_CANDIDATES with
  which the twin's min_gap is >= 1e-9 at both scales and the set reaches its cases.  That the committed seed holds both is
  what test_the_margin_condition and test_the_sets_reach_the_cases_that_can_go_wrong assert; here: no earlier one does"""
  for name in gp.NEW_SETS:
    for seed in gp.SEED_CANDIDATES[:gp.SEED_CANDIDATES.index(gp.SETS[name][4])]:
      c = gp.case(name, seed=seed)
      host, plain = host_search(c, 1.0), host_search(c, 0.0)
      assert min(host['min_gap'], plain['min_gap']) < 1e-9 or _unreached(name, c, host, plain), (name, hex(seed))


@pytest.mark.parametrize('name', list(gp.SETS))
@pytest.mark.parametrize('scale', [1.0, 0.0], ids=['given_G', 'no_noise'])
def test_the_margin_condition(searched, name, scale):
  host, _ = searched[name, scale]
  assert host['min_gap'] >= 1e-9, host['min_gap']


def test_one_root_by_hand():
  """three legal actions (0, 2, 3 of A = 4), four simulations, two players, bounds -1 .. 1, scale 1.  seq(3, 4) = 0 0 0 1."""
  from model_based_rl_amd.engine import gz_search_host, mz_config
  A, d = 4, 0.997
  logit = {0: 0.5, 2: -0.25, 3: 0.125}
  G = {0: -0.5, 2: 1.0, 3: 0.25}
  v_root = 0.25
  leaf_v = {0: 0.5, 2: -0.25, 3: 0.125}      # value of the child reached by action a, in ITS mover's view
  leaf_r = {0: 0.0, 2: 0.25, 3: -0.125}
  deep_v, deep_r = 0.0625, 0.0
  uniform = np.zeros(A, np.float32)          # logits of every expanded node: uniform priors below the root

  def ev(sim, slot, act):
    a = int(act[0])
    if int(slot[0]) == 0:
      return [leaf_v[a]], [leaf_r[a]], [uniform]
    return [deep_v], [deep_r], [uniform]
  cfg = mz_config(1, 4, A, 4, two_players=True, known_bounds=(-1.0, 1.0), discount=d)
  lg = np.array([[logit.get(a, 9.0) for a in range(A)]], np.float32)      # (the illegal action's logit must not matter)
  gm = np.array([[G.get(a, 9.0) for a in range(A)]])
  host = gz_search_host(cfg, [v_root], lg, ev, to_play=[1], legal=[[1, 0, 1, 1]], gumbel=gm, gumbel_scale=1.0)
  # simulations 0 - 2: every child is unvisited when it is chosen among the unvisited, sigma is the same for all of those,
  # so they go in descending order of g + logit: action 2 (0.75), 3 (0.375), 0 (0.0)
  assert host['sel_action'][0, :3].tolist() == [2, 3, 0] and host['sel_slot'][0, :3].tolist() == [0, 0, 0]
  z = sum(math.exp(x) for x in logit.values())
  P = {a: math.exp(logit[a]) / z for a in logit}
  norm = lambda x: (x + 1.0) / 2.0           # MinMaxStats with the known bounds; no q leaves them here
  q = {a: leaf_r[a] + d * -leaf_v[a] for a in logit}
  # simulation 3: all three have one visit = seq[3]; sigma = (50 + 1) * normalize(q)
  score = {a: G[a] + logit[a] + 51.0 * norm(q[a]) for a in logit}
  a3 = max((s, a) for a, s in score.items())[1]
  assert a3 == 2
  # below it every child is unvisited: pi' = the uniform prior, no visits -> the largest action, 3
  assert host['sel_action'][0, 3] == 3 and host['sel_slot'][0, 3] == 1 and host['plens'][0, 3] == 3
  # after the backup child 2 has two visits.  The deeper leaf's mover is the child's opponent: what it passes up,
  # -deep_r + d * deep_v in its own view, reaches the child negated
  W2 = leaf_v[2] - (-deep_r + d * deep_v)
  q[2] = leaf_r[2] + d * -(W2 / 2)
  assert host['N'][0, 1:5].tolist() == [1, 0, 2, 1] and host['W'][0, 3] == pytest.approx(W2, abs=1e-15)
  sum_n, max_n = 4, 2
  v_mix = (v_root + sum_n * sum(P[a] * q[a] for a in logit) / sum(P.values())) / (1 + sum_n)
  sigma = {a: (50.0 + max_n) * norm(q[a]) for a in logit}
  w = {a: P[a] * math.exp(sigma[a] - max(sigma.values())) for a in logit}
  pi = [w.get(a, 0.0) / sum(w.values()) for a in range(A)]
  assert host['action'][0] == 2 and host['pred_reward'][0] == np.float32(leaf_r[2])      # the only action with two visits
  assert np.abs(host['pi'][0] - np.array(pi)).max() <= 1e-12 and host['pi'][0, 1] == 0
  assert abs(host['v_mix'][0] - v_mix) <= 1e-12


@pytest.mark.parametrize('name,scale', gp.HAND_RUNS)
def test_hand_built_roots_twin_equals_the_restatement(searched, name, scale):
  """the guarded branches of mz_gz_node (gp.underflow, gp._ties), with the bars of test_host_twin_equals_the_restatement; the
  margin holds on them as on the sets, so the GPU test demands equality on them too"""
  _twin_equals_the_restatement(searched[name, scale], gp.case(name))
  assert searched[name, scale][0]['min_gap'] >= 1e-9


def check_underflow_is_reached(first, whole, c):
  """first: the search after ONE simulation, whole: after all of them (the twin's, the restatement's or the device's arrays).
  The first simulation visits the action G lifts, whose prior is 0: sum N > 0 and sp == 0 at the root, so v_mix is v^ to
  the bit and pi' is the prior -- 1 on the logit-0 action, 0 on every P == 0 child"""
  A = c['A']
  for b, (one, up) in enumerate(gp.UNDERFLOW):
    kids = np.asarray(first['N'])[b, 1:1 + A]
    assert kids[up] == 1 and kids.sum() == 1 and np.asarray(first['P'])[b, 1 + up] == 0
    assert first['v_mix'][b] == np.float64(c['root_value'][b]), 'v_mix is not v^'
    zero = (np.asarray(whole['P'])[b, 1:1 + A] == 0) & (c['legal'][b] == 1)
    assert zero.sum() == c['legal'][b].sum() - 1 and not zero[one]
    assert first['pi'][b, one] == 1 and not np.asarray(first['pi'])[b, np.arange(A) != one].any()
    assert (np.asarray(whole['pi'])[b, zero] == 0).all() and whole['pi'][b, one] == 1
    assert (np.asarray(whole['N'])[b, 1:1 + A][zero] > 0).any()      # (visited children among them)


def test_prior_underflow_by_hand(searched):
  c = gp.case('underflow')
  host, want = searched['underflow', 1.0]
  first = host_search(c, 1.0, num_simulations=1)
  check_underflow_is_reached(first, host, c)
  check_underflow_is_reached(gp.search_batch(c, 1.0, num_simulations=1), want, c)
  assert np.array_equal(first['v_mix'], gp.search_batch(c, 1.0, num_simulations=1)['v_mix'])


def check_ties_break_to_the_largest_action(d, c):
  """d: a search of a gp._ties root.  The first m simulations stay at the root and take its legal actions in descending
  order.  The next m (seq asks for one visit) go through the same actions in the same order -- the largest of those visited
  once -- and on below the root, where no child is visited yet, to action A - 1.  The move is the largest legal action"""
  A = c['A']
  for b in range(c['trees']):
    legal = [a for a in range(A) if c['legal'][b, a]]
    m = min(16, len(legal))
    top = sorted(legal, reverse=True)[:m]
    assert d['sel_action'][b, :m].tolist() == top and not d['sel_slot'][b, :m].any(), b
    assert d['plens'][b, :m].tolist() == [2] * m
    again = np.arange(m, min(2 * m, c['sims']))
    assert len(again) >= 3 and (d['sel_action'][b, again] == A - 1).all() and (d['plens'][b, again] == 3).all(), b
    assert [(int(k) - 1) % A for k in d['paths'][b, again, 1]] == top[:len(again)], b      # (the path's first step: the root's choice)
    assert d['sel_slot'][b, again].tolist() == list(range(1, 1 + len(again))), b           # (its slot: first taken, first revisited)
    assert d['action'][b] == top[0] and d['sel_action'][b].max() < A


@pytest.mark.parametrize('name', ['ties18', 'ties32'])
def test_all_ties_by_hand(searched, name):
  c = gp.case(name)
  for scale in (1.0, 0.0):
    host, want = searched[name, scale]
    check_ties_break_to_the_largest_action(host, c)
    check_ties_break_to_the_largest_action(want, c)
    assert np.array_equal(host['sel_action'], want['sel_action'])


def test_host_twin_refusals():
  c = gp.case('single_player')
  with pytest.raises(RuntimeError, match='simulations exceed'):
    host_search(c, 0.0, num_simulations=SIMS + 1)
  with pytest.raises(RuntimeError, match='max_considered >= 2'):
    host_search(c, 0.0, max_considered=1)
  with pytest.raises(RuntimeError, match='needs the draws'):
    from model_based_rl_amd.engine import gz_search_host
    gz_search_host(_cfg(c), c['root_value'], c['root_logits'], gp.fake_eval(c['seed'], c['A']), gumbel_scale=1.0)


def test_a_partial_search_is_a_prefix():
  c = gp.case('connect_four')
  part, want = host_search(c, 1.0, num_simulations=5), gp.search_batch(c, 1.0, num_simulations=5)
  ex = want['EX'] == 1
  for key in ('N', 'E', 'W', 'R'):
    assert np.array_equal(part[key][ex], want[key][ex]), key
  assert np.array_equal(part['sel_action'][:, :5], want['sel_action'][:, :5]) and np.array_equal(part['action'], want['action'])


# ---- the command line
def _args(**kv):
  base = dict(gumbel=1, device_env=True, environment='TicTacToe', apply_mcts_actions=1, only_prior=0, only_value=0,
              use_exploration_noise=0, temperatures=[0.0], true_model=0, architecture='FCNetwork', gumbel_considered=16,
              gumbel_c_visit=50.0, gumbel_c_scale=1.0, gumbel_scale=0.0)
  base.update(kv)
  return types.SimpleNamespace(**base)


def _refused(pattern, match=False, **kv):
  from model_based_rl_amd.evaluate import refuse_gumbel
  with pytest.raises(NotImplementedError, match=pattern):
    refuse_gumbel(_args(**kv), match=match)


def test_cli_refuses_the_host_path():
  from model_based_rl_amd.evaluate import refuse_gumbel
  _refused(r'^--gumbel: .*needs --device_env \(or --match\)\.$', device_env=False)
  refuse_gumbel(_args(device_env=False), match=True)


@pytest.mark.parametrize('m', [2, 0, [1, 3]])
def test_cli_refuses_more_than_one_applied_action(m):
  _refused(r'^--gumbel: .*--apply_mcts_actions 1 only\.$', apply_mcts_actions=m)


def test_cli_refuses_exploration_noise():
  _refused(r'^--gumbel: the Gumbel draw replaces the exploration noise', use_exploration_noise=1)
  _refused(r'^--gumbel: the Gumbel draw replaces the exploration noise', match=True, gumbel=[0, 1], use_exploration_noise=[0, 1])


def test_cli_refuses_a_temperature_on_that_side():
  from model_based_rl_amd.evaluate import refuse_gumbel
  _refused(r'^--gumbel: the move is chosen by the rule of the search, not sampled', temperatures=[0.5])
  _refused(r'^--gumbel: the move is chosen by the rule of the search, not sampled', match=True, gumbel=[0, 1], temperatures=[0.0, 1.0])
  refuse_gumbel(_args(gumbel=[0, 1], temperatures=[1.0, 0.0]), match=True)      # the other side's temperature is its own business
  refuse_gumbel(_args(temperature=0.0, temperatures=None))                      # (a Config carries one temperature)
  _refused(r'^--gumbel: the move is chosen by the rule', temperature=0.25, temperatures=None)


def test_cli_refuses_a_lookahead_on_the_same_side():
  from model_based_rl_amd.evaluate import refuse_gumbel
  for kv in (dict(only_prior=1), dict(only_value=1), dict(only_prior=[0, 1], gumbel=[1])):
    _refused(r'^--gumbel: --only_prior / --only_value run no search', **kv)
  _refused(r'^--gumbel: --only_prior / --only_value run no search', match=True, gumbel=[0, 1], only_value=[0, 1])
  refuse_gumbel(_args(gumbel=[0, 1], only_value=[1, 0]), match=True)


def test_cli_refuses_the_true_rules_on_the_same_side():
  from model_based_rl_amd.evaluate import refuse_gumbel
  _refused(r'^--gumbel: an engine searches the true rules or with the Gumbel search', true_model=1)
  _refused(r'^--gumbel: an engine searches the true rules or with the Gumbel search', match=True, gumbel=[0, 1], true_model=[0, 1])
  refuse_gumbel(_args(gumbel=[0, 1], true_model=[1, 0]), match=True)


def test_cli_refuses_another_architecture():
  _refused(r'^--gumbel: the architecture MuZeroNetwork has no engine path', architecture='MuZeroNetwork')


def test_cli_refuses_parameters_out_of_range():
  _refused(r'^--gumbel: --gumbel_considered must be at least 2, got 1\.$', gumbel_considered=1)
  _refused(r'^--gumbel: --gumbel_c_visit must not be negative', gumbel_c_visit=-1.0)
  _refused(r'^--gumbel: --gumbel_c_scale must be positive', gumbel_c_scale=0.0)
  _refused(r'^--gumbel: --gumbel_scale must not be negative', gumbel_scale=-0.5)
  _refused(r'^--gumbel: the values are 0 .* and 1', gumbel=3)


def test_cli_parses_the_flags_and_the_default_refuses_nothing():
  from model_based_rl_amd.config import get_evaluation_args
  from model_based_rl_amd.evaluate import refuse_gumbel
  a = get_evaluation_args([])
  assert a.gumbel == [0] and (a.gumbel_considered, a.gumbel_c_visit, a.gumbel_c_scale, a.gumbel_scale) == (16, 50.0, 1.0, 0.0)
  assert get_evaluation_args(['--match', '--gumbel', '0', '1']).gumbel == [0, 1]
  refuse_gumbel(a)
  refuse_gumbel(_args(gumbel=0, device_env=False, apply_mcts_actions=5, use_exploration_noise=1, gumbel_considered=0))
  refuse_gumbel(_args(environment='CartPole-v1'))      # nothing here depends on the game


def test_main_refuses_before_loading_anything():
  from model_based_rl_amd import evaluate
  with pytest.raises(NotImplementedError, match=r'^--gumbel: '):
    evaluate.main(['--gumbel', '1', '--nets', 'missing'])
  with pytest.raises(NotImplementedError, match=r'^--gumbel: '):
    evaluate.main(['--match', '--gumbel', '1', '--only_prior', '1', '--nets', 'missing', 'missing'])


class StubEngine(object):
  """what Evaluator._play_batch_device calls, recording the calls; every game is over after the first chunk"""
  made = []

  def __init__(self, B, A, sims):
    self.B, self.A, self.sims, self.calls = B, A, sims, []
    StubEngine.made.append(self)

  @classmethod
  def from_config(cls, config, num_envs, device=None, seed=None, env_id_offset=0):
    return cls(num_envs, config.action_space, config.num_simulations)

  def set_weights(self, w):
    self.calls.append('set_weights')

  def set_gumbel(self, on=True, max_considered=16, c_visit=50.0, c_scale=1.0, gumbel_scale=0.0):
    self.calls.append(('set_gumbel', on, max_considered, c_visit, c_scale, gumbel_scale))

  def eval_env_reset(self, kind, max_steps, time_limit, random_opp, keep_history):
    self.calls.append('eval_env_reset')
    self.eval_log_cap = 9

  def eval_env_moves(self, n, mode, M, T, noise_on):
    self.calls.append('eval_env_moves')
    return 0

  def eval_env_results(self):
    z = lambda *s: np.zeros(s)
    return dict(step=np.full(self.B, 5, np.int32), n_moves=np.full(self.B, 5, np.int32), sum_reward=z(self.B), sum_pred_reward=z(self.B),
                sum_pred_value=z(self.B), sum_root_value=z(self.B), depth_mean=z(self.B), depth_max=z(self.B, self.sims))

  def close(self):
    pass


def test_label_line_and_out_key_on_a_stub_engine(tmp_path, monkeypatch, capsys):
  """evaluate --device_env --gumbel 0 1: two configurations, the second labelled and run with the engine's Gumbel search set,
  with the command line's parameters, before the games start; the printed line and --out carry the choice"""
  import torch
  from model_based_rl_amd import evaluate
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.networks import get_network
  cfg = make_config(['--environment', 'TicTacToe', '--two_players', '--architecture', 'FCNetwork', '--num_simulations', '4'])
  torch.manual_seed(0)
  state = {'config': cfg, 'weights': get_network(cfg, torch.device('cpu')).state_dict(), 'training_step': 7}
  torch.save(state, str(tmp_path / 'net'))
  monkeypatch.setattr(evaluate, 'Engine', StubEngine)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  StubEngine.made = []
  out = tmp_path / 'out.json'
  res = evaluate.main(['--saves_dir', str(tmp_path) + '/', '--nets', 'net', '--num_games', '3', '--seed', '0', '--device_env',
                       '--detailed_label', '--gumbel', '0', '1', '--gumbel_considered', '4', '--gumbel_scale', '1', '--out', str(out)])
  assert [r['gumbel'] for r in res] == [0, 1]
  assert 'gumbel' not in res[0]['label'] and res[1]['label'].endswith('gumbel')
  assert [c['gumbel'] for c in json.load(open(str(out)))['configurations']] == [0, 1]
  printed = capsys.readouterr().out
  assert 'Search: PUCT' in printed and 'Search: Gumbel, m = 4, c_visit = 50, c_scale = 1, gumbel_scale = 1' in printed
  plain, gz = StubEngine.made
  assert not [c for c in plain.calls if c[0] == 'set_gumbel']
  assert gz.calls.index(('set_gumbel', True, 4, 50.0, 1.0, 1.0)) < gz.calls.index('eval_env_reset') < gz.calls.index('eval_env_moves')
  # play_games(gumbel=True) on a config without the flag takes the same path, with the defaults
  ev = evaluate.Evaluator(dict(state, config=evaluate._with(cfg, temperature=0, only_prior=0, only_value=0, use_exploration_noise=0,
                                                            apply_mcts_actions=1, random_opp=None, label='x', batch=4)))
  ev.load_network()
  StubEngine.made = []
  ev.play_games(2, [0, 1], device_env=True, gumbel=True)
  assert ('set_gumbel', True, 16, 50.0, 1.0, 0.0) in StubEngine.made[0].calls
  with pytest.raises(NotImplementedError, match=r'^--gumbel: .*needs --device_env'):
    ev.play_games(2, [0, 1], gumbel=True)


def test_host_twin_under_the_sanitizers(tmp_path):
  """tests/gumbel_host.cpp -- the twin's own file in a stand-alone program -- under AddressSanitizer + UBSan"""
  import os
  import subprocess
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  exe = str(tmp_path / 'gumbel_host')
  cmd = ['hipcc', '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(root, 'include'),
         '-I', os.path.join(root, 'model-based-rl_amd', 'csrc'), os.path.join(root, 'tests', 'gumbel_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.strip().splitlines()[-1] == 'ok 600'
