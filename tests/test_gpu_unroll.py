"""The unroll diagnostic on the device (csrc/mz_unroll.hip.h, DESIGN s7f, "Grading by unroll depth"):
  host      the device's lines equal the host hook mz_unroll_lines_host.  The tolerance is zero: one integer body on both sides
  network   teacher-forced, so no new tolerance: the device's own hidden_u[k - 1] and the action through FC64.recurrent, the
            real observation through FC64.initial; hidden states and logits within the project's 1e-5, values and rewards
            within tests/fc64.scalar_bound; unrolled and fresh outputs at k = 0 equal bit for bit
  batch     a row unrolled alone gives the bits it gave inside the batch
  terms     the device's terms against mz_unroll_terms_host on the device's own raw outputs, at the CPU test's tolerance
  grade     evaluate --grade --grade_unroll through Evaluator.play_games: the unroll report equals the one recomputed from the
            kept histories with the restatement of tests/unroll_util.py; the --grade report is the one of a run without the flag
  state     an engine that unrolled rows plays the evaluation games it played without the call"""
import numpy as np
import pytest

from tests import fc64
from tests import unroll_util as uu
from tests.eval_device_util import eval_state, weights

pytestmark = pytest.mark.gpu

B = 64
N = 2 * B + 3      # two full chunks and a tail
WSEED = 5
SUPPORT = (-15, 15)


@pytest.fixture(scope='module')
def engines():
  from model_based_rl_amd.engine import Engine
  made = {}

  def get(kind, num_envs=B, with_weights=True):
    key = (kind, num_envs, with_weights)
    if key not in made:
      O, A = uu.O_OF[kind], uu.A_OF[kind]
      made[key] = Engine(num_envs, O, A, 4, two_players=True, known_bounds=(-1, 1), discount=1.0, seed=0, device='cuda:0')
      if with_weights:
        made[key].set_weights(weights(O, A, WSEED))
    return made[key]
  yield get
  for e in made.values():
    e.close()


_rows = {}


def rows(kind):
  """N rows with K = 5 actions: prefixes of random games; Connect Four's come from the last plies of long games, so that
  lines end inside K and positions with few empty cells occur.  (boards, turn, step, actions, truth [N, 6, A])"""
  if kind not in _rows:
    games = uu.random_games(kind, 40, 11) if kind == 1 else uu.random_games(3, 12, 11, min_len=36)
    bd, tn, st, ac, where = uu.rows_of(games, kind, 5)
    keep = np.arange(len(bd)) if kind == 1 else np.flatnonzero(st >= 24)
    assert len(keep) >= N
    keep = keep[:N]
    truth = uu.minimax_truth(games, kind, 5, [where[i] for i in keep], None if kind == 1 else 8)
    _rows[kind] = (bd[keep], tn[keep], st[keep], ac[keep], truth)
  return _rows[kind]


_raw = {}


def unrolled(engines, kind):
  """the K = 5 unroll of the N rows with truth and raw outputs, computed once and left unchanged"""
  if kind not in _raw:
    bd, tn, st, ac, truth = rows(kind)
    _raw[kind] = engines(kind).unroll(kind, bd, tn, st, ac, truth=truth, raw=True)
  return _raw[kind]


LINE_KEYS = ('obs', 'legal', 'terminal', 'reward_true', 'depth')
RAW_KEYS = LINE_KEYS + ('hidden_u', 'logits_u', 'logits_f', 'value_u', 'reward_u', 'value_f', 'terms')


@pytest.mark.parametrize('kind', [1, 3])
@pytest.mark.parametrize('K', [0, 1, 5])
def test_lines_equal_the_host_hook(kind, K, engines):
  bd, tn, st, ac, _ = rows(kind)
  want = uu.host_lines(kind, bd, tn, st, ac[:, :K])
  assert want['flags'].max() == 0
  got = unrolled(engines, kind) if K == 5 else engines(kind).unroll(kind, bd, tn, st, ac[:, :K], raw=True)
  for key in LINE_KEYS:
    assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (kind, K, key)
  if K == 5:
    assert want['depth'].min() < K and want['depth'].max() == K and want['terminal'].any()      # lines that end inside K, lines that do not
  one = engines(kind, 1).unroll(kind, bd[7:8], tn[7:8], st[7:8], ac[7:8, :K], raw=True)      # n = 1 on an engine of one row
  for key in LINE_KEYS:
    assert np.array_equal(one[key], want[key][7:8]), (kind, K, key, 'alone')


@pytest.mark.parametrize('kind', [1, 3])
def test_network_teacher_forced(kind, engines):
  bd, tn, st, ac, _ = rows(kind)
  got = unrolled(engines, kind)
  O, A = uu.O_OF[kind], uu.A_OF[kind]
  net = fc64.FC64(weights(O, A, WSEED), O, A)
  close = lambda g, w, what: np.testing.assert_allclose(g, w, rtol=0, atol=1e-5, err_msg=str((kind, what)))

  def scalar(g, w, what):
    err, bound = np.abs(np.asarray(g, np.float64) - w), fc64.scalar_bound(w, SUPPORT, True)
    print(kind, what, 'max error', float(err.max()), 'smallest bound', float(bound.min()))
    assert np.all(err <= bound), (kind, what, float((err - bound).max()))
  # k = 0: one computation, so unrolled and fresh are the same bits
  for u, f in (('value_u', 'value_f'), ('logits_u', 'logits_f')):
    assert np.array_equal(got[u][:, 0].view(np.uint32), got[f][:, 0].view(np.uint32)), (kind, u)
  assert not got['reward_u'][:, 0].any()
  h, v, lg = net.initial(got['obs'][:, 0])
  close(got['hidden_u'][:, 0], h, 'h_0'); close(got['logits_u'][:, 0], lg, 'logits_0'); scalar(got['value_u'][:, 0], v, 'v_0')
  for k in range(1, 6):
    live = got['depth'] >= k
    assert live.any()
    h, r, v, lg = net.recurrent(got['hidden_u'][live, k - 1], ac[live, k - 1])      # the device's own h_{k-1}
    close(got['hidden_u'][live, k], h, ('h_u', k)); close(got['logits_u'][live, k], lg, ('logits_u', k))
    scalar(got['value_u'][live, k], v, ('v_u', k)); scalar(got['reward_u'][live, k], r, ('r_u', k))
    _, v, lg = net.initial(got['obs'][live, k])      # the real p_k afresh
    close(got['logits_f'][live, k], lg, ('logits_f', k)); scalar(got['value_f'][live, k], v, ('v_f', k))
    dead = ~live
    for key in RAW_KEYS[5:]:      # a row whose line is shorter keeps its lane; its outputs are zero
      assert not got[key][dead, k].any(), (kind, key, k)


@pytest.mark.parametrize('kind', [1, 3])
def test_a_row_alone_gives_the_bits_it_gave_in_the_batch(kind, engines):
  bd, tn, st, ac, truth = rows(kind)
  got = unrolled(engines, kind)
  for i in (0, 3, N - 1):
    alone = engines(kind, 1).unroll(kind, bd[i:i + 1], tn[i:i + 1], st[i:i + 1], ac[i:i + 1], truth=truth[i:i + 1], raw=True)
    for key in RAW_KEYS:
      a, b = np.ascontiguousarray(alone[key]), np.ascontiguousarray(got[key][i:i + 1])
      assert a.tobytes() == b.tobytes(), (kind, i, key)


@pytest.mark.parametrize('kind', [1, 3])
def test_terms_equal_the_host_hook(kind, engines):
  bd, tn, st, ac, truth = rows(kind)
  got = unrolled(engines, kind)
  A, K1 = uu.A_OF[kind], 6
  live = (np.arange(K1)[None, :] <= got['depth'][:, None]).astype(np.uint8)
  flat = lambda x: np.ascontiguousarray(x).reshape((N * K1,) + x.shape[2:])
  want = uu.host_terms(A, flat(got['logits_u']), flat(got['logits_f']), flat(got['legal']), flat(got['terminal']), flat(live),
                       np.tile(np.arange(K1, dtype=np.int32), N), flat(got['reward_true']), flat(got['reward_u']), flat(got['value_u']),
                       flat(got['value_f']), truth=flat(truth)).reshape(N, K1, -1)
  uu.assert_terms(got['terms'], want, kind)
  T = {name: i for i, name in enumerate(uu.TERMS)}
  t = got['terms']
  assert np.all(t[:, 0, T['policy_tv']] == 0) and np.all(t[:, 0, T['value_drift']] == 0) and np.all(t[:, 0, T['top1_agree']] == 1)
  assert t[:, 1:, T['policy_tv']].max() > 0 and t[..., T['solved']].any() and t[..., T['reward_true']].any()
  if kind == 3:
    assert (t[..., T['position']] > t[..., T['solved']]).any()      # out of the solver's scope: a position, not a solved one
  no_truth = engines(kind).unroll(kind, bd[:5], tn[:5], st[:5], ac[:5])['terms']
  assert not no_truth[..., T['solved']:].any() and np.array_equal(no_truth[..., :T['solved']], t[:5, :, :T['solved']])


def test_refusals(engines):
  bd, tn, st, ac, _ = rows(1)
  args = (bd[:4], tn[:4], st[:4])
  with pytest.raises(RuntimeError, match='mz_unroll: kind must be 1'):
    engines(1).unroll(2, *args, ac[:4])
  with pytest.raises(RuntimeError, match='mz_unroll: kind must be 1'):
    engines(1).unroll(0, *args, ac[:4])
  with pytest.raises(RuntimeError, match='mz_unroll: Connect Four needs'):
    engines(1).unroll(3, *args, ac[:4])
  with pytest.raises(RuntimeError, match='mz_unroll: K must be in 0 .. 16, got 17'):
    engines(1).unroll(1, *args, np.full((4, 17), -1, np.int32))
  with pytest.raises(RuntimeError, match='mz_unroll: n must be >= 1'):
    engines(1).unroll(1, bd[:0], tn[:0], st[:0], ac[:0])
  with pytest.raises(RuntimeError, match='mz_unroll: weights not set'):
    engines(1, 8, with_weights=False).unroll(1, *args, ac[:4])
  bad = ac[:4].copy()
  bad[2, 1] = bad[2, 0]      # the cell just taken
  with pytest.raises(ValueError, match='row 2 holds an action that is illegal'):
    engines(1).unroll(1, *args, bad)


def _play(env_name, n_games, seeds0, unroll, **over):
  from model_based_rl_amd.evaluate import Evaluator
  state = eval_state(env_name, sims=8, wseed=WSEED, grade=True, grade_nodes=1 << 20, grade_unroll=unroll, **over)
  ev = Evaluator(state)
  ev.load_network()
  games = ev.play_games(n_games, list(range(seeds0, seeds0 + n_games)), device_env=True)
  return ev, games


@pytest.mark.parametrize('env_name,kind,n_games,empties,over', [
    ('TicTacToe', 1, 64, None, dict(random_opp=-1)),      # the network moves first against the random mover: its positions are the rows
    ('TicTacToe', 1, 64, None, dict(temperature=1.0)),    # both seats the network's, sampling (at T = 0 every game would be one game)
    ('ConnectFour', 3, 32, 8, dict(temperature=1.0)),
], ids=['ttt_vs_random', 'ttt_both_seats', 'c4_empties_8'])
def test_graded_unroll(env_name, kind, n_games, empties, over):
  K = 3
  over = dict(over, grade_empties=empties if empties is not None else 14)
  ev, games = _play(env_name, n_games, 700, K, **over)
  assert len({tuple(g.history.actions) for g in games}) > 8      # some variety: the rows are not one game's
  seat = -over['random_opp'] if 'random_opp' in over else None
  O, A = uu.O_OF[kind], uu.A_OF[kind]
  bd, tn, st, ac, where = uu.rows_of(games, kind, K, seat)
  truth = uu.minimax_truth(games, kind, K, where, empties)
  ref = uu.fc_unroll(uu.FC32Scalars(weights(O, A, WSEED), O, A), kind, bd, tn, st, ac, truth)
  got, want = ev.grade_unroll_report, uu.py_report(ref['terms'], K)
  print(got)
  for g, w in zip(got['depth'], want['depth']):
    print(g['k'], {key: (g[key], w[key]) for key in w if key not in uu.COUNTS and w[key] is not None and abs(g[key] - w[key]) > 1e-7})
  assert got['rows'] == len(bd) > 0
  uu.assert_report({key: got[key] for key in ('K', 'rows', 'depth')}, want, 1e-5, env_name)
  d0 = got['depth'][0]
  assert d0['value_drift'] == 0.0 and d0['policy_tv'] == 0.0 and d0['top1_agree'] == 1.0
  if kind == 1:
    # TicTacToe is solved everywhere: depth 0's fresh value error is --grade's pred_value_mae, the same observations through the
    # same inference, to within the mean of scalar_bound over the graded values
    assert all(d['solved'] == d['positions'] for d in got['depth'])
    pred = np.array([games[gi].pred_values[p] for gi, p in where], np.float64)
    assert ev.grade_report['graded'] == d0['solved'] == len(pred)
    bound = float(fc64.scalar_bound(pred, SUPPORT, True).mean())
    print('value_mae_fresh', d0['value_mae_fresh'], 'pred_value_mae', ev.grade_report['pred_value_mae'], 'bound', bound)
    assert abs(d0['value_mae_fresh'] - ev.grade_report['pred_value_mae']) <= bound
  else:
    # a scope: solved < positions at small k, and nothing in scope is dropped (the restatement's minimax solves all of it)
    assert 0 < d0['solved'] < d0['positions']
    assert d0['solved'] == sum(1 for _, p in where if 42 - p <= empties)
  # the --grade report itself is the one of a run without the flag, key for key
  plain, games2 = _play(env_name, n_games, 700, None, **over)
  assert plain.grade_unroll_report is None and [g.history.actions for g in games2] == [g.history.actions for g in games]
  a, b = dict(ev.grade_report), dict(plain.grade_report)
  a.pop('seconds'); b.pop('seconds')
  assert a == b and 'unroll' not in a


def test_unroll_state_is_its_own():
  """two engines play the same evaluation games; one of them unrolls rows before the reset and between the chunks of moves.
  Their records are equal"""
  from model_based_rl_amd.engine import Engine
  from model_based_rl_amd.evaluate import flatten_weights
  state = eval_state('ConnectFour', sims=6)
  bd, tn, st, ac, truth = rows(3)
  first = None
  results = []
  for unrolling in (False, True):
    eng = Engine.from_config(state['config'], 16, device='cuda:0', seed=0, env_id_offset=40)
    try:
      eng.set_weights(flatten_weights(state['weights']))
      if unrolling:
        first = eng.unroll(3, bd[:40], tn[:40], st[:40], ac[:40], truth=truth[:40], raw=True)
      eng.eval_env_reset('ConnectFour', 42, 0, None, True)
      live, chunks = 16, 0
      while live > 0 and chunks < 6:
        live = eng.eval_env_moves(8, 0, 1, 0.0, False)
        chunks += 1
        if unrolling:
          again = eng.unroll(3, bd[:40], tn[:40], st[:40], ac[:40], truth=truth[:40], raw=True)
          for key in RAW_KEYS:      # and the games leave the unroll alone
            assert np.ascontiguousarray(again[key]).tobytes() == np.ascontiguousarray(first[key]).tobytes(), key
      assert live == 0
      results.append(eng.eval_env_results())
    finally:
      eng.close()
  plain, unrolled_ = results
  assert set(plain) == set(unrolled_)
  for key in plain:
    assert np.array_equal(np.asarray(plain[key]), np.asarray(unrolled_[key])), key
