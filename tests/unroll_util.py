"""Helpers of the unroll-diagnostic tests (no test functions here): the ctypes host hooks mz_unroll_lines_host and
mz_unroll_terms_host, and a Python restatement of the definition (DESIGN s7f, "Grading by unroll depth") written from it
alone: lines on the rules of tests/playout_py.py, the network as tests/fc64.FC64, the terms with math.exp, the report as
plain loops.  Nothing of the native code or of solver.grade_unroll is used by the restatement."""
import ctypes as C
import math
import types

import numpy as np

from tests import fc64
from tests import playout_py as pp
from tests import solve_util as su

A_OF, O_OF = {1: 9, 3: 7}, {1: 9, 3: 42}
TERMS = ('live', 'transition', 'position', 'reward_true', 'reward', 'reward_err', 'value', 'value_fresh', 'value_drift', 'policy_tv',
         'top1_agree', 'illegal_mass', 'illegal_mass_fresh', 'solved', 'vstar', 'value_err', 'value_err_fresh', 'sign', 'sign_fresh',
         'optimal_mass', 'optimal_mass_fresh')      # the documented order (include/mz_engine.h -> csrc/mz_unroll.hip.h MzUnrollTerm)
EXACT = ('live', 'transition', 'position', 'reward_true', 'top1_agree', 'solved', 'vstar', 'sign', 'sign_fresh')      # counts and outcomes
TOL = 1e-12      # masses and means: the sides differ in exp() only, a few ulp a term, over at most A + 1 terms of a quantity in [0, 1]

_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
  from model_based_rl_amd import _abi
  return _abi, _abi.load()


def host_lines(kind, boards, turn, step, actions):
  """mz_unroll_lines_host -> dict(obs [n, K + 1, O] f32, legal [n, K + 1, A] u8, terminal [n, K + 1] u8, reward_true [n, K + 1] f32,
  depth [n], flags [n])"""
  abi, lib = _lib()
  bd = np.ascontiguousarray(boards, np.int8).reshape(-1, 42)
  tn, st = np.ascontiguousarray(turn, np.int8), np.ascontiguousarray(step, np.int32)
  ac = np.ascontiguousarray(actions, np.int32)
  ac = ac.reshape(len(bd), ac.shape[-1] if ac.ndim == 2 else -1)
  n, K = ac.shape
  O, A = O_OF.get(kind, 9), A_OF.get(kind, 9)
  obs, legal = np.full((n, K + 1, O), 7, np.float32), np.full((n, K + 1), 7, np.uint32)
  term, rt = np.full((n, K + 1), 7, np.uint8), np.full((n, K + 1), 7, np.float32)
  depth, flags = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
  abi.check(lib.mz_unroll_lines_host(kind, _p(bd), _p(tn), _p(st), _p(ac), n, K, _p(obs), _p(legal), _p(term), _p(rt), _p(depth), _p(flags)),
            'mz_unroll_lines_host')
  return dict(obs=obs, legal=((legal[..., None] >> np.arange(A)) & 1).astype(np.uint8), terminal=term, reward_true=rt, depth=depth,
              flags=flags)


def host_terms(A, logits_u, logits_f, legal, terminal, live, k, reward_true, reward_u, value_u, value_f, truth=None):
  """mz_unroll_terms_host over items: legal [items, A] 0 / 1 -> terms [items, len(TERMS)] float64"""
  abi, lib = _lib()
  f = lambda x: np.ascontiguousarray(x, np.float32)
  lu, lf = f(logits_u).reshape(-1, A), f(logits_f).reshape(-1, A)
  n = len(lu)
  mask = np.ascontiguousarray((np.asarray(legal, np.int64).reshape(n, A) << np.arange(A)).sum(1), np.uint32)
  u8 = lambda x: np.ascontiguousarray(x, np.uint8).reshape(n)
  th = None if truth is None else np.ascontiguousarray(truth, np.int8).reshape(n, A)
  assert lib.mz_unroll_num_terms() == len(TERMS)
  out = np.full((n, len(TERMS)), 7.0, np.float64)
  abi.check(lib.mz_unroll_terms_host(A, n, _p(lu), _p(lf), _p(mask), _p(u8(terminal)), _p(u8(live)),
                                     _p(np.ascontiguousarray(k, np.int32).reshape(n)), _p(f(reward_true).reshape(n)),
                                     _p(f(reward_u).reshape(n)), _p(f(value_u).reshape(n)), _p(f(value_f).reshape(n)), _p(th), _p(out)),
            'mz_unroll_terms_host')
  return out


# ---- the restatement: lines
def py_line(kind, board, turn, step, actions):
  """one row: dict(obs [K + 1][O], legal [K + 1][A], terminal [K + 1], reward_true [K + 1], acts [K + 1] (the action applied in
  p_k, 0 where none), depth, flag); depths past the line's end are zero"""
  O, A, K = O_OF[kind], A_OF[kind], len(actions)
  bd, mover, term, rt = [int(x) for x in board], int(turn), False, 0.0
  out = dict(obs=np.zeros((K + 1, O), np.float32), legal=np.zeros((K + 1, A), np.uint8), terminal=np.zeros(K + 1, np.uint8),
             reward_true=np.zeros(K + 1, np.float32), acts=np.zeros(K + 1, np.int32), depth=0, flag=0)
  for k in range(K + 1):
    legal = pp.legal_actions(kind, bd)
    out['obs'][k] = [mover * c for c in bd[:O]]
    out['legal'][k, legal] = 1
    out['terminal'][k], out['reward_true'][k], out['depth'] = int(term), rt, k
    if term or k == K or actions[k] < 0:
      break
    a = int(actions[k])
    if a not in legal:
      out['flag'] = 1
      break
    end = pp.play(kind, bd, mover, a)
    term, rt, mover = end != 0, 1.0 if end == 1 else 0.0, -mover
    out['acts'][k] = a
  return out


def py_lines(kind, boards, turn, step, actions):
  rows = [py_line(kind, b, t, s, a) for b, t, s, a in zip(boards, turn, step, np.asarray(actions).reshape(len(boards), -1))]
  out = {key: np.array([r[key] for r in rows]) for key in ('obs', 'legal', 'terminal', 'reward_true', 'acts')}
  out['depth'], out['flags'] = np.array([r['depth'] for r in rows], np.int32), np.array([r['flag'] for r in rows], np.int32)
  return out


# ---- the restatement: terms
def _softmax(lg):
  lg = [float(x) for x in lg]
  e = [math.exp(x - max(lg)) for x in lg]
  s = 0.0
  for x in e:
    s += x
  return [x / s for x in e]


def py_terms(lu, lf, legal, terminal, live, k, rtrue, ru, vu, vf, truth=None):
  """the scalars of one (row, k) as a dict over TERMS"""
  t = dict.fromkeys(TERMS, 0.0)
  if not live:
    return t
  t['live'] = 1.0
  if k >= 1:
    t.update(transition=1.0, reward_true=float(rtrue), reward=float(ru), reward_err=abs(float(ru) - float(rtrue)))
  if terminal:
    return t
  A = len(lu)
  pu, pf = _softmax(lu), _softmax(lf)
  top = lambda lg: max(range(A), key=lambda a: (float(lg[a]), a))      # ties: the largest action
  t.update(position=1.0, value=float(vu), value_fresh=float(vf), value_drift=abs(float(vu) - float(vf)),
           policy_tv=0.5 * sum(abs(a - b) for a, b in zip(pu, pf)), top1_agree=float(top(lu) == top(lf)),
           illegal_mass=sum(pu[a] for a in range(A) if not legal[a]), illegal_mass_fresh=sum(pf[a] for a in range(A) if not legal[a]))
  if truth is None:
    return t
  vals = [int(truth[a]) for a in range(A) if legal[a]]
  best = max(vals)
  if not (best == 1 or (best >= -1 and all(v >= -1 for v in vals))):
    return t
  sign = lambda v: (v > 0) - (v < 0)
  opt = [a for a in range(A) if legal[a] and int(truth[a]) == best]
  t.update(solved=1.0, vstar=float(best), value_err=abs(float(vu) - best), value_err_fresh=abs(float(vf) - best),
           optimal_mass=sum(pu[a] for a in opt), optimal_mass_fresh=sum(pf[a] for a in opt))
  if best != 0:
    t.update(sign=float(sign(float(vu)) == best), sign_fresh=float(sign(float(vf)) == best))
  return t


def terms_array(items):
  return np.array([[d[name] for name in TERMS] for d in items], np.float64).reshape(len(items), len(TERMS))


def assert_terms(got, want, what=''):
  """two terms arrays [..., len(TERMS)]: counts and outcomes exactly, the rest within TOL"""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  for i, name in enumerate(TERMS):
    g, w = got[..., i], want[..., i]
    if name in EXACT:
      assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())
    else:
      assert np.all(np.abs(g - w) <= TOL), (what, name, float(np.abs(g - w).max()))


# ---- the restatement: the network along a line
class FC32Scalars(fc64.FC64):
  """FC64 whose value / reward scalars take the inverse transform in float32, as the reference network computes it: in float32
  its sqrt(...) - 1 cancellation makes the reference's own output a staircase (fc64.inverse_h), and a report's means are held
  more tightly than one step of it"""

  def _scalar(self, out, smin):
    if self.ns:
      return out[:, 0].copy()
    x = fc64.support_to_scalar64(out, smin, True)
    return x if self.nt else fc64.inverse_h(x.astype(np.float32), np.float32).astype(np.float64)


def fc_unroll(net, kind, boards, turn, step, actions, truth=None):
  """the model unrolled along the lines of the rows through `net` (an FC64): dict(depth, flags, terms [n, K + 1, len(TERMS)]
  and the raw arrays under Engine.unroll's names); the network outputs are rounded to float32 before the terms, as the device
  hands them on"""
  actions = np.asarray(actions, np.int32).reshape(len(boards), -1)
  n, K = actions.shape
  A = A_OF[kind]
  L = py_lines(kind, boards, turn, step, actions)
  f32 = lambda x: np.asarray(x, np.float32)
  hid, val_u, rew_u, lg_u = (np.zeros((n, K + 1, fc64.H), np.float32), np.zeros((n, K + 1), np.float32), np.zeros((n, K + 1), np.float32),
                              np.zeros((n, K + 1, A), np.float32))
  val_f, lg_f = np.zeros((n, K + 1), np.float32), np.zeros((n, K + 1, A), np.float32)
  h, v, lg = net.initial(L['obs'][:, 0])
  hid[:, 0], val_u[:, 0], lg_u[:, 0], val_f[:, 0], lg_f[:, 0] = f32(h), f32(v), f32(lg), f32(v), f32(lg)
  for k in range(1, K + 1):
    live = L['depth'] >= k
    if not live.any():
      break
    h, r, v, lg = net.recurrent(hid[live, k - 1], L['acts'][live, k - 1])
    hid[live, k], rew_u[live, k], val_u[live, k], lg_u[live, k] = f32(h), f32(r), f32(v), f32(lg)
    _, v, lg = net.initial(L['obs'][live, k])
    val_f[live, k], lg_f[live, k] = f32(v), f32(lg)
  items = [py_terms(lg_u[i, k], lg_f[i, k], L['legal'][i, k], L['terminal'][i, k], k <= L['depth'][i], k, L['reward_true'][i, k],
                    rew_u[i, k], val_u[i, k], val_f[i, k], None if truth is None else truth[i][k])
           for i in range(n) for k in range(K + 1)]
  return dict(depth=L['depth'], flags=L['flags'], terms=terms_array(items).reshape(n, K + 1, len(TERMS)), obs=L['obs'], hidden_u=hid,
              logits_u=lg_u, logits_f=lg_f, value_u=val_u, reward_u=rew_u, value_f=val_f, reward_true=L['reward_true'], legal=L['legal'],
              terminal=L['terminal'])


class StubEngine(object):
  """what solver.grade_unroll takes for an engine, without a device: unroll through the restatement, solve through the host hook"""

  def __init__(self, net, kind):
    self.net, self.kind, self.solve_calls = net, kind, 0

  def unroll(self, kind, boards, turn, step, actions, truth=None, raw=False):
    out = fc_unroll(self.net, kind, boards, turn, step, actions, truth)
    if out['flags'].any():
      raise ValueError('unroll: a row holds an action that is illegal in its position')
    return out

  def solve(self, kind, boards, turn, step, max_nodes=su.BUDGET, table=False):
    self.solve_calls += 1
    return su.host_solve(kind, boards, turn, step, max_nodes=max_nodes)


# ---- games, and the report recomputed in plain Python
def random_games(kind, n, seed, min_len=0):
  """n games of uniformly random legal play, each of at least min_len plies, as keep_history games (history.actions,
  history.to_play, step)"""
  rng = np.random.RandomState(seed)
  games = []
  while len(games) < n:
    bd, mover, acts, movers = [0] * 42, 1, [], []
    while True:
      legal = pp.legal_actions(kind, bd)
      a = int(legal[rng.randint(len(legal))])
      acts.append(a); movers.append(mover)
      if pp.play(kind, bd, mover, a):
        break
      mover = -mover
    if len(acts) >= min_len:
      games.append(types.SimpleNamespace(history=types.SimpleNamespace(actions=acts, to_play=movers), step=len(acts)))
  return games


def rows_of(games, kind, K, seat=None):
  """the rows of solver.grade_unroll from the kept histories: (boards, turn, step, actions [n, K], where [(game, ply)])"""
  boards, turn, step, actions, where = [], [], [], [], []
  for gi, g in enumerate(games):
    bd, mover = [0] * 42, 1
    for p, a in enumerate(g.history.actions):
      if seat in (None, mover):
        boards.append(list(bd)); turn.append(mover); step.append(p); where.append((gi, p))
        nxt = [int(x) for x in g.history.actions[p:p + K]]
        actions.append(nxt + [-1] * (K - len(nxt)))
      pp.play(kind, bd, mover, int(a))
      mover = -mover
  return (np.array(boards, np.int8).reshape(-1, 42), np.array(turn, np.int8), np.array(step, np.int32),
          np.array(actions, np.int32).reshape(len(boards), K), where)


def minimax_truth(games, kind, K, where, max_empties=None):
  """truth [n, K + 1, A] by the Python minimax of tests/solve_util.py: the values of the actions of p_k = the position before
  ply + k of the same game, -3 everywhere where that position has more than max_empties empty cells or the game is over"""
  cells, A = (9 if kind == 1 else 42), A_OF[kind]
  before = []      # per game: the position before every ply
  for g in games:
    bd, mover, ps = [0] * 42, 1, []
    for a in g.history.actions:
      ps.append((list(bd), mover))
      pp.play(kind, bd, mover, int(a))
      mover = -mover
    before.append(ps)
  truth = np.full((len(where), K + 1, A), -3, np.int8)
  for r, (gi, p) in enumerate(where):
    for k in range(K + 1):
      if p + k < len(before[gi]) and (max_empties is None or cells - (p + k) <= max_empties):
        truth[r, k] = su.action_values(kind, *before[gi][p + k])
  return truth


def py_report(terms, K):
  """dict(K, rows, depth=[...]) from terms [n, K + 1, len(TERMS)] by plain loops"""
  T = {name: i for i, name in enumerate(TERMS)}
  mean = lambda xs: None if not xs else sum(xs) / len(xs)
  depth = []
  for k in range(K + 1):
    rows = [terms[i, k] for i in range(len(terms))]
    col = lambda name, sel: [float(r[T[name]]) for r in rows if sel(r)]
    live = lambda r: r[T['live']] != 0
    tr = lambda r: r[T['transition']] != 0
    win = lambda r: tr(r) and r[T['reward_true']] == 1
    ps = lambda r: r[T['position']] != 0
    sv = lambda r: r[T['solved']] != 0
    dec = lambda r: sv(r) and r[T['vstar']] != 0
    depth.append(dict(
        k=k, n=len(col('live', live)), transitions=len(col('live', tr)), reward_mae=mean(col('reward_err', tr)), wins=len(col('live', win)),
        reward_at_wins=mean(col('reward', win)), reward_elsewhere=mean(col('reward', lambda r: tr(r) and not win(r))),
        positions=len(col('live', ps)), value_drift=mean(col('value_drift', ps)), policy_tv=mean(col('policy_tv', ps)),
        top1_agree=mean(col('top1_agree', ps)), illegal_mass=mean(col('illegal_mass', ps)), illegal_mass_fresh=mean(col('illegal_mass_fresh', ps)),
        solved=len(col('live', sv)), value_mae=mean(col('value_err', sv)), value_mae_fresh=mean(col('value_err_fresh', sv)),
        decisive=len(col('live', dec)), value_sign=mean(col('sign', dec)), value_sign_fresh=mean(col('sign_fresh', dec)),
        optimal_mass=mean(col('optimal_mass', sv)), optimal_mass_fresh=mean(col('optimal_mass_fresh', sv))))
  return dict(K=K, rows=len(terms), depth=depth)


COUNTS = ('k', 'n', 'transitions', 'wins', 'positions', 'solved', 'decisive')


def assert_report(got, want, tol, what=''):
  """counts exactly, means within tol (None where the set is empty on both sides)"""
  assert got['K'] == want['K'] and got['rows'] == want['rows'] and len(got['depth']) == len(want['depth']) == want['K'] + 1, what
  for g, w in zip(got['depth'], want['depth']):
    assert set(g) == set(w), (what, set(g) ^ set(w))
    for key in w:
      if key in COUNTS or w[key] is None or g[key] is None:
        assert g[key] == w[key], (what, w['k'], key, g[key], w[key])
      else:
        assert abs(g[key] - w[key]) <= tol, (what, w['k'], key, g[key], w[key])
