"""Grading of evaluation games against the exact solver (Engine.solve; DESIGN s7f): the positions of keep_history games are
rebuilt on the host rules of envs.py, solved on the device, and every graded decision is compared with the game-theoretic
value of its position.

Perspective: history.root_values[k] is the searched root's value and pred_values[k] the value head's output at move k.  The
root is expanded with to_play = the mover and the backup adds a leaf's value to a node with the sign of that node's own
to_play (mcts.py:126-128), and the value head reads the observation turn * board: both are the MOVER's view, which is the
view of the solver's values, so no sign is applied."""
import numpy as np

from .engine import Engine
from .envs import BOARD_KINDS as KINDS, CELLS, ConnectFour, TicTacToe

ILLEGAL, UNSOLVED = -2, -3
BLUNDERS = ('win_to_draw', 'win_to_loss', 'draw_to_loss')
DEFAULT_EMPTIES = 12      # Connect Four: positions with at most this many empty cells are graded (derived from profiles/solve_bench.json: README)
DEFAULT_NODES = Engine.SOLVE_NODES


def _kind(kind):
  k = KINDS[kind] if isinstance(kind, str) else int(kind)
  if k not in CELLS:
    raise ValueError('the solver plays TicTacToe (1) and ConnectFour (3), got kind %r' % (kind,))
  return k


def positions_of(games, kind, min_step=0):
  """the position before every action of keep_history games, replayed from history.actions on envs.TicTacToe /
  envs.ConnectFour; min_step: only the positions with at least so many plies played (a game that ended before is not
  replayed at all).  Returns a dict of arrays over the P positions: boards [P, 42] int8, turn [P] int8 (the mover), step [P]
  int32, game [P] int32 (index into games), ply [P] int32, action [P] int32 (the action taken there)."""
  k = _kind(kind)
  cells = CELLS[k]
  boards, turn, step, game, ply, action = [], [], [], [], [], []
  for gi, g in enumerate(games):
    if g.history is None:
      raise ValueError('positions_of: game %d carries no history (play the games with keep_history)' % gi)
    if len(g.history.actions) <= min_step:
      continue
    env = TicTacToe() if k == 1 else ConnectFour()
    done = False
    for p, a in enumerate(g.history.actions):
      if done:
        raise ValueError('positions_of: game %d goes on after its end at ply %d' % (gi, p))
      if p >= min_step:
        bd = np.zeros(42, np.int8)
        bd[:cells] = env.board
        boards.append(bd); turn.append(env.turn); step.append(p); game.append(gi); ply.append(p); action.append(int(a))
      _, _, done, _ = env.step(int(a))
  return dict(boards=np.array(boards, np.int8).reshape(-1, 42), turn=np.array(turn, np.int8), step=np.array(step, np.int32),
              game=np.array(game, np.int32), ply=np.array(ply, np.int32), action=np.array(action, np.int32))


def grade_games(games, kind, engine, max_empties=None, graded_seat=None, max_nodes=DEFAULT_NODES, table=False):
  """grade the decisions of keep_history games (one applied action per move).  engine: an Engine of the game's shape (its
  solve() is all that is used).  max_empties: only positions with at most so many empty cells (None: all).  graded_seat: +1
  / -1 grades the moves of that seat only (the network's, when the other seat is an opponent's), None both.  table: solve
  with the table search (engine.solve(table=True)); the report then carries solver: 'table'.

  Per decision, with value[a] the solver's outcome for the mover after a: v* = max over a of value[a], c = value[action].
  A decision is graded when both are solved: c is not -3, and v* is +1 or no legal action is -3.  Returns a dict: graded;
  unsolved (in scope but left out, counted); optimal (c == v*) and optimal_rate; blunders {win_to_draw, win_to_loss,
  draw_to_loss}; root_value_mae / pred_value_mae (mean |x - v*|, the mover's view); decisive (graded with v* != 0) and
  root_value_sign / pred_value_sign, the share of the decisive ones with sign(x) == v*; nodes, the solver's total.  Rates
  over an empty set are None."""
  k = _kind(kind)
  pos = positions_of(games, k, 0 if max_empties is None else max(0, CELLS[k] - int(max_empties)))
  scope = np.ones(len(pos['turn']), bool)
  if graded_seat is not None:
    scope &= pos['turn'] == int(graded_seat)
  idx = np.flatnonzero(scope)
  report = dict(graded=0, unsolved=0, optimal=0, optimal_rate=None, blunders={b: 0 for b in BLUNDERS}, root_value_mae=None,
                pred_value_mae=None, decisive=0, root_value_sign=None, pred_value_sign=None, nodes=0,
                max_empties=None if max_empties is None else int(max_empties), max_nodes=int(max_nodes))
  if table:
    report['solver'] = 'table'
  if len(idx) == 0:
    return report
  values, nodes = engine.solve(k, pos['boards'][idx], pos['turn'][idx], pos['step'][idx], max_nodes=int(max_nodes),
                               **(dict(table=True) if table else {}))
  values = np.asarray(values).astype(np.int64)
  report['nodes'] = int(np.asarray(nodes, np.uint64).sum())
  best = values.max(1)
  chosen = values[np.arange(len(idx)), pos['action'][idx]]
  if np.any(chosen == ILLEGAL):
    raise ValueError('grade_games: a game record holds an action that is illegal in its position')
  solved = (chosen != UNSOLVED) & ((best == 1) | ~(values == UNSOLVED).any(1))
  report['unsolved'] = int((~solved).sum())
  report['graded'] = n = int(solved.sum())
  if n == 0:
    return report
  best, chosen, at = best[solved], chosen[solved], idx[solved]
  report['optimal'] = int((chosen == best).sum())
  report['optimal_rate'] = report['optimal'] / n
  report['blunders'] = dict(win_to_draw=int(((best == 1) & (chosen == 0)).sum()), win_to_loss=int(((best == 1) & (chosen == -1)).sum()),
                            draw_to_loss=int(((best == 0) & (chosen == -1)).sum()))
  root = np.array([games[g].history.root_values[p] for g, p in zip(pos['game'][at], pos['ply'][at])], np.float64)
  pred = np.array([games[g].pred_values[p] for g, p in zip(pos['game'][at], pos['ply'][at])], np.float64)
  report['root_value_mae'] = float(np.mean(np.abs(root - best)))
  report['pred_value_mae'] = float(np.mean(np.abs(pred - best)))
  dec = best != 0
  report['decisive'] = int(dec.sum())
  if report['decisive']:
    report['root_value_sign'] = float(np.mean(np.sign(root[dec]) == best[dec]))
    report['pred_value_sign'] = float(np.mean(np.sign(pred[dec]) == best[dec]))
  return report


def _mean(x, where):
  """the mean of x over the set `where`, summed in float64 in row order; None over an empty set"""
  x = np.asarray(x, np.float64)[where]
  return None if x.size == 0 else float(np.cumsum(x)[-1] / x.size)


def grade_unroll(games, kind, engine, K, max_empties=None, graded_seat=None, max_nodes=DEFAULT_NODES, table=False):
  """the learned model by unroll depth against the true game (Engine.unroll; DESIGN s7f, "Grading by unroll depth").  A row
  is a position of the keep_history games whose mover is graded_seat (None: both seats; every ply counts, not only the
  solver's scope) with the next K actions of the same game, whoever played them.  Along those actions the model is unrolled
  (h_k = dynamics(h_{k-1}, a_{k-1}): the UNROLLED value, reward and policy at depth k) next to the real positions p_k they
  lead to, each seen afresh through the representation (the FRESH value and policy).  Truth comes from one engine.solve over
  every position of those games, both seats, with at most max_empties empty cells (None: all), looked up by (game, ply + k):
  v*(p) is known when the best value is +1 or no legal action is unsolved (grade_games's rule without the chosen-action
  clause), and the optimal actions are the legal ones whose value is v*.

  Perspective: no sign is applied.  The value target of an unrolled position is its n-step return in the view of that
  position's own mover (replay_buffer.py:177-190), so the value at depth k -- unrolled or fresh -- is in the view of p_k's
  mover, which is the view of the solver's values of p_k.

  Returns dict(K, rows, depth=[one dict per k = 0 .. K]); each count is followed by means over its own set (None over an empty
  set): n (rows whose line reaches k); transitions (n at k >= 1), reward_mae, wins (the move into p_k won), reward_at_wins,
  reward_elsewhere; positions (p_k not terminal), value_drift (mean |v_u - v_f|), policy_tv (mean 1/2 sum |softmax u - softmax
  f|), top1_agree, illegal_mass / illegal_mass_fresh (softmax mass on actions illegal in p_k); solved (v* known), value_mae /
  value_mae_fresh (against v*), decisive (v* != 0), value_sign / value_sign_fresh (share of the decisive with sign(v) == v*),
  optimal_mass / optimal_mass_fresh.  The means are sums in float64 in row order over the per-(row, k) scalars, so a report
  does not depend on the engine's num_envs."""
  k = _kind(kind)
  K = int(K)
  if K < 0 or K > Engine.UNROLL_MAX_K:
    raise ValueError('grade_unroll: K must be in 0 .. %d, got %d' % (Engine.UNROLL_MAX_K, K))
  A = 9 if k == 1 else 7
  pos = positions_of(games, k)
  P = len(pos['turn'])
  taken = pos['action'].astype(np.int64)
  if np.any((taken < 0) | (taken >= A)) or np.any(pos['boards'][np.arange(P), np.clip(taken, 0, A - 1) + (35 if k == 3 else 0)] != 0):
    raise ValueError('grade_unroll: a game record holds an action that is illegal in its position')
  rows = np.ones(P, bool) if graded_seat is None else pos['turn'] == int(graded_seat)
  idx = np.flatnonzero(rows)
  report = dict(K=K, rows=int(len(idx)), depth=[])
  T = {name: i for i, name in enumerate(Engine.UNROLL_TERMS)}
  if len(idx):
    scope = np.ones(P, bool) if max_empties is None else CELLS[k] - pos['step'] <= int(max_empties)
    values = np.full((P, A), UNSOLVED, np.int8)
    if scope.any():
      values[scope] = engine.solve(k, pos['boards'][scope], pos['turn'][scope], pos['step'][scope], max_nodes=int(max_nodes),
                                   **(dict(table=True) if table else {}))[0]
    # positions_of lists a game's positions one after the other from ply 0, so (game, ply + j) is position i + j while
    # ply + j stays inside the game
    plies = np.bincount(pos['game'], minlength=len(games))[pos['game']]
    inside = pos['ply'][idx, None] + np.arange(K + 1)[None, :] < plies[idx, None]
    q = np.where(inside, idx[:, None] + np.arange(K + 1)[None, :], 0)
    actions = np.where(inside[:, :K], pos['action'][q[:, :K]], -1).astype(np.int32)
    truth = np.where(inside[:, :, None], values[q], UNSOLVED).astype(np.int8)
    try:
      terms = engine.unroll(k, pos['boards'][idx], pos['turn'][idx], pos['step'][idx], actions, truth=truth)['terms']
    except ValueError:
      raise ValueError('grade_unroll: a game record holds an action that is illegal in its position')
  else:
    terms = np.zeros((0, K + 1, len(T)), np.float64)
  for j in range(K + 1):
    t = lambda name: terms[:, j, T[name]]
    live, tr, ps, sv = t('live') != 0, t('transition') != 0, t('position') != 0, t('solved') != 0
    win, dec = tr & (t('reward_true') == 1), sv & (t('vstar') != 0)
    report['depth'].append(dict(
        k=j, n=int(live.sum()),
        transitions=int(tr.sum()), reward_mae=_mean(t('reward_err'), tr), wins=int(win.sum()), reward_at_wins=_mean(t('reward'), win),
        reward_elsewhere=_mean(t('reward'), tr & ~win),
        positions=int(ps.sum()), value_drift=_mean(t('value_drift'), ps), policy_tv=_mean(t('policy_tv'), ps),
        top1_agree=_mean(t('top1_agree'), ps), illegal_mass=_mean(t('illegal_mass'), ps), illegal_mass_fresh=_mean(t('illegal_mass_fresh'), ps),
        solved=int(sv.sum()), value_mae=_mean(t('value_err'), sv), value_mae_fresh=_mean(t('value_err_fresh'), sv),
        decisive=int(dec.sum()), value_sign=_mean(t('sign'), dec), value_sign_fresh=_mean(t('sign_fresh'), dec),
        optimal_mass=_mean(t('optimal_mass'), sv), optimal_mass_fresh=_mean(t('optimal_mass_fresh'), sv)))
  return report


def format_unroll(r, label=''):
  """the block the evaluate CLI prints per configuration with --grade_unroll: one line per depth.  u: the model unrolled k
  steps along the moves played; f: the real position p_k seen afresh (at k = 0 the two are one computation)"""
  pct = lambda x: 'n/a' if x is None else '{:.1f}%'.format(100.0 * x)
  num = lambda x: 'n/a' if x is None else '{:.3f}'.format(x)
  lines = ['The model by unroll depth against the true game{}: {} rows, K = {}'.format(
      ' - label: ({})'.format(label) if label else '', r['rows'], r['K'])]
  for d in r['depth']:
    lines.append(
        'k={:<2d} n {} | reward mae {} at wins {} ({}) elsewhere {} | drift {} tv {} top1 {} illegal u {} f {} | solved {} of {}: '
        'value mae u {} f {} sign u {} f {} ({} decisive) optimal mass u {} f {}'.format(
            d['k'], d['n'], num(d['reward_mae']), num(d['reward_at_wins']), d['wins'], num(d['reward_elsewhere']), num(d['value_drift']),
            num(d['policy_tv']), pct(d['top1_agree']), num(d['illegal_mass']), num(d['illegal_mass_fresh']), d['solved'], d['positions'],
            num(d['value_mae']), num(d['value_mae_fresh']), pct(d['value_sign']), pct(d['value_sign_fresh']), d['decisive'],
            num(d['optimal_mass']), num(d['optimal_mass_fresh'])))
  lines.append('')
  return '\n'.join(lines)


def format_report(r, label=''):
  """the block the evaluate CLI prints per configuration"""
  pct = lambda x: 'n/a' if x is None else '{:.1f}%'.format(100.0 * x)
  num = lambda x: 'n/a' if x is None else '{:.3f}'.format(x)
  b = r['blunders']
  scope = 'every position' if r['max_empties'] is None else 'positions with at most {} empty cells'.format(r['max_empties'])
  return '\n'.join([
      'Graded against the exact solver{}{}: {} decisions ({}), {} left out as unsolved within {} nodes'.format(
          ' (table search)' if r.get('solver') == 'table' else '', ' - label: ({})'.format(label) if label else '', r['graded'],
          scope, r['unsolved'], r['max_nodes']),
      'Optimal moves: {} of {} ({})'.format(r['optimal'], r['graded'], pct(r['optimal_rate'])),
      'Blunders: win to draw {}, win to loss {}, draw to loss {}'.format(b['win_to_draw'], b['win_to_loss'], b['draw_to_loss']),
      'Value error against the true value: mcts {} (sign right {}), predicted {} (sign right {}) - {} decisive positions'.format(
          num(r['root_value_mae']), pct(r['root_value_sign']), num(r['pred_value_mae']), pct(r['pred_value_sign']), r['decisive']),
      ''])
