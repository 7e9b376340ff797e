"""Helpers of the evaluation front end's record test (no test functions here): the configurations whose games are pinned and
the SHA-256 of everything such a run returns.  scripts/make_eval_front_end_digests.py writes the digests of CASES to
tests/golden/eval_front_end_sha256.json; tests/test_gpu_eval_front_end.py recomputes them.

Shapes: 8 games, seeds 100 .. 107, batches of 4 -- two engines with different env_id_offset, the smallest run that crosses a
batch boundary -- on eval_device_util.eval_state(env, sims=8) (a match seats wseed 5 against wseed 6)."""
import copy
import functools
import hashlib

import numpy as np

from tests.eval_device_util import eval_state

GAMES, SEED0, BATCH = 8, 100, 4
BOARD = ('TicTacToe', 'ConnectFour')


def _cases():
  """name -> ('games', env, config attributes, play_games keywords) or ('match', env, (attributes of A, of B), play_match
  keywords)"""
  out = {}
  for name, over in (('plain', {}), ('only_prior', dict(only_prior=1)), ('only_value', dict(only_value=1)),
                     ('noise_t1_m3', dict(use_exploration_noise=1, temperature=1.0, apply_mcts_actions=3))):
    out['host/TicTacToe/' + name] = ('games', 'TicTacToe', over, {})
  for env in BOARD + ('CartPole-v0',):
    out['device/%s/plain' % env] = ('games', env, {}, dict(device_env=True))
    out['device/%s/keep_history' % env] = ('games', env, {}, dict(device_env=True, keep_history=True))
  kept = dict(device_env=True, keep_history=True)
  for env in BOARD:
    out['device/%s/true_model' % env] = ('games', env, {}, dict(kept, true_model=True))
    out['device/%s/gumbel' % env] = ('games', env, {}, dict(kept, gumbel=True))
    out['device/%s/gumbel_scale1' % env] = ('games', env, dict(gumbel_scale=1.0), dict(kept, gumbel=True))
    out['device/%s/random_opp' % env] = ('games', env, dict(random_opp=-1), kept)
    out['device/%s/random_opp_playouts64' % env] = ('games', env, dict(random_opp=-1, opp_playouts=64), kept)
  out['device/TicTacToe/grade_unroll2'] = ('games', 'TicTacToe', dict(grade=True, grade_unroll=2), kept)
  for env in BOARD:
    for name, sides, kw in (('plain', ({}, {}), {}), ('opening2', ({}, {}), dict(opening_plies=2)),
                            ('only_value_vs_search', (dict(only_value=1), {}), {}),
                            ('true_model_1_0', ({}, {}), dict(true_model=(1, 0))), ('gumbel_0_1', ({}, {}), dict(gumbel=(0, 1))),
                            ('temperature_noise_1_0', (dict(temperature=1.0, use_exploration_noise=1), {}), {})):
      out['match/%s/%s' % (env, name)] = ('match', env, sides, dict(kw, keep_history=True))
  return out


CASES = _cases()


def feed(h, x):
  """x into the hash: floats by their float64 bytes, integers and strings by their text, lists in order, dicts and objects
  by their sorted keys, every value behind a tag of its kind"""
  if x is None:
    h.update(b'N')
  elif isinstance(x, (bool, np.bool_)):
    h.update(b'b1' if x else b'b0')
  elif isinstance(x, (int, np.integer)):
    h.update(b'i%d;' % int(x))
  elif isinstance(x, (float, np.floating)):
    h.update(b'f' + np.float64(x).tobytes())
  elif isinstance(x, str):
    h.update(b's' + x.encode() + b';')
  elif isinstance(x, (list, tuple, range, np.ndarray)):
    h.update(b'[%d;' % len(x))
    for y in x:
      feed(h, y)
    h.update(b']')
  elif hasattr(x, 'tolist'):      # (a tensor)
    feed(h, x.tolist())
  elif isinstance(x, dict) or hasattr(x, '__dict__'):
    d = x if isinstance(x, dict) else vars(x)
    h.update(b'{')
    for k in sorted(d):
      feed(h, str(k))
      feed(h, d[k])
    h.update(b'}')
  else:
    raise TypeError('no digest for a %s' % type(x).__name__)


def _without_seconds(report):
  if isinstance(report, dict):
    return {k: _without_seconds(v) for k, v in report.items() if k != 'seconds'}
  return report


@functools.lru_cache(maxsize=None)
def _state(env, wseed=5):
  return eval_state(env, sims=8, wseed=wseed)


def _with(state, over):
  cfg = copy.copy(state['config'])
  for k, v in over.items():
    setattr(cfg, k, v)
  return dict(state, config=cfg)


def returned(name):
  """what the run of CASES[name] returns: the games, the summary and any grade reports without their seconds"""
  kind, env, over, kw = CASES[name]
  seeds = list(range(SEED0, SEED0 + GAMES))
  if kind == 'match':
    from model_based_rl_amd.match import play_match
    games, summary = play_match(_with(_state(env), over[0]), _with(_state(env, 6), over[1]), GAMES, seeds, batch=BATCH, **kw)
    return dict(games=games, summary=summary)
  from model_based_rl_amd.evaluate import Evaluator
  ev = Evaluator(_with(_state(env), dict(over, batch=BATCH)))
  ev.load_network()
  games = ev.play_games(GAMES, seeds, **kw)
  return dict(games=games, summary=ev.summary(games), grade=_without_seconds(ev.grade_report),
              grade_unroll=_without_seconds(ev.grade_unroll_report))


def digest(name):
  h = hashlib.sha256()
  feed(h, returned(name))
  return h.hexdigest()
