"""How the device self-play loop searches a move, and what each choice requires, each stated once (DESIGN s7l): PUCT (the default);
--selfplay_gumbel, the Gumbel MuZero search (s7i): the policy slots of a record carry the root's improved policy pi', the action is the
Gumbel pick, the layout stays; --selfplay_true_model, PUCT on the game's true rules (s7k), AlphaZero's search feeding MuZero's learner.
The flags have names of their own (not gumbel*, true_model): sides.Side.of reads those of a saved checkpoint's config, and a training
flag under them would turn the checkpoint's evaluation into that search.
MODES is the table of refusals, as sides.OPTIONS is the evaluator's: per mode its flag, its options, the words its sentences differ
by and its requirements in order -- the shared ones, each a predicate with the mode's phrase, then the mode's own."""
import collections
import functools

from .envs import BOARD_KINDS, KIND_OF_ENV

DEFAULTS = dict(selfplay_gumbel_considered=16, selfplay_gumbel_c_visit=50.0, selfplay_gumbel_c_scale=1.0, selfplay_gumbel_scale=1.0)
VALUES = ('mean', 'vmix')


def selfplay_gumbel_params(config):
  """(max_considered, c_visit, c_scale, gumbel_scale) of a config, Engine.set_gumbel's order; the defaults where it has none"""
  return tuple(type(v)(v if getattr(config, k, None) is None else getattr(config, k)) for k, v in DEFAULTS.items())


# the requirements: (predicate(config, ranks, mode), sentence[, its % arguments]); True where one is NOT met.  %(..)s: the mode's words
_get = lambda c, name, default=False: getattr(c, name, default)
_reanalyse = lambda c: int(_get(c, 'reanalyse_rows', 0) or 0) > 0
_param = lambda i, bad=None: lambda c, *_: bad(selfplay_gumbel_params(c)[i]) if bad else selfplay_gumbel_params(c)[i]
_TWO = '--selfplay_gumbel searches the learned model with the Gumbel search; a run takes one of the two.'
_SHARED = (
    (lambda c, ranks, m: str(c.environment) not in m.envs, '%(runs)s (%(envs)s), %(env)s has none.'),
    (lambda c, ranks, m: _get(c, 'architecture', 'FCNetwork') != 'FCNetwork', 'only FCNetwork is searched by the engine\'s own kernels, %(architecture)s has no %(search)s.'),
    (lambda c, ranks, m: bool(_get(c, 'parity_rng')) or int(_get(c, 'num_envs', 1)) == 1, 'host-environment actors (--num_envs 1 or --parity_rng) search %(host)s; use the device self-play loop.'),
    (lambda c, ranks, m: _get(c, 'split_f16'), '--split_f16 is a fused search kernel, which this search does not run.'),
    (lambda c, ranks, m: int(ranks or 0) > 1, 'multi-rank runs (--ranks above 1) are not built for it.'),
)
_GUMBEL = (
    (lambda c, ranks, m: _reanalyse(c) and not _get(c, 'reanalyse_gumbel'),
     '--reanalyse_rows would mix visit-share and pi\' policy targets in one replay; Reanalyse does not write pi\' unless --reanalyse_gumbel is given.'),
    (_param(0, lambda x: x < 2), '--selfplay_gumbel_considered must be at least 2, got %d.', _param(0)),
    (_param(1, lambda x: not x >= 0), '--selfplay_gumbel_c_visit must not be negative, got %g.', _param(1)),
    (_param(2, lambda x: not x > 0), '--selfplay_gumbel_c_scale must be positive, got %g.', _param(2)),
    (_param(3, lambda x: not x >= 0), '--selfplay_gumbel_scale must not be negative, got %g.', _param(3)),
    (lambda c, ranks, m: _get(c, 'selfplay_gumbel_value', 'mean') not in VALUES, '--selfplay_gumbel_value is mean or vmix, got %r.', lambda c: (c.selfplay_gumbel_value,)),
)
_TRUE_RULES = (
    (lambda c, ranks, m: _get(c, 'selfplay_gumbel'), _TWO),
    # (--reanalyse_true_model is the way through: reanalyse.refuse_reanalyse_true_model, DESIGN s7n)
    (lambda c, ranks, m: _reanalyse(c) and not _get(c, 'reanalyse_true_model'), '--reanalyse_rows would write learned-model targets into the same replay; a true-rules Reanalyse is not built.'),
)
Mode = collections.namedtuple('Mode', 'flag options envs words requires')
# In the order train's preflight asks.  A new mode is one more row here (and one in csrc/mz_selfplay_mode.inc).
MODES = dict(
    puct=Mode(None, (), None, None, ()),
    gumbel=Mode('selfplay_gumbel', (), tuple(KIND_OF_ENV),
                dict(runs='the Gumbel self-play runs on the device games', search='Gumbel search', host='with PUCT'), _SHARED + _GUMBEL),
    true_rules=Mode('selfplay_true_model', ('selfplay_true_model_loop',), tuple(BOARD_KINDS),
                    dict(runs='the true rules are those of the device board games', search='true-rules search', host='the learned model'),
                    _SHARED + _TRUE_RULES))


def mode_of(config):
  """'puct', 'gumbel' or 'true_rules': the mode a config's flags select; two flags at once are refused"""
  on = [name for name, m in MODES.items() if m.flag and getattr(config, m.flag, False)]
  if len(on) > 1:
    raise SystemExit('--selfplay_true_model: ' + _TWO)
  return on[0] if on else 'puct'


def check(name, config, ranks=0):
  """row `name` of MODES on a config, before any device is touched: SystemExit with the sentence of the first requirement that is
  not met; while the mode's flag is off, with that of an option of it that is given"""
  m = MODES[name]
  on = m.flag and getattr(config, m.flag, False)
  for option in () if on else m.options:
    if getattr(config, option, False):
      raise SystemExit('--%s: an option of --%s, which is not given.' % (option, m.flag))
  for unmet, sentence, *args in m.requires if on else ():
    if unmet(config, ranks, m):
      words = dict(m.words, envs=', '.join(m.envs), env=config.environment, architecture=getattr(config, 'architecture', None))
      raise SystemExit('--%s: %s' % (m.flag, sentence % (args[0](config) if args else words)))


refuse_selfplay_gumbel, refuse_selfplay_true_model = (functools.partial(check, name) for name in ('gumbel', 'true_rules'))      # refuse_x(config, ranks=0): one row each


def refuse_selfplay_search(config, ranks=0):
  """train's preflight: every mode's row, in the table's order"""
  for name in MODES:
    check(name, config, ranks)


def configure(engine, config):
  """set the engine's self-play search (after selfplay_set_env, before selfplay_reset)"""
  mode = mode_of(config)
  if mode == 'gumbel':      # the records carry pi'
    engine.set_gumbel(True, *selfplay_gumbel_params(config))
    engine.selfplay_set_gumbel(True, getattr(config, 'selfplay_gumbel_value', 'mean'))
  elif mode == 'true_rules':
    engine.set_true_model(KIND_OF_ENV[config.environment])
    engine.selfplay_set_true_model(True, fused=not getattr(config, 'selfplay_true_model_loop', False))
