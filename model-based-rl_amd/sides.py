"""What an evaluation side plays by, and what each option of the evaluator requires, each stated once (DESIGN s7b).

Side is the move rule of one side of a game: the mode (search, or the lookahead of --only_prior / --only_value), the
actions applied per move, temperature, exploration noise, and which search runs (PUCT, the true rules, Gumbel) with the
Gumbel parameters.  evaluate.py and match.py build one per engine and read everything about the rule from it.

OPTIONS is the table of refusals: per option when it counts as on and its requirements in order, each a predicate shared
between the options plus that option's own sentence.  refuse_unsupported ... refuse_gumbel and refuse_match check one row;
refuse() checks them all in one order, for a command line, a config, or a config read through a Side."""
import collections
import functools

from .engine import Engine
from .envs import BOARD_ENVS, DEVICE_ENVS

PLAYOUT_ENVS = GRADE_ENVS = TRUE_MODEL_ENVS = MATCH_ENVS = BOARD_ENVS

GUMBEL_DEFAULTS = dict(gumbel_considered=16, gumbel_c_visit=50.0, gumbel_c_scale=1.0, gumbel_scale=0.0)
GUMBEL_ARGS = ('max_considered', 'c_visit', 'c_scale', 'gumbel_scale')      # Engine.set_gumbel's names, in the order above


def gumbel_params(args_or_config):
  """(max_considered, c_visit, c_scale, gumbel_scale) of a command line or a config, the defaults where it has none"""
  g = lambda k: getattr(args_or_config, k, None)
  return tuple(type(v)(v if g(k) is None else g(k)) for k, v in GUMBEL_DEFAULTS.items())


def _all(x):
  return list(x) if isinstance(x, (list, tuple)) else [x]


def per_side(values, side, strict=False):
  """side `side`'s value of a scalar or a command-line list: one value means both sides, two mean one per side; strict
  refuses any other length"""
  values = _all(values)
  if strict and len(values) not in (1, 2):
    raise ValueError('--match takes per-side lists of length one (both sides) or two, got %r' % (values,))
  return values[side if len(values) == 2 else 0]


class _View(object):
  """a config read through some overriding attributes; nothing is copied"""

  def __init__(self, cfg, **over):
    self.__dict__.update(over, _cfg=cfg)

  def __getattr__(self, name):      # (only what `over` does not hold)
    if name == '_cfg':
      raise AttributeError(name)
    return getattr(self._cfg, name)


class Side(collections.namedtuple('Side', 'mode apply_mcts_actions temperature noise_on true_model gumbel num_simulations')):
  """The move rule of one side.  mode: 0 search, 1 only_prior, 2 only_value; true_model: the search runs on the true rules
  (Engine.tm_search); gumbel: Engine.set_gumbel's arguments where the search is the Gumbel search (Engine.gz_search), else
  None.  A side with both is refused by the table below."""
  __slots__ = ()

  @classmethod
  def of(cls, cfg, true_model=None, gumbel=None):
    """the side a config describes.  true_model / gumbel: None reads the config's; gumbel may be True (the config's
    gumbel_* parameters, their defaults where it has none) or a dict of Engine.set_gumbel's arguments"""
    only_prior, only_value = bool(getattr(cfg, 'only_prior', 0)), bool(getattr(cfg, 'only_value', 0))
    if only_prior and only_value:
      raise ValueError('only_prior and only_value exclude each other')
    if gumbel is None:
      gumbel = getattr(cfg, 'gumbel', 0)
    if gumbel:
      gumbel = dict(zip(GUMBEL_ARGS, gumbel_params(cfg)), **(gumbel if isinstance(gumbel, dict) else {}))
    return cls(1 if only_prior else 2 if only_value else 0, int(getattr(cfg, 'apply_mcts_actions', 1)),
               float(getattr(cfg, 'temperature', 0) or 0), bool(getattr(cfg, 'use_exploration_noise', 0)),
               bool(getattr(cfg, 'true_model', 0) if true_model is None else true_model), gumbel or None,
               int(cfg.num_simulations))

  @property
  def search(self):
    return 'gumbel' if self.gumbel else 'true_rules' if self.true_model else 'puct'

  @property
  def max_actions(self):
    """the actions a move applies at most (apply_mcts_actions <= 0: the reference's loop runs until an unexpanded node, at
    most num_simulations + 1 actions)"""
    return self.apply_mcts_actions if self.apply_mcts_actions > 0 else self.num_simulations + 1

  @property
  def plies_args(self):
    """(mode, temperature, noise_on): a side's arguments of Match.plies"""
    return self.mode, self.temperature, self.noise_on

  def depths(self, row):
    """a searched move's entry of search_depths: the lookaheads log none"""
    return [0] if self.mode == 1 else [1] if self.mode == 2 else [int(x) for x in row[:self.num_simulations]]

  def configure(self, engine, environment):
    """set the engine's search (after set_weights, before the games are reset)"""
    if self.true_model:
      engine.set_true_model(environment)
    if self.gumbel:
      engine.set_gumbel(True, **self.gumbel)

  def view(self, cfg):
    """cfg with this side's search in it, as the requirements read it"""
    over = dict(true_model=int(self.true_model), gumbel=int(bool(self.gumbel)))
    if self.gumbel:
      over.update(zip(GUMBEL_DEFAULTS, (self.gumbel[k] for k in GUMBEL_ARGS)))
    return _View(cfg, **over)

  def label_parts(self, temperature='temp:{}', lookahead_alone=True):
    """the pieces of a label that name the rule (evaluate.get_label; a match shows the rest beside a lookahead as well)"""
    parts = [('sims:{}'.format(self.num_simulations), 'only prior', 'only value')[self.mode]]
    if self.mode and lookahead_alone:
      return parts
    if self.apply_mcts_actions > 1:
      parts.append('mcts-actions:{}'.format(self.apply_mcts_actions))
    if self.temperature:
      parts.append(temperature.format(self.temperature))
    return parts + [text for on, text in ((self.noise_on, 'with noise'), (self.true_model, 'true rules'), (self.gumbel, 'gumbel')) if on]

  def search_line(self):
    """the printed line that names the search"""
    if not self.gumbel:
      return 'Search: PUCT'
    return 'Search: Gumbel, m = %d, c_visit = %g, c_scale = %g, gumbel_scale = %g' % tuple(self.gumbel[k] for k in GUMBEL_ARGS)


# ---- what each option requires
class _Asked(object):
  """what the requirements read: a command line or a config, whether it is a match (lists are per side) or not (lists are
  alternatives), and whether the device path may still be chosen later (Evaluator.__init__)"""

  def __init__(self, c, match=False, other=None, lenient=False):
    self.c, self.match, self.other, self.lenient = c, bool(match), other, lenient

  def get(self, name, default=None, of=None):
    return getattr(self.c if of is None else of, name, default)

  def values(self, name):
    if name == 'temperatures':      # (a config carries one temperature)
      t = self.get('temperatures')
      return [float(x or 0) for x in _all(self.get('temperature', 0) if t is None else t)]
    return [int(x or 0) for x in _all(self.get(name, 0))]

  env = property(lambda self: self.get('environment'))
  device_env = property(lambda self: bool(self.get('device_env', False)))
  actions = property(lambda self: [int(x) for x in _all(self.get('apply_mcts_actions', 1))])
  playouts = property(lambda self: int(self.get('opp_playouts', 0) or 0))
  unroll = property(lambda self: self.get('grade_unroll'))


# the shared predicates: True where the requirement is NOT met
_set = lambda name: lambda q: bool(q.get(name))
_host_path = lambda q: not (q.device_env or q.lenient or q.match)      # neither on the device path nor in a match
_in_match = lambda q: q.match
_env_outside = lambda envs: lambda q: q.env is not None and q.env not in envs
_many_actions = lambda q: any(m != 1 for m in q.actions)
_other_architecture = lambda q: q.get('architecture', 'FCNetwork') != 'FCNetwork'
_outside = lambda name, allowed: lambda q: any(x not in allowed for x in q.values(name))
_gumbel = lambda i, bad: lambda q: bad(gumbel_params(q.c)[i])
_differ = lambda name, kind=lambda x: x, default=None: lambda q: kind(q.get(name, default)) != kind(q.get(name, default, q.other))


def _beside(option, *names, first=False):
  """one of `names` set on a side that has `option` on: per side in a match; without one the lists are alternatives that
  all meet (first: only the option's first value is read then, as --true_model always has)"""
  def shared(q):
    on = q.values(option)
    for x in (q.values(n) for n in names):
      if q.match and any(per_side(on, k) and per_side(x, k) for k in (0, 1)):
        return True
      if not q.match and (on[0] if first else any(on)) and any(x):
        return True
    return False
  return shared


# the sentences' % arguments
_env_and = lambda envs, sep=' and ': lambda q: (q.env, sep.join(envs))
_architecture = lambda q: q.c.architecture
_gumbel_arg = lambda i: lambda q: gumbel_params(q.c)[i]
_support = lambda key: lambda q: (key, tuple(q.get(key, (-15, 15))), tuple(q.get(key, (-15, 15), q.other)))

REFUSED = (
    ('render', 'rendering is an interactive tool and is not part of this evaluator (no display on the GPU machines).'),
    ('save_gif_as', 'saving GIFs needs rendered frames, which this evaluator does not produce.'),
    ('save_mcts', 'MCTS PNG dumps (pydot) are an interactive tool and are not part of this evaluator.'),
    ('human_opp', 'human play is an interactive tool and is not part of this evaluator; use --random_opp.'),
    ('plot_summary', 'plots are an interactive tool and are not part of this evaluator; use --out for a JSON summary.'),
)

Option = collections.namedtuple('Option', 'on requires')      # requires: (predicate, sentence[, the sentence's % arguments])
_always = lambda q: True

# In the order refuse() checks them (a match checks `match` and `unsupported` after `gumbel`, every other run `unsupported`
# and `device_env`).  A new option is one more row here.
OPTIONS = collections.OrderedDict((
    ('opp_playouts', Option(lambda q: q.playouts != 0, (      # the playout-search opponent of the device games
        (_in_match, '--opp_playouts: --match plays two networks against each other and seats no playout opponent.'),
        (lambda q: q.playouts < 64 or q.playouts > 65536 or q.playouts % 64,
         '--opp_playouts: the budget is a multiple of 64 in 64 to 65536 playouts per move, got %d.', lambda q: q.playouts),
        (_host_path, '--opp_playouts: the playout opponent is planned on the device and needs --device_env.'),
        (lambda q: q.get('random_opp') is None, '--opp_playouts: --random_opp names the seat the playout opponent takes and is missing.'),
        (_env_outside(PLAYOUT_ENVS), '--opp_playouts: %s has no playout opponent; it plays %s.', _env_and(PLAYOUT_ENVS)),
        (_many_actions, '--opp_playouts: the playout opponent answers every move and takes --apply_mcts_actions 1 only.'),
    ))),
    ('grade', Option(lambda q: bool(q.get('grade') or q.get('grade_table')), (      # moves graded against the exact solver (solver.py)
        (lambda q: not q.get('grade'), '--grade_table: it chooses the search that --grade solves with and grades nothing without --grade.'),
        (_in_match, '--grade: the games of --match are not graded; grade each network with evaluate --device_env --grade.'),
        (_host_path, '--grade: the graded games are the device environments\' and need --device_env.'),
        (_env_outside(GRADE_ENVS), '--grade: %s has no exact solver; it solves %s.', _env_and(GRADE_ENVS)),
        (_many_actions, '--grade: a graded decision is one searched move and takes --apply_mcts_actions 1 only.'),
    ))),
    # the model by unroll depth (solver.grade_unroll).  --no_support checkpoints are served: the unroll goes through
    # mz_initial_inference and mz_recurrent_inference, which read the heads' single outputs
    ('grade_unroll', Option(lambda q: q.unroll is not None and q.unroll is not False, (
        (lambda q: not q.get('grade'), '--grade_unroll: it unrolls the model along the games --grade keeps and does nothing without --grade.'),
        (lambda q: int(q.unroll) < 1 or int(q.unroll) > Engine.UNROLL_MAX_K,
         '--grade_unroll: the depth is 1 to %d dynamics steps, got %d.', lambda q: (Engine.UNROLL_MAX_K, int(q.unroll))),
    ))),
    ('true_model', Option(lambda q: any(q.values('true_model')), (      # the search on the true rules (Engine.tm_search)
        (_outside('true_model', (0, 1)), '--true_model: the values are 0 (the learned model) and 1 (the true rules), got %r.',
         lambda q: (q.values('true_model'),)),
        (_host_path, '--true_model: the true-rules search reads the device games\' positions and needs --device_env (or --match).'),
        (_env_outside(TRUE_MODEL_ENVS), '--true_model: %s has no true-rules search; it searches %s.', _env_and(TRUE_MODEL_ENVS)),
        (_many_actions, '--true_model: a move of the true-rules search applies one action and takes --apply_mcts_actions 1 only.'),
        (_beside('true_model', 'only_prior', 'only_value', first=True),
         '--true_model: --only_prior / --only_value run no search; a side takes one of them or the true-rules search.'),
        (_other_architecture, '--true_model: the architecture %s has no engine path; FCNetwork checkpoints only.', _architecture),
    ))),
    ('gumbel', Option(lambda q: any(q.values('gumbel')), (      # the Gumbel MuZero search (Engine.gz_search)
        (_outside('gumbel', (0, 1)), '--gumbel: the values are 0 (PUCT) and 1 (the Gumbel search), got %r.', lambda q: (q.values('gumbel'),)),
        (_host_path, '--gumbel: the Gumbel search is served by the device games\' move loop and needs --device_env (or --match).'),
        (_many_actions, '--gumbel: a move of the Gumbel search applies one action and takes --apply_mcts_actions 1 only.'),
        (_beside('gumbel', 'use_exploration_noise'), '--gumbel: the Gumbel draw replaces the exploration noise at the root; a side takes --use_exploration_noise or the Gumbel search (--gumbel_scale is its stochastic setting).'),
        (_beside('gumbel', 'temperatures'), '--gumbel: the move is chosen by the rule of the search, not sampled from the visits; a side takes temperature 0 (--gumbel_scale is the stochastic setting).'),
        (_beside('gumbel', 'only_prior', 'only_value'), '--gumbel: --only_prior / --only_value run no search; a side takes one of them or the Gumbel search.'),
        (_beside('gumbel', 'true_model'), '--gumbel: an engine searches the true rules or with the Gumbel search; a side takes --true_model or --gumbel.'),
        (_other_architecture, '--gumbel: the architecture %s has no engine path; FCNetwork checkpoints only.', _architecture),
        (_gumbel(0, lambda m: m < 2), '--gumbel: --gumbel_considered must be at least 2, got %d.', _gumbel_arg(0)),
        (_gumbel(1, lambda cv: not cv >= 0), '--gumbel: --gumbel_c_visit must not be negative, got %g.', _gumbel_arg(1)),
        (_gumbel(2, lambda cs: not cs > 0), '--gumbel: --gumbel_c_scale must be positive, got %g.', _gumbel_arg(2)),
        (_gumbel(3, lambda sc: not sc >= 0), '--gumbel: --gumbel_scale must not be negative, got %g.', _gumbel_arg(3)),
    ))),
    ('match', Option(_always, (      # a checkpoint, or the command line, of a match (match.py)
        (_env_outside(MATCH_ENVS), '--match: the environment %s is not a two-player device game; matches are played on %s.', _env_and(MATCH_ENVS)),
        (_many_actions, '--match: --apply_mcts_actions must be 1; a ply of a match applies exactly one action.'),
        (_set('norm_obs'), '--match: --norm_obs is not applied by the device games.'),
        (_set('random_opp'), '--match: --random_opp has no place in a match; both sides are networks (give --nets two names).'),
        (_set('human_opp'), '--match: --human_opp is an interactive tool; both sides of a match are networks.'),
        (_other_architecture, '--match: the architecture %s has no device match path; FCNetwork checkpoints only.', _architecture),
    ))),
    ('match_pair', Option(lambda q: q.other is not None, (      # what the two checkpoints of a match share
        (_differ('environment'), '--match: the two checkpoints play a different environment (%s and %s).',
         lambda q: (q.get('environment'), q.get('environment', None, q.other))),
        (_differ('no_support', bool, False), '--match: the two checkpoints differ in no_support; their value heads are not comparable.'),
        (_differ('value_support', tuple, (-15, 15)), '--match: the two checkpoints have different supports (%s %s and %s).', _support('value_support')),
        (_differ('reward_support', tuple, (-15, 15)), '--match: the two checkpoints have different supports (%s %s and %s).', _support('reward_support')),
    ))),
    ('unsupported', Option(_always, tuple((_set(name), '--%s: %s' % (name, why)) for name, why in REFUSED))),      # the interactive tools
    ('device_env', Option(lambda q: q.device_env, (      # the games on the device environments
        (_env_outside(DEVICE_ENVS), '--device_env: %s has no device form; the device environments are %s.', _env_and(DEVICE_ENVS, ', ')),
        (_set('norm_obs'), '--device_env: --norm_obs is not applied by the device environments; use the host path.'),
        (lambda q: q.env == 'ConnectFour' and _many_actions(q),
         '--device_env: ConnectFour takes --apply_mcts_actions 1 only; below the root the walk offers full '
         'columns, which the host class refuses and a device game cannot.'),
    ))),
))


def check(name, c, match=False, other=None, lenient=False):
  """row `name` of OPTIONS on a command line or a config: NotImplementedError with the sentence of the first requirement
  that is not met, nothing while the option is off"""
  q = _Asked(c, match, other, lenient)
  option = OPTIONS[name]
  if option.on(q):
    for unmet, sentence, *args in option.requires:
      if unmet(q):
        raise NotImplementedError(sentence % args[0](q) if args else sentence)


# the per-option entry points, refuse_x(args_or_config[, match=False]): one row each, one sentence per configuration the option
# leaves out.  What --grade refuses stays refused by --grade's own sentence, not --grade_unroll's (its row comes first)
refuse_unsupported, refuse_device_env, refuse_opp_playouts, refuse_grade, refuse_grade_unroll, refuse_true_model, refuse_gumbel = (
    functools.partial(check, name) for name in ('unsupported', 'device_env', 'opp_playouts', 'grade', 'grade_unroll', 'true_model', 'gumbel'))


def refuse_match(args_or_config, other=None):
  """one sentence per configuration --match leaves out (starting '--match: '); other: the second checkpoint's config, held
  to the same rules, and what the two must share.  Host arithmetic only: no device is touched."""
  check('match', args_or_config)
  if other is not None:
    check('match', other)
    check('match_pair', args_or_config, other=other)


def refuse(args_or_config, match=False, device_env=None, side=None, other=None, lenient=False):
  """every row in one order: opp_playouts, grade, grade_unroll, true_model, gumbel, then match and unsupported in a match,
  unsupported and device_env otherwise.  device_env: whether the device path is taken (None: the config's flag); side: the
  Side whose search is checked instead of the config's; lenient: the device path may still be chosen (its own row keeps
  reading the flag)"""
  c = args_or_config if side is None else side.view(args_or_config)
  if device_env is not None:
    c = _View(c, device_env=bool(device_env))
  for name in ('opp_playouts', 'grade', 'grade_unroll', 'true_model', 'gumbel'):
    check(name, c, match, lenient=lenient)
  if match:
    refuse_match(c, other)
    check('unsupported', c)
  else:
    check('unsupported', c)
    check('device_env', c)
