"""--selfplay_gumbel: self-play on the device games searched with the Gumbel MuZero search (DESIGN s7i; Engine.selfplay_set_gumbel;
csrc/mz_gumbel_selfplay.hip.h).  The records keep their layout -- the policy slots carry the root's improved policy pi', the action
is the Gumbel pick -- so the replay, the learner and --symmetry take them as they take visit shares.

The flags have names of their own (selfplay_gumbel*, not gumbel*): sides.Side.of reads config.gumbel* of a saved checkpoint's
config, and a training flag under those names would turn the checkpoint's evaluation into the Gumbel search at scale 1."""
from .envs import KIND_OF_ENV

DEFAULTS = dict(selfplay_gumbel_considered=16, selfplay_gumbel_c_visit=50.0, selfplay_gumbel_c_scale=1.0, selfplay_gumbel_scale=1.0)
VALUES = ('mean', 'vmix')


def selfplay_gumbel_params(config):
  """(max_considered, c_visit, c_scale, gumbel_scale) of a config, Engine.set_gumbel's order; the defaults where it has none"""
  return tuple(type(v)(v if getattr(config, k, None) is None else getattr(config, k)) for k, v in DEFAULTS.items())


def refuse_selfplay_gumbel(config, ranks=0):
  """what --selfplay_gumbel is not built for, one sentence each, before any device is touched"""
  if not getattr(config, 'selfplay_gumbel', False):
    return
  no = lambda why: SystemExit('--selfplay_gumbel: ' + why)
  if str(config.environment) not in KIND_OF_ENV:
    raise no('the Gumbel self-play runs on the device games (%s), %s has none.' % (', '.join(KIND_OF_ENV), config.environment))
  if getattr(config, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise no('only FCNetwork is searched by the engine\'s own kernels, %s has no Gumbel search.' % config.architecture)
  if bool(getattr(config, 'parity_rng', False)) or int(getattr(config, 'num_envs', 1)) == 1:
    raise no('host-environment actors (--num_envs 1 or --parity_rng) search with PUCT; use the device self-play loop.')
  if getattr(config, 'split_f16', False):
    raise no('--split_f16 is a fused search kernel, which this search does not run.')
  if int(ranks or 0) > 1:
    raise no('multi-rank runs (--ranks above 1) are not built for it.')
  if int(getattr(config, 'reanalyse_rows', 0) or 0) > 0 and not getattr(config, 'reanalyse_gumbel', False):
    raise no('--reanalyse_rows would mix visit-share and pi\' policy targets in one replay; Reanalyse does not write pi\' unless --reanalyse_gumbel is given.')
  m, c_visit, c_scale, scale = selfplay_gumbel_params(config)
  if m < 2:
    raise no('--selfplay_gumbel_considered must be at least 2, got %d.' % m)
  if not c_visit >= 0:
    raise no('--selfplay_gumbel_c_visit must not be negative, got %g.' % c_visit)
  if not c_scale > 0:
    raise no('--selfplay_gumbel_c_scale must be positive, got %g.' % c_scale)
  if not scale >= 0:
    raise no('--selfplay_gumbel_scale must not be negative, got %g.' % scale)
  if getattr(config, 'selfplay_gumbel_value', 'mean') not in VALUES:
    raise no('--selfplay_gumbel_value is mean or vmix, got %r.' % (config.selfplay_gumbel_value,))
