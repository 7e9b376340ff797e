"""--selfplay_true_model: self-play on the device board games whose search runs on the true rules (DESIGN s7k;
Engine.selfplay_set_true_model; csrc/mz_truemodel.hip.h).  AlphaZero's search feeding MuZero's learner: a node below the root is
a real position, the policy and value targets come from that search, and everything else is PUCT self-play -- the records keep
their layout, the learner still unrolls and trains the dynamics network along the played actions, the checkpoint is a complete
MuZero network that every evaluation instrument reads under either search.

The flag has a name of its own (selfplay_true_model, not true_model): sides.Side.of reads config.true_model of a saved
checkpoint's config, and a training flag under that name would turn the checkpoint's evaluation into the true-rules search."""
from .envs import BOARD_KINDS


def refuse_selfplay_true_model(config, ranks=0):
  """what --selfplay_true_model is not built for, one sentence each, before any device is touched"""
  if not getattr(config, 'selfplay_true_model', False):
    if getattr(config, 'selfplay_true_model_loop', False):
      raise SystemExit('--selfplay_true_model_loop: an option of --selfplay_true_model, which is not given.')
    return
  no = lambda why: SystemExit('--selfplay_true_model: ' + why)
  if str(config.environment) not in BOARD_KINDS:
    raise no('the true rules are those of the device board games (%s), %s has none.' % (', '.join(BOARD_KINDS), config.environment))
  if getattr(config, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise no('only FCNetwork is searched by the engine\'s own kernels, %s has no true-rules search.' % config.architecture)
  if bool(getattr(config, 'parity_rng', False)) or int(getattr(config, 'num_envs', 1)) == 1:
    raise no('host-environment actors (--num_envs 1 or --parity_rng) search the learned model; use the device self-play loop.')
  if getattr(config, 'split_f16', False):
    raise no('--split_f16 is a fused search kernel, which this search does not run.')
  if int(ranks or 0) > 1:
    raise no('multi-rank runs (--ranks above 1) are not built for it.')
  if getattr(config, 'selfplay_gumbel', False):
    raise no('--selfplay_gumbel searches the learned model with the Gumbel search; a run takes one of the two.')
  if int(getattr(config, 'reanalyse_rows', 0) or 0) > 0:
    raise no('--reanalyse_rows would write learned-model targets into the same replay; a true-rules Reanalyse is not built.')
