"""MuZero Reanalyse: the policy targets (child_visits) and bootstrap values (root_value) the replay stores are those of the
weights that played the move; a Reanalyser searches stored positions again under the latest weights and writes the fresh
statistics back in place.  The replay builds its n-step targets at sampling time from exactly these two fields
(mzr_sample_batch), so the learner, its kernels and the sampling code see nothing but fresher targets.

  replay.reanalyse_pick   whole history slices out, all their rows (include/mz_replay.h)        -> pinned rows
  Engine.reanalyse        per chunk of B rows: observe, initial inference, root without noise,
                          search, store (csrc/mz_reanalyse.hip.h; no host work between chunks)    -> pinned fresh
                          (--reanalyse_gumbel: Engine.reanalyse_gumbel, the Gumbel search, pi' and
                          the value kind of --selfplay_gumbel's records; DESIGN s7j)
                          (--reanalyse_true_model: Engine.reanalyse_true_model, PUCT on the true rules
                          of TicTacToe / ConnectFour below the stored position; DESIGN s7n)
  replay.reanalyse_write  child_visits and root_value of exactly those rows                       <- pinned fresh

Not part of this: exploration noise at the reanalysed root; refreshing the stored error or the priorities (the learner's own
refresh does that); propagating a refreshed row to the copy of the same step in an overlapping slice; byte observations and
--norm_obs; multi-rank runs; reanalysing on the actor's own engine (the Reanalyser owns one, as the Evaluator does).
"""
import time

import numpy as np
import torch

from .actors import _call
from .engine import Engine
from .record import rec_floats
from .envs import BOARD_KINDS, KIND_OF_ENV
from .selfplay_search import selfplay_gumbel_params

KINDS = KIND_OF_ENV      # (envs.DEVICE_GAMES; anything else: 0, all actions legal)


def env_kind(config):
  return KINDS.get(str(getattr(config, 'environment', '')), 0)


def refuse_reanalyse_gumbel(config):
  """what --reanalyse_gumbel is not built for, one sentence each, before any device is touched (--reanalyse_rows' own refusals
  apply beside these: refuse_reanalyse)"""
  if not getattr(config, 'reanalyse_gumbel', False):
    return
  no = lambda why: SystemExit('--reanalyse_gumbel: ' + why)
  if int(getattr(config, 'reanalyse_rows', 0) or 0) <= 0:
    raise no('it chooses the search of the Reanalyse passes and does nothing without --reanalyse_rows above 0.')
  if not getattr(config, 'selfplay_gumbel', False):
    raise no('without --selfplay_gumbel it would mix the visit shares of PUCT self-play and pi\' policy targets in one replay.')
  scale = float(getattr(config, 'reanalyse_gumbel_scale', 0.0))
  if not scale >= 0:
    raise no('--reanalyse_gumbel_scale must not be negative, got %g.' % scale)


def refuse_reanalyse_true_model(config):
  """what --reanalyse_true_model is not built for, one sentence each, before any device is touched (--reanalyse_rows' own refusals
  apply beside these: refuse_reanalyse).  Without --selfplay_true_model it is allowed: PUCT self-play on the learned model whose
  targets are refreshed on the true rules -- visit shares and mean values on both sides, one kind of target in the replay"""
  if not getattr(config, 'reanalyse_true_model', False):
    return
  no = lambda why: SystemExit('--reanalyse_true_model: ' + why)
  if int(getattr(config, 'reanalyse_rows', 0) or 0) <= 0:
    raise no('it chooses the search of the Reanalyse passes and does nothing without --reanalyse_rows above 0.')
  if str(getattr(config, 'environment', '')) not in BOARD_KINDS:
    raise no('the true rules are those of the device board games (%s), %s has none.' % (', '.join(BOARD_KINDS), config.environment))
  if int(getattr(config, 'stack_obs', 1) or 1) > 1:
    raise no('--stack_obs above 1 stores several frames per row, and a position is read from one board.')
  if getattr(config, 'selfplay_gumbel', False) or getattr(config, 'reanalyse_gumbel', False):
    raise no('--selfplay_gumbel and --reanalyse_gumbel put pi\' into the replay and this writes visit shares; a replay holds one of the two.')


def refuse_reanalyse(config, ranks=0):
  """what --reanalyse_rows is not built for, one sentence each, before any device is touched"""
  if int(getattr(config, 'reanalyse_rows', 0) or 0) <= 0:
    return
  no = lambda why: SystemExit('--reanalyse_rows: ' + why)
  if int(ranks or 0) > 1:
    raise no('multi-rank runs (--ranks above 1) are not reanalysed; the one replay lives on rank 0 and the other ranks have none.')
  if getattr(config, 'architecture', 'FCNetwork') != 'FCNetwork':
    raise no('only FCNetwork is searched by the engine\'s own kernels, %s is not reanalysed.' % config.architecture)
  if getattr(config, 'obs_u8', False):
    raise no('byte observations (image frames, -ram- environments) are not reanalysed.')
  if getattr(config, 'norm_obs', False):
    raise no('--norm_obs is not reanalysed (the stored observations are raw).')
  if getattr(config, 'episode_life', False):
    raise no('--episode_life histories do not come from device records and are not reanalysed.')
  host_env = str(config.environment) in KINDS
  if host_env and (bool(getattr(config, 'parity_rng', False)) or int(getattr(config, 'num_envs', 1)) == 1):
    raise no('host-environment actors (--num_envs 1 or --parity_rng) are not reanalysed; use the device self-play loop.')


class Reanalyser(object):
  """Reanalyser(config, replay, device=None, batch=None): an Engine of its own (B = batch or min(num_envs, 4096), the actor's
  search settings) and two pinned buffers; set_weights(flat or state_dict), then run(max_rows) per pass.  With
  config.reanalyse_gumbel the engine searches with the Gumbel search and run(max_rows, draw_key) writes pi' (DESIGN s7j); with
  config.reanalyse_true_model it searches the true rules of the board game, all simulations of a chunk in one launch, and
  run(max_rows) writes what it always does (DESIGN s7n)."""

  def __init__(self, config, replay, device=None, batch=None, max_rows=None):
    self.config, self.replay = config, replay
    self.B = int(batch or min(int(getattr(config, 'num_envs', 1)), 4096))
    self.O, self.A = int(np.prod(config.obs_space)), int(config.action_space)
    self.kind = env_kind(config)
    self.engine = Engine.from_config(config, self.B, device=device)
    self.device = self.engine.device
    # --reanalyse_gumbel (DESIGN s7j): the search and the value kind of the --selfplay_gumbel run that filled the replay -- one
    # replay holds one kind of policy target and one kind of value --, with a noise scale of its own
    self.gumbel = bool(getattr(config, 'reanalyse_gumbel', False))
    self.gumbel_value = getattr(config, 'selfplay_gumbel_value', 'mean') if self.gumbel else None
    if self.gumbel:
      self.engine.set_gumbel(True, *selfplay_gumbel_params(config)[:3], float(getattr(config, 'reanalyse_gumbel_scale', 0.0) or 0.0))
    # --reanalyse_true_model (DESIGN s7n): the stored positions are searched on the game's own rules; no draw, no key
    self.true_model = bool(getattr(config, 'reanalyse_true_model', False))
    if self.true_model:
      self.engine.set_true_model(self.kind)
    self.rows = self.fresh = None
    self.max_rows = 0
    self._size(int(max_rows or getattr(config, 'reanalyse_rows', 0) or 0))

  def _size(self, max_rows):
    if max_rows > self.max_rows:
      self.rows = torch.empty(max_rows, rec_floats(self.O, self.A), dtype=torch.float32).pin_memory()
      self.fresh = torch.empty(max_rows, self.A + 2, dtype=torch.float32).pin_memory()
      self.max_rows = max_rows

  def set_weights(self, weights):
    self.engine.set_weights(weights)

  def run(self, max_rows=None, draw_key=0):
    """one pass: pick -> Engine.reanalyse (Engine.reanalyse_gumbel under --reanalyse_gumbel, draw_key in the key of its draws;
    Engine.reanalyse_true_model under --reanalyse_true_model) -> write.  -> dict(rows, slices, skipped_slices, seconds, mean_abs_value_change,
    mean_policy_l1, busy): rows written, and the means over them of |new - old root_value| and of the L1 distance between the old
    and the new child_visits.  busy: another pass over the same replay holds its one ticket (several actors share a replay and
    pull weights at the same steps): this pass is skipped, nothing is searched or written"""
    n_max = int(max_rows or self.max_rows)
    self._size(n_max)
    t0 = time.perf_counter()
    pick = _call(self.replay, 'reanalyse_pick', n_max, self.rows, True)
    out = {'busy': bool(pick['busy']), 'rows': 0, 'slices': int(len(pick['slice_rows'])), 'skipped_slices': int(pick['skipped_slices']), 'seconds': 0.0,
           'mean_abs_value_change': 0.0, 'mean_policy_l1': 0.0}
    if pick['ticket']:
      n = int(pick['n_rows'])
      try:
        if self.gumbel:
          self.engine.reanalyse_gumbel(self.rows, self.fresh, n, self.kind, value=self.gumbel_value, draw_key=draw_key)
        elif self.true_model:
          self.engine.reanalyse_true_model(self.rows, self.fresh, n, self.kind, fused=True)
        else:
          self.engine.reanalyse(self.rows, self.fresh, n, self.kind)
      except BaseException:
        _call(self.replay, 'reanalyse_release', pick['ticket'])
        raise
      st = _call(self.replay, 'reanalyse_write', pick['ticket'], self.fresh[:n])
      out['rows'] = int(st['rows'])
      if st['rows']:
        out['mean_abs_value_change'] = st['abs_value_change'] / st['rows']
        out['mean_policy_l1'] = st['policy_l1'] / st['rows']
    out['seconds'] = time.perf_counter() - t0
    return out

  def close(self):
    self.engine.close()
