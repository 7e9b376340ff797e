"""The experience record of one self-play move, as Python reads and writes it.  include/mz_record.h is the statement of the
layout (obs | child_visits[A] | the tail: root_value f64, error f64, reward, then int32 action, flags, step, env_id,
episode); the numbers below repeat it and tests/test_record_cpu.py holds them to the header."""
import numpy as np

# float slots of the tail's fields from the tail's start (MZ_REC_*), and the tail's length
ROOT_VALUE, ERROR, REWARD, ACTION, FLAGS, STEP, ENV_ID, EPISODE, REC_EXTRA = 0, 2, 4, 5, 6, 7, 8, 9, 10
FLAG_DONE, FLAG_P2 = 1, 2      # the move ended the game; the mover was player -1 (History.to_play, game.py:100-101)


def obs_slots(O, packed=False):
  """float slots of an observation of O elements: O float32, or O bytes packed four per slot"""
  return (O + 3) // 4 if packed else O


def rec_floats(O, A, packed=False):
  return obs_slots(O, packed) + A + REC_EXTRA


def records_view(rec, O, A, obs_u8=False):
  """Named views into experience records (numpy float32 [..., rec_floats]):
  obs, child_visits, root_value / error (float64), reward, action / done / step / env_id / episode (int32).
  obs_u8: the observation is O bytes packed into ceil(O / 4) float slots (image frames, torch_search.TorchSelfplay)."""
  rec = np.asarray(rec)
  OS = obs_slots(O, obs_u8)
  assert rec.dtype == np.float32 and rec.shape[-1] == rec_floats(O, A, obs_u8), (rec.dtype, rec.shape)
  tail = rec[..., OS + A:]
  ints = tail.view(np.int32)
  f64 = lambda k: np.ascontiguousarray(tail[..., k:k + 2]).view(np.float64)[..., 0]
  flags = ints[..., FLAGS]
  obs = np.ascontiguousarray(rec[..., :OS]).view(np.uint8)[..., :O] if obs_u8 else rec[..., :O]
  return dict(obs=obs, child_visits=rec[..., OS:OS + A], root_value=f64(ROOT_VALUE), error=f64(ERROR), reward=tail[..., REWARD],
              action=ints[..., ACTION], done=flags & FLAG_DONE, to_play=1 - (flags & FLAG_P2), step=ints[..., STEP],
              env_id=ints[..., ENV_ID], episode=ints[..., EPISODE])


def records_fill(out, O, A, obs_u8=False, obs=None, child_visits=None, root_value=None, error=None, reward=None, action=None,
                 flags=None, step=None, env_id=None, episode=None):
  """The writer to records_view: the given fields into the records out [..., rec_floats], a numpy float32 array or a torch
  float32 tensor on any device; a field is an array / tensor of out's kind and place shaped like out without its last
  axis (obs [..., O], child_visits [..., A]), flags the whole word (FLAG_DONE | FLAG_P2).  Fields not given keep what out
  holds.  Neighbouring fields go out in one copy.  Returns out."""
  if isinstance(out, np.ndarray):
    xp, cast = np, lambda x, dt: np.ascontiguousarray(x, dt)
  else:
    import torch as xp
    cast = lambda x, dt: x.to(dt).contiguous()
  OS = obs_slots(O, obs_u8)
  assert out.dtype == xp.float32 and out.shape[-1] == rec_floats(O, A, obs_u8), (out.dtype, out.shape)
  # (first slot, float32 words [..., n]): a float64 is two words, an int32 one -- bit patterns, never value conversions
  words = lambda x, dt: cast(x, dt)[..., None].view(xp.float32)
  pieces = []
  if obs is not None:
    if obs_u8:
      out.view(xp.uint8)[..., :O] = cast(obs, xp.uint8)
    else:
      pieces.append((0, cast(obs, xp.float32)))
  if child_visits is not None:
    pieces.append((OS, cast(child_visits, xp.float32)))
  for slot, x, dt in ((ROOT_VALUE, root_value, xp.float64), (ERROR, error, xp.float64), (REWARD, reward, xp.float32),
                      (ACTION, action, xp.int32), (FLAGS, flags, xp.int32), (STEP, step, xp.int32), (ENV_ID, env_id, xp.int32),
                      (EPISODE, episode, xp.int32)):
    if x is not None:
      pieces.append((OS + A + slot, words(x, dt)))
  i = 0
  while i < len(pieces):
    j, end = i + 1, pieces[i][0] + pieces[i][1].shape[-1]
    while j < len(pieces) and pieces[j][0] == end:
      end += pieces[j][1].shape[-1]
      j += 1
    run = [p[1] for p in pieces[i:j]]
    out[..., pieces[i][0]:end] = run[0] if len(run) == 1 else xp.concatenate(run, -1)
    i = j
  return out
