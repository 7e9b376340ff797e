"""--reanalyse_true_model without a GPU (DESIGN s7n):
  decode     tests/reanalyse_tm_host.cpp under AddressSanitizer + UBSan: mz_reanalyse_position (csrc/mz_reanalyse.hip.h) on stored
             observations of random games of envs.TicTacToe / envs.ConnectFour and of the positions of tests/c4_positions.py seen by
             both movers gives the environment's board and ply count, in buffers of exactly the game's size; mz_game_legal of the
             decoded board is mz_reanalyse_legal_mask of the observation
  preflight  every sentence of refuse_reanalyse_true_model; --selfplay_true_model --reanalyse_rows without the flag keeps its old
             sentence, with it the three preflight functions pass, as does the flag beside PUCT self-play; flag off: nothing asked
  symbols    mz_reanalyse_true_model in the header and in _abi.py, Engine.reanalyse_true_model, the scripts' flag"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '30']
TRUE = PLAIN + ['--selfplay_true_model']
OLD = '--selfplay_true_model: --reanalyse_rows would write learned-model targets into the same replay; a true-rules Reanalyse is not built.'


def _config(argv):
  from model_based_rl_amd.config import make_config
  return make_config(argv)


# -------------------------------------------------------------------------------------------------------------- decode
def position_cases():
  """(kind, mover, ply count, the environment's board, the stored observation mover * board)"""
  from model_based_rl_amd import envs
  from tests.c4_positions import POSITIONS
  cases = []
  for _, turn, _, board in POSITIONS:      # six full columns; a position is a position for either mover
    for t in (turn, -turn):
      e = envs.ConnectFour()
      e.set_position(board, t)
      cases.append((3, t, e._elapsed_steps, e.board.copy(), (t * e.board).astype(np.float32)))
  rng = np.random.RandomState(2)
  for kind, make, games in ((3, envs.ConnectFour, 2), (1, envs.TicTacToe, 3)):
    for _ in range(games):                 # random games from the start to the end: every ply count, both movers
      e = make()
      e.reset()
      done = False
      while not done:
        cases.append((kind, e.turn, e._elapsed_steps, np.asarray(e.board).reshape(-1).copy(),
                      (e.turn * np.asarray(e.board).reshape(-1)).astype(np.float32)))
        _, _, done, _ = e.step(int(rng.choice(e.legal_actions())))
  return cases


def test_position_decode_under_sanitizers(tmp_path):
  exe, data = str(tmp_path / 'reanalyse_tm_host'), str(tmp_path / 'positions.txt')
  cases = position_cases()
  for kind, least in ((3, 20), (1, 5)):
    movers = {m for k, m, _, _, _ in cases if k == kind}
    assert sum(k == kind for k, _, _, _, _ in cases) >= least and movers == {1, -1}
  assert any(s == 0 for _, _, s, _, _ in cases) and any(k == 1 and s >= 7 for k, _, s, _, _ in cases) and any(k == 3 and s >= 30 for k, _, s, _, _ in cases)
  assert all(s == np.count_nonzero(b) for _, _, s, b, _ in cases)      # (the environments' ply count is the stones on the board)
  with open(data, 'w') as f:
    for kind, mover, step, board, obs in cases:
      f.write('%d %d %d %s %s\n' % (kind, mover, step, ' '.join('%d' % v for v in board), ' '.join('%d' % v for v in obs)))
  csrc = os.path.join(ROOT, 'model-based-rl_amd', 'csrc')
  cmd = ['hipcc', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-mavx2', '-pthread', '-ffp-contract=off', '-fno-omit-frame-pointer',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'include'), '-I', csrc,
         '-x', 'hip', os.path.join(ROOT, 'tests', 'reanalyse_tm_host.cpp'), '-o', exe]
  r = subprocess.run(cmd, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-3000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  run = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=300)
  assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
  assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
  assert run.stdout.strip().splitlines()[-1] == 'ok %d positions' % len(cases), run.stdout[-2000:]


# ----------------------------------------------------------------------------------------------------------- preflight
def test_the_flag_and_its_default():
  assert _config(PLAIN).reanalyse_true_model is False
  cfg = _config(PLAIN + ['--reanalyse_rows', '512', '--reanalyse_true_model'])
  assert cfg.reanalyse_true_model is True and cfg.reanalyse_rows == 512 and cfg.selfplay_true_model is False


def test_every_sentence_of_the_preflight():
  from model_based_rl_amd.reanalyse import refuse_reanalyse_true_model
  on = ['--reanalyse_rows', '512', '--reanalyse_true_model']
  cases = [(PLAIN + ['--reanalyse_true_model'], 'reanalyse_rows'),
           (TRUE + ['--reanalyse_true_model', '--reanalyse_rows', '0'], 'reanalyse_rows'),
           (['--environment', 'CartPole-v1', '--num_envs', '64'] + on, 'CartPole-v1'),
           (['--environment', 'LunarLander-v2', '--num_envs', '64'] + on, 'TicTacToe, ConnectFour'),
           (PLAIN + on + ['--stack_obs', '2'], 'stack_obs'),
           (PLAIN + on + ['--selfplay_gumbel'], 'selfplay_gumbel'),
           (PLAIN + on + ['--selfplay_gumbel', '--reanalyse_gumbel'], 'reanalyse_gumbel'),
           (PLAIN + on + ['--reanalyse_gumbel'], 'reanalyse_gumbel')]
  seen = set()
  for argv, word in cases:
    with pytest.raises(SystemExit) as exc:
      refuse_reanalyse_true_model(_config(argv))
    msg = str(exc.value)
    assert msg.startswith('--reanalyse_true_model: ') and word in msg and msg.count('. ') == 0 and msg.endswith('.'), msg
    seen.add(msg.split(',')[0][:60])
  assert len(seen) == 4      # (four requirements, four different sentences)


def test_the_old_sentence_stays_and_the_flag_is_the_way_through():
  from model_based_rl_amd.reanalyse import refuse_reanalyse, refuse_reanalyse_gumbel, refuse_reanalyse_true_model
  from model_based_rl_amd.selfplay_search import refuse_selfplay_search, refuse_selfplay_true_model
  for base in (TRUE, ['--environment', 'ConnectFour'] + TRUE[2:]):
    cfg = _config(base + ['--reanalyse_rows', '512'])
    for refuse in (refuse_selfplay_search, refuse_selfplay_true_model):
      with pytest.raises(SystemExit) as exc:
        refuse(cfg)
      assert str(exc.value) == OLD
    refuse_reanalyse_true_model(cfg)      # (the flag is off: nothing is asked here)
    both = _config(base + ['--reanalyse_rows', '512', '--reanalyse_true_model'])
    for refuse in (refuse_selfplay_search, refuse_reanalyse, refuse_reanalyse_gumbel, refuse_reanalyse_true_model):
      refuse(both)
    # the second arm: PUCT self-play on the learned model, its targets refreshed on the true rules
    alone = _config(base[:-1] + ['--reanalyse_rows', '512', '--reanalyse_true_model'])
    assert alone.selfplay_true_model is False
    for refuse in (refuse_selfplay_search, refuse_reanalyse, refuse_reanalyse_gumbel, refuse_reanalyse_true_model):
      refuse(alone)
  # --reanalyse_rows' own refusals apply beside the flag's
  with pytest.raises(SystemExit) as exc:
    refuse_reanalyse(_config(TRUE + ['--reanalyse_rows', '512', '--reanalyse_true_model']), ranks=2)
  assert str(exc.value).startswith('--reanalyse_rows: ')
  # the flag off: nothing is asked, whatever else is given
  for argv in (PLAIN, ['--environment', 'CartPole-v1', '--num_envs', '64', '--reanalyse_rows', '512'], PLAIN + ['--stack_obs', '2'],
               PLAIN + ['--selfplay_gumbel', '--reanalyse_rows', '512', '--reanalyse_gumbel']):
    refuse_reanalyse_true_model(_config(argv))


def test_train_asks_in_the_preflight(monkeypatch):
  """train.main raises the flag's sentence before any device is touched"""
  from model_based_rl_amd import train
  called = []
  monkeypatch.setattr(train, 'launch', lambda *a, **k: called.append(a))
  for argv, start in ((PLAIN + ['--reanalyse_true_model'], '--reanalyse_true_model: '),
                      (PLAIN + ['--reanalyse_rows', '512', '--reanalyse_true_model', '--selfplay_gumbel', '--reanalyse_gumbel'], '--reanalyse_true_model: '),
                      (TRUE + ['--reanalyse_rows', '512'], '--selfplay_true_model: '),
                      (TRUE + ['--reanalyse_rows', '512', '--reanalyse_true_model', '--num_envs', '1'], '--reanalyse_rows: ')):
    with pytest.raises(SystemExit) as exc:
      train.main(argv)
    assert str(exc.value).startswith(start) and not called, (argv, str(exc.value))
  for argv, selfplay in ((TRUE + ['--reanalyse_rows', '512', '--reanalyse_true_model'], True),
                         (PLAIN + ['--reanalyse_rows', '512', '--reanalyse_true_model'], False)):
    del called[:]
    train.main(argv)
    assert len(called) == 1
    cfg = called[0][0]
    assert cfg.reanalyse_true_model is True and cfg.selfplay_true_model is selfplay and cfg.reanalyse_rows == 512


def test_the_reanalyser_reads_the_mode_from_the_config(monkeypatch):
  """no device: Reanalyser.__init__ with a stand-in engine sets the true-rules search iff the flag is given, and run() takes the
  new call with fused=True and no key"""
  import types
  from model_based_rl_amd import reanalyse
  calls = []

  class Stand(object):
    device = 'cpu'

    def set_true_model(self, kind):
      calls.append(('set_true_model', kind))

    def reanalyse(self, rows, fresh, n, kind):
      calls.append(('reanalyse', n, kind))

    def reanalyse_true_model(self, rows, fresh, n, kind, **kw):
      calls.append(('reanalyse_true_model', n, kind, kw))
  monkeypatch.setattr(reanalyse.Engine, 'from_config', staticmethod(lambda config, B, device=None: Stand()))
  monkeypatch.setattr(reanalyse.Reanalyser, '_size', lambda self, n: None)
  replay = types.SimpleNamespace(
      reanalyse_pick=lambda n, rows, busy_ok: dict(busy=False, slice_rows=[7], skipped_slices=0, ticket=1, n_rows=7),
      reanalyse_write=lambda ticket, fresh: dict(rows=0, abs_value_change=0.0, policy_l1=0.0))
  for env, kind in (('TicTacToe', 1), ('ConnectFour', 3)):
    base = ['--environment', env] + PLAIN[2:] + ['--reanalyse_rows', '512']
    for flag in (True, False):
      del calls[:]
      re = reanalyse.Reanalyser(_config(base + (['--reanalyse_true_model'] if flag else [])), replay)
      re.fresh = np.zeros((7, 11), np.float32)
      re.run(512)
      assert re.true_model is flag and not re.gumbel
      assert calls == ([('set_true_model', kind), ('reanalyse_true_model', 7, kind, {'fused': True})] if flag else [('reanalyse', 7, kind)])


# ------------------------------------------------------------------------------------------------------------- symbols
def test_entry_point_is_declared():
  import ctypes as C
  from model_based_rl_amd import _abi
  from model_based_rl_amd.engine import Engine
  from tests.test_abi import declared_symbols
  assert 'mz_reanalyse_true_model' in declared_symbols(('mz_engine.h',))
  res, args = _abi.SIGNATURES['mz_reanalyse_true_model']
  assert res is C.c_int and len(args) == 9 and args[7] is C.c_int      # (e, kind, rows, rec_floats, n_rows, fresh, sims, fused, stream)
  assert callable(Engine.reanalyse_true_model)
  with open(os.path.join(ROOT, 'model-based-rl_amd', 'csrc', 'mz_reanalyse.hip.h')) as f:
    text = f.read()
  assert 'mz_reanalyse_position(int kind, const float *obs, int to_play, int8_t *bd, int32_t *step)' in text
  assert 'void k_tm_root_reanalyse(TreeView t, TmState tm, int O, ReanalyseState rs)' in text


def test_the_learning_script_passes_the_flag_on():
  import importlib.util
  spec = importlib.util.spec_from_file_location('tictactoe_learning', os.path.join(ROOT, 'scripts', 'tictactoe_learning.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  ap = mod.build_parser()
  base, extra = mod.recipe(ap.parse_args(['--reanalyse_rows', '4096', '--reanalyse_true_model']))
  assert '--reanalyse_true_model' in extra and '--selfplay_true_model' not in extra
  cfg = _config(base + extra)
  assert cfg.reanalyse_true_model is True and cfg.reanalyse_rows == 4096
  base, extra = mod.recipe(ap.parse_args(['--selfplay_true_model', '--reanalyse_rows', '4096', '--reanalyse_true_model']))
  assert _config(base + extra).selfplay_true_model is True and '--reanalyse_true_model' in extra
  base, extra = mod.recipe(ap.parse_args([]))
  assert '--reanalyse_true_model' not in base + extra
