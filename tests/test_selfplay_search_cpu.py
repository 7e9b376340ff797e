"""The table of the self-play loop's search modes without a GPU (selfplay_search.py, DESIGN s7l): for every config that
tests/test_selfplay_gumbel_cpu.py and tests/test_selfplay_true_model_cpu.py build, and some with both flags, train's one preflight call
raises what the two per-flag functions raised one after the other before the table existed.  The sentences below are copies of
those functions' text, not derived from the table."""
import pytest

G = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '8', '--selfplay_gumbel']
T = ['--environment', 'TicTacToe', '--two_players', '--num_envs', '64', '--num_simulations', '30', '--selfplay_true_model']
C4G, C4T = ['--environment', 'ConnectFour'] + G[2:], ['--environment', 'ConnectFour'] + T[2:]

GUMBEL_HOST = '--selfplay_gumbel: host-environment actors (--num_envs 1 or --parity_rng) search with PUCT; use the device self-play loop.'
GUMBEL_SPLIT = '--selfplay_gumbel: --split_f16 is a fused search kernel, which this search does not run.'
GUMBEL_REANALYSE = ("--selfplay_gumbel: --reanalyse_rows would mix visit-share and pi' policy targets in one replay; Reanalyse does not write pi' "
                    "unless --reanalyse_gumbel is given.")
TRUE_HOST = '--selfplay_true_model: host-environment actors (--num_envs 1 or --parity_rng) search the learned model; use the device self-play loop.'
TRUE_TWO = '--selfplay_true_model: --selfplay_gumbel searches the learned model with the Gumbel search; a run takes one of the two.'
LOOP_ALONE = '--selfplay_true_model_loop: an option of --selfplay_true_model, which is not given.'

CASES = [      # (argv, ranks, the sentence or None)
    # ---- tests/test_selfplay_gumbel_cpu.py
    (G, 0, None), (G + ['--symmetry'], 0, None), (C4G, 0, None), (C4G + ['--symmetry'], 0, None),
    (['--environment', 'CartPole-v0', '--num_envs', '64', '--selfplay_gumbel'], 1, None),
    (['--environment', 'CartPole-v1', '--num_envs', '64', '--selfplay_gumbel'], 1, None),
    (['--environment', 'LunarLander-v2', '--split_f16', '--reanalyse_rows', '8'], 4, None),
    (G[:-1], 0, None), (G + ['--selfplay_gumbel_value', 'vmix'], 0, None),
    (G + ['--selfplay_gumbel_considered', '4', '--selfplay_gumbel_c_visit', '25', '--selfplay_gumbel_c_scale', '0.5', '--selfplay_gumbel_scale', '0.25',
          '--selfplay_gumbel_value', 'vmix'], 0, None),
    (['--environment', 'LunarLander-v2', '--num_envs', '64', '--selfplay_gumbel'], 0,
     '--selfplay_gumbel: the Gumbel self-play runs on the device games (TicTacToe, ConnectFour, CartPole-v0, CartPole-v1), LunarLander-v2 has none.'),
    (G + ['--architecture', 'TinyNetwork'], 0, "--selfplay_gumbel: only FCNetwork is searched by the engine's own kernels, TinyNetwork has no Gumbel search."),
    (G + ['--parity_rng'], 0, GUMBEL_HOST),
    (G[:3] + ['--num_envs', '1', '--selfplay_gumbel'], 0, GUMBEL_HOST),
    (G + ['--split_f16'], 0, GUMBEL_SPLIT),
    (G, 2, '--selfplay_gumbel: multi-rank runs (--ranks above 1) are not built for it.'),
    (G + ['--reanalyse_rows', '512'], 0, GUMBEL_REANALYSE),
    (G + ['--selfplay_gumbel_considered', '1'], 0, '--selfplay_gumbel: --selfplay_gumbel_considered must be at least 2, got 1.'),
    (G + ['--selfplay_gumbel_c_visit', '-1'], 0, '--selfplay_gumbel: --selfplay_gumbel_c_visit must not be negative, got -1.'),
    (G + ['--selfplay_gumbel_c_scale', '0'], 0, '--selfplay_gumbel: --selfplay_gumbel_c_scale must be positive, got 0.'),
    (G + ['--selfplay_gumbel_scale', '-0.5'], 0, '--selfplay_gumbel: --selfplay_gumbel_scale must not be negative, got -0.5.'),
    (G + ['--selfplay_gumbel_scale', 'nan'], 0, '--selfplay_gumbel: --selfplay_gumbel_scale must not be negative, got nan.'),
    # ---- tests/test_selfplay_true_model_cpu.py
    (T, 0, None), (T + ['--symmetry'], 0, None), (T + ['--selfplay_true_model_loop'], 1, None),
    (C4T, 0, None), (C4T + ['--symmetry'], 0, None), (C4T + ['--selfplay_true_model_loop'], 1, None),
    (T[:-1], 0, None), (T + ['--selfplay_true_model_loop'], 0, None),
    (['--environment', 'LunarLander-v2', '--num_envs', '64', '--selfplay_true_model'], 0,
     '--selfplay_true_model: the true rules are those of the device board games (TicTacToe, ConnectFour), LunarLander-v2 has none.'),
    (['--environment', 'CartPole-v1', '--num_envs', '64', '--selfplay_true_model'], 0,
     '--selfplay_true_model: the true rules are those of the device board games (TicTacToe, ConnectFour), CartPole-v1 has none.'),
    (T + ['--architecture', 'MuZeroNetwork'], 0,
     "--selfplay_true_model: only FCNetwork is searched by the engine's own kernels, MuZeroNetwork has no true-rules search."),
    (T[:3] + ['--num_envs', '1', '--selfplay_true_model'], 0, TRUE_HOST),
    (T + ['--parity_rng'], 0, TRUE_HOST),
    (T + ['--split_f16'], 0, '--selfplay_true_model: --split_f16 is a fused search kernel, which this search does not run.'),
    (T, 2, '--selfplay_true_model: multi-rank runs (--ranks above 1) are not built for it.'),
    (T + ['--selfplay_gumbel'], 0, TRUE_TWO),
    (T + ['--reanalyse_rows', '512'], 0,
     '--selfplay_true_model: --reanalyse_rows would write learned-model targets into the same replay; a true-rules Reanalyse is not built.'),
    (T[:-1] + ['--selfplay_true_model_loop'], 0, LOOP_ALONE),
    # ---- both flags, and the option beside the other flag: --selfplay_gumbel's row is asked first, whole
    (T + ['--selfplay_gumbel', '--split_f16'], 0, GUMBEL_SPLIT),
    (T + ['--selfplay_gumbel', '--reanalyse_rows', '512'], 0, GUMBEL_REANALYSE),
    (T + ['--selfplay_gumbel', '--reanalyse_rows', '512', '--reanalyse_gumbel'], 0, TRUE_TWO),
    (['--environment', 'CartPole-v1', '--num_envs', '64', '--selfplay_gumbel', '--selfplay_true_model'], 0,
     '--selfplay_true_model: the true rules are those of the device board games (TicTacToe, ConnectFour), CartPole-v1 has none.'),
    (G + ['--selfplay_true_model_loop'], 0, LOOP_ALONE),
    (G + ['--selfplay_true_model_loop', '--parity_rng'], 0, GUMBEL_HOST),
]


def test_one_preflight_call_raises_what_the_two_raised_in_turn():
  from model_based_rl_amd.config import make_config
  from model_based_rl_amd.selfplay_search import MODES, mode_of, refuse_selfplay_search
  for argv, ranks, sentence in CASES:
    cfg = make_config(argv)
    if sentence is None:
      refuse_selfplay_search(cfg, ranks)
      flags = [m for m in ('selfplay_gumbel', 'selfplay_true_model') if getattr(cfg, m)]
      assert MODES[mode_of(cfg)].flag == (flags[0] if flags else None), argv      # an accepted config selects one mode
      continue
    with pytest.raises(SystemExit) as exc:
      refuse_selfplay_search(cfg, ranks)
    assert str(exc.value) == sentence, argv
  both = make_config(T + ['--selfplay_gumbel'])
  with pytest.raises(SystemExit) as exc:      # two flags at once: --selfplay_true_model's sentence, wherever it is asked
    mode_of(both)
  assert str(exc.value) == TRUE_TWO


def test_engine_attributes_follow_the_switches():
  """Engine.selfplay_search and its two read-only views, without a device: the bookkeeping behind the two set calls"""
  from model_based_rl_amd.engine import Engine
  eng = Engine.__new__(Engine)
  assert (eng.selfplay_search, eng.selfplay_gumbel, eng.selfplay_true_model) == ('puct', False, False)
  for mode, on, after in (('gumbel', True, 'gumbel'), ('true_rules', False, 'gumbel'), ('gumbel', False, 'puct'), ('gumbel', False, 'puct'),
                          ('true_rules', True, 'true_rules'), ('gumbel', False, 'true_rules'), ('true_rules', False, 'puct')):
    eng._selfplay_switched(mode, on)
    assert (eng.selfplay_search, eng.selfplay_gumbel, eng.selfplay_true_model) == (after, after == 'gumbel', after == 'true_rules')
  with pytest.raises(AttributeError):
    eng.selfplay_gumbel = True
