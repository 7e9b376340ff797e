"""Configuration for the self-play path: the flags of the reference's config.py:87-231 that the search /
actor / replay-ingest path reads, with the reference's names and defaults, plus the pool size of the GPU
actor (`--num_envs`).  `Config` carries the helper methods callers use on it (config.py:21-84).
Flags outside the path (optimizer, lr schedule, Atari wrappers, ...) are accepted where they are cheap to
carry and otherwise not re-created."""
import argparse

import numpy as np


class Config(object):

  def __init__(self, args):
    self.__dict__.update(args)
    lo, hi = self.value_support
    self.value_support_min, self.value_support_max = lo, hi
    self.value_support_range = list(range(lo, hi + 1))
    self.value_support_size = hi - lo + 1
    lo, hi = self.reward_support
    self.reward_support_min, self.reward_support_max = lo, hi
    self.reward_support_range = list(range(lo, hi + 1))
    self.reward_support_size = hi - lo + 1

  # config.py:41-49
  def visit_softmax_temperature(self, training_step):
    steps, temps = self.visit_softmax_steps, self.visit_softmax_temperatures
    for boundary, temp in zip(steps, temps):
      if training_step <= boundary:
        return temp
    return temps[len(steps)]

  # config.py:70-81 (for Node objects; the batched engine does this in mz_finalize)
  @staticmethod
  def select_action(node, temperature=0.):
    actions = list(node.children.keys())
    counts = np.array([child.visit_count for child in node.children.values()])
    if temperature:
      dist = counts ** (1 / temperature)
      dist = dist / dist.sum()
      idx = np.random.choice(len(actions), p=dist)
    else:
      idx = np.random.choice(np.where(counts == counts.max())[0])
    return actions[idx]

  def new_game(self, environment):
    from .game import Game
    return Game(environment, self)


def build_parser():
  p = argparse.ArgumentParser(description='MI355X-native MuZero self-play (reference flag names)')
  a = p.add_argument
  a('--architecture', type=str, default='FCNetwork', choices=['FCNetwork', 'MuZeroNetwork', 'TinyNetwork'])
  a('--stack_obs', type=int, default=1)
  a('--stack_actions', action='store_true')
  a('--value_support', nargs=2, type=int, default=[-15, 15])
  a('--reward_support', nargs=2, type=int, default=[-15, 15])
  a('--no_support', action='store_true')
  a('--no_target_transform', action='store_true')
  a('--seed', type=int, default=None)
  a('--environment', type=str, default='LunarLander-v2')
  a('--two_players', action='store_true')
  a('--obs_range', nargs='+', type=float, default=None)
  a('--norm_obs', action='store_true')
  a('--clip_rewards', action='store_true')
  a('--episode_life', action='store_true')
  a('--sticky_actions', type=int, default=1)
  a('--num_actors', type=int, default=1)
  a('--num_envs', type=int, default=4096, help='environments searched in lock-step by one GPU actor')
  a('--episode_length', type=int, default=256, help='synthetic fixed-length episodes (gym is not installed)')
  a('--ingest_threads', type=int, default=None,
    help='threads of the native replay: environments of a record chunk, the samples of a batch, a large priority refresh (default: 4, 8 from batch size 1024 up, bounded by the CPUs)')
  a('--max_steps', type=int, default=40000)
  a('--num_simulations', type=int, default=30)
  a('--max_history_length', type=int, default=500)
  a('--visit_softmax_temperatures', nargs=3, type=float, default=[1.0, 0.5, 0.25])
  a('--visit_softmax_steps', nargs=2, type=int, default=[15000, 30000])
  a('--fixed_temperatures', nargs='+', type=float, default=[])
  a('--root_dirichlet_alpha', type=float, default=0.25)
  a('--root_exploration_fraction', type=float, default=0.25)
  a('--init_value_score', type=float, default=0.0)
  a('--known_bounds', nargs=2, type=float, default=[None, None])
  a('--pb_c_base', type=int, default=19652)
  a('--pb_c_init', type=float, default=1.25)
  a('--window_size', type=int, default=100000)
  a('--window_step', type=int, default=None)
  a('--epsilon', type=float, default=0.01)
  a('--alpha', type=float, default=1.)
  a('--beta', type=float, default=1.)
  a('--beta_increment_per_sampling', type=float, default=0.001)
  a('--training_steps', type=int, default=100000000)
  a('--num_unroll_steps', type=int, default=5)
  a('--td_steps', type=int, default=10)
  a('--batch_size', type=int, default=256)
  a('--stored_before_train', type=int, default=50000)
  a('--send_weights_frequency', type=int, default=500)
  a('--weight_sync_frequency', type=int, default=1000)
  a('--discount', type=float, default=0.997)
  a('--optimizer', type=str, default='AdamW', choices=['RMSprop', 'Adam', 'AdamW', 'SGD'])
  a('--lr_init', type=float, default=0.0008)
  a('--weight_decay', type=float, default=1e-4)
  a('--momentum', type=float, default=0.9)
  a('--clip_grad', type=int, default=0)
  a('--scalar_loss', type=str, default='MSE', choices=['MSE', 'Huber'])
  a('--lr_scheduler', type=str, default=None, choices=['ExponentialLR', 'MuZeroLR', 'WarmUpLR'])
  a('--lr_decay_rate', type=float, default=0.1)
  a('--lr_decay_steps', type=int, default=100000)
  a('--learner_gpu_device_id', type=int, default=None)
  a('--unbatched_learner', action='store_true',
    help='FCNetwork learner step position by position as the reference writes it, instead of the three heads batched over '
         'all K + 1 unroll positions (learners.py)')
  a('--no_tune_gemms', action='store_true',
    help='graphed learner: keep the BLAS libraries\' default kernel choice instead of PyTorch TunableOp picking the fastest per shape')
  a('--no_hip_learner_ops', action='store_true',
    help='learner targets and categorical losses as PyTorch elementwise kernels instead of the single HIP launches of csrc/mz_learner.hip.h')
  a('--batches_per_fetch', type=int, default=15,
    help='reference config.py:173: batches sampled ahead of the updates that consume them; here a background thread keeps '
         'min(this, 4) batches sampled ahead (1: sample in the learner\'s own thread, just before each update)')
  a('--no_native_learner', action='store_true',
    help='FCNetwork learner step through PyTorch operators (GEMM library + autograd) instead of the HIP launches (three at batch 256) of '
         'csrc/mz_fcl.hip.h (mz_fcl_step)')
  a('--no_native_loop', action='store_true',
    help='drive the native learner step from Python, one update per call (learners.py), instead of mz_fcl_run taking the loop body '
         '-- sampling, update, priority refresh -- for a whole stretch of updates')
  a('--no_graph_learner', action='store_true',
    help='run the learner step as eager PyTorch launches instead of one captured hipGraph per update (learners.py)')
  a('--learner_log_frequency', type=int, default=100)
  a('--frames_before_fps_log', type=int, default=10000)
  a('--runs_dir', type=str, default='runs', help='root of the run directories (the reference writes ./runs)')
  a('--save_state_frequency', type=int, default=1000)
  a('--use_gpu_for', nargs='+', type=str, default=['actors'], choices=['actors', 'learner'])
  a('--actors_gpu_device_ids', nargs='+', type=int, default=None)
  a('--group_tag', type=str, default=None)
  a('--run_tag', type=str, default=None)
  a('--actor_log_frequency', type=int, default=1)
  a('--selfplay_chunk', type=int, default=None,
    help='moves per launch / drain / ingest chunk of the device self-play loop (default 16: one launch of the persistent search kernel)')
  a('--no_gpu_turns', action='store_true',
    help='do NOT let an actor and the learner of one process take turns on a GPU they share (train.share_gpu_in_turns switches turns on '
         'whenever both resolve to the same device; this flag is for measuring what the turns are worth)')
  a('--gpu_turns', action='store_true',
    help='an actor and a learner of this process share ONE GPU: they take turns, one chunk of moves / one update at a time (gpu_turns.py)')
  a('--gpu_turn_updates', type=int, default=8,
    help='with --gpu_turns: updates the learner runs per turn (the actor holds the GPU for one chunk of moves per turn)')
  a('--split_f16', action='store_true',
    help='FCNetwork GEMMs of the search as float16 high/low splits on the f16 matrix pipe (float32-level accuracy, not '
         'bit-identical to the exact-float32 default; include/mz_engine.h mz_config.split_f16)')
  a('--reanalyse_rows', type=int, default=0,
    help='MuZero Reanalyse: stored replay rows searched again under the just-pulled weights per pass, their child_visits and '
         'root_value rewritten in place (reanalyse.py); 0: off')
  a('--reanalyse_every', type=int, default=None,
    help='learner steps between Reanalyse passes (default: --weight_sync_frequency); a pass follows the first weight pull past each multiple')
  a('--reanalyse_gumbel', action='store_true',
    help='--reanalyse_rows with --selfplay_gumbel: the passes search with the Gumbel MuZero search (--selfplay_gumbel_considered / '
         '_c_visit / _c_scale) and write the root\'s improved policy pi\' and the value --selfplay_gumbel_value names, what the '
         'self-play records of that mode hold (reanalyse.py)')
  a('--reanalyse_gumbel_scale', type=float, default=0.0,
    help='--reanalyse_gumbel: the scale of the Gumbel noise at a reanalysed root; 0 (the default) draws none: a reanalysed root '
         'needs a policy target, not exploration')
  a('--reanalyse_true_model', action='store_true',
    help='--reanalyse_rows on TicTacToe / ConnectFour: the passes search the stored positions on the TRUE rules below the root, as '
         '--selfplay_true_model searches its moves, and write visit shares and the root\'s mean value; with --selfplay_true_model '
         '(one kind of target in the replay), or alone: PUCT self-play whose targets are refreshed on the true rules (reanalyse.py)')
  a('--selfplay_gumbel', action='store_true',
    help='TicTacToe / ConnectFour / CartPole-v0 / -v1 on the device: the self-play moves are searched with the Gumbel MuZero '
         'search at --num_simulations (8 or 16 are its range), the records carry the improved policy pi\' as the policy target and '
         'the Gumbel pick as the action; the visit-softmax temperature plays no part (selfplay_search.py; evaluation keeps its '
         'own --gumbel flags)')
  a('--selfplay_gumbel_considered', type=int, default=16, help='--selfplay_gumbel: the actions sequential halving starts from (at least 2)')
  a('--selfplay_gumbel_c_visit', type=float, default=50.0, help='--selfplay_gumbel: sigma = (c_visit + max visits) * c_scale * normalised Q')
  a('--selfplay_gumbel_c_scale', type=float, default=1.0, help='--selfplay_gumbel: see --selfplay_gumbel_c_visit')
  a('--selfplay_gumbel_scale', type=float, default=1.0,
    help='--selfplay_gumbel: the scale of the Gumbel noise at the root, the exploration of this mode; 1 is the training setting of the paper')
  a('--selfplay_gumbel_value', type=str, default='mean', choices=['mean', 'vmix'],
    help='--selfplay_gumbel: what a record stores as the root value, the n-step targets\' bootstrap: the root\'s mean value, or its v_mix')
  a('--selfplay_true_model', action='store_true',
    help='TicTacToe / ConnectFour on the device: the self-play moves are PUCT moves searched on the TRUE rules below the root '
         '(real positions, legal moves only, the game\'s end), AlphaZero\'s search feeding MuZero\'s learner; records, learner and '
         'checkpoint are unchanged (selfplay_search.py; evaluation keeps its own --true_model flag)')
  a('--selfplay_true_model_loop', action='store_true',
    help='--selfplay_true_model: two launches per simulation (mz_tm_search) instead of one launch per move (mz_tm_search_fused); '
         'the records are the same')
  a('--symmetry', action='store_true',
    help='TicTacToe / ConnectFour: train every sample of a batch on one of the equivalent images of its position (8 rotations and '
         'mirrors / the left-right mirror), drawn per (seed, update, sample); observation, unrolled actions and policy targets move '
         'together (symmetry.py; on the native learner step one HIP launch, mz_fcl_set_symmetry)')
  a('--parity_rng', action='store_true',
    help="draw Dirichlet noise / action samples from numpy's global stream in the reference's order")
  return p


CARTPOLE_TIME_LIMITS = {'CartPole-v1': 500, 'CartPole-v0': 200}      # (envs.CartPole.max_episode_steps)
ENV_SHAPES = {   # (action_space, obs_space) of the environments the reference's README runs
    'TicTacToe': (9, (9,)), 'LunarLander-v2': (4, (8,)), 'Pong-ramNoFrameskip-v4': (6, (128,)),
    'Breakout-ramNoFrameskip-v4': (4, (128,)),
    'CartPole-v1': (2, (4,)), 'CartPole-v0': (2, (4,)),      # envs.CartPole, on the device too (csrc/mz_selfplay.hip.h)
    'ConnectFour': (7, (42,)),                                # envs.ConnectFour, likewise (two players)
    # image observations of the Atari wrappers (wrappers.py:422-444: 96x96 uint8 frames) -- what MuZeroNetwork /
    # TinyNetwork take (SURVEY.md s7 on BASELINE configs[4]).  The channel count is NOT a property of the environment:
    # utils.py:27-35 builds the network with input_channels = stack_obs, doubled with --stack_actions (None below;
    # env_shapes() fills it in from the flags, so the same flags build the same conv1 as the reference's)
    'BreakoutNoFrameskip-v4': (4, (None, 96, 96)), 'PongNoFrameskip-v4': (6, (None, 96, 96)),
}


def env_shapes(config):
  """(action_space, obs_space) of config.environment (train.py:66-68 probes the environment for these).  Image
  environments: channels = stack_obs * (2 if stack_actions else 1), as utils.get_network does (utils.py:27-35);
  their frames are bytes (config.obs_u8: the experience records and the replay keep them as bytes, game.py:93-96)."""
  A, obs = ENV_SHAPES[config.environment]
  if obs[0] is None:
    ch = int(getattr(config, 'stack_obs', 1)) * (2 if getattr(config, 'stack_actions', False) else 1)
    obs = (ch,) + tuple(obs[1:])
  return A, tuple(obs)


def obs_are_bytes(cfg):
  """image frames and the 128 bytes of console RAM of the -ram- environments travel as bytes in the experience records and
  the replay (game.py:93-96 keeps the raw uint8 observation)"""
  return len(tuple(getattr(cfg, 'obs_space', ()))) == 3 or '-ram' in str(getattr(cfg, 'environment', ''))


def make_config(argv=None, **overrides):
  args = vars(build_parser().parse_args(argv))
  args.update(overrides)
  cfg = Config(args)
  if cfg.environment in ENV_SHAPES and not hasattr(cfg, 'action_space'):
    cfg.action_space, cfg.obs_space = env_shapes(cfg)   # train.py:66-68 probes the env for these
  if not hasattr(cfg, 'obs_u8'):
    cfg.obs_u8 = obs_are_bytes(cfg)
  if cfg.environment in CARTPOLE_TIME_LIMITS:      # gym's TimeLimit: the episode length is the environment's, not a flag
    cfg.episode_length = cfg.max_episode_steps = CARTPOLE_TIME_LIMITS[cfg.environment]
  return cfg


def get_evaluation_args(argv=None):
  """The reference's evaluation flags (config.py:233-262) with its defaults, plus --batch (games played in lock-step on one
  engine; default min(num_games, 4096)), --out (a JSON summary), --device_env / --keep_history (the games on the device
  environments, evaluate.py), --opp_playouts (a playout-search opponent in --random_opp's seat), --grade / --grade_empties / --grade_nodes / --grade_table (moves graded against the exact solver, solver.py), --grade_unroll (the model by unroll depth on the graded games), --true_model (the search on the true rules of the device games), --gumbel / --gumbel_considered / --gumbel_c_visit / --gumbel_c_scale / --gumbel_scale (the Gumbel MuZero search) and --match / --opening_plies (matches between the nets, match.py).  Checkpoints are
  saves_dir + net for every pair."""
  p = argparse.ArgumentParser(description='evaluate saved networks on the GPU (reference evaluate.py)')
  a = p.add_argument
  a('--seed', type=int, default=None)
  a('--num_games', type=int, default=1)
  a('--saves_dir', nargs='+', type=str, default=[''])
  a('--nets', nargs='+', type=str, default=[''])
  a('--num_simulations', nargs='+', type=int, default=[None])
  a('--temperatures', nargs='+', type=float, default=[0])
  a('--only_prior', nargs='+', type=int, default=[0])
  a('--only_value', nargs='+', type=int, default=[0])
  a('--use_exploration_noise', nargs='+', type=int, default=[0])
  a('--apply_mcts_actions', nargs='+', type=int, default=[1])
  a('--render', action='store_true')
  a('--sleep', type=float, default=0)
  a('--human_opp', type=int, choices=[-1, 1], default=None)
  a('--random_opp', type=int, choices=[-1, 1], default=None)
  a('--plot_summary', action='store_true')
  a('--include_bounds', action='store_true')
  a('--include_policy', action='store_true')
  a('--detailed_label', action='store_true')
  a('--smooth', type=int, default=None)
  a('--save_gif_as', type=str, default='')
  a('--save_mcts', action='store_true')
  a('--save_mcts_after_step', type=int, default=0)
  a('--parallel', action='store_true', help='accepted and ignored: the games are already played in lock-step batches')
  a('--use_gpu', action='store_true', help='accepted and implied: there is no CPU path')
  a('--verbose', action='store_true')
  a('--batch', type=int, default=None, help='games played in lock-step on one engine (default: min(num_games, 4096))')
  a('--out', type=str, default=None, help='write the summary of every configuration to this JSON file')
  a('--device_env', action='store_true',
    help='play the games on the device environments (TicTacToe, ConnectFour, CartPole-v0 / -v1): no host work between moves')
  a('--keep_history', action='store_true', help='--device_env: keep the per-move lists of every game, not only its summary')
  a('--opp_playouts', type=int, default=0,
    help='--device_env --random_opp SEAT: that seat is played by a playout search (UCT on the true rules, no network) of this '
         'many playouts per move, a multiple of 64 in 64 .. 65536; 0: the uniformly random mover')
  a('--grade', action='store_true',
    help='--device_env, TicTacToe / ConnectFour: grade the moves against the exact solver (the network\'s moves with '
         '--random_opp, both sides\' without): optimal-move rate, blunders by class, value errors against the true value')
  a('--grade_empties', type=int, default=12,
    help='--grade on ConnectFour: positions with at most this many empty cells are graded (TicTacToe grades every position)')
  a('--grade_nodes', type=int, default=4096,
    help='--grade: the solver\'s node budget per (position, action); a decision it does not settle is counted as unsolved')
  a('--grade_table', action='store_true',
    help='--grade: solve with the table search (non-losing moves, ordered by threats, a transposition table a unit): the same '
         'exact values from far fewer nodes, so --grade_empties can be raised at the same --grade_nodes')
  a('--grade_unroll', type=int, default=None, metavar='K',
    help='--grade: also unroll the model K (1 .. 16) dynamics steps along the moves of the graded games and report, per '
         'depth, reward, value and policy against the real positions and the exact solver (solver.grade_unroll)')
  a('--true_model', nargs='+', type=int, default=[0],
    help='--device_env or --match, TicTacToe / ConnectFour: 1 searches the real game below the root -- positions by the '
         'device rules, legal actions only, true rewards and ends -- with the same weights and the same MCTS (evaluation '
         'only); one value for all, or with --match one per side')
  a('--gumbel', nargs='+', type=int, default=[0],
    help='--device_env or --match: 1 searches with the Gumbel MuZero search (Gumbel-top-k with sequential halving at the '
         'root, a deterministic rule below it, the move chosen by the rule) instead of PUCT, with the same weights '
         '(evaluation only); one value for all, or with --match one per side')
  a('--gumbel_considered', type=int, default=16, help='--gumbel: the actions sequential halving starts from (at least 2)')
  a('--gumbel_c_visit', type=float, default=50.0, help='--gumbel: sigma = (c_visit + max visits) * c_scale * normalised Q')
  a('--gumbel_c_scale', type=float, default=1.0, help='--gumbel: see --gumbel_c_visit')
  a('--gumbel_scale', type=float, default=0.0,
    help='--gumbel: the scale of the Gumbel noise at the root; 0 (the default) draws none and is deterministic, 1 is the '
         'acting setting of the paper')
  a('--match', action='store_true',
    help='play every pair of --nets against each other on the device games (TicTacToe, ConnectFour), every seed from both '
         'seats; --temperatures / --num_simulations / --only_prior / --only_value / --use_exploration_noise / --true_model / --gumbel then take one '
         'value for both sides or two, one per side')
  a('--opening_plies', type=int, default=0,
    help='--match: uniform random legal plies before the first searched one, the same in both seatings of a seed')
  args = p.parse_args(argv)
  if args.batch is None:
    args.batch = min(args.num_games, 4096)
  return args
