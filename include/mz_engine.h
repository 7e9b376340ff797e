/*
 * mz_engine.h -- C ABI of the MI355X-native MuZero self-play / MCTS engine (libmz_hip.so).
 *
 * The reference (JimOhman/model-based-rl) is pure Python with no FFI: its search path is reached by
 * duck-typed calls.  This header is the boundary a native replacement of that path
 * exports; the Python mirror in model-based-rl_amd/ (mcts.py, actors.py, ...) binds it with ctypes
 * (cffi.dlopen works on the same symbols) and keeps the reference's class surface on top.
 * Each entry point cites the reference code it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; the message is mz_last_error() (thread-local).
 *     Nothing throws across the ABI.  (Reference convention: Python exceptions, e.g. actors.py:41.)
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     asynchronous on it.  An engine is not thread-safe; use one engine per GPU per process.
 *   - pointers marked [dev] are device pointers (e.g. tensor.data_ptr()), owned by the caller and
 *     alive until the stream reaches the end of the call's work; [host] are host pointers.
 *   - B = num_envs trees are searched in lock-step; A = action_space; H = 50 (FCNetwork hidden_dim).
 *   - node numbering inside a tree: expansion index e: root 0, the leaf expanded by simulation s is
 *     s+1 (also its hidden-state slot); node index: root 0, child a of the node with expansion index
 *     e is 1 + e*A + a.  NN = 1 + (num_simulations+1)*A nodes per tree.
 */
#ifndef MZ_ENGINE_H
#define MZ_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#include "mz_record.h"      /* the experience record's layout: MZ_REC_EXTRA, the tail's offsets, the flag bits */

#ifdef __cplusplus
extern "C" {
#endif

#define MZ_HIDDEN 50       /* networks.py:135 */
#define MZ_FC_WIDTH 512    /* networks.py:60,75,88,101,114 */
#define MZ_MAX_ACTIONS 32
#define MZ_MAX_SUPPORT 32

typedef struct mz_engine mz_engine;

/* The subset of the reference's Config (config.py:87-231) the search path reads. */
typedef struct mz_config {
  int32_t num_envs;             /* B; rounded up internally to a multiple of 16 */
  int32_t obs_dim;              /* prod(config.obs_space) */
  int32_t action_space;         /* config.action_space, <= MZ_MAX_ACTIONS */
  int32_t num_simulations;      /* --num_simulations */
  int32_t two_players;          /* --two_players */
  int32_t has_min_bound;        /* --known_bounds[0] is not None */
  int32_t has_max_bound;        /* --known_bounds[1] is not None */
  int32_t value_support_min, value_support_max;    /* --value_support, size <= MZ_MAX_SUPPORT */
  int32_t reward_support_min, reward_support_max;  /* --reward_support */
  int32_t no_target_transform;  /* --no_target_transform */
  double min_bound, max_bound;  /* --known_bounds */
  double discount;              /* --discount */
  double pb_c_base, pb_c_init;  /* --pb_c_base / --pb_c_init */
  double init_value_score;      /* --init_value_score */
  double root_dirichlet_alpha;  /* --root_dirichlet_alpha */
  double root_exploration_fraction; /* --root_exploration_fraction */
  uint64_t seed;                /* counter-based device RNG key (throughput mode) */
  int32_t env_id_offset;        /* global id of env 0 (rank * num_envs when actors are sharded over GPUs) */
  int32_t no_support;           /* --no_support: value / reward heads are single scalars (networks.py:135-136), returned
                                 * untransformed in eval mode (networks.py:153,161); the supports above are ignored */
  int32_t split_f16;            /* 0 (default): the FCNetwork GEMMs of mz_search / the self-play loop run on
                                 * v_mfma_f32_16x16x4_f32 -- exact float32, the reference's arithmetic type.
                                 * 1: opt-in fast path (action_space <= 13): every float32 operand is split into two
                                 * float16 parts and every product block is three v_mfma_f32_16x16x32_f16 with float32
                                 * accumulation (csrc/mz_fused_h2.hip.h): float32-level accuracy (deviation from a float64
                                 * evaluation 1-2x that of the exact path, inside the 1e-5 bound), NOT bit-identical to the
                                 * exact path.  The environment variable MZ_SPLIT_F16=1 sets it for every engine.
                                 * Range: the high part of a split value is its float16 rounding, so mz_set_weights FAILS for
                                 * weights that are not finite or exceed 65504 in magnitude; weights below 6.1e-5 in magnitude
                                 * are carried with an absolute error of ~3e-8 (float16 subnormals) instead of a relative one --
                                 * far inside the 1e-5 bound on outputs.  Activations are split at run time the same way: hidden
                                 * states are min-max free here (ReLU(LayerNorm), |x| < ~10), head pre-activations are sums of
                                 * 512 products of such values and PyTorch-initialised weights. */
} mz_config;

const char *mz_last_error(void);
int mz_version(void);

/* MCTS.__init__ (mcts.py:66-76) + Actor.__init__'s network/device set-up (actors.py:33-47).
 * Allocates every device pool (node SoA, hidden-state pool, packed weights, scratch). */
int mz_create(const mz_config *cfg, mz_engine **out);
int mz_destroy(mz_engine *e);

/* Number of float32 parameters of FCNetwork for this config (networks.py:137-144). */
size_t mz_num_weights(const mz_engine *e);

/* BaseNetwork.load_weights (networks.py:36-37; actors.py:81-85).  `flat` is the reference's
 * state_dict concatenated in its own key order: representation_head.{fc1,out}.{weight,bias},
 * value_head.{fc1,value}, policy_head.{fc1,policy}, reward_head.{fc1,reward},
 * transition_head.{fc1,out}, LN.{weight,bias}; Linear weights [out][in] row-major.
 * on_device != 0: flat is [dev] (e.g. the buffer an RCCL broadcast just filled); else [host].
 * Synchronises `stream` before it returns (a 16-byte read back decides which kernel set this weight set runs on,
 * mz_weight_scale below; a host buffer may be released as soon as the call returns). */
int mz_set_weights(mz_engine *e, const float *flat, size_t n, int on_device, void *stream);

/* Actor.sync_weights (actors.py:81-85) without draining the launch-ahead pipeline: mz_set_weights whose host side waits for
 * NOTHING queued on `stream`.  The repack runs in stream order -- moves queued before the call keep the old weights, everything
 * queued after it sees the new ones; a [host] source is copied into the engine's pinned staging before the call returns
 * (the caller's buffer is free again), a [dev] source must stay valid until the stream has passed the call (e.g. the buffer
 * mz_broadcast_weights filled on the same stream).  No read back: which kernel set the weights run on is the caller's
 * `scale_ok` = mz_weights_scale_ok(...) evaluated on a HOST copy of the SAME weights (the learner rank has one; it travels
 * with the training step).  Nothing in it synchronises or allocates after the first call with a [host] source: with a
 * [dev] source the call can be captured into a graph.  split_f16 engines fall back to mz_set_weights (range check).
 * mz_weights_scale_ok: 1 if this weight set admits the power-of-two scale of the search kernel's stream (mz_weight_scale),
 * 0 if not, < 0 on error; host arithmetic only, no GPU.  value_outputs / reward_outputs: the support sizes (1 with
 * --no_support). */
int mz_set_weights_async(mz_engine *e, const float *flat, size_t n, int on_device, int scale_ok, void *stream);
int mz_weights_scale_ok(const float *flat_host, size_t n, int obs_dim, int action_space, int value_outputs, int reward_outputs);

/* The path's ONE collective (reference: every actor pulls the pickled state_dict from the storage actor,
 * actors.py:81-85, shared_storage.py:12-18, learners.py:85-86): the flat float32 weights from the learner rank to every
 * actor rank as an RCCL broadcast issued on the caller's HIP stream -- ordered by the stream with the repack that follows
 * (mz_set_weights_async(on_device = 1) on the same stream), no host wait in between.  librccl is bound at run time:
 * mz_comm_load(path) (NULL / "": the copy the process already holds, else the loader's search path); mz_comm_unique_id
 * (rank 0) -> 128 bytes, handed to every rank by the caller (torch.distributed / any channel); mz_comm_create on every rank
 * (collective: ncclCommInitRank on the calling thread's current device); mz_broadcast_weights: flat [dev][n] in place,
 * from rank `root`. */
typedef struct mz_comm mz_comm;
int mz_comm_load(const char *librccl_path);
int mz_comm_unique_id(void *out128);
int mz_comm_create(int rank, int world, const void *unique_id128, mz_comm **out);
int mz_comm_destroy(mz_comm *c);
/* ranks the communicator spans, as RCCL reports it (ncclCommCount) */
int mz_comm_count(const mz_comm *c, int *ranks_out);
int mz_broadcast_weights(mz_comm *c, float *flat, size_t n, int root, void *stream);

/* Diagnostic: how the last mz_set_weights packed the search kernel's weight stream.  out [host][4] =
 * {1, 2^-k, 2^k, chosen}: with chosen = 1 the stream carries the four 512-wide hidden layers of the search
 * (networks.py:70-93,96-119: reward / transition / value / policy fc1) times 2^-k and the layers reading their
 * activations times 2^k -- bit-neutral (powers of two), it lets the kernel apply nn.ReLU as a [0, 1] clamp on two
 * elements per instruction; 2^k exceeds a bound of every activation computed from this weight set.  chosen = 0
 * (non-finite or absurdly large weights): unscaled stream, ordinary maximum.  Synchronises `stream` after an
 * mz_set_weights_async (the four floats are read back on demand). */
int mz_weight_scale(mz_engine *e, float *out, void *stream);

/* BaseNetwork.initial_inference (networks.py:26-29) for B observations, actors.py:139.
 * obs [dev][B][obs_dim] float32 (already normalised, actors.py:134-137).  Fills hidden slot 0, the
 * root value and the root policy logits inside the engine. */
int mz_initial_inference(mz_engine *e, const float *obs, void *stream);

/* Same, but with network outputs computed elsewhere (any torch network): hidden [dev][B][50] or NULL,
 * value [dev][B], logits [dev][B][A]. */
int mz_root_load(mz_engine *e, const float *hidden, const float *value, const float *logits, void *stream);

/* Read back what initial inference produced: value [dev][B], logits [dev][B][A], hidden [dev][B][50]
 * (any may be NULL). */
int mz_root_outputs(mz_engine *e, float *value, float *logits, float *hidden, void *stream);

/* Node(0) + root.expand + root.add_exploration_noise + MinMaxStats.reset
 * (actors.py:132,141-143; mcts.py:47-61,79).
 * to_play [dev][B] int8 or NULL (= +1);  legal [dev][B][A] uint8 or NULL (= all legal);
 * noise [dev][B][A] float64: the Dirichlet draw scattered to the legal positions (parity mode, drawn
 * by the host's numpy in the reference's order), or NULL with use_device_rng != 0 to draw it on the
 * device from the counter-based RNG keyed (seed, env, move), or NULL with use_device_rng == 0 for no
 * noise at all (evaluation, evaluate.py). */
int mz_root_prepare(mz_engine *e, const int8_t *to_play, const uint8_t *legal, const double *noise,
                    int use_device_rng, uint64_t move_counter, void *stream);

/* Root from priors the caller already holds (its own Node.expand + add_exploration_noise, mcts.py:47-61):
 * priors [dev][B][A] float64 (entries of illegal actions ignored).  Used by the batch-1 MCTS.run front-end. */
int mz_root_set_priors(mz_engine *e, const int8_t *to_play, const uint8_t *legal, const double *priors,
                       void *stream);

/* The search path of the pending descent (after mz_select): paths [dev][B][num_simulations+2] node indices,
 * lengths [dev][B].  (MCTS.run returns these as `search_paths`, mcts.py:101-102.) */
int mz_last_paths(mz_engine *e, int32_t *paths, int32_t *lengths, void *stream);

/* MCTS.run (mcts.py:78-102) for all B trees with the engine's own FCNetwork kernels:
 * num_simulations x { select_child descent, recurrent_inference, expand, backpropagate },
 * no host synchronisation. */
int mz_search(mz_engine *e, int num_simulations, void *stream);




/* The same loop opened up for an external network (MuZeroNetwork/TinyNetwork through PyTorch, or
 * recorded outputs in the parity tests):
 *   mz_select        = the descent of mcts.py:83-94; outputs (any may be NULL):
 *                      leaf_node, parent_slot (hidden slot of search_path[-2]), action, depth [dev][B] int32
 *   mz_gather_hidden = hidden_out[b] = hidden pool[b][parent_slot[b]]  ([dev][B][50])
 *   mz_expand_backup = node.expand (mcts.py:97) + backpropagate (mcts.py:99,126-143) with
 *                      value/reward [dev][B], logits [dev][B][A], hidden [dev][B][50] or NULL. */
int mz_select(mz_engine *e, int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth,
              void *stream);
int mz_gather_hidden(mz_engine *e, float *hidden_out, void *stream);
int mz_expand_backup(mz_engine *e, const float *value, const float *reward, const float *logits,
                     const float *hidden, void *stream);
/* mz_expand_backup followed by the next simulation's mz_select (mcts.py:97-99 then 83-94 of the next iteration) in ONE launch:
 * the descent reads the lines the backup has just written from cache, and a simulation of an external network costs one tree
 * launch instead of three.  Same arguments as mz_expand_backup, then mz_select's outputs (any may be null).  At a move's
 * last simulation there is no next descent: it is mz_expand_backup alone and the outputs are left untouched. */
int mz_expand_backup_select(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                            int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth, void *stream);

/* BaseNetwork.recurrent_inference (networks.py:31-34) on arbitrary rows, outside any tree:
 * hidden_in [dev][n][50], action [dev][n] int32 -> hidden_out [dev][n][50], reward/value [dev][n],
 * logits [dev][n][A].  n <= num_envs.  (Network parity tests; evaluate.py-style callers.) */
int mz_recurrent_inference(mz_engine *e, const float *hidden_in, const int32_t *action, int n,
                           float *hidden_out, float *reward, float *value, float *logits, void *stream);

/* End of a move: Config.select_action (config.py:70-81), Game.store_search_statistics
 * (game.py:106-115), root error (actors.py:147-148).
 * temperature [dev][B] float64; uniform [dev][B] float64 in [0,1) (the draw np.random.choice would
 * consume; NULL = device RNG keyed (seed, env, move)).  temperature 0 picks the
 * floor(u*n_ties)-th arg-max child.  Outputs (any may be NULL): action [dev][B] int32,
 * child_visits [dev][B][A] float64, root_value [dev][B] float64, error [dev][B] float64
 * (root value - initial value), visit_counts [dev][B][A] int32. */
int mz_finalize(mz_engine *e, const double *temperature, const double *uniform, uint64_t move_counter,
                int32_t *action, double *child_visits, double *root_value, double *error,
                int32_t *visit_counts, void *stream);

/* Evaluator.play_game's move after the search (evaluate.py:305-327), B evaluation games in lock-step:
 *   actions: from the root, while the node is expanded, Config.select_action (config.py:70-81) over its children -- the legal
 *   actions in ascending order at the root (mcts.py:47-55), range(A) below it (mcts.py:97) -- and on to the chosen child,
 *   at most max_actions = M times (--apply_mcts_actions).  temperature [dev][B] float64; uniform [dev][B][M] float64 in [0,1):
 *   the draw of each step (temperature 0: the floor(u*n_ties)-th arg-max child, as mz_finalize), or NULL = device RNG keyed
 *   (seed, env, move, step).  Outputs: actions [dev][B][M] int32 (-1 past the last), pred_rewards [dev][B][M] float32
 *   (the chosen child's reward, evaluate.py:318; 0 for a child never expanded), n_actions [dev][B] int32, path_lengths
 *   [dev][B][num_simulations] int32 or NULL: len(search_path) of every simulation of the last search (evaluate.py:306-307,
 *   mcts.py:101-102; 0 past the simulations run).  Reads the trees mz_search (or the stepwise loop) left. */
int mz_eval_walk(mz_engine *e, int max_actions, const double *temperature, const double *uniform, uint64_t move,
                 int32_t *actions, float *pred_rewards, int32_t *n_actions, int32_t *path_lengths, void *stream);

/* --only_prior / --only_value (evaluate.py:278-304) after mz_initial_inference + mz_root_prepare, no search: two launches,
 * no host synchronisation between or after them.  mode 2 (only_value): BaseNetwork.recurrent_inference (networks.py:31-34) of every root's hidden
 * state with every action (B*A rows, the arithmetic of mz_recurrent_inference), q = reward + discount * value (reward -
 * discount * value with two players) in float32; the first strict maximum over the legal actions in ascending order;
 * child_visits 1/|legal| on the legal actions.  mode 1 (only_prior): max((prior, action)) over the root's children -- the
 * largest float64 prior after mz_root_prepare's noise, ties to the largest action -- and one recurrent inference for its
 * reward; child_visits one-hot.  Outputs: action [dev][B] int32, pred_reward [dev][B] float32 (the chosen action's reward),
 * child_visits [dev][B][A] float64 or NULL, row_reward / row_value [dev] or NULL: the rows' rewards and values ([B][A] in
 * mode 2, [B] in mode 1).  The root value is Node.value() of a root never visited: 0.  The FIRST call allocates the rows' scratch
 * (B*A rows) and so synchronises; later calls do not. */
int mz_eval_lookahead(mz_engine *e, int mode, int32_t *action, float *pred_reward, double *child_visits, float *row_reward,
                      float *row_value, void *stream);

/* Evaluation games that live on the device from the first move to the last (Evaluator.play_game's loop, evaluate.py:242-385,
 * for B games in lock-step): the host touches no game between moves.  One evaluation state per engine, separate from the
 * self-play loop's.  Game b of the engine is the game with seed env_id_offset + b.
 *
 * mz_eval_env_reset: kind 1 TicTacToe, 2 CartPole, 3 Connect Four (the device rules of mz_selfplay_set_env; the engine must
 * have that game's obs_dim / action_space / two_players).  max_steps: the game is cut when its step count reaches it
 * (evaluate.py:372); time_limit: CartPole's TimeLimit (500 / 200), ignored otherwise; random_opp +1 / -1: that player's moves
 * are the random opponent's (two players), 0: none; keep_history != 0: per-move logs are kept ([B][cap] per entry, cap =
 * min(max_steps, the game's longest: 9 / 42 / time_limit), mz_eval_env_log_capacity).  Every game starts from env.reset();
 * CartPole's start state is the counter RNG's mz_cartpole_reset_state(env_id_offset + b, episode 0).  Synchronous.
 *
 * mz_eval_env_set_draws (after reset, before the first move; parity runs): every draw given by the caller instead of the
 * counter RNG, as [dev] arrays the caller keeps alive until the games are over; any may be NULL.  walk [B][walk_moves][walk_m]
 * float64: the uniforms of mz_eval_walk (walk_m == max_actions); noise [B][noise_moves][A] float64: the Dirichlet draw of
 * every move at the legal positions; opp [B][opp_n] int32: the random opponent's choices in the order it makes them, each
 * an index into the legal actions of the move's root position; start_states [B][4] float64: CartPole's start states.
 * Moves past the given ones draw zeros.
 *
 * mz_eval_env_moves: n whole moves enqueued on the stream, each: observe (state -> obs / legal / to_play; a finished game
 * gets a zero observation, all actions legal, to_play +1) -> mz_initial_inference -> mz_root_prepare (noise_on: the given
 * draw, or the device Dirichlet keyed by the move) -> mode 0: mz_search + mz_eval_walk (max_actions, temperature; device
 * uniforms under MZ_RNG_EVAL keyed by the move) + mz_finalize, mode 1 / 2: mz_eval_lookahead (--only_prior / --only_value)
 * -> apply (evaluate.py:331-374 on the device rules: the predicted value, root value and child visits once, then per
 * walked action the predicted reward, the random opponent's replacement -- drawn from the legal list OF THE MOVE'S ROOT
 * POSITION, the reference's stale list, index min(floor(u * n), n - 1) with u from the counter RNG under MZ_RNG_OPP keyed
 * (seed, game's seed, move, step) -- the env step, the cut at done or max_steps with the sign flip of an opponent's last
 * reward; then the lexicographic maximum of the search-depth lists).  No host synchronisation between the moves; one
 * copy at the end returns the number of games still live in *live_out [host].  The first call sizes the walk's buffers
 * and uploads the temperature, and so synchronises once more.  Connect Four takes max_actions == 1 only.
 *
 * mz_eval_env_results (synchronous, [host] arrays, any may be NULL): step [B] int32 (game length), n_moves [B] int32,
 * acc [5][B] float64 (sum of rewards, of predicted rewards, of predicted values, of root values -- added in move order --
 * and the mean of the lexicographic-maximum depth list), depth_max [B][num_simulations] int32 (that list; one entry with
 * modes 1 / 2); the logs, kept with keep_history: per applied action [B][cap] actions int32 (the opponent's included),
 * rewards float64, mover int8 (+1 / -1, doubled on the step env.step itself reported done), pred_rewards float32; per move [B][cap] pred_values float32, root_values float64,
 * child_visits [B][cap][A] float64, n_actions int32, depths [B][cap][num_simulations] int32 (mode 0). */
int mz_eval_env_reset(mz_engine *e, int kind, int max_steps, int time_limit, int random_opp, int keep_history, void *stream);
int mz_eval_env_set_draws(mz_engine *e, const double *walk, int walk_moves, int walk_m, const double *noise, int noise_moves,
                          const int32_t *opp, int opp_n, const double *start_states, void *stream);
int mz_eval_env_moves(mz_engine *e, int n, int mode, int max_actions, double temperature, int noise_on, int *live_out,
                      void *stream);
int mz_eval_env_results(mz_engine *e, int32_t *step, int32_t *n_moves, double *acc, int32_t *depth_max, int32_t *actions,
                        double *rewards, int8_t *mover, float *pred_rewards, float *pred_values, double *root_values,
                        double *child_visits, int32_t *n_actions, int32_t *depths, void *stream);
int mz_eval_env_log_capacity(const mz_engine *e);

/* The playout-search (UCT) opponent: a classical Monte-Carlo tree search on the true rules of TicTacToe (kind 1) and Connect
 * Four (kind 3) -- random playouts, no network, planned on the device by one wave per game (DESIGN s7d;
 * csrc/mz_playout.hip.h).  playouts: the budget per move, a multiple of 64 in 64 .. 65536.
 *
 * mz_playout_plan: one move for each of n_games <= num_envs given positions; game i has the seed env_id_offset + i and its
 * plan depends on (engine seed, that seed, move, its position, playouts) only.  [host] boards [n_games][42] int8 (cell
 * 7 * row + col; TicTacToe uses the first 9 cells of a row and the rest must be 0), turn [n_games] int8 (+1 / -1, the
 * mover), step [n_games] int32 (plies played: the number of stones).  Every position must be one of the game's with a
 * legal action.  Out, [host]: action_out [n_games] int32, visits_out / wins_out [n_games][A] int32 (either may be NULL):
 * the root's playouts per action and 2 * wins + draws of the mover.  Does not need weights.  Synchronises once.
 *
 * mz_eval_env_set_opponent (after mz_eval_env_reset with a random_opp seat, before the first move): the moves of that seat
 * are planned with `playouts` playouts each, keyed by the move (0: the uniformly random mover, the state after a reset).
 * mz_eval_env_moves then takes max_actions == 1 only. */
int mz_playout_plan(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n_games,
                    int playouts, uint64_t move, int32_t *action_out, int32_t *visits_out, int32_t *wins_out, void *stream);
int mz_eval_env_set_opponent(mz_engine *e, int playouts, void *stream);

/* The exact game solver (DESIGN s7f; csrc/mz_solve.hip.h): for each of n positions of TicTacToe (kind 1) or Connect Four
 * (kind 3) and each action a, the outcome for the mover after playing a with both sides perfect from there -- +1 the mover
 * wins, 0 a draw, -1 the mover loses (the outcome only, not the distance to it), -2 a is illegal, -3 not solved within
 * max_nodes nodes.  A plain negamax with the window [-1, +1], a fixed move order and no transposition table; the unit of
 * work is the subtree under one (position, action), searched by one lane with its own budget of max_nodes (1 .. 2^30)
 * nodes, so a value depends on the position and the budget alone, not on the batch.  Takes an engine of the game's shape
 * (as mz_playout_plan); the weights are not read.  [host] boards [n][42] int8, turn [n] int8, step [n] int32 as
 * mz_playout_plan's, any n (chunks of num_envs inside); every position must be one of the game's with a legal action in
 * which neither side has a line yet.  Out, [host]: values_out [n][A] int8, nodes_out [n][A] uint32 (or NULL): the nodes
 * spent on a, saturating at max_nodes (0 where illegal).  Its device memory is its own, allocated on first use.
 * Synchronises once, at the end. */
int mz_solve(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
             int8_t *values_out, uint32_t *nodes_out, void *stream);

/* The table search (DESIGN s7f, "The table search"): mz_solve's arguments, checks, chunks, outputs and one synchronisation,
 * the same units with the same top and the same budget rule, searched with the moves that do not lose at once only, ordered
 * by the threats they make, and a transposition table of 4096 entries private to each unit.  Values are exact as
 * mz_solve's; a unit needs far fewer nodes (nodes_out counts this search's stones), so at a given max_nodes fewer are -3.
 * A unit sees no entry of another unit, so a value and a node count depend on the position and the budget alone.  Its
 * tables (32 KB a lane, for min(1024, ceil(num_envs * A / 64)) waves) are its own, allocated on first use. */
int mz_solve_tt(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                int8_t *values_out, uint32_t *nodes_out, void *stream);

/* The learned model graded by unroll depth against the true game (DESIGN s7f, "Grading by unroll depth";
 * csrc/mz_unroll.hip.h).  A row is a start position of TicTacToe (kind 1) or Connect Four (kind 3) -- [host] boards [n][42],
 * turn [n], step [n] as mz_solve takes them, any n (chunks of num_envs inside) -- and [host] actions [n][K] int32, -1 as
 * padding, K in 0 .. 16.  The row's LINE: p_0 is the start; while j < K, actions[j] >= 0 and p_j is not terminal, p_{j+1} =
 * step(p_j, actions[j]) on the true rules and the mover alternates; depth = the actions applied.  An action that is illegal
 * in p_j stops the line there and sets bit 0 of the row's flags.  Per chunk, in stream order with no host synchronisation:
 * the lines; mz_initial_inference of p_0 (h_0, v_0, logits_0); K times mz_recurrent_inference(h_{k-1}, a_{k-1}), the
 * UNROLLED h_k, r_k, v_k, logits_k; K times mz_initial_inference of the real p_k, the FRESH v_k, logits_k; the terms.  A row
 * whose line is shorter than k keeps its lane and its outputs at k are zero.
 *   truth      [host][n][K + 1][A] int8 or NULL: mz_solve's values of the actions of p_k (-2 illegal, -3 unsolved; all -3: p_k
 *              is not in scope).  NULL: the terms that need it stay zero.
 *   terms_out  [host][n][K + 1][mz_unroll_num_terms()] float64, the scalars the report averages, in the order of
 *              MzUnrollTerm (csrc/mz_unroll.hip.h; engine.Engine.UNROLL_TERMS): softmax over all A actions, float64
 *              arithmetic on the float32 outputs, sums in ascending action order.  Values are in the view of p_k's mover.
 *   depth_out, flags_out  [host][n] int32.
 *   raw_out    [host][n][K + 1][mz_unroll_raw_floats()] float32 or NULL: per (row, k) the observation [obs_dim], the unrolled
 *              hidden state [50], the unrolled and the fresh logits [A] each, then value_u, reward_u, value_f, reward_true;
 *              raw_meta_out [host][n][K + 1][2] int32 (NULL with raw_out): the legal mask of p_k and whether it is terminal.
 * Overwrites the engine's root outputs and hidden slot 0; the weights, the RNG keys, the evaluation environment and the
 * solver are left alone.  Its device memory is its own, allocated on first use.  Synchronises once, at the end. */
int mz_unroll(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, const int32_t *actions, int n,
              int K, const int8_t *truth, double *terms_out, int32_t *depth_out, int32_t *flags_out, float *raw_out,
              int32_t *raw_meta_out, void *stream);
int mz_unroll_raw_floats(const mz_engine *e);
int mz_unroll_num_terms(void);

/* A match between two networks on the device games: B games in lock-step, every ply searched by the mover's own network.
 * Replaces the per-ply host loop a match driven from Python would need (two Evaluator._play_batch loops interleaved by
 * hand: per ply one engine call sequence and one host environment step); the host touches no game between plies.
 *
 * mz_match_create: a handle over two existing engines, network 0 and network 1, each with its own weights, its own
 * num_simulations and its own trees; the handle owns neither and is destroyed before them.  kind 1 TicTacToe or 3 Connect
 * Four.  Refused: kind 2 (CartPole) and any single-player engine; engines that differ in device, num_envs, obs_dim,
 * action_space, seed or env_id_offset.  Game b is the game with seed env_id_offset + b.  max_steps: a game is cut -- a draw
 * -- when its ply count reaches it; keep_history != 0: per-ply logs are kept ([B][cap], cap = min(max_steps, 9 / 42),
 * mz_match_log_capacity).
 *
 * mz_match_reset: every game back to the empty board, player +1 to move.  opening_plies in [0, max_steps): that many plies
 * are applied with no inference before the first searched ply -- ply p of game b is the min(floor(u * n), n - 1)-th of the
 * position's n legal actions, u from the counter RNG under MZ_RNG_OPEN keyed (engine seed, the game's seed, p, 0): the
 * game's seed alone, so both seatings of a seed open alike.  A game that ends inside its opening is over, with its result.
 * first_net 0 / 1: the network that moves at ply opening_plies; the other one moves next, and so on in turn.  Synchronous.
 *
 * mz_match_set_draws (after reset, before the first ply; parity runs): draws given by the caller instead of the counter
 * RNG, [dev] arrays the caller keeps alive until the games are over; any may be NULL.  walk [B][walk_plies] float64: the
 * uniform of mz_eval_walk; noise [B][noise_plies][A] float64: the Dirichlet draw at the legal positions -- both indexed by
 * the ply, opening plies counted; opening [B][opening_n] int32: the opening plies as indices into the legal actions of
 * their positions.  Plies past the given ones draw zeros.
 *
 * mz_match_plies: the opening (once), then n plies enqueued on the stream.  Ply p (opening plies counted) is network
 * first_net's when (p - opening_plies) is even, else the other's, and runs on that network's engine: observe (state -> obs
 * / legal / to_play; a finished game gets a zero observation, all actions legal, to_play +1) -> mz_initial_inference ->
 * mz_root_prepare with move counter p (noise_on: the given draw, or the device Dirichlet keyed by p) -> mode 0: mz_search
 * (the engine's num_simulations) + mz_eval_walk (one action, that side's temperature; device uniforms under MZ_RNG_EVAL
 * keyed by p) + mz_finalize, mode 1 / 2: mz_eval_lookahead (only_prior / only_value) -> apply (the mover network's
 * accumulators and logs, then exactly one action on the device rules).  mode, temperature, noise_on: [host] arrays of two,
 * per network.  With opening_plies 0, a match of a network against itself enqueues what mz_eval_env_moves without a random
 * opponent enqueues, with the same keys.  No host synchronisation between the plies; one 4-byte copy at the end returns
 * the number of games still live in *live_out [host].
 *
 * mz_match_results (synchronous, [host] arrays, any may be NULL): result [B] int8 for player +1, the game's first mover
 * (+1 win, 0 draw, -1 loss); length [B] int32; per network k = 0 / 1: n_searched [2][B] int32 (plies it searched), acc
 * [2][4][B] float64 (sums, added in ply order, of its predicted rewards, predicted values and root values, and the mean of
 * the lexicographic-maximum depth list), depth_max [2][B][S] int32 (that list; S = the larger num_simulations); the logs,
 * kept with keep_history, per ply [B][cap]: actions int32, mover int8 (+1 / -1, doubled on the ply the rules reported
 * done), net int8 (the network that moved, -1 on an opening ply), rewards float64, pred_rewards / pred_values float32,
 * root_values float64, child_visits [B][cap][A] float64, depths [B][cap][S] int32 (the mover's num_simulations entries;
 * [0] / [1] in modes 1 / 2).  The search entries of an opening ply are zero. */
typedef struct mz_match mz_match;
int mz_match_create(mz_engine *e0, mz_engine *e1, int kind, int max_steps, int keep_history, mz_match **out);
int mz_match_destroy(mz_match *m);
int mz_match_reset(mz_match *m, int first_net, int opening_plies, void *stream);
int mz_match_set_draws(mz_match *m, const double *walk, int walk_plies, const double *noise, int noise_plies,
                       const int32_t *opening, int opening_n, void *stream);
int mz_match_plies(mz_match *m, int n, const int *mode, const double *temperature, const int *noise_on, int *live_out,
                   void *stream);
int mz_match_results(mz_match *m, int8_t *result, int32_t *length, int32_t *n_searched, double *acc, int32_t *depth_max,
                     int32_t *actions, int8_t *mover, int8_t *net, double *rewards, float *pred_rewards, float *pred_values,
                     double *root_values, double *child_visits, int32_t *depths, void *stream);
int mz_match_log_capacity(const mz_match *m);

/* The true-rules search (DESIGN s7g; csrc/mz_truemodel.hip.h): MCTS.run with the same PUCT, MinMaxStats, tie rules and backup
 * as mz_search and the same weights, in which a node below the root is a REAL position of TicTacToe (kind 1) or Connect Four
 * (kind 3): reached by the device rules from its parent's position, evaluated by representation + prediction on its
 * observation in the mover's view, expanded over its legal actions only (an illegal child: prior 0, to_play 0), and closed
 * where the game ends -- reward 1 if the move into it won, else 0, value 0, no children.  A finished node takes an expansion
 * slot at its first visit; a later visit stops there and backs up again without expanding anything.  No dynamics network
 * runs and no hidden state is kept below the root.  The tree lies in the node pool as mz_search leaves it: mz_eval_walk (one
 * action), mz_finalize and mz_export_tree read it unchanged.  Evaluation only.
 *
 * mz_set_true_model: kind 0 off (the default), 1 or 3: the engine must have that game's shape; allocates the side state
 * (per expansion slot the position, its child mask, whether it is finished) on first use.  While it is set,
 * mz_eval_env_moves and mz_match_plies search with it on this engine (mode 0, one action per move); they refuse games of
 * another kind, CartPole, modes 1 / 2 and max_actions != 1.
 * mz_tm_root (after mz_root_prepare): [dev] boards [B][42] int8, turn [B] int8, step [B] int32 (plies played) are the roots'
 * positions; the first descent is made.
 * mz_tm_search: num_simulations x { leaf inference on the leaves' observations, expand + backup + the next descent }: two
 * launches per simulation, no host synchronisation.  The move's own root value and logits (mz_root_outputs) stay; hidden
 * slot 0 is overwritten.
 * The same loop opened up for outputs the caller computes (recorded ones in the parity tests):
 *   mz_tm_select        = the descent; outputs (either may be NULL): obs_out [dev][B][obs_dim] float32, the leaves'
 *                         observations (zeros where the leaf is finished), finished_out [dev][B] uint8
 *   mz_tm_expand_backup = expand + backup with value [dev][B], logits [dev][B][A] (ignored where the leaf is finished)
 *   mz_tm_expand_backup_select = both in one launch, then mz_tm_select's outputs; at a move's last simulation it is
 *                         mz_tm_expand_backup alone and the outputs are left untouched. */
int mz_set_true_model(mz_engine *e, int kind);
int mz_tm_root(mz_engine *e, const int8_t *boards, const int8_t *turn, const int32_t *step, void *stream);
int mz_tm_select(mz_engine *e, float *obs_out, uint8_t *finished_out, void *stream);
int mz_tm_expand_backup(mz_engine *e, const float *value, const float *logits, void *stream);
int mz_tm_expand_backup_select(mz_engine *e, const float *value, const float *logits, float *obs_out, uint8_t *finished_out,
                               void *stream);
int mz_tm_search(mz_engine *e, int num_simulations, void *stream);
/* mz_tm_search in ONE launch (DESIGN s7k; k_tm_search, csrc/mz_truemodel.hip.h): every workgroup alternates the leaf inference of
 * its 16 rows with the tree step of its 16 trees, num_simulations times.  The same preconditions, the same refusals in its own
 * name, the same effect on the step protocol (a pending descent is launched first if there is none; a descent is pending
 * afterwards unless the pool is used up) and bit-identical trees, slots, leaf observations and leaf flags. */
int mz_tm_search_fused(mz_engine *e, int num_simulations, void *stream);

/* The Gumbel MuZero search (DESIGN s7h; csrc/mz_gumbel.hip.h; Danihelka et al., ICLR 2022) beside mz_search, on the same
 * node pool, weights, expansion and backup: at the root, simulation s goes to the legal action with the largest
 * g(a) + logit(a) + sigma(a) among those visited seq(m, num_simulations)[s] times (Gumbel-top-m with sequential halving,
 * m = min(max_considered, legal actions)); below the root to arg-max pi'(a) - N(a) / (1 + sum N); the move's action is the
 * arg-max of g + logit + sigma among the most visited.  sigma(a) = (c_visit + max N) * c_scale * normalize(completedQ(a))
 * with the tree's MinMaxStats; pi' = softmax over the existing children of log P + sigma; g = gumbel_scale * G.  Every
 * arg-max breaks ties to the largest action.  Evaluation only.
 *
 * mz_set_gumbel: on 0 / 1; max_considered >= 2, c_visit >= 0, c_scale > 0, gumbel_scale >= 0 (0: no draw, deterministic).
 * Allocates the side state on first use.  Refused while the true-rules search is set, and mz_set_true_model while this is.
 * While it is set, mz_eval_env_moves and mz_match_plies search with it on this engine (mode 0, one action per move, no
 * exploration noise; G drawn on the device, keyed (seed, env id, move, action): a game's draws do not depend on its batch).
 * mz_gz_root (after mz_root_prepare WITHOUT noise; refused otherwise): gumbel [dev][B][A] float64 = G, or NULL: drawn on the
 * device with `move` in the key (nothing is drawn with gumbel_scale 0); makes the first descent.
 * mz_gz_search: num_simulations x { recurrent inference on the selected rows, expand + backup + the next descent }: two
 * launches per simulation, no host synchronisation.
 * The same loop opened up for outputs the caller computes:
 *   mz_gz_select        = the descent; outputs (either may be NULL): parent_slot, action [dev][B] int32 (mz_gather_hidden
 *                         gives the parents' hidden states)
 *   mz_gz_expand_backup = expand + backup with value, reward [dev][B], logits [dev][B][A], hidden [dev][B][50] or NULL (the
 *                         caller has stored it)
 *   mz_gz_expand_backup_select = both in one launch, then mz_gz_select's outputs; at a move's last simulation it is
 *                         mz_gz_expand_backup alone and the outputs are left untouched.
 * mz_gz_pick (any output may be NULL): action [dev][B] int32, pred_reward [dev][B] float32 (the chosen child's reward),
 * improved_policy [dev][B][A] float64 (pi' of the root, 0 on illegal actions), v_mix [dev][B] float64.  mz_finalize still
 * gives the visit fractions and the root's mean value. */
int mz_set_gumbel(mz_engine *e, int on, int max_considered, double c_visit, double c_scale, double gumbel_scale);
int mz_gz_root(mz_engine *e, const double *gumbel, uint64_t move, void *stream);
int mz_gz_select(mz_engine *e, int32_t *parent_slot, int32_t *action, void *stream);
int mz_gz_expand_backup(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                        void *stream);
int mz_gz_expand_backup_select(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                               int32_t *parent_slot, int32_t *action, void *stream);
int mz_gz_search(mz_engine *e, int num_simulations, void *stream);
int mz_gz_pick(mz_engine *e, int32_t *action, float *pred_reward, double *improved_policy, double *v_mix, void *stream);

/* The self-play loop searches its moves in ONE mode (DESIGN s7l): PUCT on the learned model (the default), or one of the two
 * below.  Switching one on while the other is on is refused; switching one off while the other is on succeeds and leaves the
 * other on.  While a mode is on, the entry points named below refuse with one sentence that names the mode and the call that
 * switches it off. */

/* Self-play with the Gumbel search (DESIGN s7i; csrc/mz_gumbel_selfplay.hip.h).  While on, a move of mz_selfplay_steps /
 * mz_selfplay_steps_into on a device game (mz_selfplay_set_env 1, 2, 3) is: observe, initial inference, the root WITHOUT
 * exploration noise, mz_gz_root with G drawn on the device -- keyed (seed, env_id_offset + b, the environment's move counter,
 * action): the counter that keys the Dirichlet draw of a PUCT move, so a record does not depend on its batch --, all
 * num_simulations of mz_gz_search, and one end-of-move launch.  The record keeps its layout: the child_visits slots hold
 * (float)pi'(a) of the root (exactly 0 on illegal actions), action is the pick of mz_gz_pick, root_value the root's mean value
 * (value_kind 0) or its v_mix (value_kind 1), error = root_value - the initial inference's value.  The visit-softmax
 * temperature plays no part; exploration comes from mz_set_gumbel's gumbel_scale (1 for training).
 * The moves run in the launch-per-step form, up to 16 per hipGraph: mz_selfplay_moves_per_launch returns 0 while on.
 * Needs mz_set_gumbel on this engine and a game environment; refused with host-given draws (mz_selfplay_set_draws), with an
 * mz_sim_io mode, and while moves wait in the device ring.  While on, mz_set_gumbel(e, 0, ..), mz_selfplay_set_draws,
 * mz_selfplay_set_env, mz_sim_io modes and mz_selfplay_steps_timed are refused.  on 0: the loop runs again as it did before. */
int mz_selfplay_set_gumbel(mz_engine *e, int on, int value_kind);

/* Self-play on the true rules (DESIGN s7k).  While on, a move of mz_selfplay_steps / mz_selfplay_steps_into on a device board
 * game (mz_selfplay_set_env 1 or 3) is a PUCT move -- observe, initial inference, the Dirichlet draw keyed by the environment's
 * move counter, the root with that noise, the PUCT move's end with its temperature, sampling uniform, error and reset on done --
 * whose search is the true-rules search: the root's position is taken from the environment on the device, then num_simulations
 * of mz_tm_search_fused (fused != 0: one launch) or of mz_tm_search (fused 0: two launches per simulation); both give the same
 * records.  The record keeps its layout; only what a node below the root is differs.
 * The moves run in the launch-per-step form, up to 16 per hipGraph: mz_selfplay_moves_per_launch returns 0 while on.
 * Needs mz_set_true_model with the environment's kind; refused in the Gumbel self-play mode, with host-given draws
 * (mz_selfplay_set_draws), with an mz_sim_io mode, and while moves wait in the device ring.  While on, mz_set_true_model to
 * another kind, mz_selfplay_set_draws, mz_selfplay_set_env, mz_selfplay_set_gumbel, mz_sim_io modes and mz_selfplay_steps_timed
 * are refused.  Switching synchronises and drops the captured graphs; on 0: the loop runs again as it did before. */
int mz_selfplay_set_true_model(mz_engine *e, int on, int fused);

/* MuZero Reanalyse: stored positions of the replay searched again under the engine's CURRENT weights.  rows_host [host, pinned]
 * is [n_rows][rec_floats] record rows as mzr_reanalyse_pick (include/mz_replay.h) wrote them, rec_floats = obs_dim + action_space
 * + MZ_REC_EXTRA; fresh_host [host, pinned] receives [n_rows][action_space + 2] floats per row: child_visits as float32 (the
 * float32 of the float64 N[a] / sum N that mz_finalize returns, 0 at illegal actions), then the root's value, the float64 of
 * mz_finalize, in two float slots -- what mzr_reanalyse_write takes.  Per chunk of num_envs rows the call enqueues: the rows'
 * observation, to_play (bit 1 of the flags word) and legal actions read straight from the pinned rows; mz_initial_inference;
 * mz_root_prepare WITHOUT exploration noise; mz_search(num_simulations); the store into fresh_host.  No host synchronisation
 * between chunks, one at the end; the engine's self-play, evaluation and match states are untouched (a state of its own,
 * allocated on the first call, which therefore synchronises).  Rows past n_rows in the last chunk are searched as empty
 * positions and nothing is stored for them.
 * kind, as in mz_selfplay_set_env, says how the legal actions follow from the observation: 0 synthetic and 2 CartPole: all;
 * 1 TicTacToe: cell k iff obs[k] == 0; 3 Connect Four: column c iff obs[35 + c] == 0.
 * Refused: weights not set; another rec_floats; kind outside 0..3 or not the engine's shape; n_rows < 0; num_simulations outside
 * 1 .. the engine's; buffers that are not page-locked. */
int mz_reanalyse(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                 int num_simulations, void *stream);

/* Reanalyse with the Gumbel search (DESIGN s7j), for a replay whose records come from mz_selfplay_set_gumbel: mz_reanalyse's
 * buffers, layouts, pinned-memory requirement, kinds and chunks, but each chunk is searched as a self-play move of that mode is
 * -- observe, mz_initial_inference, the root WITHOUT noise (and without the first PUCT descent), the Gumbel root, the
 * mz_gz_search loop for num_simulations -- and fresh_host receives per row the root's improved policy pi' as float32 (exactly 0
 * at illegal actions) where mz_reanalyse puts the visit shares, then a float64 in two float slots: the root's mean value
 * (value_kind 0) or its v_mix (value_kind 1), the rule of mz_selfplay_set_gumbel's records.  mz_set_gumbel's parameters are
 * the search's; with gumbel_scale 0 nothing is drawn and the pass is deterministic.  Otherwise the Gumbel draws of a row are
 * keyed (engine seed, the row's index within the pass, draw_key, action): the row, not the tree that searched it, so a pass does
 * not depend on num_envs, and a caller that passes another draw_key per pass gets other draws.  One synchronisation at the end;
 * afterwards the engine's stepwise state is what mz_gz_search leaves after num_simulations on the last chunk.
 * Refused: everything mz_reanalyse refuses; no Gumbel search set (mz_set_gumbel); value_kind other than 0 or 1. */
int mz_reanalyse_gumbel(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                        int num_simulations, int value_kind, uint64_t draw_key, void *stream);

/* Reanalyse on the true rules (DESIGN s7n), for the two board games (kind 1 TicTacToe, 3 Connect Four): mz_reanalyse's buffers,
 * layouts, pinned-memory requirement and chunks, and what it stores -- visit shares and the root's mean value, the fields of a
 * record of mz_selfplay_set_true_model --, but each chunk is searched as a self-play move of that mode is: observe,
 * mz_initial_inference, the root WITHOUT noise, slot 0 of the true-rules tree from the stored row itself, then num_simulations
 * of the true-rules search, in one launch (fused != 0, mz_tm_search_fused's kernel) or in the two-launch loop (mz_tm_search's).
 * The root's position follows from the row alone: both games store mover * board, so board = to_play * observation with to_play
 * from bit 1 of the flags word, and the plies played are the stones on it.  The two forms give the same bits, and the same as
 * mz_root_prepare / mz_tm_root / mz_tm_search on those boards.  One synchronisation at the end; afterwards the engine's
 * stepwise state is what mz_tm_search leaves after num_simulations on the last chunk.  A row must hold a live position (as for
 * mz_reanalyse: not checked).
 * Refused: weights not set; no true-rules search set (mz_set_true_model); kind other than 1 or 3 or other than the search's
 * game; another rec_floats; n_rows < 0; num_simulations outside 1 .. the engine's; buffers that are not page-locked. */
int mz_reanalyse_true_model(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                            int num_simulations, int fused, void *stream);

/* Raw tree dump (Node objects of mcts.py:28-45 in SoA form) to [host] arrays, synchronous.
 * Each per-node array is [B][NN]; minmax [B][2]; legal_mask [B] (bit a = root child a exists);
 * noise [B][A] (the Dirichlet draw last mixed in).  Any pointer may be NULL. */
int mz_export_tree(mz_engine *e, int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP,
                   uint32_t *legal_mask, double *minmax, double *noise, float *hidden_pool);

/* Epilogue of a residual block of the conv networks in GPU inference (reference networks.py:393-410: BatchNorm2d in eval
 * mode, the skip connection, ReLU), for the torch-network path (BASELINE configs[4]; the convolutions themselves stay
 * MIOpen's): in place over a contiguous NCHW float32 tensor y [dev][n] = [N][channels][hw], hw % 4 == 0,
 *   y = relu(y * scale[c] + shift[c] (+ residual)),   scale = weight / sqrt(running_var + eps), shift = bias - mean * scale
 * (scale, shift [dev][channels]; residual [dev][n] or NULL).  One pass instead of PyTorch's 2-3 elementwise kernels. */
int mz_affine_relu(float *y, const float *scale, const float *shift, const float *residual, size_t n, int channels,
                   int hw, void *stream);

/* Introspection for tests/bench. */
int mz_nodes_per_tree(const mz_engine *e);
int mz_padded_envs(const mz_engine *e);

/* ---- on-device self-play loop (actors.py:126-176 for B synthetic fixed-length envs) ----------
 * Synthetic env (gym/ALE are not installed on either box): observation
 * obs_t[i] = Irwin-Hall(4) approximation of N(0,1) from Philox4x32-10 keyed (seed, env, episode, t),
 * reward_t = U(-1,1) keyed likewise, all actions legal, done at t == episode_len.
 * (mz_selfplay_set_obs: byte-valued observations and --norm_obs for the -ram- shapes.)
 * mz_selfplay_steps runs `moves` complete moves: obs -> initial inference -> root -> search ->
 * select_action -> env.step -> experience record appended to a device ring.
 * Each record is rec_floats() = MZ_REC_FLOATS(obs_dim, action_space, packed) float32 slots, laid out as mz_record.h states.
 * mz_selfplay_drain copies the records produced since the last drain into `out` [host, pinned
 * preferred] asynchronously on `stream` and returns their count through *n_records after the
 * stream is synchronised by the caller (records are laid out move-major: [moves][B]).  `stream` may be a
 * copy stream other than the one mz_selfplay_steps ran on, provided the caller orders it behind those steps
 * (event): later moves then overlap the copy.  The ring normally keeps them in different slots; where it cannot
 * (records so large that the ring holds few moves), mz_selfplay_steps makes its stream wait for the event the
 * drain recorded behind its copy before it launches moves into slots the copy may still be reading.
 * mz_selfplay_steps plays up to 16 moves per launch: single-player games with their trees in LDS run as whole moves
 * inside ONE launch of the search kernel (root, simulations and end of every move; no launch, no grid-wide drain and
 * no weight reload between moves); every other configuration as one hipGraph of 2 kernels per move (root, search +
 * end of move).  Both produce the same records bit for bit (MZ_NO_PERSIST=1 at mz_create selects the graph).
 * stagger != 0: env i starts its first episode at t0 = hash(env id) % episode_len (uniform episode ends).
 * temperature: Config.visit_softmax_temperature at reset; mz_selfplay_set_temperature changes what every env's
 * NEXT game starts with (actors.py:128-129: evaluated once per game), games in progress keep theirs. */
int mz_selfplay_reset(mz_engine *e, int episode_len, double temperature, int stagger, void *stream);
int mz_selfplay_set_temperature(mz_engine *e, double temperature, void *stream);
/* The move counter of every environment (Actor's count of moves played, actors.py:87-124: keys the device RNG by (seed, env, move)
 * and places the experience records).  For a caller that wants a resumed run to continue its count instead of replaying the random
 * stream of its first moves (the reference reseeds on resume: Actor.load_state does not call this), and for the tests, which start
 * close to 2^30 and 2^32.  The device ring must be drained; synchronous. */
int mz_selfplay_set_moves(mz_engine *e, unsigned long long moves);
/* The environment the loop plays (call before mz_selfplay_reset).  0 (default): the synthetic fixed-length episodes above.
 * 1: TicTacToe with the reference's rules (custom_environments/tic_tac_toe.py:5-76: observation turn * board, legal =
 * empty cells, reward 1 for the winning move, done on a win or after nine moves, players alternate) entirely on the device;
 * needs obs_dim 9, action_space 9, two_players.  mz_selfplay_reset's episode_len / stagger are ignored (real games).
 * 2: CartPole (envs.CartPole, the definition of CartPole-v1 / -v0 here: float64 state (x, x_dot, theta, theta_dot), Euler
 * step of 0.02 s with sin / cos as fixed polynomials so that host and device agree bit for bit, observation = the state as
 * float32, reward 1 per step, done outside |x| <= 2.4, |theta| <= 12 degrees or when the step count reaches the time limit)
 * entirely on the device; needs obs_dim 4, action_space 2 and a single player.  mz_selfplay_reset's episode_len is the time
 * limit (500 / 200); every environment starts episode 0 at step 0 (stagger is ignored), episode k of environment i from the
 * counter-RNG state mz_cartpole_reset_state(i, k) (mz_engine_debug.h).  With the exact-f32 kernel the moves run inside the
 * whole-moves launch (the state lives in LDS across its moves); with split_f16 or MZ_NO_PERSIST as one launch per step of a
 * move.  --norm_obs and byte observations (mz_selfplay_set_obs) are refused for it.
 * 3: Connect Four (envs.ConnectFour, the definition here: 6 rows of 7 columns, cell 7 * row + col with row 0 at the bottom,
 * an action is a column and the stone lands on its lowest empty cell, observation turn * board, legal = the columns whose
 * top cell is empty, reward 1 for the move that makes a line of four, done on such a line or a full board, players
 * alternate) entirely on the device; needs obs_dim 42, action_space 7, two_players.  mz_selfplay_reset's episode_len /
 * stagger are ignored (real games).  With the exact-f32 kernel and 1..48 simulations the moves run inside the whole-moves
 * launch; otherwise, with split_f16 or MZ_NO_PERSIST as one launch per step of a move.  --norm_obs, byte observations and
 * packed records (mz_selfplay_set_obs) are refused for it.
 * mz_selfplay_set_draws (TicTacToe only): the Dirichlet draw (noise [dev][B][A] float64 at the legal positions,
 * mcts.py:59) and / or the uniform of select_action (uniform [dev][B] float64, config.py:77) of the following moves come
 * from the caller -- numpy's stream in the reference's order -- instead of the device RNG; NULL, NULL switches back. */
int mz_selfplay_set_env(mz_engine *e, int kind);
int mz_selfplay_set_draws(mz_engine *e, const double *noise, const double *uniform, void *stream);
/* Observation format of the synthetic env (call before mz_selfplay_reset, with the ring drained; synchronous).  uint8_obs
 * 1: observations are bytes 0..255 (the -ram- envs), one per float slot of the record; 2: the same observations, and the
 * record carries them as BYTES, four per float slot -- rec_floats = ceil(obs_dim / 4) + action_space + MZ_REC_EXTRA
 * (mz_selfplay_rec_floats), the layout mz_replay.h's obs_u8 replay ingests (game.py:93-96 keeps the raw uint8 observation):
 * 208 instead of 592 bytes per env-step on the Pong-ram shapes.  obs_min / obs_range [host][obs_dim], both or neither: --norm_obs
 * (actors.py:55-58,134-137): the network input is (obs - obs_min) / obs_range in float32, the record keeps the raw
 * observation (the learner normalises its own batches, learners.py:167-168). */
int mz_selfplay_set_obs(mz_engine *e, int uint8_obs, const float *obs_min, const float *obs_range);
/* The elementwise ends of the learner step (reference learners.py:164-230) as single launches -- the step is launch-bound,
 * and PyTorch spells these as ~45 (targets) and ~11 (each categorical loss) tiny kernels.  Engine-free: device pointers,
 * sizes, a stream; capturable into a graph (no synchronisation, no allocation).
 * mz_learner_targets (learners.py:176-189; config.py:27-33,51-68): t_val, t_rew [bs][k1] as sample_batch returns them (k1 = K
 *   + 1 unroll positions), value0 [bs][sv] the value logits of the initial inference ->  sup_val [k1][bs][sv], sup_rew
 *   [k1][bs][sr]: two-hot supports of h(target) (h skipped with no_target_transform), position-major; new_errors [bs] =
 *   inverse_transform(value0) - t_val[:, 0], the priority refresh.
 * mz_soft_ce_forward / _backward (utils.py:53-60, summed over the unroll positions as learners.py:191-203 does): logits
 *   [positions][bs][bins], target element (p, b, s) at target[p * target_pos_stride + b * target_row_stride + s] -> loss [bs]
 *   = sum_p sum_s -target log_softmax(logits); backward: grad_logits = grad_loss[b] (softmax(logits) sum_s target - target). */
int mz_learner_targets(const float *t_val, const float *t_rew, const float *value0, int bs, int k1, int sv, int vmin, int sr,
                       int rmin, int no_target_transform, float *sup_val, float *sup_rew, float *new_errors, void *stream);
int mz_soft_ce_forward(const float *logits, const float *target, int positions, int bs, int bins, int64_t target_pos_stride,
                       int64_t target_row_stride, float *loss, void *stream);
int mz_soft_ce_backward(const float *logits, const float *target, const float *grad_loss, int positions, int bs, int bins,
                        int64_t target_pos_stride, int64_t target_row_stride, float *grad_logits, void *stream);
/* ---- The FCNetwork learner step as two launches at batches up to 256 (four at 512, five to six above or with gradient clipping; csrc/mz_fcl.hip.h): reference learners.py:164-230 (update_weights: K-step
 * unroll, categorical targets, soft cross-entropy, gradient hooks 0.5 and 1 / K, importance weights, clip_grad_norm_,
 * optimizer.step) with networks.py:135-180 (FCNetwork), config.py:27-33,51-68, utils.py:53-60,73-83 (Adam / AdamW,
 * eps 1.5e-4).  No GEMM library, no autograd tape: forward chain, heads + losses + their backward, backward chain, weight
 * gradients (deterministic: no atomics), gradient norm, optimiser.  Every pointer below is a DEVICE pointer unless it says
 * host; nothing synchronises or allocates after mz_fcl_create, so a step can be captured into a graph.
 * mz_fcl_create: batch (a multiple of 16), unroll steps K (1..7), FCNetwork sizes (observations <= 1024
 *   features, actions <= 14, supports <= 64 bins).
 * mz_fcl_bind: the flat float32 parameter vector (engine.WEIGHT_ORDER = mz_set_weights' order, mz_fcl_num_params
 *   floats), Adam's exp_avg / exp_avg_sq of the same shape, `nsteps` float32 step counters (torch keeps one per parameter:
 *   all are incremented, the first is read) and the learning rate as a device float; builds the packed weight copies.
 * mz_fcl_repack: after anything else wrote the parameter vector (load_state_dict).
 * mz_fcl_step: obs [batch][obs_dim] (normalised), actions int64 or int32 [batch][K], target_rewards / target_values [batch][K + 1],
 *   target_policies [batch][K + 1][actions], is_weights [batch] (float64 or float32) as replay_buffer.sample_batch returns
 *   them -> the parameters, optimiser state and step counters updated in place (unless no_update: gradients only),
 *   new_errors [batch] = inverse_transform(value_0) - target_values[:, 0] (the priority refresh, learners.py:181-182),
 *   loss_sums float64 [3] += the weighted means of the reward, value and policy losses (learners.py:228-230).
 * mz_fcl_read_grad: the last step's gradient (after the sum over positions, before clipping) into a HOST buffer; waits. */
typedef struct mz_fcl mz_fcl;
int mz_fcl_create(int batch, int unroll_steps, int obs_dim, int action_space, int value_support_min, int value_support_max,
                  int reward_support_min, int reward_support_max, int no_target_transform, mz_fcl **out);
int mz_fcl_destroy(mz_fcl *c);
size_t mz_fcl_num_params(mz_fcl *c);
int mz_fcl_bind(mz_fcl *c, float *params, float *exp_avg, float *exp_avg_sq, float *steps, int nsteps, const float *lr,
                void *stream);
int mz_fcl_repack(mz_fcl *c, void *stream);
/* mz_fcl_set_optimizer: which optimiser the steps of this handle run (utils.py:73-83).  kind 0 = Adam / AdamW (the default: a
 *   handle that never calls this steps as before; the steps' beta1, beta2 and adamw apply), 1 = SGD (torch.optim.SGD: dampening
 *   0, no Nesterov), 2 = RMSprop (torch.optim.RMSprop: not centred, smoothing constant alpha).  For kinds 1 and 2 the steps' eps,
 *   weight_decay and clip_grad apply and beta1, beta2, adamw are ignored; mz_fcl_bind's exp_avg holds the momentum buffer (not read
 *   or written with momentum 0), exp_avg_sq RMSprop's square_avg (SGD: not touched); the step counters advance as for Adam.
 *   Refuses an unknown kind, momentum < 0 and alpha outside [0, 1) (mz_last_error). */
int mz_fcl_set_optimizer(mz_fcl *c, int kind, double momentum, double alpha);
/* mz_fcl_set_scalar_loss: the loss family of the value and reward heads (utils.py:61-70, learners.py:182-206).  kind 0 = categorical
 *   (the default: soft cross-entropy against the two-hot target), 1 = MSE (torch.nn.MSELoss), 2 = Huber (torch.nn.SmoothL1Loss,
 *   beta 1), both reduction 'none': the reference's --no_support, where each of the two heads ends in ONE output trained against
 *   the scalar target (transformed unless no_target_transform, never clamped) and the priority refresh is that raw output minus the
 *   first value target.  The policy head stays categorical.  Kinds 1 and 2 need a handle created with value_support_min ==
 *   value_support_max and reward_support_min == reward_support_max (one output per head); without this call such a handle is a
 *   categorical one with one bin.  The kind holds for every later mz_fcl_step, mz_fcl_update and mz_fcl_run.  Refuses a null handle,
 *   an unknown kind and kinds 1 / 2 on a handle with wider supports (mz_last_error). */
int mz_fcl_set_scalar_loss(mz_fcl *c, int kind);
/* mz_fcl_set_symmetry: board-symmetry augmentation of every later update's batch (DESIGN s7e).  kind as mz_game_kind: 0 = off (the
 *   default), 1 = TicTacToe (8 images: g = 4 f + q, q quarter turns (r, c) -> (c, 2 - r), then the mirror (r, c) -> (r, 2 - c) if f),
 *   3 = Connect Four (2 images: g = 1 maps col -> 6 - col).  Sample b of the handle's update number u is replaced by its image
 *   under g = philox(seed, u, b).x & (n - 1): the observation's cells, the K unrolled actions (padded ones included, dtype kept) and
 *   the K + 1 policy targets move together, everything else is left alone.  One extra launch ahead of the step on its stream, into a
 *   device buffer of the handle; the caller's arrays are not written.  u starts at first_update (a resumed run passes its training
 *   step) and advances by one with every mz_fcl_step without no_update, mz_fcl_update and update of mz_fcl_run; a step with
 *   no_update set is neither transformed nor counted.  Refuses an unknown kind and a handle whose obs_dim / action_space are not the
 *   game's (9 / 9, 42 / 7) (mz_last_error); with a kind set, mz_fcl_run refuses MZ_FCL_RUN_GRAPH=1. */
int mz_fcl_set_symmetry(mz_fcl *c, int kind, uint64_t seed, uint32_t first_update);
int mz_fcl_step(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards, const float *target_values,
                const float *target_policies, const void *is_weights, int weights_are_f64, double beta1, double beta2, double eps,
                double weight_decay, double clip_grad, int adamw, int no_update, float *new_errors, double *loss_sums, void *stream);
/* mz_fcl_update: mz_fcl_step from HOST arrays (what replay_buffer.sample_batch returns, learners.py:165-180): staged through
 * pinned memory (two slots), one host-to-device copy, the step, the new errors copied back -- nothing is waited for except
 * the slot's own use mz_fcl_slots() updates ago (6 staging slots).  mz_fcl_errors(slot): the new errors of that update into host_out [batch], waiting for
 * their copy (the priority refresh goes to the replay one update behind, as the reference's fire-and-forget refresh does). */
int mz_fcl_update(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards,
                  const float *target_values, const float *target_policies, const void *is_weights, int weights_are_f64, double beta1,
                  double beta2, double eps, double weight_decay, double clip_grad, int adamw, double *loss_sums, void *stream,
                  int *slot_out);
int mz_fcl_errors(mz_fcl *c, int slot, float *host_out);
/* Learner.learn's loop body in native code (learners.py:115-131: sample_batch -> update_weights -> replay_buffer.update),
 * n_updates training steps per call: Python only at the boundaries where the reference's loop does something else
 * (send_weights, save_state, logging; learners.py:132-153).  The replay is reached through the caller's function table
 * (include/mz_replay.h: sample = mzr_sample_batches_full, refresh = mzr_update_errors_f32, last_error = mzr_last_error;
 * libmz_hip.so does not link libmz_replay.so).  words [n_updates][2 batch]: the generator words of the stratified draws
 * (random.getrandbits(64 batch n_updates), least significant word first) -- or NULL with py_key [624] / *py_pos = the state of
 * Python's `random` generator (random.getstate()[1]), from which the same words are generated per update and which comes back
 * advanced; np_key [624] / *np_pos: numpy's legacy generator
 * state for the padded actions, advanced in place; *beta_inout: the replay's beta (schedule applied per batch); obs_min /
 * obs_range [host][obs_dim] or NULL: --norm_obs; lrs [host][n_updates] or NULL: the learning rate of every update (a
 * scheduler's values; NULL: the device float bound by mz_fcl_bind); loss_sums [dev][3] as mz_fcl_step; *pads_out (may be
 * NULL): padded actions drawn.  Batch i is sampled while update i - 1 runs on the GPU; the refresh of update i reaches the
 * replay before batch i + 2 is drawn (the reference's own lag is up to batches_per_fetch = 15 batches, learners.py:124).
 * Returns with the last (up to mz_fcl_slots() - 1) updates still in flight: the next call hands their refreshes over as their staging slots come
 * up; n_updates = 0 flushes -- waits for them and hands the refreshes over (before anything else touches the replay's
 * priorities or this handle's staging: mz_fcl_update, a checkpoint, the end of Learner.learn). */
typedef struct mz_fcl_source {
  void *replay;
  int (*sample)(void *replay, const uint32_t *words, int n, int bs, float *obs, int32_t *actions, float *target_rewards,
                float *target_values, float *target_policies, int64_t *idxs, double *is_weights, uint32_t *np_key, int32_t *np_pos,
                double *beta_inout, int64_t *pads_out, uint32_t *py_key, int32_t *py_pos);
  int (*refresh)(void *replay, const int64_t *idxs, const float *errors, int64_t n);
  const char *(*last_error)(void);
} mz_fcl_source;
int mz_fcl_run(mz_fcl *c, const mz_fcl_source *src, int n_updates, const uint32_t *words, uint32_t *np_key, int32_t *np_pos,
               double *beta_inout, const float *obs_min, const float *obs_range, double beta1, double beta2, double eps,
               double weight_decay, double clip_grad, int adamw, const float *lrs, double *loss_sums, void *stream,
               int64_t *pads_out, uint32_t *py_key, int32_t *py_pos);
/* staging slots of this handle: how many updates mz_fcl_update / mz_fcl_run keep in flight before they wait for the oldest */
int mz_fcl_slots(mz_fcl *c);
int mz_selfplay_steps(mz_engine *e, int moves, void *stream);
/* mz_selfplay_steps with the records written straight into host_records [host, PAGE-LOCKED: hipHostMalloc /
 * torch pin_memory][moves][B][rec_floats] by the kernels' own stores through the buffer's device mapping (0.6 GB/s of
 * posted PCIe writes at the benched rate), instead of the device ring + mz_selfplay_drain's D2H copy.  The buffer is
 * complete once work enqueued on `stream` behind this call has completed (event / synchronise); it must stay untouched
 * until then.  The device ring must hold no undrained moves; these moves count as drained.  This is the hand-off
 * Actor.run_selfplay uses (actors.py:160-169's history hand-off): no copy stream, no cross-stream dependency for the
 * runtime to track -- that dependency kept a runtime thread of every rank spinning (profiles/r05_host_threads.txt).
 * Fails when host_records is not page-locked. */
int mz_selfplay_steps_into(mz_engine *e, int moves, float *host_records, void *stream);
/* 16 where mz_selfplay_steps plays whole moves inside one launch of the search kernel (at most that many per launch),
 * 0 where a move is a hipGraph node pair (root kernel, search kernel). */
int mz_selfplay_moves_per_launch(const mz_engine *e);
int mz_selfplay_rec_floats(const mz_engine *e);
int mz_selfplay_ring_moves(const mz_engine *e);
int mz_selfplay_drain(mz_engine *e, float *out, int max_moves, int *n_moves, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MZ_ENGINE_H */
