/* mz_engine_debug.h -- instrumentation, profiling and test hooks of libmz_hip.so.  NOT part of the drop-in boundary
 * (include/mz_engine.h is what a maintainer binds): these entry points exist for the parity tests (tests/), the benchmark's clocks
 * (bench.py: HIP events on the kernels' own dispatches) and kernel development (scripts/).  Same conventions as mz_engine.h: plain
 * C, int return codes + mz_last_error(), [dev] / [host] say where a pointer lives. */
#ifndef MZ_ENGINE_DEBUG_H
#define MZ_ENGINE_DEBUG_H
#include "mz_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic twin of mz_search (call right after mz_root_prepare): the same launches, eagerly, with a
 * hipEvent between every pair of launches on `stream`; synchronous.  ms_out[0] = summed time of the
 * num_simulations recurrent-inference launches, ms_out[1] = summed time of the tree-step launches. */
int mz_search_profiled(mz_engine *e, int num_simulations, float *ms_out, void *stream);

/* mz_search with HIP events bracketing the dispatch of the fused search kernel itself (hipExtLaunchKernelGGL start /
 * stop events on `stream`, the same timestamps rocprofv3's kernel trace reports); call right after mz_root_prepare;
 * synchronous.  ms_out[0] = duration of the launch in milliseconds.  bench.py's roofline figure comes from here. */
int mz_search_timed(mz_engine *e, int num_simulations, float *ms_out, void *stream);

/* Diagnostic build of the fused search kernel with in-kernel s_memtime stamps (never used for timing
 * claims): cycles_out [host][4 waves][14 phases] = per-wave cycle totals over num_simulations, averaged
 * over workgroups.  Phases: 0 gather, 1 barrier, 2 dynamics fc1, 3 dynamics fc2, 4 combine, 5 LN/reward,
 * 6 store + prediction fc1, 7 prediction fc2, 8 combine, 9 value/logits, 10 expand, 11 backup, 12 descent, 13 rest of the tree step. */
int mz_search_phase_profile(mz_engine *e, int num_simulations, unsigned long long *cycles_out, void *stream);

/* of the last mz_search_phase_profile: out3 [host] = mean, minimum, maximum over the workgroups of a workgroup's total
 * cycles (the launch lasts as long as its slowest workgroup) */
int mz_search_phase_spread(const mz_engine *e, double *out3);

/* One simulation's tree work with a clock on each kernel: mz_select (no outputs) + mz_expand_backup (no hidden state),
 * hipExtLaunchKernelGGL start / stop events around each of the two dispatches (the timestamps rocprofv3's kernel trace
 * reports); synchronous.  ms_out [host][2] = duration of k_tree_select (-1 where the descent was already pending: the
 * first simulation after mz_root_prepare, which selects inside the root kernel), of k_tree_expand_backup, in milliseconds.
 * The roofline clock of `bench.py --workload tree` (the tree kernels against HBM / cache bandwidth). */
int mz_tree_pair_timed(mz_engine *e, const float *value, const float *reward, const float *logits, float *ms_out,
                       void *stream);

/* keep != 0: every move of the self-play loop also writes its searched tree back to the node pool (so that
 * mz_export_tree after mz_selfplay_steps shows the last move's tree).  Default 0: the loop never reads it. */
int mz_selfplay_export_trees(mz_engine *e, int keep);

/* keep != 0: every move also stores its Dirichlet draw (mcts.py:59; drawn on the device in this loop) in a per-move log
 * as long as the experience ring; mz_selfplay_read_noise copies the draw of move `move` (0 = first move after
 * mz_selfplay_reset, one of the last ring_moves moves) to out [host][B][A] float64, synchronously.  Test
 * instrumentation: any move of a whole-moves launch can be replayed on the CPU by the parity tests with the device's own draw
 * and the observation its record carries. */
int mz_selfplay_noise_log(mz_engine *e, int keep);
int mz_selfplay_read_noise(mz_engine *e, uint64_t move, double *out);

/* Test instrumentation of the fused search kernels' TREE code (the launch mz_search and mz_selfplay_steps run; the
 * stand-alone kernels get their network outputs through mz_expand_backup anyway).  The tree step of a simulation --
 * Node.expand, MCTS.backpropagate, the next select_child descent: mcts.py:47-55,83-92,104-143 -- consumes exactly three
 * things from the network: the value and reward scalars (networks.py:153-154,161-162) and the A policy logits.
 * buf [dev][keep_moves][num_envs][num_simulations + 1][2 + A] float32 is the caller's and must outlive the mode.
 *   mode 1, log:    every simulation s of every tree stores (value, reward, logits[A]) in slot 1 + s of row
 *                   (move % keep_moves, tree); the root of a self-play move stores (value, 0, logits[A]) in slot 0;
 *                   mz_search uses row 0.  The parity tests replay the logged outputs through the CPU oracle's tree and
 *                   demand every tree identical -- no network evaluation on the checker's side, hence no tie margin.
 *   mode 2, inject: mz_search's simulations READ slot 1 + s (row 0, keep_moves = 1) instead of their own network
 *                   outputs: the reference's recorded outputs (tests/golden) reach the fused kernels' own tree code.
 *   mode 0, off:    the production state (a null pointer in the kernels' arguments; buf ignored).
 * Synchronous; drops captured graphs. */
int mz_sim_io(mz_engine *e, int mode, float *buf, int keep_moves);

/* development hook: mz_fcl_run's host time since the handle was created (or the last reset): out [host][6] = seconds waiting for
 * a staging slot's previous update, in priority refreshes, in sampling, in launching, in the calls as a whole; number of updates */
int mz_fcl_run_stats(mz_fcl *c, double *out6, int reset);

/* test hook: the assembled gradient of the last mz_fcl_step (flat, engine.WEIGHT_ORDER) into a HOST buffer; waits for the device */
int mz_fcl_read_grad(mz_fcl *c, float *host_out, size_t n);

/* test hook: tape `which` of the last step into a HOST buffer (0 chain inputs, 1 chain fc1 activations, 2 LayerNorm x-hat, 3 rstd,
 * 4 hidden states, 5 / 6 chain deltas, 7 head fc1 activations, 8 / 9 head deltas, 10 d loss / d hidden state per head, 11 per-sample
 * losses; [position][row / 16][feature][16 rows] each, heads [head][position]...); host_out null: returns the float count. */
long long mz_fcl_read_tape(mz_fcl *c, int which, float *host_out, size_t n);

/* test hooks: the plan of a learner step (csrc/mz_fcl_plan.inc) as integers.  the host variant: no handle, no device -- the plan of the
 * handle that create would make for this shape (value_bins / reward_bins: the supports' sizes) on a device of `cus` compute units under
 * the knobs knobs5 [host] = what the variables MZ_FCL_GROUPS, MZ_FCL_SLABS (their integer), MZ_FCL_FUSE_FWD, MZ_FCL_FUSE_FB,
 * MZ_FCL_FB_JOBS (1 where the value starts with '1', else 0) say, -1 each where not set (null: none set); it refuses what create
 * refuses, with its words.  The other: the plan of a created handle.
 * out [host][MZ_FCL_PLAN_FIELDS] = G, S, nwg, nln, fuse_fwd, fuse_fb, fb_jobs, KP, lds_bytes, lds_bwd_dw, njobs, njobs_heads,
 * stage_bytes, forward form (0 one launch with the backward chain, 1 one launch, 2 chain + heads), backward form (0 in the forward's
 * launch, 1 beside the heads' jobs, 2 row slabs), the LDS bytes of the last launch, cus, the tapes' floats, whether buffer descriptors
 * reach all of them, arrival counters.
 * names [host] (may be null): the kernels a step of that plan can launch under optimiser opt_kind (0 Adam, 1 SGD, 2 RMSprop; + 4 with a
 * momentum buffer) and loss form scalar_loss (0 categorical, else scalar), with their template arguments, one per line. */
#define MZ_FCL_PLAN_FIELDS 20
int mz_fcl_plan_host(int batch, int unroll_steps, int obs_dim, int action_space, int value_bins, int reward_bins, int cus, const int *knobs5,
                     int opt_kind, int scalar_loss, long long *out, char *names, size_t names_cap);
int mz_fcl_plan(mz_fcl *c, int opt_kind, int scalar_loss, long long *out, char *names, size_t names_cap);

/* test hooks: the gather tables of the weight streams (csrc/mz_pack.inc).  mz_pack_host: no engine, no device -- the plan mz_create would
 * build for this shape (value_bins / reward_bins: the supports' sizes, 1 / 1 for no_support; split_f16 != 0: with the split-f16 stream,
 * action_space <= 13).  out [host][MZ_PACK_FIELDS] = floats of the flat vector, floats of the packed vector, the segments' offsets in it
 * (w0o, b0o, w1, b1, w2, b2, w3, b3, w4, b4, lnw, lnb of the stand-alone kernels; the fused kernel's fc1 packs w1f, w3f, its stream ws,
 * the small-MFMA packs h4, p4, the root's stream is), floats per wave of the fused stream, float16 of the split-f16 stream, ks0, ks1, ks3,
 * steps per wave of the fused stream, first-stage steps and all steps of the root's, groups per wave of the split-f16 stream.
 * which = 0 idx, 1 idx2 (out[1] entries each), 2 idx_h2 (out[21] entries): copied to table [host][cap] where table is not null (cap
 * smaller than the table is refused).  mz_pack_indices: the same tables as engine e holds them on its device (synchronous). */
#define MZ_PACK_FIELDS 29
int mz_pack_host(int obs_dim, int action_space, int value_bins, int reward_bins, int split_f16, long long *out, int which, int32_t *table,
                 size_t cap);
int mz_pack_indices(mz_engine *e, int which, int32_t *out, size_t cap);

/* development hook: s_memtime stamps (shader clock) at the phase boundaries of k_fcl_heads, workgroup 0 of every head at unroll
 * position 1 (3 x 16 slots), and of k_fcl_chain_fwd4's position 2 (slots 48..53); slots 12..15, 28..31, 44..47, 59..66: the two-launch
 * step's timeline on the constant 100 MHz clock (chain workgroup 0's passes, its last two positions' value units, the last unit / job /
 * chain workgroup to end; scripts/fcl_heads_phases.py names them): enable = 1 arms it for the following steps, enable = 0 reads the stamps
 * of the last step into host_out [96]. */
int mz_fcl_heads_profile(mz_fcl *c, int enable, unsigned long long *host_out);

/* Which kernel mz_search / mz_selfplay_steps launch for this engine right now: out4 [host] = kind (0 the stand-alone
 * kernels, 1 k_search_fused, 2 k_search_h2), LDS placement of the trees (0 node pool, 1 whole trees in LDS, 2 compact in
 * LDS; -1 for kind 0), dynamics-fc1 k-steps of the instantiation, lanes per child group.  For tests: they assert the
 * instantiation they mean to exercise. */
int mz_search_kernel_info(const mz_engine *e, int *out4);

/* mz_selfplay_steps with one pair of HIP events around every search-kernel dispatch (hipExtLaunchKernelGGL start / stop
 * events on `stream`: the timestamps rocprofv3's kernel trace reports).  The k moves are launched eagerly, back to back,
 * with no synchronisation in between (the state of the timed loop); synchronous at the end.  ms_out [host][k] =
 * duration of each search launch in milliseconds.  bench.py's roofline figure is the mean of these. */
int mz_selfplay_steps_timed(mz_engine *e, int k, float *ms_out, void *stream);

/* Diagnostic: `moves` (<= 16) whole moves in ONE launch of the persistent self-play kernel with s_memtime stamps between
 * the phases of a move; cycles_out [host][8] = shader cycles per move, mean over all waves, in the order of a move:
 * root first stage (observation, obs_dim+1 -> 512), representation out + LayerNorm, prediction, root tree part (Dirichlet
 * draw, root.expand, first descent), resident weight steps + tree set-up, ring priming + barrier, all simulations, end of
 * the move (select_action, env step, record).  Synchronous; the moves' records land in the ring like any others.
 * Exact-f32 kernel only; fails where the self-play loop does not run as whole moves in one launch (two-player games,
 * trees in the global pool, MZ_NO_PERSIST) and for split_f16. */
int mz_selfplay_phase_profile(mz_engine *e, int moves, double *cycles_out, void *stream);

/* observation the synthetic env would emit for (env, episode, t): [host] out[obs_dim]; and reward */
int mz_synth_obs(const mz_engine *e, int env, int episode, int t, float *out_obs, float *out_reward);

/* The device CartPole environment (mz_selfplay_set_env kind 2).  mz_cartpole_reset_state: out [host][4] = the float64 state
 * episode `episode` of (global) environment `env` starts from -- the counter RNG keyed (seed, env, episode), the same
 * integer code on host and device, so a test can start a host envs.CartPole where the device started.
 * mz_selfplay_env_state: out [host][B][4] = the environments' current states (synchronous).  mz_selfplay_set_env_state:
 * state [host][4] replaces environment env's (after mz_selfplay_reset; synchronous): a test starts next to a threshold. */
int mz_cartpole_reset_state(const mz_engine *e, int env, int episode, double *out);
int mz_selfplay_env_state(mz_engine *e, double *out);
int mz_selfplay_set_env_state(mz_engine *e, int env, const double *state);

/* The device Connect Four environment (mz_selfplay_set_env kind 3; any other kind is refused).  mz_selfplay_board_state:
 * out [host][B][44] int8 = per environment the 42 cells (7 * row + col, row 0 at the bottom), the turn and the step
 * (synchronous).  mz_selfplay_set_board_state: cells42 [host][42] and turn replace environment env's position (after
 * mz_selfplay_reset; synchronous); its step becomes the number of stones.  The position need not be reachable, but it
 * needs a column that is not full. */
int mz_selfplay_board_state(mz_engine *e, int8_t *out);
int mz_selfplay_set_board_state(mz_engine *e, int env, const int8_t *cells42, int turn);

/* test hook: mz_playout_plan's planning with the 64 lanes looped on the HOST -- the same __host__ __device__ bodies of
 * csrc/mz_playout.hip.h (pick, playout, per-action results, backup), only the reduction over the lanes differs.  Takes no engine
 * and touches no device: A is the game's action count (9 / 7), seed and env_id_offset what the engine's config would hold.
 * Arguments and outputs as mz_playout_plan's; the two agree bit for bit. */
int mz_playout_plan_host(int kind, int A, uint64_t seed, int env_id_offset, const int8_t *boards, const int8_t *turn,
                         const int32_t *step, int n_games, int playouts, uint64_t move, int32_t *action_out,
                         int32_t *visits_out, int32_t *wins_out);

/* test hook: mz_solve's units searched one after the other on the HOST -- the same __host__ __device__ bodies of
 * csrc/mz_solve.hip.h in the same order with the same budget, so values, the unsolved pattern and the node counts equal the
 * device's exactly.  Takes no engine and touches no device: A is the game's action count (9 / 7).  Arguments, checks and
 * outputs as mz_solve's. */
int mz_solve_host(int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                  int8_t *values_out, uint32_t *nodes_out);

/* test hooks of mz_solve_tt.  mz_solve_tt_host: its units searched one after the other on the HOST with one table and one
 * generation counter, as one lane has them -- the same __host__ __device__ bodies, so values, the unsolved pattern and the
 * node counts equal the device's exactly; arguments, checks and outputs as mz_solve_host's.  mz_solve_tt_set_generation:
 * every lane's generation counter becomes `generation` (0 .. 2047; the tables are allocated if they were not; synchronous),
 * so a test can cross the wrap at 2048, where a lane clears its table.  The tables keep their entries: set a value no
 * entry carries yet, or one from which the wrap is crossed before an entry's generation comes round. */
int mz_solve_tt_host(int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                     int8_t *values_out, uint32_t *nodes_out);
int mz_solve_tt_set_generation(mz_engine *e, int generation);

/* test hooks of mz_unroll: its two __host__ __device__ bodies (csrc/mz_unroll.hip.h) looped on the HOST; no engine, no device.
 * mz_unroll_lines_host: the lines of n rows (arguments and checks as mz_unroll's), row-major: obs_out [n][K + 1][obs_dim]
 * float32, legal_out [n][K + 1] uint32 masks, terminal_out [n][K + 1] uint8, reward_true_out [n][K + 1] float32, depth_out and
 * flags_out [n].  Integers and casts of -1 / 0 / +1: the device's lines equal these bit for bit.
 * mz_unroll_terms_host: the terms of `items` independent (row, k) in the device's operation order (exp() is the host
 * library's): logits_u / logits_f [items][A] float32, legal [items] uint32, terminal / live [items] uint8, k [items] int32,
 * reward_true / reward_u / value_u / value_f [items] float32, truth [items][A] int8 or NULL -> terms_out
 * [items][mz_unroll_num_terms()] float64. */
int mz_unroll_lines_host(int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, const int32_t *actions, int n, int K,
                         float *obs_out, uint32_t *legal_out, uint8_t *terminal_out, float *reward_true_out, int32_t *depth_out,
                         int32_t *flags_out);
int mz_unroll_terms_host(int A, int items, const float *logits_u, const float *logits_f, const uint32_t *legal, const uint8_t *terminal,
                         const uint8_t *live, const int32_t *k, const float *reward_true, const float *reward_u, const float *value_u,
                         const float *value_f, const int8_t *truth, double *terms_out);

/* test hooks of the true-rules search (mz_set_true_model).  mz_tm_export (synchronous, [host] arrays, any may be NULL): the side
 * state per expansion slot, [B][num_simulations + 1] each -- boards [..][42] int8, mover int8, step int32, mask uint32 (bit a =
 * child a exists; 0 for a finished position), finished uint8 -- and nexp [B] int32, the slots taken (the root's included).
 * mz_tm_search_host: the same search as plain sequential C++ on the HOST -- no engine, no device; exp() is the host library's.
 * cfg: the engine's configuration (num_simulations sizes the trees); n positions of `kind` (1 / 3): boards [n][42], turn [n],
 * step [n]; root_logits [n][A] float32; noise [n][A] float64 or NULL (no noise).  The root's children are the position's legal
 * actions.  eval is called once per simulation on the leaves' observations obs [n][obs_dim] (zeros where the leaf is finished)
 * and fills value [n] and logits [n][A].  Outputs (any may be NULL): the trees in mz_export_tree's layout (N, W, P, R, E, TP
 * [n][NN], legal_mask [n], minmax [n][2]; E is -1 for a node that was never created), nexp [n], the side state as
 * mz_tm_export's ([n][num_simulations + 1]), and leaf_depth [n][num_simulations]: len(search_path) - 1 of every simulation. */
int mz_tm_export(mz_engine *e, int8_t *boards, int8_t *mover, int32_t *step, uint32_t *mask, uint8_t *finished, int32_t *nexp);
int mz_tm_search_host(const mz_config *cfg, int kind, int n, const int8_t *boards, const int8_t *turn, const int32_t *step,
                      const float *root_logits, const double *noise, int num_simulations,
                      void (*eval)(void *ctx, const float *obs, int n, float *value, float *logits), void *ctx,
                      int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP, uint32_t *legal_mask, double *minmax,
                      int32_t *nexp_out, int8_t *slot_boards, int8_t *slot_mover, int32_t *slot_step, uint32_t *slot_mask,
                      uint8_t *slot_finished, int32_t *leaf_depth);

/* test hooks of the Gumbel search (mz_set_gumbel).  mz_gz_export (synchronous, [host], either may be NULL): gumbel [B][A]
 * float64, this move's G (0 with gumbel_scale 0), and vhat [B][num_simulations + 1] float32, the raw network value per
 * expansion slot.  mz_gz_seq_host: out[n] = seq(m, n), mctx's sequence of considered visits.
 * mz_gz_search_host: the same search as plain sequential C++ on the HOST -- no engine, no device; exp() is the host library's.
 * cfg: the engine's configuration (num_simulations sizes the trees); n roots: to_play [n] int8 (NULL: 1), legal [n][A] uint8
 * (NULL: all), root_value [n], root_logits [n][A] float32, gumbel [n][A] float64 = G (NULL only with gumbel_scale 0).  eval is
 * called once per simulation with the descents' parent_slot [n] and action [n] and fills value [n], reward [n], logits
 * [n][A].  Outputs (any may be NULL): the trees in mz_export_tree's layout (N, W, P, R, E, TP [n][NN], legal_mask [n], minmax
 * [n][2]), vhat [n][num_simulations + 1], per simulation sel_slot / sel_action [n][num_simulations], the search paths
 * [n][num_simulations][num_simulations + 2] (-1 behind their end) with plens [n][num_simulations], mz_gz_pick's four outputs,
 * and min_gap [1]: the smallest non-zero difference between the best and the second-best score over every arg-max taken
 * (inf if there was none). */
int mz_gz_export(mz_engine *e, double *gumbel, float *vhat);
int mz_gz_seq_host(int m, int n, int32_t *out);
int mz_gz_search_host(const mz_config *cfg, int n, const int8_t *to_play, const uint8_t *legal, const float *root_value,
                      const float *root_logits, const double *gumbel, int max_considered, double c_visit, double c_scale,
                      double gumbel_scale, int num_simulations,
                      void (*eval)(void *ctx, int sim, const int32_t *parent_slot, const int32_t *action, int n, float *value,
                                   float *reward, float *logits),
                      void *ctx, int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP, uint32_t *legal_mask,
                      double *minmax, float *vhat_out, int32_t *sel_slot, int32_t *sel_action, int32_t *paths, int32_t *plens,
                      int32_t *action_out, float *pred_reward, double *improved_policy, double *v_mix, double *min_gap);

/* test hooks of mz_fcl_set_symmetry.  mz_fcl_symmetry_apply: the symmetry kernel alone, with the handle's kind and seed and the
 * given update number, on device-visible arrays of the handle's batch (obs [batch][obs_dim], actions [batch][K] int32 / int64,
 * target_policies [batch][K + 1][A]; device memory, or mapped pinned host memory as mz_fcl_run's staging is -- the hook looks its
 * device address up) into [dev] obs_out / actions_out / policies_out of the same shapes (not the sources themselves) and
 * elements_out [batch] (may be NULL): the element drawn for every sample; enqueued on `stream`, the handle's counter stays.
 * mz_fcl_symmetry_host: the same __host__ __device__ bodies of csrc/mz_symmetry.hip.h looped on the HOST over host arrays: no
 * handle, no device.  The two agree bit for bit. */
int mz_fcl_symmetry_apply(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_policies,
                          uint32_t update, float *obs_out, void *actions_out, float *policies_out, int32_t *elements_out, void *stream);
int mz_fcl_symmetry_host(int kind, uint64_t seed, uint32_t update, int batch, int K, const float *obs, const void *actions,
                         int actions_are_i32, const float *target_policies, float *obs_out, void *actions_out, float *policies_out,
                         int32_t *elements_out);

#ifdef __cplusplus
}
#endif
#endif
