// mz_eval_env.hip.h -- evaluation games that live on the device from the first move to the last (mz_eval_env_*,
// mz_eval_abi.inc), for B games in lock-step (gfx950; included by mz_engine.hip, -ffp-contract=off):
//
//   k_eval_observe       from the games' state to the engine's obs / legal / to_play inputs, and the move's given draws
//                        laid out for mz_root_prepare and mz_eval_walk, one thread per game
//   k_eval_apply         evaluate.py:331-374 on the device environments -- the games of mz_games.h, not restated -- with
//                        the summary's accumulators and the optional per-move logs, one thread per game
//
// A separate header from mz_eval.hip.h, whose kernels are the walk and the lookahead every evaluation path shares.
#pragma once
#include "mz_common.h"
#include "mz_rng.h"
#include "mz_games.h"

// The engine's inputs of one searched move and the outputs of its walk / lookahead / finalize: what ply_search
// (mz_eval_abi.inc) runs over, for evaluation games and matches alike (a match takes one action per ply: M = 1).
struct PlyIO {
  float *obs;            // [Bp][O]
  uint8_t *legal;        // [B][A]
  int8_t *to_play;       // [B]
  double *noise;         // [B][A] the move's given Dirichlet draws
  double *walk_u;        // [B][M] the move's given walk uniforms
  int32_t *actions;      // [B][M]
  float *pred_rewards;   // [B][M]
  int32_t *n_actions;    // [B]
  int32_t *path_lengths; // [B][sims of the searching engine]
  double *child_visits;  // [B][A]
  double *root_value;    // [B]
  // the games themselves, as far as a search on the true rules needs them (ply_search with mz_set_true_model)
  int kind;              // 1 TicTacToe, 2 CartPole, 3 Connect Four (the numbering of mz_selfplay_set_env)
  int8_t *board;         // [B][42] (TicTacToe uses the first 9 cells of its row)
  int8_t *turn;          // [B] the player about to move
  int32_t *step;         // [B] game.step: plies applied
};

// ---- evaluation games on the device environments (mz_eval_env_*): the game and everything the summary needs stay here
// from the first move to the last.  Separate from SelfplayState: self-play on the same engine is untouched.
struct EvalState : PlyIO {
  int max_steps;         // evaluate.py:372: the game is cut when game.step reaches it
  int time_limit;        // CartPole: gym's TimeLimit (envs.CartPole.max_episode_steps)
  int random_opp;        // +1 / -1: that player's moves are the random opponent's; 0: none
  int two_players;
  int cap;               // capacity of the per-move / per-step logs: min(max_steps, the game's own longest)
  int sims;
  bool ready;
  // the game (PlyIO: kind, board, turn, step)
  double *cart;          // [B][4]
  uint8_t *terminal;     // [B]
  int32_t *live;         // [1] games not yet terminal
  // accumulators, float64, added in move order: [5][B] = sum reward, sum predicted reward, sum predicted value, sum root
  // value, mean of the lexicographic-maximum depth list
  double *acc;
  int32_t *n_moves;      // [B] moves searched (the count of the value sums)
  int32_t *depth_max;    // [B][sims] the lexicographic maximum of the per-move lists of search depths (evaluate.py:102)
  // (PlyIO: the engine's inputs of the coming move, laid out by k_eval_observe, and the search's outputs)
  double *temp;          // [B]
  int walk_cap;          // M the walk buffers are sized for
  // draws given by the caller (mz_eval_env_set_draws; device memory the caller keeps alive), or null = the counter RNG
  const double *d_walk; int d_walk_moves, d_walk_m;       // [B][moves][M]
  const double *d_noise; int d_noise_moves;               // [B][moves][A]
  const int32_t *d_opp; int d_opp_n;                      // [B][n] indices into the root position's legal actions
  int32_t *opp_pos;      // [B] how many of them the game has consumed
  // the playout-search opponent (mz_eval_env_set_opponent; mz_playout.hip.h): its budget per move (0: the random mover) and
  // the move it planned for the games whose mover is random_opp (null with the random mover)
  int opp_playouts;
  int32_t *opp_action;   // [B]
  int32_t *opp_action_buf;      // (the allocation opp_action points to while the opponent is set)
  // per-move logs (null unless asked for): per applied action [B][cap], per move [B][cap]
  int32_t *log_action; double *log_reward; int8_t *log_mover; float *log_pred_reward;
  float *log_pred_value; double *log_root_value; double *log_child_visits; int32_t *log_n_actions; int32_t *log_depths;
};

// From the state to the engine's inputs (evaluate.py's per-move host loop): observation, legal mask, to_play; a finished
// game gets a zero observation, all actions legal and to_play +1.  The move's given draws are laid out for mz_root_prepare
// ([B][A], zero at illegal actions) and mz_eval_walk ([B][M]).
static __global__ void k_eval_observe(EvalState es, int B, int O, int A, int M, int move) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint8_t *legal = es.legal + (size_t)b * A;
  const bool live = !es.terminal[b];
  es.to_play[b] = (int8_t)mz_game_observe(es.kind, es.board + (size_t)b * 42, (int)es.turn[b], es.cart + (size_t)b * 4, live,
                                          O, A, es.obs + (size_t)b * O, legal);
  if (es.d_noise) {
    const bool have = live && move < es.d_noise_moves;
    const double *src = es.d_noise + ((size_t)b * es.d_noise_moves + (have ? move : 0)) * A;
    for (int a = 0; a < A; ++a) es.noise[(size_t)b * A + a] = (have && legal[a]) ? src[a] : 0.0;
  }
  if (es.d_walk) {
    const bool have = live && move < es.d_walk_moves;
    const double *src = es.d_walk + ((size_t)b * es.d_walk_moves + (have ? move : 0)) * es.d_walk_m;
    for (int j = 0; j < M; ++j) es.walk_u[(size_t)b * M + j] = (have && j < es.d_walk_m) ? src[j] : 0.0;
  }
}

// evaluate.py:331-374 for one game per thread, after the walk (mode 0: actions / pred_rewards [B][M], n_actions,
// path_lengths, and mz_finalize's child visits and root value) or the lookahead (mode 1 --only_prior, 2 --only_value: one
// action per game, root value 0, search depths [0] / [1]).  net_value: the network's root values (TreeView::root_value).
// A finished game is left alone.
static __global__ void k_eval_apply(EvalState es, const float *net_value, int B, int A, int M, int mode, int move,
                                    uint64_t seed, int env_offset) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (es.terminal[b]) return;
  const int cap = es.cap, sims = es.sims;
  double *acc_reward = es.acc + b, *acc_pred_reward = es.acc + (size_t)B + b, *acc_pred_value = es.acc + (size_t)2 * B + b,
         *acc_root_value = es.acc + (size_t)3 * B + b, *acc_depth = es.acc + (size_t)4 * B + b;
  // (1) once per move: predicted value, root value, child visits
  const int mv = es.n_moves[b];
  const float pv = net_value[b];
  const double rv = mode == 0 ? es.root_value[b] : 0.0;
  *acc_pred_value = *acc_pred_value + (double)pv;
  *acc_root_value = *acc_root_value + rv;
  es.n_moves[b] = mv + 1;
  const bool logs = es.log_action != nullptr && mv < cap;
  if (logs) {
    es.log_pred_value[(size_t)b * cap + mv] = pv;
    es.log_root_value[(size_t)b * cap + mv] = rv;
    for (int a = 0; a < A; ++a) es.log_child_visits[((size_t)b * cap + mv) * A + a] = es.child_visits[(size_t)b * A + a];
  }
  // (2) the walked actions
  uint32_t legal = 0;      // the legal actions of the move's ROOT position (the reference's stale list)
  for (int a = 0; a < A; ++a) legal |= (es.legal[(size_t)b * A + a] ? 1u : 0u) << a;
  const int nlegal = __builtin_popcount(legal);
  const int nact = mode == 0 ? es.n_actions[b] : 1;
  int step = es.step[b], turn = es.two_players ? (int)es.turn[b] : 1;
  double sum_reward = *acc_reward, sum_pred = *acc_pred_reward;
  bool terminal = false;
  int applied = 0;
  for (int j = 0; j < nact && j < M && step < cap; ++j) {
    int action = es.actions[(size_t)b * M + j];
    const float pr = es.pred_rewards[(size_t)b * M + j];
    sum_pred = sum_pred + (double)pr;
    const int mover = turn;
    const bool opp = es.two_players && mover == es.random_opp;
    if (opp && nlegal > 0) {
      int idx;
      if (es.opp_action) {      // the playout opponent's plan for this position (M == 1: the root position is the game's)
        idx = __builtin_popcount(legal & ((1u << es.opp_action[b]) - 1u));
      } else if (es.d_opp) {
        const int pos = es.opp_pos[b];
        idx = pos < es.d_opp_n ? es.d_opp[(size_t)b * es.d_opp_n + pos] : 0;
        es.opp_pos[b] = pos + 1;
      } else {
        const mz_u4 r = mz_philox(seed, (uint32_t)(env_offset + b), (uint32_t)move, 0u,
                                  (MZ_RNG_OPP << 24) | ((uint32_t)j & 0xFFFFFFu));
        idx = (int)(mz_u01(r.x, r.y) * (double)nlegal);
      }
      action = mz_pick_legal(legal, idx);
    }
    if (action < 0 || action >= A) break;      // (the walk never hands one out; no cell outside the board is ever touched)
    bool done, won = false;
    if (es.kind == 2) done = mz_cartpole_step(es.cart + (size_t)b * 4, action) || step + 1 >= es.time_limit;
    else done = mz_game_step(es.kind, es.board + (size_t)b * 42, turn, action, step, &won);
    double reward = es.kind == 2 ? 1.0 : (won ? 1.0 : 0.0);
    if (es.two_players) turn = -turn;
    const int at = step;
    ++step; ++applied;
    terminal = done || step >= es.max_steps;
    if (terminal && opp) reward = -reward;      // evaluate.py:373-374: the opponent's winning move counts against the agent
    sum_reward = sum_reward + reward;
    if (logs) {
      es.log_action[(size_t)b * cap + at] = action;
      es.log_reward[(size_t)b * cap + at] = reward;
      es.log_mover[(size_t)b * cap + at] = (int8_t)(done ? 2 * mover : mover);      // doubled: env.step's own done
      es.log_pred_reward[(size_t)b * cap + at] = pr;
    }
    if (terminal) break;
  }
  if (!terminal && step >= cap) terminal = true;      // (unreachable: cap is the longest game; a guard for the logs' bounds)
  *acc_reward = sum_reward; *acc_pred_reward = sum_pred;
  es.step[b] = step;
  if (es.two_players) es.turn[b] = (int8_t)turn;
  if (logs) es.log_n_actions[(size_t)b * cap + mv] = applied;
  // (3) max() over the per-move lists of search depths is the lexicographic maximum list; its mean is what is reported
  int32_t *dm = es.depth_max + (size_t)b * sims;
  if (mode == 0) {
    const int32_t *pl = es.path_lengths + (size_t)b * sims;
    mz_depth_list_max(dm, pl, sims, mv == 0, acc_depth);
    if (logs)
      for (int s = 0; s < sims; ++s) es.log_depths[((size_t)b * cap + mv) * sims + s] = pl[s];
  } else if (mv == 0) {
    dm[0] = mode == 1 ? 0 : 1;
    *acc_depth = mode == 1 ? 0.0 : 1.0;
  }
  // (4)
  if (terminal) {
    es.terminal[b] = 1;
    atomicSub(es.live, 1);
  }
}
