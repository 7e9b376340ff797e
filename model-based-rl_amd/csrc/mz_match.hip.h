// mz_match.hip.h -- a match between two networks on the device games (mz_match_*, mz_match_abi.inc), B games in lock-step
// (gfx950; included by mz_engine.hip, -ffp-contract=off).  A match is a handle over two engines, one per network: every
// ply is the mover's own initial inference and search on its own engine; the game between them lives here.
//
//   k_match_open         the opening plies, applied with no inference: the min(floor(u * n), n - 1)-th legal action
//   k_match_observe      from the games' state to the engines' obs / legal / to_play inputs and the ply's given draws
//   k_match_apply        the mover's one action on the games of mz_games.h (not restated), the per-network
//                        accumulators and the optional per-ply logs
//   k_match_temperature  the two sides' temperatures, [2][B]
//
// One thread per game.  The per-game bodies are __host__ __device__ functions, so the CPU suite plays them against a rule
// check of its own (tests/match_rules_host.cpp).
#pragma once
#include "mz_common.h"
#include "mz_rng.h"
#include <vector>
#include "mz_games.h"
#include "mz_eval_env.hip.h"      // (PlyIO)

// Separate from EvalState and SelfplayState: evaluation and self-play on the two engines are untouched.
struct MatchState : PlyIO {
  int max_steps;         // the game is cut (a draw) when its step count reaches it
  int cap;               // capacity of the per-ply logs: min(max_steps, the game's own longest)
  int opening;           // plies applied by k_match_open before the first searched ply
  int S;                 // the larger of the two engines' num_simulations: row length of the depth lists
  // the game (PlyIO: kind 1 TicTacToe / 3 Connect Four; board; turn, +1 moves first; step = the game's length once it is over)
  uint8_t *terminal;     // [B]
  int32_t *live;         // [1] games not yet terminal
  int8_t *result;        // [B] for player +1, the game's first mover: +1 win, 0 draw (the cut included), -1 loss
  // per game and per network (0 / 1 = the handle's first / second engine), float64, added in ply order:
  // [2][4][B] = sum predicted reward, sum predicted value, sum root value, mean of the lexicographic-maximum depth list
  double *acc;
  int32_t *n_searched;   // [2][B] plies that network searched
  int32_t *depth_max;    // [2][B][S] the lexicographic maximum of its per-ply lists of search depths
  // (PlyIO, M = 1: the mover engine's inputs of the coming ply, laid out by k_match_observe, and the search's outputs)
  double *temp;          // [2][B] per network
  // draws given by the caller (mz_match_set_draws; device memory the caller keeps alive), or null = the counter RNG
  const double *d_walk; int d_walk_plies;       // [B][plies][1], indexed by the ply (opening plies counted)
  const double *d_noise; int d_noise_plies;     // [B][plies][A]
  const int32_t *d_open; int d_open_n;          // [B][n] indices into the legal actions of the opening positions
  // per-ply logs (null unless asked for), [B][cap]; the search entries of an opening ply stay zero
  int32_t *log_action; int8_t *log_mover; int8_t *log_net; double *log_reward; float *log_pred_reward;
  float *log_pred_value; double *log_root_value; double *log_child_visits; int32_t *log_depths;
};

// env.step(action) of game b for the player about to move, and everything that follows from it for the game: the step
// count, the turn, the per-ply logs of the action, and at the end of the game (the rules' done, or the cut at max_steps)
// the result for player +1.  Returns whether the game ended.  The caller has checked that the game is live, step < cap
// and 0 <= action < A.
__host__ __device__ inline bool mz_match_step_game(const MatchState &ms, int b, int action, int net, float pred_reward) {
  const int step = ms.step[b], mover = (int)ms.turn[b];
  int8_t *bd = ms.board + (size_t)b * 42;
  bool won = false;
  const bool done = mz_game_step(ms.kind, bd, mover, action, step, &won);
  ms.turn[b] = (int8_t)-mover;
  ms.step[b] = step + 1;
  if (ms.log_action) {
    const size_t at = (size_t)b * ms.cap + step;
    ms.log_action[at] = action;
    ms.log_mover[at] = (int8_t)(done ? 2 * mover : mover);      // doubled: env.step's own done, not the cut
    ms.log_net[at] = (int8_t)net;
    ms.log_reward[at] = won ? 1.0 : 0.0;
    ms.log_pred_reward[at] = pred_reward;
  }
  const bool terminal = done || step + 1 >= ms.max_steps || step + 1 >= ms.cap;
  if (terminal) {
    ms.result[b] = (int8_t)(won ? mover : 0);
    ms.terminal[b] = 1;
  }
  return terminal;
}

// The opening of game b: ply p is the min(floor(u * n), n - 1)-th of the position's n legal actions, u from the counter
// RNG keyed (seed, env = the game's seed, p, 0) under MZ_RNG_OPEN -- the game's seed alone, so both seatings of a seed
// open alike -- or the caller's index.  A game that ends inside its opening is terminal with its result, as any other.
// Returns whether the game ended.
__host__ __device__ inline bool mz_match_open_game(const MatchState &ms, int b, int A, uint64_t seed, uint32_t env) {
  for (int p = 0; p < ms.opening; ++p) {
    if (ms.terminal[b] || ms.step[b] >= ms.cap) return false;
    const uint32_t mask = mz_game_legal(ms.kind, ms.board + (size_t)b * 42);
    const int n = __builtin_popcount(mask);
    if (n == 0) return false;      // (unreachable: a live game has a legal action)
    int idx;
    if (ms.d_open) {
      idx = p < ms.d_open_n ? ms.d_open[(size_t)b * ms.d_open_n + p] : 0;
    } else {
      const mz_u4 r = mz_philox(seed, env, (uint32_t)p, 0u, MZ_RNG_OPEN << 24);
      idx = (int)(mz_u01(r.x, r.y) * (double)n);
    }
    if (mz_match_step_game(ms, b, mz_pick_legal(mask, idx), -1, 0.f)) return true;
  }
  return false;
}

// From game b's state to the mover engine's inputs: observation (turn * board as float32), legal mask, to_play; a
// finished game gets a zero observation, all actions legal and to_play +1 (as k_eval_observe feeds it).  The ply's given
// draws are laid out for mz_root_prepare ([B][A], zero at illegal actions) and mz_eval_walk ([B]).
__host__ __device__ inline void mz_match_observe_game(const MatchState &ms, int b, int O, int A, int ply) {
  uint8_t *legal = ms.legal + (size_t)b * A;
  const bool live = !ms.terminal[b];
  ms.to_play[b] = (int8_t)mz_game_observe(ms.kind, ms.board + (size_t)b * 42, (int)ms.turn[b], nullptr, live, O, A,
                                          ms.obs + (size_t)b * O, legal);
  if (ms.d_noise) {
    const bool have = live && ply < ms.d_noise_plies;
    const double *src = ms.d_noise + ((size_t)b * ms.d_noise_plies + (have ? ply : 0)) * A;
    for (int a = 0; a < A; ++a) ms.noise[(size_t)b * A + a] = (have && legal[a]) ? src[a] : 0.0;
  }
  if (ms.d_walk) {
    const bool have = live && ply < ms.d_walk_plies;
    ms.walk_u[b] = have ? ms.d_walk[(size_t)b * ms.d_walk_plies + ply] : 0.0;
  }
}

// One ply of game b after network `net`'s walk (mode 0: actions / pred_rewards [B], path_lengths [B][sims], and
// mz_finalize's child visits and root value) or lookahead (mode 1 only_prior, 2 only_value: root value 0, search depths
// [0] / [1]): that network's accumulators and the ply's search logs, then exactly one action on the rules.  pred_value:
// the mover engine's network root value.  A finished game is left alone.  Returns whether the game ended.
__host__ __device__ inline bool mz_match_apply_game(const MatchState &ms, int b, int B, int A, int net, int mode, int sims,
                                                    float pred_value) {
  if (ms.terminal[b]) return false;
  const int step = ms.step[b], cap = ms.cap, S = ms.S;
  const int action = ms.actions[b];
  if (step >= cap || action < 0 || action >= A) {      // (unreachable: a live game is below the cap and the walk hands an
    ms.terminal[b] = 1;                                //  action out; no cell outside the board or the logs is ever touched)
    return true;
  }
  double *acc = ms.acc + (size_t)net * 4 * B + b;      // [4] at stride B
  const float pr = ms.pred_rewards[b];
  const double rv = mode == 0 ? ms.root_value[b] : 0.0;
  acc[0] = acc[0] + (double)pr;
  acc[(size_t)B] = acc[(size_t)B] + (double)pred_value;
  acc[(size_t)2 * B] = acc[(size_t)2 * B] + rv;
  const int searched = ms.n_searched[(size_t)net * B + b];
  ms.n_searched[(size_t)net * B + b] = searched + 1;
  const bool logs = ms.log_action != nullptr;
  const size_t at = (size_t)b * cap + step;
  if (logs) {
    ms.log_pred_value[at] = pred_value;
    ms.log_root_value[at] = rv;
    for (int a = 0; a < A; ++a) ms.log_child_visits[at * A + a] = ms.child_visits[(size_t)b * A + a];
  }
  // max() over a network's per-ply lists of search depths is the lexicographic maximum list; its mean is what is reported
  int32_t *dm = ms.depth_max + ((size_t)net * B + b) * S;
  if (mode == 0) {
    const int32_t *pl = ms.path_lengths + (size_t)b * sims;
    mz_depth_list_max(dm, pl, sims, searched == 0, acc + (size_t)3 * B);
    if (logs)
      for (int s = 0; s < sims; ++s) ms.log_depths[at * S + s] = pl[s];
  } else {
    if (searched == 0) {
      dm[0] = mode == 1 ? 0 : 1;
      acc[(size_t)3 * B] = mode == 1 ? 0.0 : 1.0;
    }
    if (logs) ms.log_depths[at * S] = mode == 1 ? 0 : 1;
  }
  return mz_match_step_game(ms, b, action, net, pr);
}

static __global__ void k_match_open(MatchState ms, int B, int A, uint64_t seed, int env_offset) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (mz_match_open_game(ms, b, A, seed, (uint32_t)(env_offset + b))) atomicSub(ms.live, 1);
}

static __global__ void k_match_observe(MatchState ms, int B, int O, int A, int ply) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  mz_match_observe_game(ms, b, O, A, ply);
}

static __global__ void k_match_apply(MatchState ms, const float *net_value, int B, int A, int net, int mode, int sims) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (mz_match_apply_game(ms, b, B, A, net, mode, sims, net_value[b])) atomicSub(ms.live, 1);
}

static __global__ void k_match_temperature(double *temp, int B, double t0, double t1) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  temp[b] = t0;
  temp[(size_t)B + b] = t1;
}

// The handle of mz_match_* (mz_match_abi.inc).
struct mz_engine;
struct mz_match {
  mz_engine *e[2] = {nullptr, nullptr};   // the two networks' engines; the handle owns neither
  int device = 0, B = 0, A = 0, O = 0;
  MatchState ms;
  std::vector<void *> allocs;
  bool keep = false;
  bool ready = false;               // mz_match_reset has run
  bool opened = false;              // the opening plies of the current games have been applied
  int first_net = 0;
  unsigned long long plies = 0;     // plies enqueued since mz_match_reset, the opening's included
  double temp[2] = {0.0, 0.0};      // the temperatures ms.temp holds
  bool temp_set = false;
};
