// mz_symmetry.hip.h -- board-symmetry augmentation of a training batch (DESIGN s7e): every sample of a batch is replaced by
// one of the equivalent images of its position -- TicTacToe (kind 1): the 8 elements of the square's group, Connect Four
// (kind 3): the position or its left-right mirror (gfx950; included by mz_engine.hip).  The observation, the K unrolled
// actions and the K + 1 policy targets of a sample move together; rewards, values, weights and indices are the same for
// every image and are not touched.
//
// The element of sample b is g = mz_philox(seed, update, b, 0, MZ_RNG_SYM << 24).x & (n - 1): it depends on (seed, update, b)
// and nothing else, and a sample's image on its own data only.  p_g permutes the cells, a_g the actions:
//   obs'[p_g(c)] = obs[c]      actions'[k] = a_g(actions[k])      policies'[k][a_g(a)] = policies[k][a]
// TicTacToe: cell 3 * row + col, action = cell, g = 4 f + q: q quarter turns (r, c) -> (c, 2 - r) first, then, if f is set,
// (r, c) -> (r, 2 - c); a_g = p_g.  Connect Four: cell 7 * row + col, action = column, g = 1 maps col -> 6 - col.
//
// The kernel is a gather: one thread per DESTINATION element reads its source through the inverse tables (constant data),
// so the stores are coalesced.  No LDS, no atomics, no scratch.  Everything is integer code and copies of whole words: the
// bodies below are __host__ __device__, and mz_fcl_symmetry_host (include/mz_engine_debug.h) runs them in a loop on the
// host, bit for bit the kernel's result.
#pragma once
#include <stdint.h>
#include "mz_rng.h"
#include "mz_games.h"

#define MZ_SYM_THREADS 256

// the kind's (cells, actions) of mz_games.h and its group size; 0 elements: not a kind with symmetries
__host__ __device__ inline int sym_cells(int kind) { return mz_game_info(kind).cells; }
__host__ __device__ inline int sym_actions(int kind) { return mz_game_info(kind).actions; }
__host__ __device__ inline int sym_elements(int kind) { return kind == 1 ? 8 : (kind == 3 ? 2 : 0); }

// TicTacToe: p_g(c) and its inverse (rows g = 4 f + q)
__host__ __device__ inline int sym_ttt_fwd(int g, int c) {
  static constexpr uint8_t T[8][9] = {{0, 1, 2, 3, 4, 5, 6, 7, 8}, {2, 5, 8, 1, 4, 7, 0, 3, 6}, {8, 7, 6, 5, 4, 3, 2, 1, 0}, {6, 3, 0, 7, 4, 1, 8, 5, 2},
                                      {2, 1, 0, 5, 4, 3, 8, 7, 6}, {0, 3, 6, 1, 4, 7, 2, 5, 8}, {6, 7, 8, 3, 4, 5, 0, 1, 2}, {8, 5, 2, 7, 4, 1, 6, 3, 0}};
  return T[g][c];
}
__host__ __device__ inline int sym_ttt_inv(int g, int d) {
  static constexpr uint8_t T[8][9] = {{0, 1, 2, 3, 4, 5, 6, 7, 8}, {6, 3, 0, 7, 4, 1, 8, 5, 2}, {8, 7, 6, 5, 4, 3, 2, 1, 0}, {2, 5, 8, 1, 4, 7, 0, 3, 6},
                                      {2, 1, 0, 5, 4, 3, 8, 7, 6}, {0, 3, 6, 1, 4, 7, 2, 5, 8}, {6, 7, 8, 3, 4, 5, 0, 1, 2}, {8, 5, 2, 7, 4, 1, 6, 3, 0}};
  return T[g][d];
}
// Connect Four: the mirror of a cell (its own inverse)
__host__ __device__ inline int sym_c4_cell(int g, int d) {
  static constexpr uint8_t T[42] = {6,  5,  4,  3,  2,  1,  0,  13, 12, 11, 10, 9,  8,  7,  20, 19, 18, 17, 16, 15, 14,
                                    27, 26, 25, 24, 23, 22, 21, 34, 33, 32, 31, 30, 29, 28, 41, 40, 39, 38, 37, 36, 35};
  return g ? (int)T[d] : d;
}

// the element drawn for sample b of update `update`
__host__ __device__ inline int sym_draw(int kind, uint64_t seed, uint32_t update, uint32_t b) {
  return (int)(mz_philox(seed, update, b, 0u, MZ_RNG_SYM << 24).x & (uint32_t)(sym_elements(kind) - 1));
}
// the source cell of destination cell d: p_g^-1(d)
__host__ __device__ inline int sym_cell_src(int kind, int g, int d) { return kind == 1 ? sym_ttt_inv(g, d) : sym_c4_cell(g, d); }
// the source action of destination action d: a_g^-1(d)
__host__ __device__ inline int sym_action_src(int kind, int g, int d) { return kind == 1 ? sym_ttt_inv(g, d) : (g ? 6 - d : d); }
// a_g(a); a value that is no action of the game stays what it is
__host__ __device__ inline int64_t sym_action(int kind, int g, int64_t a) {
  if (a < 0 || a >= (int64_t)sym_actions(kind)) return a;
  return kind == 1 ? (int64_t)sym_ttt_fwd(g, (int)a) : (g ? 6 - a : a);
}

// one batch: obs [bs][O], actions [bs][K] (int32 or int64), policies [bs][K + 1][A], and their images; elements [bs] or null
struct SymBatch {
  const float *obs;
  const void *act;
  const float *pol;
  float *obs_out;
  void *act_out;
  float *pol_out;
  int32_t *elements;
  uint64_t seed;
  uint32_t update;
  int kind, bs, K, act_i32;
};

__host__ __device__ inline size_t sym_total(const SymBatch &s) {
  return (size_t)s.bs * ((size_t)sym_cells(s.kind) + (size_t)s.K + (size_t)(s.K + 1) * sym_actions(s.kind));
}

// destination element t of [0, sym_total): the observations' cells first, then the actions, then the policies' entries
__host__ __device__ inline void sym_element(const SymBatch &s, size_t t) {
  const int O = sym_cells(s.kind), A = sym_actions(s.kind), K = s.K, PA = (K + 1) * A;
  const size_t n_obs = (size_t)s.bs * O, n_act = (size_t)s.bs * K;
  if (t < n_obs) {
    const uint32_t b = (uint32_t)(t / (size_t)O);
    const int d = (int)(t - (size_t)b * O), g = sym_draw(s.kind, s.seed, s.update, b);
    s.obs_out[t] = s.obs[(size_t)b * O + sym_cell_src(s.kind, g, d)];
    if (d == 0 && s.elements) s.elements[b] = g;
  } else if (t < n_obs + n_act) {
    const size_t u = t - n_obs;
    const int g = sym_draw(s.kind, s.seed, s.update, (uint32_t)(u / (size_t)K));
    if (s.act_i32) ((int32_t *)s.act_out)[u] = (int32_t)sym_action(s.kind, g, (int64_t)((const int32_t *)s.act)[u]);
    else ((int64_t *)s.act_out)[u] = sym_action(s.kind, g, ((const int64_t *)s.act)[u]);
  } else {
    const size_t u = t - n_obs - n_act;
    const uint32_t b = (uint32_t)(u / (size_t)PA);
    const int r = (int)(u - (size_t)b * PA), k = r / A, d = r - k * A, g = sym_draw(s.kind, s.seed, s.update, b);
    s.pol_out[u] = s.pol[(size_t)b * PA + (size_t)k * A + sym_action_src(s.kind, g, d)];
  }
}

static __global__ __launch_bounds__(MZ_SYM_THREADS) void k_fcl_symmetry(SymBatch s) {
  const size_t t = (size_t)blockIdx.x * MZ_SYM_THREADS + threadIdx.x;
  if (t < sym_total(s)) sym_element(s, t);
}
