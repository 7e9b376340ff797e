// mz_reanalyse.hip.h -- MuZero Reanalyse on the device (mz_reanalyse, mz_reanalyse_abi.inc): stored positions of the replay are
// searched again under the current weights, B rows at a time, and only what the replay needs comes back (gfx950; included by
// mz_engine.hip, -ffp-contract=off):
//
//   k_reanalyse_observe  from a chunk of record rows in PINNED HOST memory (the layout of mz_selfplay_drain / mzr_reanalyse_pick)
//                        to the engine's obs / legal / to_play inputs, one thread per observation element
//   k_reanalyse_store    from the searched trees to the rows' fresh statistics in pinned host memory: child_visits[A] as float32,
//                        then the root's value as a float64 in two float slots -- the record's own layout from the observation's
//                        end on --, one thread per output float; the arithmetic is mz_finalize_tree's (mz_root_visit_sum /
//                        mz_root_visit_share / mz_root_mean_value, mz_tree.hip.h), not restated
//
// Between the two run mz_initial_inference, mz_root_prepare (no noise) and mz_search, unchanged.
//
// Reanalyse with the Gumbel search (mz_reanalyse_gumbel; DESIGN s7j) keeps k_reanalyse_observe, searches as a self-play move of
// mz_selfplay_set_gumbel does (the root without noise, k_gz_root, the mz_gz_search loop; mz_gumbel.hip.h) and stores with
//
//   k_reanalyse_store_gumbel  the root's improved policy pi' as float32 where k_reanalyse_store puts the visit shares, then the
//                             root's mean value or its v_mix as the float64; k_gz_pick's mapping and mz_gz_root_pick, not restated
//
// Reanalyse on the true rules (mz_reanalyse_true_model; DESIGN s7n) keeps k_reanalyse_observe and k_reanalyse_store, and searches a
// stored position as a self-play move of mz_selfplay_set_true_model does (mz_truemodel.hip.h), from
//
//   k_tm_root_reanalyse       slot 0 of the true-rules tree = the position the stored observation and the record's mover determine
//                             (mz_reanalyse_position), then the root's first descent: k_tm_root_selfplay with the row as the environment
#pragma once
#include "mz_common.h"
#include "mz_tree.hip.h"
#include "mz_gumbel.hip.h"
#include "mz_truemodel.hip.h"
#include "mz_record.h"

// Separate from SelfplayState / EvalState / MatchState: self-play, evaluation and matches on the same engine are untouched.
struct ReanalyseState {
  float *obs;            // [Bp][O]
  uint8_t *legal;        // [B][A]
  int8_t *to_play;       // [B]
};

// The legal actions of a stored position, from its observation alone, as a bit mask; kind as in mz_selfplay_set_env:
//   0 synthetic, 2 CartPole: every action;
//   1 TicTacToe: the observation is to_play * board, cell k is free iff obs[k] == 0;
//   3 Connect Four: the observation is turn * board, column c is open iff its top cell obs[35 + c] == 0 (mz_c4_view on it).
__host__ __device__ inline uint32_t mz_reanalyse_legal_mask(int kind, const float *obs, int A) {
  uint32_t mask = 0;
  if (kind == 1) {
    for (int k = 0; k < 9; ++k) mask |= (obs[k] == 0.f ? 1u : 0u) << k;
  } else if (kind == 3) {
    for (int c = 0; c < 7; ++c) mask |= (obs[35 + c] == 0.f ? 1u : 0u) << c;
  } else {
    mask = A >= 32 ? 0xFFFFFFFFu : ((1u << A) - 1u);
  }
  return mask;
}

// The position of a stored row of a board game (kind 1 TicTacToe: 9 cells, 3 Connect Four: 42), from its observation and its mover:
// both games store mover * board, so the board is to_play * obs, and a ply puts one stone: *step = the non-zero cells.  to_play is
// the record's (MZ_REC_FLAG_P2), never the stones' parity: a position is a position for either mover.  bd: the game's cells, no more.
__host__ __device__ inline void mz_reanalyse_position(int kind, const float *obs, int to_play, int8_t *bd, int32_t *step) {
  const int cells = mz_game_info(kind).cells;      // (mz_games.h: the one statement of the games' sizes)
  int32_t n = 0;
  for (int k = 0; k < cells; ++k) {
    const int v = to_play * (int)obs[k];
    bd[k] = (int8_t)v;
    n += v != 0 ? 1 : 0;
  }
  *step = n;
}

// rows: the chunk's first row, [n][R] of unpacked records (include/mz_record.h; the mover is read from the flags word).  One thread per (row, observation element): neighbouring threads read neighbouring floats of the host row;
// the row's first thread also derives legal / to_play.  Rows b >= n of the chunk get what k_eval_observe feeds a finished game:
// a zero observation, every action legal, to_play +1.
static __global__ void k_reanalyse_observe(ReanalyseState rs, const float *rows, int n, int R, int kind, int B, int O, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * O) return;
  const int b = i / O, k = i - b * O;
  const bool real = b < n;
  const float *row = rows + (size_t)(real ? b : 0) * R;      // (never dereferenced for a row past n)
  rs.obs[i] = real ? row[k] : 0.f;
  if (k != 0) return;
  uint8_t *legal = rs.legal + (size_t)b * A;
  const uint32_t mask = real ? mz_reanalyse_legal_mask(kind, row, A) : 0xFFFFFFFFu;
  for (int a = 0; a < A; ++a) legal[a] = (uint8_t)((mask >> a) & 1u);
  const int32_t flags = real ? mz_rec_flags(mz_rec_tail(row, O, A)) : 0;
  rs.to_play[b] = (flags & MZ_REC_FLAG_P2) ? (int8_t)-1 : (int8_t)1;
}

// fresh: the chunk's first row, [n][A + 2]; nothing is stored for b >= n.  One thread per (row, float slot): slots 0..A-1 the
// visit shares, slots A and A + 1 the low and the high half of the root value's float64 (a row of A + 2 floats is 4-byte
// aligned only).  Plain vector stores.
static __global__ void k_reanalyse_store(TreeView t, float *fresh, int n) {
  const int A = t.A, F = A + 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = i / F, j = i - b * F;
  if (b >= t.B || b >= n) return;
  const size_t o = mz_slab(t, b);
  if (j < A) {
    const uint32_t legal = t.legal[b];
    fresh[i] = (float)mz_root_visit_share(t, o, legal, j, mz_root_visit_sum(t, o, legal));
  } else {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(mz_root_mean_value(t, o));
    ((uint32_t *)fresh)[i] = j == A ? (uint32_t)bits : (uint32_t)(bits >> 32);
  }
}

// fresh: the chunk's first row, [n][A + 2]; nothing is stored for b >= n.  k_gz_pick's mapping: one 64-lane workgroup per row
// (its 64 / G groups compute the same), lane = action.  Lanes wl < A store (float)pi'(a) -- exactly 0 on an illegal action --,
// lane 0 the two halves of the float64 value: the root's mean value (value_kind 0) or its v_mix (1), k_gz_move_record's rule.
// No LDS; plain vector stores.
template <int G>
__global__ __launch_bounds__(64) void k_reanalyse_store_gumbel(TreeView t, GzState gz, float *fresh, int n, int value_kind) {
  const int b = blockIdx.x, wl = threadIdx.x, lane = wl % G;
  if (b >= t.B || b >= n) return;
  const int A = t.A;
  double pi, vmix;
  float cR;
  (void)mz_gz_root_pick<G>(t, gz, b, lane, &pi, &vmix, &cR);
  float *row = fresh + (size_t)b * (A + 2);
  if (wl < A) row[wl] = (float)pi;
  if (wl != 0) return;
  const double rv = value_kind ? vmix : mz_root_mean_value(t, mz_slab(t, b));
  const unsigned long long bits = (unsigned long long)__double_as_longlong(rv);
  ((uint32_t *)row)[A] = (uint32_t)bits;
  ((uint32_t *)row)[A + 1] = (uint32_t)(bits >> 32);
}

// mz_tm_root for a reanalysed row (mz_reanalyse_true_model; DESIGN s7n): k_tm_root_selfplay's shape, one G-lane group per tree, the
// root's position from what k_reanalyse_observe left on the device -- rs.obs at stride O, rs.to_play --, no host copy.  A row past
// the chunk's n is the empty board with +1 to move and every action legal; k_reanalyse_store stores nothing for it.
template <int G>
__global__ void k_tm_root_reanalyse(TreeView t, TmState tm, int O, ReanalyseState rs) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  if (lane == 0) {
    MzTmSlotBits u;
    u.q[0] = u.q[1] = u.q[2] = u.q[3] = mz_i32x4{0, 0, 0, 0};
    const int tp = (int)rs.to_play[b];
    int32_t step;
    mz_reanalyse_position(tm.kind, rs.obs + (size_t)b * O, tp, u.s.bd, &step);
    u.s.mask = t.legal[b];
    u.s.step = step;
    u.s.mover = (int8_t)tp;
    mz_tm_slot_store(tm.slots + (size_t)b * (size_t)(t.sims + 1), u);
  }
  __threadfence_block();
  mz_tm_select<G>(t, tm, O, b, lane);
}
