// mz_gumbel_selfplay.hip.h -- the end of a self-play move searched with the Gumbel search (DESIGN s7i; gfx950, wave64; included
// by mz_engine.hip, -ffp-contract=off).  A move of a device game in this mode is k_game_observe, the initial inference,
// k_tree_root without noise, k_gz_root with the move read from the environments' counter, the mz_gz_search loop, and ONE launch
// of the kernel below: the pick of k_gz_pick, the experience record and the game's step.
//
// The record keeps its layout (mz_selfplay.hip.h): the child_visits slots hold (float)pi'(a) of the root -- exactly 0 on an
// illegal action --, the action is the Gumbel pick, root_value the root's mean value W / N (value_kind 0) or its v_mix
// (value_kind 1), error = root_value - the initial inference's value.  The visit-softmax temperature plays no part; the game
// step and the reset on done are mz_board_apply / mz_cartpole_apply, as k_board_step_record / k_cartpole_step_record call them
// (sp.temp[b] = *sp.temp_next included, so that the mode switched off finds the state a PUCT move would have left).
//
// Mapping: k_gz_pick's.  One 64-lane workgroup per tree, lane = action, mz_gz_root_pick over GzLanes<G>; the lanes store the
// observation and their own policy slot, lane 0 the record's tail and the game.  No LDS.  Latency bound: one round trip for the
// root's children, one for the game state.
#pragma once
#include "mz_gumbel.hip.h"
#include "mz_selfplay.hip.h"

// KIND: 1 TicTacToe, 2 CartPole, 3 Connect Four (mz_selfplay_set_env)
template <int G, int KIND>
__global__ __launch_bounds__(64) void k_gz_move_record(TreeView t, GzState gz, SelfplayState sp, int value_kind, uint64_t seed) {
  const int b = blockIdx.x, wl = threadIdx.x, lane = wl % G;
  if (b >= t.B) return;
  const int A = t.A;
  constexpr int O = KIND == 2 ? 4 : mz_game_info(KIND).cells;
  const unsigned long long move = sp.movecnt[b];      // (one wavefront: every lane has read it before lane 0 advances it)
  double pi, vmix;
  float cR;
  const int best = mz_gz_root_pick<G>(t, gz, b, lane, &pi, &vmix, &cR);
  (void)cR;
  float *rec = mz_rec_slot(sp.ring, move, sp.ring_moves, t.B, b, sp.rec_floats);
  for (int k = wl; k < O; k += 64) rec[k] = sp.obs[(size_t)b * O + k];
  if (wl < A) {
    rec[O + wl] = (float)pi;
    sp.child_visits[(size_t)b * A + wl] = pi;
  }
  if (wl != 0) return;
  sp.movecnt[b] = move + 1ull;
  const double rv = value_kind ? vmix : mz_root_mean_value(t, mz_slab(t, b));
  const double err = rv - (double)t.root_value[b];
  const int action = best < 0 ? 0 : best;      // (a root without a legal action: no device game has one)
  sp.action[b] = action; sp.root_value[b] = rv; sp.error[b] = err;
  if constexpr (KIND == 2) {
    const int tt = sp.t[b], ep = sp.episode[b];
    double st[4];
    for (int k = 0; k < 4; ++k) st[k] = sp.cart[(size_t)b * 4 + k];
    const int done = mz_cartpole_apply(sp, b, action, rv, err, rec, A, st, tt, ep, seed);
    for (int k = 0; k < 4; ++k) sp.cart[(size_t)b * 4 + k] = st[k];
    mz_store_next_move(sp, b, mz_next_move(sp, done, tt, ep));
  } else {
    mz_board_apply<KIND>(sp, b, action, rv, err, rec, A);
  }
}
