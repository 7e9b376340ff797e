// mz_playout.hip.h -- the playout-search (UCT) opponent of the device evaluation games (DESIGN s7d): a classical
// Monte-Carlo tree search on the TRUE rules of TicTacToe (kind 1) and Connect Four (kind 3), random playouts, no network
// (gfx950; included by mz_engine.hip, -ffp-contract=off).  One wave plans one game's move; the tree and the 64 lanes'
// playout boards live in LDS.  Every iteration spends exactly 64 playouts (one per lane), so a budget of N playouts is
// I = N / 64 iterations and the tree holds at most 1 + I nodes.
//
// Everything is integer arithmetic except the UCB1 score, which uses only exactly rounded float64 operations (int ->
// double, *, /, +, sqrt) on integers and a table of logarithms the HOST computes: the bodies below are __host__ __device__
// and mz_playout_plan_host (include/mz_engine_debug.h) runs them with the lanes looped on the host, bit for bit the
// device's plan.  Only po_evaluate's reduction over the lanes differs between the two (wave ballots / a loop).
//
// The rules are mz_game_step / mz_game_legal / mz_nth_legal of mz_games.h and nothing else (no second form).
#pragma once
#include <math.h>
#include "mz_common.h"
#include "mz_rng.h"
#include "mz_games.h"

#define MZ_PO_LANES 64
#define MZ_PO_MIN_PLAYOUTS 64
#define MZ_PO_MAX_PLAYOUTS 65536
#define MZ_PO_MAX_ITERS (MZ_PO_MAX_PLAYOUTS / MZ_PO_LANES)
#define MZ_PO_BOARD_STRIDE 44      // bytes between two lanes' boards: 11 words, an odd count, so the lanes' cells fall on distinct banks

#if defined(__HIP_DEVICE_COMPILE__)
#define MZ_PO_DEVICE 1
// the lanes of one wave run in lock-step; what lane 0 wrote to LDS is ordered before what all lanes read next
#define MZ_PO_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define MZ_PO_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // a value every lane computed alike, handed to the scalar unit
#else
#define MZ_PO_DEVICE 0
#define MZ_PO_SYNC() do { } while (0)
#define MZ_PO_UNIFORM(x) (x)
#endif

// A node is a position; its statistics live on its A edges.  n: playouts through the edge; w: 2 * wins + draws of the
// node's mover; kid: the child node or -1; end: 0 open, 1 the mover wins by the action, 2 the action ends the game drawn.
// parent / pact: the edge that leads to the node (the backup walks them up to the root, node 0).
struct PoTree {
  int32_t *n, *w;
  int16_t *kid, *parent;
  uint8_t *end, *pact;
  int A, nodes;
};

// bytes of one wave's planning memory: the tree of `nodes` nodes, 64 playout boards and the root board
__host__ __device__ inline size_t po_wave_bytes(int nodes, int A) {
  const size_t na = (size_t)nodes * A;
  size_t b = 4 * na + 4 * na + 2 * na + 2 * (size_t)nodes + na + (size_t)nodes;
  b = (b + 3) & ~(size_t)3;
  b += (size_t)MZ_PO_LANES * MZ_PO_BOARD_STRIDE + MZ_PO_BOARD_STRIDE;
  return (b + 15) & ~(size_t)15;
}
__host__ __device__ inline void po_carve(unsigned char *mem, int nodes, int A, PoTree *t, int8_t **boards, int8_t **root) {
  const size_t na = (size_t)nodes * A;      // (offsets, not pointer arithmetic on integers: the LDS address space stays known)
  const size_t w = 4 * na, kid = 8 * na, parent = 10 * na, end = parent + 2 * (size_t)nodes, pact = end + na;
  const size_t lanes = (pact + (size_t)nodes + 3) & ~(size_t)3;
  t->A = A; t->nodes = nodes;
  t->n = (int32_t *)mem;
  t->w = (int32_t *)(mem + w);
  t->kid = (int16_t *)(mem + kid);
  t->parent = (int16_t *)(mem + parent);
  t->end = mem + end;
  t->pact = mem + pact;
  *boards = (int8_t *)(mem + lanes);
  *root = (int8_t *)(mem + lanes + (size_t)MZ_PO_LANES * MZ_PO_BOARD_STRIDE);
}

// ---- the rules, under the planner's names: the shared functions of mz_games.h, nothing restated
__host__ __device__ inline uint32_t po_legal(int kind, const int8_t *bd) { return mz_game_legal(kind, bd); }
__host__ __device__ inline bool po_step(int kind, int8_t *bd, int turn, int action, int t, bool *won) {
  return mz_game_step(kind, bd, turn, action, t, won);
}
__host__ __device__ inline int po_nth(uint32_t mask, int i) { return mz_nth_legal(mask, i); }

// ---- one lane's playout from a fresh node: `first` by the node's mover `turn` (t plies played before it), then uniformly
// random legal moves to the end.  Byte j of the 16 bytes of Philox call c (x, y, z, w, each low byte first) serves random
// ply 16 c + j: index (byte * k) >> 8 of the position's k legal actions in ascending order.  Returns 2 / 1 / 0: the node's
// mover wins / a draw / loses; *endflag: `first` itself ended the game (1 won, 2 drawn) or not (0).  bd is used up.
__host__ __device__ inline int po_playout(int kind, int8_t *bd, int turn, int t, int first, uint64_t seed, uint32_t env,
                                          uint32_t move, uint32_t iter, int lane, int *endflag) {
  const int mover = turn;
  bool won = false;
  bool done = po_step(kind, bd, turn, first, t, &won);
  *endflag = done ? (won ? 1 : 2) : 0;
  mz_u4 r = {0u, 0u, 0u, 0u};
  for (int p = 0; !done && p < 48; ++p) {      // (a game lasts 42 plies at the most; the bound is a guard, not a rule)
    turn = -turn; ++t;
    const int j = p & 15;
    if (j == 0) r = mz_philox(seed, env, move, iter, (MZ_RNG_PLAYOUT << 24) | ((uint32_t)lane << 4) | (uint32_t)(p >> 4));
    const uint32_t word = j < 4 ? r.x : (j < 8 ? r.y : (j < 12 ? r.z : r.w));
    const uint32_t byte = (word >> (8 * (j & 3))) & 255u;
    const uint32_t mask = po_legal(kind, bd);
    const int k = __builtin_popcount(mask);
    if (k == 0) { won = false; break; }      // (no legal action and not done: not a position of the game; a guard)
    done = po_step(kind, bd, turn, po_nth(mask, (int)((byte * (uint32_t)k) >> 8)), t, &won);
  }
  return won ? (turn == mover ? 2 : 0) : 1;
}

// ---- UCB1 at a node with statistics: the legal a (n[a] > 0: a fresh node's evaluation gives every legal action at least
// 64 / 9 playouts) that maximises w / (2 n) + sqrt(2 LN[V] / n), V = sum n / 64; ties to the lowest a
__host__ __device__ inline int po_pick(const PoTree &t, int node, const double *LN) {
  const int32_t *n = t.n + (size_t)node * t.A, *w = t.w + (size_t)node * t.A;
  int total = 0;
  for (int a = 0; a < t.A; ++a) total += n[a];
  const double ln = LN[total / 64];
  int best = 0;
  double best_score = 0.0;
  bool have = false;
  for (int a = 0; a < t.A; ++a) {
    if (n[a] <= 0) continue;
    const double na = (double)n[a];
    const double score = (double)w[a] / (2.0 * na) + sqrt(2.0 * ln / na);
    if (!have || score > best_score) { best = a; best_score = score; have = true; }
  }
  return best;
}

// the reduced results of one action of a fresh node
__host__ __device__ inline void po_node_set(const PoTree &t, int node, int a, int count, int w, int end) {
  t.n[(size_t)node * t.A + a] = count;
  t.w[(size_t)node * t.A + a] = w;
  t.end[(size_t)node * t.A + a] = (uint8_t)end;
}

// every edge taken gets 64 playouts and the iteration's value as its node's mover sees it: v at (node, a), 128 - v one up
__host__ __device__ inline void po_backup(const PoTree &t, int node, int a, int v) {
  for (;;) {
    t.n[(size_t)node * t.A + a] += 64;
    t.w[(size_t)node * t.A + a] += v;
    if (node == 0) break;
    a = t.pact[node];
    node = t.parent[node];
    v = 128 - v;
  }
}

// the root action with the most playouts; ties to the larger w, then to the lowest a
__host__ __device__ inline int po_move(const PoTree &t) {
  int best = 0;
  for (int a = 1; a < t.A; ++a)
    if (t.n[a] > t.n[best] || (t.n[a] == t.n[best] && t.w[a] > t.w[best])) best = a;
  return best;
}

// ---- a fresh node: lane l takes the (l % k)-th of its k legal actions and plays it out; the results are summed per action
// into the node's edges.  Returns the 64 lanes' sum (0 .. 128) as the node's mover sees it.  pb: the node's position
// (device: this lane's own copy, used up by its playout; host: the one copy, left as it is).
__host__ __device__ inline int po_evaluate(int kind, const PoTree &t, int node, int8_t *pb, int turn, int step, uint64_t seed,
                                           uint32_t env, uint32_t move, uint32_t iter, int lane) {
  const uint32_t mask = MZ_PO_UNIFORM(po_legal(kind, pb));
  const int k = __builtin_popcount(mask);
  if (k == 0) return 64;      // (never reached: an edge that ends the game has no child)
  int total = 0;
#if MZ_PO_DEVICE
  const int first = po_nth(mask, lane % k);
  int endflag;
  const int res = po_playout(kind, pb, turn, step, first, seed, env, move, iter, lane, &endflag);
  for (int a = 0; a < t.A; ++a) {      // lanes whose playout ended early wait here
    if (!((mask >> a) & 1u)) continue;
    const bool mine = first == a;
    const int count = __popcll(__ballot(mine));
    const int w = 2 * __popcll(__ballot(mine && res == 2)) + __popcll(__ballot(mine && res == 1));
    const int end = __ballot(mine && endflag == 1) ? 1 : (__ballot(mine && endflag == 2) ? 2 : 0);
    if (lane == 0) po_node_set(t, node, a, count, w, end);
    total += w;
  }
#else
  int count[9] = {0}, w[9] = {0}, end[9] = {0};
  for (int l = 0; l < MZ_PO_LANES; ++l) {
    int8_t lb[42];
    for (int c = 0; c < 42; ++c) lb[c] = pb[c];
    const int first = po_nth(mask, l % k);
    int endflag;
    const int res = po_playout(kind, lb, turn, step, first, seed, env, move, iter, l, &endflag);
    count[first] += 1; w[first] += res;
    if (endflag) end[first] = endflag;
  }
  for (int a = 0; a < t.A; ++a) {
    if (!((mask >> a) & 1u)) continue;
    po_node_set(t, node, a, count[a], w[a], end[a]);
    total += w[a];
  }
  (void)lane;
#endif
  MZ_PO_SYNC();
  return total;
}

// ---- one game's plan: I iterations from the root position (root[42], mover turn0, step0 plies played), then the move.
// Device: called by all 64 lanes of the wave with the wave's memory (po_carve); lane_board is this lane's own board.
// Host: called once (lane 0); lane_board is the one path board.  visits_out / wins_out [A] may be null.
__host__ __device__ inline void po_plan(int kind, const PoTree &t, int8_t *lane_board, const int8_t *root, int turn0, int step0,
                                        int iters, const double *LN, uint64_t seed, uint32_t env, uint32_t move, int lane,
                                        int32_t *action_out, int32_t *visits_out, int32_t *wins_out) {
  const int A = t.A, na = t.nodes * A;
  for (int i = MZ_PO_DEVICE ? lane : 0; i < na; i += MZ_PO_DEVICE ? MZ_PO_LANES : 1) {
    t.n[i] = 0; t.w[i] = 0; t.kid[i] = -1; t.end[i] = 0;
  }
  MZ_PO_SYNC();
  int count = 1;      // nodes in use; one more per iteration after the first at the most, so never above iters = nodes - 1
  for (int it = 0; it < iters; ++it) {
    for (int c = 0; c < 42; ++c) lane_board[c] = root[c];
    int turn = turn0, step = step0, node = 0, a = 0, v;
    if (it == 0) {      // the root, fresh; no edge was taken, so nothing is backed up
      (void)po_evaluate(kind, t, 0, lane_board, turn, step, seed, env, move, (uint32_t)it, lane);
      continue;
    }
    for (;;) {
      a = MZ_PO_UNIFORM(po_pick(t, node, LN));
      const int end = MZ_PO_UNIFORM((int)t.end[(size_t)node * A + a]);
      if (end) { v = end == 1 ? 128 : 64; break; }
      bool won;
      po_step(kind, lane_board, turn, a, step, &won);
      turn = -turn; ++step;
      int kid = MZ_PO_UNIFORM((int)t.kid[(size_t)node * A + a]);
      if (kid < 0) {
        if (count >= t.nodes) { v = 64; break; }      // (unreachable, see count; no node outside the tree is ever written)
        kid = count++;
        if (lane == 0) {
          t.kid[(size_t)node * A + a] = (int16_t)kid;
          t.parent[kid] = (int16_t)node;
          t.pact[kid] = (uint8_t)a;
        }
        MZ_PO_SYNC();
        v = 128 - po_evaluate(kind, t, kid, lane_board, turn, step, seed, env, move, (uint32_t)it, lane);
        break;
      }
      node = kid;
    }
    if (lane == 0) po_backup(t, node, a, v);
    MZ_PO_SYNC();
  }
  if (lane == 0) {
    *action_out = po_move(t);
    for (int a = 0; a < A; ++a) {
      if (visits_out) visits_out[a] = t.n[a];
      if (wins_out) wins_out[a] = t.w[a];
    }
  }
}

// The planner's own device memory (mz_playout_plan and the opponent of mz_eval_env_moves), allocated on first use: the
// table of logarithms and the staging of mz_playout_plan's positions and plans.  Separate from EvalState, as ReanalyseState is.
struct PlayoutState {
  double *ln;            // [MZ_PO_MAX_ITERS + 1] LN[v] = log(64 v) as the host's std::log rounds it (LN[0] = 0, never read)
  int8_t *boards;        // [B][42]
  int8_t *turn;          // [B]
  int32_t *step;         // [B]
  int32_t *action;       // [B]
  int32_t *visits;       // [B][A]
  int32_t *wins;         // [B][A]
};

// One wave per game, blockDim.x / 64 games per block, no barrier between the waves of a block (they plan different games).
// per_wave: po_wave_bytes(iters + 1, A), the wave's share of the dynamic LDS.  A game that is over (terminal, where given)
// or whose mover is not only_mover (where nonzero) leaves at once and its outputs stay as they are.
static __global__ __launch_bounds__(256) void k_playout_plan(int kind, int A, const int8_t *boards, const int8_t *turn,
                                                              const int32_t *step, const uint8_t *terminal, int only_mover,
                                                              int n, int iters, const double *LN, uint64_t seed,
                                                              int env_offset, uint32_t move, int per_wave, int32_t *action_out,
                                                              int32_t *visits_out, int32_t *wins_out) {
  extern __shared__ __align__(16) unsigned char po_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x * (blockDim.x >> 6) + wave;
  if (g >= n) return;
  if (terminal && terminal[g]) return;
  const int turn0 = turn[g];
  if (only_mover && turn0 != only_mover) return;
  PoTree t;
  int8_t *lane_boards, *root;
  po_carve(po_lds + (size_t)wave * per_wave, iters + 1, A, &t, &lane_boards, &root);
  if (lane < 42) root[lane] = boards[(size_t)g * 42 + lane];
  MZ_PO_SYNC();
  po_plan(kind, t, lane_boards + lane * MZ_PO_BOARD_STRIDE, root, turn0, step[g], iters, LN, seed, (uint32_t)(env_offset + g),
          move, lane, action_out + g, visits_out ? visits_out + (size_t)g * A : nullptr,
          wins_out ? wins_out + (size_t)g * A : nullptr);
}
