// mz_truemodel.hip.h -- the true-rules search of evaluation games and matches (DESIGN s7g; gfx950; included by mz_engine.hip,
// -ffp-contract=off).  The MCTS of mz_tree.hip.h -- the same PUCT, MinMaxStats, tie rules and backup, in the same node pool --
// in which a node below the root is a REAL position of TicTacToe or Connect Four: reached by mz_game_step from its parent's
// position, evaluated by the engine's representation + prediction on mz_game_observe of it, expanded over its legal actions
// only and closed where the game ends, with the true reward.  No hidden state is kept below the root; the side state of an
// expansion slot is one 64-byte record (MzTmSlot): the position, its child mask and whether it is finished.
//
// The mapping is that of the stand-alone tree kernels: G lanes per tree, lane = action, shuffle arg-max, whole 32-byte node
// records.  The descent does not track the board: it reads one word (the child mask) of every slot it passes beside the
// children's records, and lane 0 then forms the leaf's position from the PARENT slot's record and one mz_game_step.  Latency
// bound gather / scatter, like the tree kernels; the position record moves in four 16-byte accesses.
#pragma once
#include "mz_common.h"
#include "mz_games.h"
#include "mz_tree.hip.h"

// side state of one expansion slot, and (pend) of the leaf the last descent selected
struct alignas(16) MzTmSlot {
  int8_t bd[48];      // the position's cells (TicTacToe 9, Connect Four 42; the rest 0)
  uint32_t mask;      // bit a = child a exists: the legal actions of a live position, 0 of a finished one
  int32_t step;       // plies played
  float reward;       // of the move into it, in the view of the player who moved: 1 if it won, else 0
  int8_t mover;       // the player to move in it
  uint8_t fin;        // finished: won, or no cell left
  uint8_t revisit;    // pend only: the descent stopped at a finished node that has its slot already
  uint8_t pad_;
};
static_assert(sizeof(MzTmSlot) == 64, "MzTmSlot is four 16-byte words");
union MzTmSlotBits { MzTmSlot s; mz_i32x4 q[4]; };

struct TmState {
  int kind;            // 0 off, 1 TicTacToe, 3 Connect Four (mz_set_true_model)
  MzTmSlot *slots;     // [B][sims + 1], slot 0 = the root
  MzTmSlot *pend;      // [B] the selected leaf
  float *obs;          // [Bp][O] the leaves' observations (zeros for a finished leaf): the next inference's input
  uint8_t *leaf_fin;   // [B] pend[b].fin, flat for mz_tm_select's caller
  float *value;        // [Bp] the leaf inference's outputs (launch_root through a TreeView copy aimed here)
  float *logits;       // [Bp][A]
  bool root_set;       // mz_tm_root has recorded this move's root positions
};

__device__ __forceinline__ void mz_tm_slot_load(MzTmSlotBits &u, const MzTmSlot *src) {
  const mz_i32x4 *p = (const mz_i32x4 *)src;
  u.q[0] = p[0]; u.q[1] = p[1]; u.q[2] = p[2]; u.q[3] = p[3];
}
__device__ __forceinline__ void mz_tm_slot_store(MzTmSlot *dst, const MzTmSlotBits &u) {
  mz_i32x4 *p = (mz_i32x4 *)dst;
  p[0] = u.q[0]; p[1] = u.q[1]; p[2] = u.q[2]; p[3] = u.q[3];
}

// The leaf q = step(parent position, action) as a slot record: the rules are mz_games.h's.  Returns through u (the
// parent's record on entry); obs[O] = mz_game_observe(q) in the mover's view, zeros when q is finished.
__host__ __device__ inline void mz_tm_leaf(int kind, MzTmSlot &u, int action, int O, int A, float *obs) {
  const int mp = (int)u.mover, st = u.step;
  bool won = false;
  const bool done = mz_game_step(kind, u.bd, mp, action, st, &won);
  const uint32_t mask = done ? 0u : mz_game_legal(kind, u.bd);
  u.mover = (int8_t)-mp;
  u.step = st + 1;
  u.reward = won ? 1.f : 0.f;
  u.mask = mask;
  u.fin = (uint8_t)(mask == 0u ? 1 : 0);      // (a live position always has a legal action: a full board is done)
  u.revisit = 0;
  uint8_t legal[MZ_GAME_MAX_ACTIONS];
  mz_game_observe(kind, u.bd, -mp, nullptr, mask != 0u, O, A, obs, legal);
}

// The descent of MCTS.run (mz_tree_select's arithmetic, operation for operation) over the children that exist: at every
// expanded node the legal actions of its stored position.  It ends at a node that is not expanded, or at a finished one (a
// slot with an empty child mask): that is a revisit, nothing will be expanded.  Lane 0 then leaves the leaf's record in
// tm.pend[b] and its observation in tm.obs[b].
template <int G>
__device__ __forceinline__ void mz_tm_select(const TreeView &t, const TmState &tm, int O, int b, int lane) {
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  int32_t *path = t.path + (size_t)b * t.PL;
  MzTmSlot *slots = tm.slots + (size_t)b * (size_t)(t.sims + 1);
  const double mn = t.mn[b], mx = t.mx[b];
  int node = 0, parent_e = 0, len = 1, a_sel = -1;
  const MzNode root = mz_node_load(t, o);
  int tp = root.TP;
  if (lane == 0) path[0] = 0;
  int e = root.E, Np = root.N;
  bool revisit = false;
  while (e >= 0) {
    const uint32_t mask = slots[e].mask;      // (requested beside the children's records and the tables)
    const int ch = 1 + e * A + lane;
    const bool valid = lane < A && ((mask >> lane) & 1u);
    double score = 0.0;
    int best = -1, ce = -1, cn = 0;
    const double lgn = t.logtab[Np], sqn = t.sqrttab[Np];
    if (mask == 0u) { revisit = true; break; }      // a finished node: the same word in every lane of the group
    if (valid) {
      const MzNode c = mz_node_load(t, o + ch);
      const int Nc = c.N;
      const double p = c.P;
      ce = c.E; cn = Nc;
      if (Np == 0) {
        score = p;                                     // fresh root: rank by prior (mcts.py:105-108)
      } else {
        const double pb_c = lgn * (sqn / (double)(Nc + 1));
        const double prior_score = pb_c * p;
        double value_score;
        if (Nc > 0) {
          value_score = mz_normalize(mz_child_q(c.W, Nc, c.R, t.two_players, t.discount), mn, mx);
        } else {
          value_score = t.init_value_score;
        }
        score = prior_score + value_score;
      }
      best = lane;
    }
    // tuple max over (score, action): ties go to the largest action (mcts.py:106-112)
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) {
      const double os = __shfl_xor(score, off, G);
      const int ob = __shfl_xor(best, off, G), oe = __shfl_xor(ce, off, G), on = __shfl_xor(cn, off, G);
      const bool take = ob >= 0 && (best < 0 || os > score || (os == score && ob > best));
      if (take) { score = os; best = ob; ce = oe; cn = on; }
    }
    a_sel = best;
    parent_e = e;
    node = 1 + e * A + a_sel;
    if (lane == 0) path[len] = node;
    ++len;
    if (t.two_players) tp = -tp;
    e = ce;
    Np = cn;
  }
  if (lane == 0) {
    t.plen[b] = len;
    t.leaf_tp[b] = (int8_t)tp;
    t.leaf[b] = node;
    t.slot[b] = parent_e;
    t.act[b] = a_sel;
    t.depth[b] = len - 1;
    float *obs = tm.obs + (size_t)b * O;
    MzTmSlotBits u;
    if (revisit) {
      u.q[0] = u.q[1] = u.q[2] = u.q[3] = mz_i32x4{0, 0, 0, 0};
      u.s.reward = t.R[o + node];      // stored at its first visit
      u.s.mover = (int8_t)tp;
      u.s.fin = 1;
      u.s.revisit = 1;
      for (int k = 0; k < O; ++k) obs[k] = 0.f;
    } else {
      mz_tm_slot_load(u, slots + parent_e);
      mz_tm_leaf(tm.kind, u.s, a_sel, O, A, obs);
    }
    mz_tm_slot_store(tm.pend + b, u);
    tm.leaf_fin[b] = u.s.fin;
  }
}

// Node.expand over the leaf's legal actions (priors as mz_tree_root forms the root's: exp(logit) in double over the legal
// actions in ascending order, no max-shift, divided by their sum; an illegal child is marked TP = 0, prior 0) + the
// unchanged MCTS.backpropagate.  A finished leaf backs up value 0 with the true reward; at its first visit it takes its
// slot with an empty child mask, a revisit expands nothing.  value / logits: this tree's network outputs (unused when
// the leaf is finished).
template <int G>
__device__ __forceinline__ void mz_tm_expand_backup(const TreeView &t, const TmState &tm, int b, int lane, float value,
                                                    const float *logits) {
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  const int32_t *path = t.path + (size_t)b * t.PL;
  const int len = t.plen[b];
  const int tp = t.leaf_tp[b];
  const int e = t.nexp[b];
  const int leafnode = path[len - 1];
  MzTmSlotBits u;
  mz_tm_slot_load(u, tm.pend + b);      // (one address for the group's lanes)
  const bool revisit = u.s.revisit != 0, fin = u.s.fin != 0;
  const float reward = u.s.reward;
  if (!revisit) {
    const bool ok = lane < A && ((u.s.mask >> lane) & 1u);
    const double p = ok ? exp((double)logits[lane]) : 0.0;
    double sum = 0.0;
    for (int a = 0; a < A; ++a) sum = sum + __shfl(p, a, G);      // + 0.0 for illegal slots is exact
    if (lane < A) mz_node_fresh(t, o + 1 + e * A + lane, ok ? p / sum : 0.0, ok ? 1 : 0);
    if (lane < 4) ((mz_i32x4 *)(tm.slots + (size_t)b * (size_t)(t.sims + 1) + e))[lane] = u.q[lane];
  }
  double mn = 0.0, mx = 0.0, v = fin ? 0.0 : (double)value;
  if (lane == 0) { mn = t.mn[b]; mx = t.mx[b]; if (!revisit) t.nexp[b] = e + 1; }
  mz_tree_backup_path<G>(t, o, path, len, tp, lane, reward, v, mn, mx);
  if (lane == 0) {
    if (!revisit) {
      t.E[o + leafnode] = e;
      t.TP[o + leafnode] = (int8_t)tp;
      t.R[o + leafnode] = reward;
    }
    t.mn[b] = mn;
    t.mx[b] = mx;
  }
}

// ------------------------------------------------------------------ kernels
// mz_tm_root: slot 0 = the root's position (its child mask is the root's own, t.legal), then the first descent again, now
// with the leaf's position (mz_root_prepare's own first descent chose the same child: a fresh root ranks by prior)
template <int G>
__global__ void k_tm_root(TreeView t, TmState tm, int O, const int8_t *boards, const int8_t *turn, const int32_t *step) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  if (lane == 0) {
    MzTmSlotBits u;
    u.q[0] = u.q[1] = u.q[2] = u.q[3] = mz_i32x4{0, 0, 0, 0};
    const int cells = mz_game_info(tm.kind).cells;
    for (int k = 0; k < cells; ++k) u.s.bd[k] = boards[(size_t)b * 42 + k];
    u.s.mask = t.legal[b];
    u.s.step = step[b];
    u.s.mover = turn[b];
    mz_tm_slot_store(tm.slots + (size_t)b * (size_t)(t.sims + 1), u);
  }
  __threadfence_block();
  mz_tm_select<G>(t, tm, O, b, lane);
}

template <int G>
__global__ void k_tm_select(TreeView t, TmState tm, int O) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  mz_tm_select<G>(t, tm, O, b, lane);
}

// expand + backup of simulation s and (do_select) the descent of simulation s + 1 in one launch, as k_tree_step_ext
template <int G>
__global__ void k_tm_step(TreeView t, TmState tm, int O, const float *value, const float *logits, int do_select) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  mz_tm_expand_backup<G>(t, tm, b, lane, value[b], logits + (size_t)b * t.A);
  if (do_select) {
    __threadfence_block();          // lane 0's node and slot updates -> visible to the group's other lanes
    mz_tm_select<G>(t, tm, O, b, lane);
  }
}
