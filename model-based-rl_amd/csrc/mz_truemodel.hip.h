// mz_truemodel.hip.h -- the true-rules search of evaluation games and matches (DESIGN s7g) and of self-play (s7k: k_tm_search, all
// simulations in one launch, and k_tm_root_selfplay, at the end of this file); gfx950; included by mz_engine.hip, -ffp-contract=off.  The MCTS of mz_tree.hip.h -- the same PUCT, MinMaxStats, tie rules and backup, in the same node pool --
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
#include "mz_tree_host.h"      // (the host twin's trees, mz_truemodel_host.inc)
#include "mz_root.hip.h"       // (k_tm_search runs the leaf inference, mz_root_body, itself)

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
// legal: room for the A legal bytes mz_game_observe also writes (MZ_GAME_MAX_ACTIONS of them; not read here)
__host__ __device__ inline void mz_tm_leaf(int kind, MzTmSlot &u, int action, int O, int A, float *obs, uint8_t *legal) {
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
  mz_game_observe(kind, u.bd, -mp, nullptr, mask != 0u, O, A, obs, legal);
}

// the children that exist in a true-rules tree: at every expanded node the legal actions of its stored position (slot 0 holds
// the root's own mask); a finished node has none, and the descent stops at it
struct MzTmChildren {
  static constexpr bool stops = true;
  const MzTmSlot *slots;
  __device__ __forceinline__ bool exists(int e, int, int lane, bool &none) const {
    const uint32_t mask = slots[e].mask;      // (the same word in every lane of the group)
    none = mask == 0u;
    return (mask >> lane) & 1u;
  }
};

// The descent (mz_tree_descend by PUCT, mz_tree.hip.h) over those children.  It ends at a node that is not expanded, or at a
// finished one: that is a revisit, nothing will be expanded.  Lane 0 then leaves the leaf's record in tm.pend[b] and its
// observation in tm.obs[b].  WS (k_tm_search: LDS): lane 0 forms the record, which it indexes by cell at run time, in
// *ws and leaves mz_tm_leaf's legal bytes in legal_ws; else in private memory, 80 bytes of scratch in the stand-alone kernels.
template <int G, bool WS = false>
__device__ __forceinline__ void mz_tm_select(const TreeView &t, const TmState &tm, int O, int b, int lane,
                                             MzTmSlotBits *ws = nullptr, uint8_t *legal_ws = nullptr) {
  const size_t o = mz_slab(t, b);
  const MzTmSlot *slots = tm.slots + (size_t)b * (size_t)(t.sims + 1);
  MzPuctRule<G, MzTmChildren> rule = {t, o, lane, t.mn[b], t.mx[b], {slots}, 0};
  const MzDescent d = mz_tree_descend<G>(t, b, lane, rule);
  if (lane == 0) {
    float *obs = tm.obs + (size_t)b * O;
    MzTmSlotBits own;
    uint8_t own_legal[MZ_GAME_MAX_ACTIONS];
    MzTmSlotBits &u = WS ? *ws : own;
    uint8_t *legal = WS ? legal_ws : own_legal;
    if (d.stopped) {
      u.q[0] = u.q[1] = u.q[2] = u.q[3] = mz_i32x4{0, 0, 0, 0};
      u.s.reward = t.R[o + d.node];      // stored at its first visit
      u.s.mover = (int8_t)d.tp;
      u.s.fin = 1;
      u.s.revisit = 1;
      for (int k = 0; k < O; ++k) obs[k] = 0.f;
    } else {
      mz_tm_slot_load(u, slots + d.slot);
      mz_tm_leaf(tm.kind, u.s, d.act, O, t.A, obs, legal);
    }
    mz_tm_slot_store(tm.pend + b, u);
    tm.leaf_fin[b] = u.s.fin;
  }
}

// expand + backup (mz_tree_expand_backup) of the pending leaf over its position's legal actions.  A finished leaf backs up
// value 0 with the true reward; at its first visit it takes its slot with an empty child mask, a revisit expands nothing.
// value / logits: this tree's network outputs (unused when the leaf is finished).
template <int G>
__device__ __forceinline__ void mz_tm_expand_backup(const TreeView &t, const TmState &tm, int b, int lane, float value,
                                                    const float *logits) {
  MzTmSlotBits u;
  mz_tm_slot_load(u, tm.pend + b);      // (one address for the group's lanes)
  const bool grow = u.s.revisit == 0;
  const int e = mz_tree_expand_backup<G>(t, b, lane, u.s.fin != 0 ? 0.f : value, u.s.reward, logits, MzExpandMask{u.s.mask, grow});
  if (grow && lane < 4) {      // (the word picked by compares: indexing u.q by the lane would put the record into private memory)
    const mz_i32x4 q = lane == 0 ? u.q[0] : (lane == 1 ? u.q[1] : (lane == 2 ? u.q[2] : u.q[3]));
    ((mz_i32x4 *)(tm.slots + (size_t)b * (size_t)(t.sims + 1) + e))[lane] = q;
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

// mz_tm_root for a self-play move (mz_selfplay_set_true_model; DESIGN s7k): the root's position is the environment's own --
// sp.board at the game's own stride (TicTacToe [B][9], Connect Four [B][42]), sp.turn and sp.t -- on the stream, no host copy
template <int G>
__global__ void k_tm_root_selfplay(TreeView t, TmState tm, int O, SelfplayState sp) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  if (lane == 0) {
    MzTmSlotBits u;
    u.q[0] = u.q[1] = u.q[2] = u.q[3] = mz_i32x4{0, 0, 0, 0};
    const int cells = mz_game_info(tm.kind).cells;
    for (int k = 0; k < cells; ++k) u.s.bd[k] = sp.board[(size_t)b * cells + k];
    u.s.mask = t.legal[b];
    u.s.step = sp.t[b];
    u.s.mover = sp.turn[b];
    mz_tm_slot_store(tm.slots + (size_t)b * (size_t)(t.sims + 1), u);
  }
  __threadfence_block();
  mz_tm_select<G>(t, tm, O, b, lane);
}

// All the simulations of a true-rules search in ONE launch (mz_tm_search_fused; DESIGN s7k).  A true-rules simulation keeps no
// hidden state, and a tree's next leaf depends on that tree alone: the workgroup that runs the leaf inference of its 16 rows
// (mz_root_body, k_root's body, on tm.obs) also runs the tree step of those 16 trees, and goes round nsims times.  No grid-wide
// dependency arises.  Grid Bp / MZ_ROWS, 256 threads; tree m of the workgroup has the 16-lane slot [16 m, 16 m + 16) -- the
// threads that combined row m's value and logits --, of which the first G lanes work (lane = action; G-aligned, as the shuffles
// of mz_group_argmax need).  sel_last: the descent behind the call's last simulation is made (the pool is not used up).
// Every thread reaches every barrier: rows past B and the idle lanes are predicated, not returned.  The leaf's value and logits
// are read from the body's LDS copies; tm.obs, written by lane 0 of a tree and read by the next inference's loader threads,
// passes through global memory behind the barrier (the waves of a workgroup share the CU's L1; __syncthreads waits for the
// outstanding stores).  Bound by the latency chain of 2 nsims dependent phases per workgroup.
template <int JTP, int G>
__global__ __launch_bounds__(256, 1) void k_tm_search(NetView n, TreeView t, TmState tm, const f32x4 *istream, int nst0,
                                                       int nsims, int sel_last) {
  static_assert(G <= 16, "one 16-lane slot per tree");
  __shared__ __attribute__((aligned(16))) float smem[MZ_ROOT_LDS_FLOATS];
  const float *s_val = smem + MZ_ROOT_LDS_VAL, *s_lg = s_val + 16;      // (mz_root_body's)
  const int tid = (int)threadIdx.x, mt = tid >> 4, tl = tid & 15;
  const int b = blockIdx.x * MZ_ROWS + mt;
  const bool work = b < t.B && tl < G;
  // lane 0's position record and legal bytes: in the observation tile, which is dead between the body's first stage and the next
  // body's (both lie behind a barrier)
  MzTmSlotBits *ws = (MzTmSlotBits *)smem + mt;
  uint8_t *legal_ws = (uint8_t *)(smem + 16 * (sizeof(MzTmSlotBits) / sizeof(float))) + mt * MZ_GAME_MAX_ACTIONS;
  static_assert(16 * sizeof(MzTmSlotBits) + 16 * MZ_GAME_MAX_ACTIONS <= 16 * MZ_ROOT_XS * sizeof(float), "inside the observation tile");
  TreeView leaf_tv = t;      // the leaf inference's outputs land in the true-model state (as mz_tm_search's)
  leaf_tv.root_value = tm.value;
  leaf_tv.root_logits = tm.logits;
  const SelfplayState no_sp = {};
  for (int s = 0; s < nsims; ++s) {
    mz_root_body<JTP, 4, false, 0>(n, leaf_tv, tm.obs, istream, nst0, no_sp, 0ull, 0.0, 0.0, smem, tid, nullptr, MzNoStamp(), nullptr);
    __syncthreads();
    if (work) {
      mz_tm_expand_backup<G>(t, tm, b, tl, s_val[mt], s_lg + mt * 32);
      if (s + 1 < nsims || sel_last) {
        __threadfence_block();          // lane 0's node and slot updates -> visible to the group's other lanes
        mz_tm_select<G, true>(t, tm, n.O, b, tl, ws, legal_ws);
      }
    }
    __syncthreads();
  }
}
