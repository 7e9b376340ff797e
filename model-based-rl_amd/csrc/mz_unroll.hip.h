// mz_unroll.hip.h -- the learned model graded by unroll depth against the true game (DESIGN s7f, "Grading by unroll depth";
// gfx950; included by mz_engine.hip).  A row is a start position p_0 of TicTacToe (kind 1) or Connect Four (kind 3) and up
// to K <= 16 actions.  Its LINE is p_0, p_1 = step(p_0, a_0), ... on the true rules of mz_games.h, while an action is given
// (>= 0), the position is not terminal and the action is legal; depth = the actions applied.  Beside the line the network is
// unrolled along the same actions (mz_unroll, mz_unroll_abi.inc): h_0 = representation(p_0), h_k = dynamics(h_{k-1},
// a_{k-1}), and every real p_k is seen afresh through the representation.  The TERMS reduce, per (row, k), the unrolled and
// the fresh outputs, the legal mask and the solver's values of p_k to the scalars the report averages.
//
// Both bodies are __host__ __device__: mz_unroll_lines_host and mz_unroll_terms_host (include/mz_engine_debug.h) run them on
// the CPU.  Lines are integers (and float casts of -1 / 0 / +1), so the two sides agree bit for bit.  The terms are float64
// sums in ascending action order on both sides; only exp() differs between the libraries, in the last places.
//
// Layout on the device: everything per (depth, row) is DEPTH-MAJOR, [K + 1][num_envs][...], so the rows of one depth are
// the contiguous batch mz_initial_inference and mz_recurrent_inference take as it stands.
#pragma once
#include "mz_common.h"
#include "mz_games.h"

#define MZ_UR_MAXK 16
#define MZ_UR_FLAG_ILLEGAL 1      // the line stopped at an action that is illegal in its position

// the scalars of one (row, k), float64 each.  Zero unless their set holds: LIVE k <= depth; TRANS LIVE and k >= 1 (transition
// k, p_{k-1} -> p_k); POS LIVE and p_k not terminal; SOLVED POS and the true value v* of p_k is known.
enum MzUnrollTerm {
  MZ_UR_LIVE, MZ_UR_TRANS, MZ_UR_POS,
  MZ_UR_RTRUE, MZ_UR_REW, MZ_UR_REW_ERR,                                  // TRANS: true reward, predicted reward, |difference|
  MZ_UR_VAL, MZ_UR_VAL_F, MZ_UR_DRIFT,                                    // POS: v_u, v_f, |v_u - v_f|
  MZ_UR_TV, MZ_UR_TOP1, MZ_UR_ILL, MZ_UR_ILL_F,                           // POS: 1/2 sum |softmax u - softmax f|, arg-max agree, illegal mass
  MZ_UR_SOLVED, MZ_UR_VSTAR, MZ_UR_VERR, MZ_UR_VERR_F,                    // SOLVED: v*, |v_u - v*|, |v_f - v*|
  MZ_UR_SIGN, MZ_UR_SIGN_F, MZ_UR_OPT, MZ_UR_OPT_F,                       // SOLVED: sign(v) == v* (v* != 0), mass on optimal actions
  MZ_UR_NT
};

// ---- the line of one row.  start[42], turn, step: p_0 (not terminal: the caller checked).  actions[K]: -1 ends the line.
// bd: scratch [K + 1][42] of the row's own.  Everything per depth is written at index k * ks of the pointers given, which
// point at the row's depth 0 (ks: the items between two depths of one row -- num_envs on the device, 1 on the host): obs[O]
// = turn * board as float32 (mz_game_observe's formula), legal = mz_game_legal of p_k, terminal, rtrue = 1.0 if the move into
// p_k won, act = the action applied IN p_k (0 where none is).  Depths past the line's end are written as zero.
__host__ __device__ inline void ur_line(int kind, int O, int A, int K, const int8_t *start, int turn, int step, const int32_t *actions,
                                        int8_t *bd, size_t ks, float *obs, uint32_t *legal, uint8_t *terminal, float *rtrue,
                                        int32_t *act, int32_t *depth_out, int32_t *flags_out) {
  for (int c = 0; c < 42; ++c) bd[c] = start[c];
  bool alive = true, term = false;
  float rt = 0.f;
  int depth = 0, flags = 0;
  int8_t *cur = bd;
  for (int k = 0; k <= K; ++k) {
    float *ob = obs + (size_t)k * ks * (size_t)O;
    uint32_t mask = 0;
    if (alive) {
      mask = mz_game_legal(kind, cur);
      for (int c = 0; c < O; ++c) ob[c] = mz_c4_obs_cell(cur, turn, c);
      depth = k;
    } else {
      for (int c = 0; c < O; ++c) ob[c] = 0.f;
    }
    legal[(size_t)k * ks] = mask;
    terminal[(size_t)k * ks] = (uint8_t)(alive && term ? 1 : 0);
    rtrue[(size_t)k * ks] = alive ? rt : 0.f;
    int applied = 0;
    bool next = false;
    if (alive && !term && k < K) {
      const int a = actions[k];
      if (a >= 0) {
        if (a >= A || !((mask >> a) & 1u)) {
          flags |= MZ_UR_FLAG_ILLEGAL;
        } else {
          int8_t *nx = cur + 42;
          for (int c = 0; c < 42; ++c) nx[c] = cur[c];
          bool won;
          term = mz_game_step(kind, nx, turn, a, step + k, &won);
          rt = won ? 1.f : 0.f;
          turn = -turn;
          cur = nx;
          applied = a;
          next = true;
        }
      }
    }
    act[(size_t)k * ks] = applied;
    alive = next;
  }
  *depth_out = depth;
  *flags_out = flags;
}

// ---- the terms of one (row, k).  lu / lf [A]: the unrolled and the fresh policy logits (float32 as the network gave them);
// eu / ef [A]: exp(logit - max logit) in float64 (ur_exp_arg gives the argument; the caller takes the exponential with its
// own library).  truth [A] or null: the solver's values of p_k's actions (+1 / 0 / -1, -2 illegal, -3 unsolved).  Every sum
// runs over the actions in ascending order; ties of the arg-max go to the largest action.
__host__ __device__ inline double ur_exp_arg(const float *lg, int A, int a) {
  float mx = lg[0];
  for (int i = 1; i < A; ++i) mx = lg[i] > mx ? lg[i] : mx;
  return (double)lg[a] - (double)mx;
}
__host__ __device__ inline double ur_abs(double x) { return x < 0.0 ? -x : x; }
__host__ __device__ inline void ur_terms(int A, const float *lu, const float *lf, const double *eu, const double *ef, uint32_t legal,
                                         bool terminal, bool live, int k, float rtrue, float ru, float vu, float vf,
                                         const int8_t *truth, double *out) {
  for (int i = 0; i < MZ_UR_NT; ++i) out[i] = 0.0;
  if (!live) return;
  out[MZ_UR_LIVE] = 1.0;
  if (k >= 1) {
    out[MZ_UR_TRANS] = 1.0;
    out[MZ_UR_RTRUE] = (double)rtrue;
    out[MZ_UR_REW] = (double)ru;
    out[MZ_UR_REW_ERR] = ur_abs((double)ru - (double)rtrue);
  }
  if (terminal) return;
  out[MZ_UR_POS] = 1.0;
  out[MZ_UR_VAL] = (double)vu;
  out[MZ_UR_VAL_F] = (double)vf;
  out[MZ_UR_DRIFT] = ur_abs((double)vu - (double)vf);
  double su = 0.0, sf = 0.0;
  for (int a = 0; a < A; ++a) { su += eu[a]; sf += ef[a]; }
  double tv = 0.0, ill = 0.0, illf = 0.0;
  int bu = 0, bf = 0;
  for (int a = 0; a < A; ++a) {
    const double pu = eu[a] / su, pf = ef[a] / sf;
    tv += ur_abs(pu - pf);
    if (!((legal >> a) & 1u)) { ill += pu; illf += pf; }
    if (lu[a] >= lu[bu]) bu = a;
    if (lf[a] >= lf[bf]) bf = a;
  }
  out[MZ_UR_TV] = 0.5 * tv;
  out[MZ_UR_TOP1] = bu == bf ? 1.0 : 0.0;
  out[MZ_UR_ILL] = ill;
  out[MZ_UR_ILL_F] = illf;
  if (!truth) return;
  // v* = the best value of a legal action; known when it is +1 or no legal action is unsolved (solver.grade_games's rule
  // without the chosen-action clause)
  int best = -3;
  bool unsolved = false;
  for (int a = 0; a < A; ++a) {
    if (!((legal >> a) & 1u)) continue;
    const int t = (int)truth[a];
    if (t > best) best = t;
    if (t < -1) unsolved = true;
  }
  if (!(best == 1 || (!unsolved && best >= -1))) return;
  out[MZ_UR_SOLVED] = 1.0;
  out[MZ_UR_VSTAR] = (double)best;
  out[MZ_UR_VERR] = ur_abs((double)vu - (double)best);
  out[MZ_UR_VERR_F] = ur_abs((double)vf - (double)best);
  if (best != 0) {
    out[MZ_UR_SIGN] = ((vu > 0.f) - (vu < 0.f)) == best ? 1.0 : 0.0;
    out[MZ_UR_SIGN_F] = ((vf > 0.f) - (vf < 0.f)) == best ? 1.0 : 0.0;
  }
  double opt = 0.0, optf = 0.0;
  for (int a = 0; a < A; ++a)
    if (((legal >> a) & 1u) && (int)truth[a] == best) { opt += eu[a] / su; optf += ef[a] / sf; }
  out[MZ_UR_OPT] = opt;
  out[MZ_UR_OPT_F] = optf;
}

// mz_unroll's own device memory, allocated on first use for num_envs rows and MZ_UR_MAXK + 1 depths; K1 = K + 1 of the call
struct UnrollState {
  int8_t *start;         // [B][42] the chunk's start positions
  int8_t *turn;          // [B]
  int32_t *step;         // [B]
  int32_t *actions;      // [B][K]
  int8_t *truth;         // [B][K1][A]
  int8_t *boards;        // [B][17][42] the line kernel's scratch
  float *obs;            // [17][B][O]
  uint32_t *legal;       // [17][B]
  uint8_t *terminal;     // [17][B]
  float *rtrue;          // [17][B]
  int32_t *act;          // [17][B]
  int32_t *depth;        // [B]
  int32_t *flags;        // [B]
  float *hid_u;          // [17][B][MZ_H]
  float *rew_u, *val_u, *val_f;      // [17][B]
  float *lg_u, *lg_f;    // [17][B][A]
  double *terms;         // [B][K1][MZ_UR_NT]
  float *raw;            // [B][K1][O + MZ_H + 2 A + 4]: obs, hidden_u, logits_u, logits_f, value_u, reward_u, value_f, reward_true
  int32_t *raw_meta;     // [B][K1][2]: legal mask, terminal
};

// one thread a row of the staging (B rows: rows m .. B - 1 are written as empty lines, so that no depth's batch carries a
// former chunk's rows)
static __global__ __launch_bounds__(64) void k_unroll_lines(int kind, int O, int A, int K, int m, int B, UnrollState u) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  if (r < m) {
    ur_line(kind, O, A, K, u.start + (size_t)r * 42, (int)u.turn[r], u.step[r], u.actions + (size_t)r * K,
            u.boards + (size_t)r * (MZ_UR_MAXK + 1) * 42, (size_t)B, u.obs + (size_t)r * O, u.legal + r, u.terminal + r, u.rtrue + r,
            u.act + r, u.depth + r, u.flags + r);
    return;
  }
  for (int k = 0; k <= K; ++k) {
    const size_t it = (size_t)k * B + r;
    for (int c = 0; c < O; ++c) u.obs[it * O + c] = 0.f;
    u.legal[it] = 0; u.terminal[it] = 0; u.rtrue[it] = 0.f; u.act[it] = 0;
  }
  u.depth[r] = -1; u.flags[r] = 0;
}

// scatter: the engine's root outputs (mz_initial_inference of the depth-k batch) -> the fresh value and logits of depth k;
// at k = 0 also the unrolled ones and h_0 (unrolled and fresh are one computation there).  64 threads a row; a row whose
// line does not reach k is written as zero.
static __global__ __launch_bounds__(64) void k_unroll_take_root(TreeView t, int k, int B, int A, UnrollState u) {
  const int r = blockIdx.x, j = threadIdx.x;
  if (r >= B) return;
  const bool live = k <= u.depth[r];
  const size_t it = (size_t)k * B + r;
  if (j < A) {
    const float lg = live ? t.root_logits[(size_t)r * A + j] : 0.f;
    u.lg_f[it * A + j] = lg;
    if (k == 0) u.lg_u[it * A + j] = lg;
  }
  if (j == A) {
    const float v = live ? t.root_value[r] : 0.f;
    u.val_f[it] = v;
    if (k == 0) { u.val_u[it] = v; u.rew_u[it] = 0.f; }
  }
  if (k == 0 && j < MZ_H) u.hid_u[it * MZ_H + j] = live ? t.hpool[(size_t)r * (t.sims + 1) * MZ_HS + j] : 0.f;
}

// the unrolled outputs of depth k (mz_recurrent_inference wrote rows 0 .. m - 1 in place): rows whose line does not reach k,
// and the rows past m, become zero
static __global__ __launch_bounds__(64) void k_unroll_mask(int k, int B, int A, UnrollState u) {
  const int r = blockIdx.x, j = threadIdx.x;
  if (r >= B || k <= u.depth[r]) return;
  const size_t it = (size_t)k * B + r;
  if (j < MZ_H) u.hid_u[it * MZ_H + j] = 0.f;
  if (j < A) u.lg_u[it * A + j] = 0.f;
  if (j == A) { u.val_u[it] = 0.f; u.rew_u[it] = 0.f; }
}

// the terms: 16 lanes a (row, k), 16 of them a block.  Lane a < A takes the two exponentials of action a; the group's
// first lane then runs ur_terms over them in ascending order -- the order of the host hook -- and stores the scalars.
static __global__ __launch_bounds__(256) void k_unroll_terms(int A, int K1, int m, int B, int has_truth, UnrollState u) {
  __shared__ double s_eu[16][16], s_ef[16][16];
  const int g = threadIdx.x >> 4, a = threadIdx.x & 15;
  const int item = blockIdx.x * 16 + g;      // row * K1 + k
  const bool in = item < m * K1;
  const int r = in ? item / K1 : 0, k = in ? item - r * K1 : 0;
  const size_t it = (size_t)k * B + r;
  const float *lu = u.lg_u + it * A, *lf = u.lg_f + it * A;
  if (in && a < A) {
    s_eu[g][a] = exp(ur_exp_arg(lu, A, a));
    s_ef[g][a] = exp(ur_exp_arg(lf, A, a));
  }
  __syncthreads();
  if (!in || a != 0) return;
  double out[MZ_UR_NT];
  ur_terms(A, lu, lf, s_eu[g], s_ef[g], u.legal[it], u.terminal[it] != 0, k <= u.depth[r], k, u.rtrue[it], u.rew_u[it], u.val_u[it],
           u.val_f[it], has_truth ? u.truth + (size_t)item * A : nullptr, out);
  for (int i = 0; i < MZ_UR_NT; ++i) u.terms[(size_t)item * MZ_UR_NT + i] = out[i];
}

// raw: everything of a (row, k) as one row-major record, 64 threads an item
static __global__ __launch_bounds__(64) void k_unroll_export(int O, int A, int K1, int m, int B, UnrollState u) {
  const int item = blockIdx.x, j = threadIdx.x;
  if (item >= m * K1) return;
  const int r = item / K1, k = item - r * K1;
  const size_t it = (size_t)k * B + r;
  const int W = O + MZ_H + 2 * A + 4;
  float *rec = u.raw + (size_t)item * W;
  for (int c = j; c < O; c += 64) rec[c] = u.obs[it * O + c];
  if (j < MZ_H) rec[O + j] = u.hid_u[it * MZ_H + j];
  if (j < A) { rec[O + MZ_H + j] = u.lg_u[it * A + j]; rec[O + MZ_H + A + j] = u.lg_f[it * A + j]; }
  if (j == 0) {
    float *sc = rec + O + MZ_H + 2 * A;
    sc[0] = u.val_u[it]; sc[1] = u.rew_u[it]; sc[2] = u.val_f[it]; sc[3] = u.rtrue[it];
    u.raw_meta[2 * (size_t)item] = (int32_t)u.legal[it];
    u.raw_meta[2 * (size_t)item + 1] = (int32_t)u.terminal[it];
  }
}
