// mz_eval.hip.h -- the device work of evaluate.py's Evaluator.play_game (reference evaluate.py:242-385) that the search
// kernels do not already do, for B evaluation games in lock-step (gfx950; included by mz_engine.hip, -ffp-contract=off):
//
//   k_eval_walk          after mz_search: the actions to apply and their predicted rewards (evaluate.py:314-326) and the
//                        per-simulation search depths (evaluate.py:306-307), one wave per tree
//   k_eval_rows<JTP>     one recurrent inference per (tree, action) row on the root's hidden state (hpool slot 0), the body
//                        of k_net_recurrent_rows (mz_net_recurrent): rewards / values bit-identical to mz_recurrent_inference
//   k_eval_choose_value  --only_value's choice over those rows (evaluate.py:286-303), one thread per tree
//   k_eval_choose_prior  --only_prior's choice over the root priors (evaluate.py:278-284), one thread per tree
//
// The games that live on the device environments (their state, k_eval_observe, k_eval_apply) are in mz_eval_env.hip.h.
//
// A lookahead move is two launches: rows then choice (--only_value), choice then one row per tree (--only_prior).  The rows
// of one tree straddle 16-row workgroup tiles for A = 9 and 18, so the choice is a second per-tree kernel over the [B][A]
// reward / value rows instead of a reduction inside the network kernel.
#pragma once
#include "mz_common.h"
#include "mz_net.hip.h"
#include "mz_rng.h"
#include "mz_tree.hip.h"

// One wave per tree.
// (1) path_lengths [B][sims] (may be null): len(search_path) of simulation s = depth of the node expanded into slot s + 1,
//     plus one.  The children of expansion slot e are nodes 1 + e*A .. e*A + A, so a node k >= 1 whose expansion index is
//     s >= 1 has parent slot (k - 1) / A; the lanes scan the nexp * A children of expanded nodes for that map (LDS), then
//     every slot climbs to the root.  Entries from nexp - 1 on (simulations not run) are 0.
// (2) actions / pred_rewards [B][M], n_actions [B]: from the root, while the node is expanded and fewer than M actions are
//     taken, Config.select_action (config.py:70-81, mz_sample_index) over the node's children -- the legal actions in
//     ascending order at the root (mcts.py:47-55), range(A) below it (mcts.py:97) -- then move to the chosen child; its
//     float32 reward is the predicted one (0 for a child never expanded: Node.reward's default, mcts.py:34).  Every step
//     consumes one uniform: uniform [B][M] from the caller, or Philox keyed (seed, env id, move, step) under MZ_RNG_EVAL.
//     Entries from n_actions on are action -1, reward 0.
// own_nexp (after a true-rules search, mz_tm_search): the tree's own count of expansions, t.nexp[b], where it is smaller --
// a simulation that revisits a finished node expands nothing, so the trees of a batch differ in it.
__global__ __launch_bounds__(64) void k_eval_walk(TreeView t, int nexp, int own_nexp, int M, const double *temperature,
                                                  const double *uniform, uint64_t seed, uint64_t move, int env_offset,
                                                  int32_t *actions, float *pred_rewards, int32_t *n_actions,
                                                  int32_t *path_lengths) {
  extern __shared__ int32_t par[];            // [sims + 1] parent slot of every expansion slot
  __shared__ double d[MZ_MAX_ACTIONS_K];
  __shared__ int32_t acts[MZ_MAX_ACTIONS_K];
  __shared__ int32_t next_node;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= t.B) return;
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  if (own_nexp) nexp = t.nexp[b] < nexp ? t.nexp[b] : nexp;
  // what the walk's first step reads, issued together with the scan below (one memory round trip less on the path)
  const uint32_t legal = t.legal[b];
  const double T = temperature[b];
  const int e_root = t.E[o];
  const int n_root = lane < A ? t.N[o + 1 + lane] : 0;
  if (path_lengths) mz_walk_path_lengths(t, o, b, lane, nexp, par, path_lengths);
  const uint32_t amask = A >= 32 ? 0xFFFFFFFFu : ((1u << A) - 1u);
  int node = 0, taken = 0;
  for (; taken < M; ++taken) {
    const int e = node == 0 ? e_root : t.E[o + node];     // (the same address in every lane: wave-uniform)
    if (e < 0 || e >= nexp) break;               // not expanded (an index past the expansions so far: no tree here)
    const int n = node == 0 ? __builtin_popcount(legal & amask) : A;
    if (n == 0) break;
    if (lane < A) {
      const int ch = 1 + e * A + lane;      // (the root's children: nodes 1 .. A, read above)
      if (node != 0) {
        d[lane] = (double)t.N[o + ch]; acts[lane] = lane;
      } else if ((legal >> lane) & 1u) {
        const int pos = __builtin_popcount(legal & ((1u << lane) - 1u));
        d[pos] = (double)(e == 0 ? n_root : t.N[o + ch]); acts[pos] = lane;
      }
    }
    __syncthreads();
    if (lane == 0) {
      double u;
      if (uniform) {
        u = uniform[(size_t)b * M + taken];
      } else {
        mz_u4 r = mz_philox(seed, (uint32_t)(env_offset + b), (uint32_t)move, (uint32_t)(move >> 32),
                            (MZ_RNG_EVAL << 24) | ((uint32_t)taken & 0xFFFFFFu));
        u = mz_u01(r.x, r.y);
      }
      const int a = acts[mz_sample_index(d, n, T, u)];
      const int ch = 1 + e * A + a;
      actions[(size_t)b * M + taken] = a;
      pred_rewards[(size_t)b * M + taken] = t.R[o + ch];
      next_node = ch;
    }
    __syncthreads();
    node = next_node;
  }
  if (lane == 0) n_actions[b] = taken;
  for (int i = taken + lane; i < M; i += 64) {
    actions[(size_t)b * M + i] = -1;
    pred_rewards[(size_t)b * M + i] = 0.f;
  }
}

// Recurrent inference on rows r = tree * per_tree + j: hidden state = the tree's root (hpool slot 0, what
// initial_inference produced), action = act[r / per_tree] when act is given (one row per tree), else j (one row per
// (tree, action)).  The staging and the network body are k_net_recurrent_rows's.
template <int JTP>
__global__ __launch_bounds__(256, 1) void k_eval_rows(NetView n, TreeView t, int per_tree, const int32_t *act, int nrows,
                                                      float *hout, float *reward, float *value, float *logits) {
  __shared__ NetSmem sm;
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * MZ_ROWS;
  const int rows = (nrows - b0) < 16 ? (nrows - b0) : 16;
  const size_t tree_stride = (size_t)(t.sims + 1) * MZ_HS;
  for (int idx = tid; idx < 16 * MZ_H; idx += 256) {
    const int m = idx / MZ_H, k = idx % MZ_H;
    sm.xT[k * 16 + m] = (m < rows) ? t.hpool[(size_t)((b0 + m) / per_tree) * tree_stride + k] : 0.f;
  }
  const int extra = n.ks1 * 4 - MZ_H;
  for (int idx = tid; idx < 16 * extra; idx += 256) {
    const int m = idx & 15, kk = idx >> 4;
    int a = -1;
    if (m < rows) a = act ? act[(b0 + m) / per_tree] : (b0 + m) % per_tree;
    sm.xT[(MZ_H + kk) * 16 + m] = (kk == a) ? 1.f : 0.f;
  }
  __syncthreads();
  NetSink o;
  o.h_base = hout + (size_t)b0 * MZ_H; o.h_stride = MZ_H; o.h_pad = 0;
  o.reward = reward + b0; o.value = value + b0; o.logits = logits + (size_t)b0 * n.A;
  o.rows = rows;
  mz_net_recurrent<JTP>(sm, n, o, tid);
}

// --only_value (evaluate.py:286-303) over the [B][A] rows of k_eval_rows: q = r + discount * v (r - discount * v with two
// players) in float32 as torch forms it -- the float32 discount times v, then the add, two roundings (no contraction in
// this translation unit); the FIRST strict maximum over the legal children in ascending order; its reward is the predicted
// one.  Every legal child got one visit: child_visits = 1 / |legal| there (game.py:106-115), 0 elsewhere.
__global__ void k_eval_choose_value(TreeView t, const float *row_reward, const float *row_value, float discount,
                                    int32_t *action, float *pred_reward, double *child_visits) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const int A = t.A;
  const uint32_t legal = t.legal[b];
  float best = -__builtin_inff();
  int chosen = -1;
  float rew = 0.f;
  int n = 0;
  for (int a = 0; a < A; ++a) {
    if (!((legal >> a) & 1u)) continue;
    ++n;
    const float r = row_reward[(size_t)b * A + a], v = row_value[(size_t)b * A + a];
    const float dv = discount * v;
    const float q = t.two_players ? r - dv : r + dv;
    if (q > best) { best = q; chosen = a; rew = r; }
  }
  action[b] = chosen;
  pred_reward[b] = rew;
  if (child_visits)
    for (int a = 0; a < A; ++a) child_visits[(size_t)b * A + a] = ((legal >> a) & 1u) ? 1.0 / (double)n : 0.0;
}

// --only_prior (evaluate.py:278-284): max((prior, action)) over the root's children -- the largest float64 prior as the
// tree holds it after mz_root_prepare (Dirichlet noise included), ties to the LARGEST action; child_visits one-hot.
__global__ void k_eval_choose_prior(TreeView t, int32_t *action, double *child_visits) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  const uint32_t legal = t.legal[b];
  double best = 0.0;
  int chosen = -1;
  for (int a = 0; a < A; ++a) {
    if (!((legal >> a) & 1u)) continue;
    const double p = t.P[o + 1 + a];
    if (chosen < 0 || p >= best) { best = p; chosen = a; }
  }
  action[b] = chosen;
  if (child_visits)
    for (int a = 0; a < A; ++a) child_visits[(size_t)b * A + a] = a == chosen ? 1.0 : 0.0;
}
