// mz_gumbel.hip.h -- the Gumbel MuZero search of evaluation games and matches (DESIGN s7h; gfx950; included by mz_engine.hip,
// -ffp-contract=off).  Danihelka et al., "Policy improvement by planning with Gumbel" (ICLR 2022): at the root Gumbel-top-k
// with sequential halving -- simulation s goes to the legal action with the largest g + logit + sigma among those visited
// seq(m, n)[s] times --, below the root the deterministic rule arg-max pi'(a) - N(a) / (1 + sum N), and at the end of the move
// the improved policy pi' from completed Q-values.  The tree lies in the engine's node pool as mz_search leaves it; expansion,
// rewards, hidden states and the backup with its MinMaxStats are mz_tree_expand_backup's, unchanged.  The side state is one
// float per expansion slot (the raw network value of the node, v^) and one double per root action (the Gumbel draw).
//
// The mapping is that of the stand-alone tree kernels: G lanes per tree, lane = action, shuffle reductions, whole 32-byte
// node records.  The per-node body (completed Q, sigma, pi', both arg-max rules) is ONE function, mz_gz_node, written over an
// execution X: GzLanes<G> holds one action per lane and reduces by shuffles inside the group, GzSeq holds all actions in one
// thread (the host twin, mz_gumbel_host.inc).  Sums run over the actions in ascending order in both, so the two differ in
// exp() alone.  Latency bound gather / scatter like the tree kernels: one dependent round trip per level.
#pragma once
#include "mz_common.h"
#include "mz_rng.h"
#include "mz_tree.hip.h"
#include "mz_tree_host.h"      // (the host twin's trees, mz_gumbel_host.inc)

#define MZ_RNG_GUMBEL 11u    // the root's Gumbel draws (k_gz_root): counter (env, move, action)

struct GzPar {
  int max_considered;      // m = min(this, legal actions): the actions sequential halving starts from
  double c_visit, c_scale; // sigma(a) = (c_visit + max_b N(b)) * c_scale * q^(a)
  double gumbel_scale;     // g(a) = gumbel_scale * G(a); 0: no noise, the search is deterministic
};

struct GzState {
  int on;                  // mz_set_gumbel
  GzPar par;
  double *G;               // [B][A] this move's G(a): given, drawn, or 0 with gumbel_scale 0
  float *vhat;             // [B][sims + 1] raw network value of the node in expansion slot e, in its mover's view
  const int32_t *seq;      // [A + 1][sims] seq(m, sims)[s] (mz_gz_seq; host-built)
  float *hid;              // [Bp][MZ_H] the selected leaves' parents' hidden states: the next inference's rows
  int32_t *act;            // [Bp] and actions
  float *hout;             // [Bp][MZ_H] its hidden-state output (value / reward / logits land in the TreeView's)
  bool root_set;           // mz_gz_root has made this move's first descent
};

// mctx's get_sequence_of_considered_visits: out[s], s < n, is the visit count a root action must have to be considered at
// simulation s, with m actions considered at the start and n simulations in all
inline void mz_gz_seq(int m, int n, int32_t *out) {
  if (m <= 1) { for (int s = 0; s < n; ++s) out[s] = s; return; }
  int L = 0;
  while ((1 << L) < m) ++L;                     // ceil(log2 m)
  int32_t visits[MZ_MAX_ACTIONS_K];
  for (int i = 0; i < m; ++i) visits[i] = 0;
  int k = m, len = 0;
  while (len < n) {
    const int times = n / (L * k) > 1 ? n / (L * k) : 1;
    for (int r = 0; r < times && len < n; ++r)
      for (int i = 0; i < k; ++i) { if (len < n) out[len++] = visits[i]; visits[i] += 1; }
    k = k / 2 > 2 ? k / 2 : 2;
  }
}

// ---- the two executions of mz_gz_node
// one action per lane of a G-lane group; every reduction leaves its result in every lane
template <int G>
struct GzLanes {
  static constexpr int K = 1;
  int lane;
  __device__ __forceinline__ int count(int) const { return 1; }
  __device__ __forceinline__ double sum_d(const double *v, int A) const {      // ascending action order, as Python's sum()
    double s = 0.0;
    for (int a = 0; a < A; ++a) s = s + __shfl(v[0], a, G);
    return s;
  }
  __device__ __forceinline__ int sum_i(const int *v) const {
    int s = v[0];
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, G);
    return s;
  }
  __device__ __forceinline__ int max_i(const int *v) const {
    int s = v[0];
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) { const int o = __shfl_xor(s, off, G); s = o > s ? o : s; }
    return s;
  }
  __device__ __forceinline__ double max_d(const double *v) const {
    double s = v[0];
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) { const double o = __shfl_xor(s, off, G); s = o > s ? o : s; }
    return s;
  }
  __device__ __forceinline__ bool any(const bool *v) const {
    const int x = v[0] ? 1 : 0;
    return max_i(&x) != 0;
  }
  __device__ __forceinline__ int argmax(const double *score, const bool *cand) const {
    return mz_group_argmax<G>(cand[0] ? score[0] : 0.0, cand[0] ? lane : -1);
  }
};

// all A actions in one thread; min_gap (may be null): the smallest non-zero difference between the best and the
// second-best score over every arg-max taken
struct GzSeq {
  static constexpr int K = MZ_MAX_ACTIONS_K;
  int A;
  double *min_gap;
  __host__ __device__ int count(int) const { return A; }
  __host__ __device__ double sum_d(const double *v, int) const {
    double s = 0.0;
    for (int a = 0; a < A; ++a) s = s + v[a];
    return s;
  }
  __host__ __device__ int sum_i(const int *v) const { int s = 0; for (int a = 0; a < A; ++a) s += v[a]; return s; }
  __host__ __device__ int max_i(const int *v) const { int s = v[0]; for (int a = 1; a < A; ++a) s = v[a] > s ? v[a] : s; return s; }
  __host__ __device__ double max_d(const double *v) const { double s = v[0]; for (int a = 1; a < A; ++a) s = v[a] > s ? v[a] : s; return s; }
  __host__ __device__ bool any(const bool *v) const { for (int a = 0; a < A; ++a) if (v[a]) return true; return false; }
  __host__ __device__ int argmax(const double *score, const bool *cand) const {
    int best = -1;
    for (int a = 0; a < A; ++a)
      if (cand[a] && (best < 0 || score[a] >= score[best])) best = a;
    if (min_gap && best >= 0)
      for (int a = 0; a < A; ++a) {
        const double gap = score[best] - score[a];
        if (cand[a] && a != best && gap > 0.0 && gap < *min_gap) *min_gap = gap;
      }
    return best;
  }
};

// One node of the Gumbel search (DESIGN s7h).  The caller holds X::K children (k-th = action k of GzSeq, the lane's own of
// GzLanes): has (the child exists: legal at the root, every action below it), its record's P, W, N, R; vhat: the node's raw
// network value; mn / mx: the tree's MinMaxStats.  Out: pi[k] = pi'(a) (0 where the child does not exist), vmix, and the
// chosen action --
//   root (gl[k] = g(a) + logit(a)): arg-max of gl + sigma over the existing children with N == want, or, with
//     want < 0 (the end of the move), with N == max_b N(b).  No child with N == want cannot happen in a search that follows
//     seq from its first simulation; every existing child is then a candidate, so that the choice is always a child.
//   below the root (gl is not read): arg-max of pi' - N / (1 + sum N) over the existing children.
// Every arg-max breaks ties to the largest action; -1: the node has no child.
template <class X>
__host__ __device__ __forceinline__ int mz_gz_node(const X &x, int A, const GzPar &gp, int two_players, double discount,
                                                   double mn, double mx, double vhat, const bool *has, const double *P,
                                                   const double *W, const int *N, const float *R, bool root, const double *gl,
                                                   int want, double *pi, double *vmix_out) {
  constexpr int K = X::K;
  const int n = x.count(A);
  double q[K], sg[K], t1[K], t2[K];
  int nn[K];
  bool vis[K], cand[K];
  for (int k = 0; k < n; ++k) {
    vis[k] = has[k] && N[k] > 0;
    nn[k] = has[k] ? N[k] : 0;
    q[k] = vis[k] ? mz_child_q(W[k], N[k], R[k], two_players, discount) : 0.0;
    t1[k] = vis[k] ? P[k] * q[k] : 0.0;
    t2[k] = vis[k] ? P[k] : 0.0;
  }
  const int sumN = x.sum_i(nn), maxN = x.max_i(nn);
  const double spq = x.sum_d(t1, A), sp = x.sum_d(t2, A);
  // (sp == 0: every visited child's prior underflowed to 0 -- nothing to weigh by)
  const double vmix = (sumN > 0 && sp > 0.0) ? (vhat + (double)sumN * spq / sp) / (1.0 + (double)sumN) : vhat;
  const double cs = (gp.c_visit + (double)maxN) * gp.c_scale;
  for (int k = 0; k < n; ++k) {
    sg[k] = cs * mz_normalize(vis[k] ? q[k] : vmix, mn, mx);
    t1[k] = has[k] ? sg[k] : -__builtin_inf();
  }
  const double smax = x.max_d(t1);
  for (int k = 0; k < n; ++k) t1[k] = has[k] ? P[k] * exp(sg[k] - smax) : 0.0;
  const double ws = x.sum_d(t1, A);
  for (int k = 0; k < n; ++k) pi[k] = has[k] ? t1[k] / ws : 0.0;
  *vmix_out = vmix;
  if (root) {
    const int w = want < 0 ? maxN : want;
    for (int k = 0; k < n; ++k) cand[k] = has[k] && nn[k] == w;
    const bool some = x.any(cand);
    for (int k = 0; k < n; ++k) {
      cand[k] = some ? cand[k] : has[k];
      t2[k] = gl[k] + sg[k];
    }
  } else {
    for (int k = 0; k < n; ++k) {
      cand[k] = has[k];
      t2[k] = pi[k] - (double)nn[k] / (1.0 + (double)sumN);
    }
  }
  return x.argmax(t2, cand);
}

// m of this root: the actions sequential halving starts from
__host__ __device__ __forceinline__ int mz_gz_considered(const GzPar &gp, uint32_t legal, int A) {
  const uint32_t amask = A >= 32 ? 0xFFFFFFFFu : ((1u << A) - 1u);
  const int nl = __builtin_popcount(legal & amask);
  return gp.max_considered < nl ? gp.max_considered : nl;
}

// The rule of the descent (mz_tree_descend, mz_tree.hip.h): mz_gz_node at every level -- the root rule, then the rule below
// the root -- over the legal actions at the root and every action below it; the chosen child's expansion index is fetched
// from its lane.  At the leaf it copies the parent's hidden state into gz.hid[b], the next inference's row.
template <int G>
struct GzRule {
  const TreeView &t;
  const GzState &gz;
  int b, lane;
  double mn, mx;
  uint32_t legal;
  int want;             // seq(m, sims)[sim]
  double gl;            // g(a) + logit(a) of this lane's root action
  __device__ __forceinline__ void begin(const MzNode &) {}
  __device__ __forceinline__ bool choose(int e, int node, int &best, int &ce) {
    const int A = t.A;
    const bool has = lane < A && (node != 0 || ((legal >> lane) & 1u));
    const double vhat = (double)gz.vhat[(size_t)b * (size_t)(t.sims + 1) + e];      // (requested beside the children's records)
    double cP = 0.0, cW = 0.0, pi, vmix;
    int cN = 0, cE = -1;
    float cR = 0.f;
    if (has) {
      const MzNode c = mz_node_load(t, mz_slab(t, b) + 1 + e * A + lane);
      cP = c.P; cW = c.W; cN = c.N; cE = c.E; cR = c.R;
    }
    best = mz_gz_node(GzLanes<G>{lane}, A, gz.par, t.two_players, t.discount, mn, mx, vhat, &has, &cP, &cW, &cN, &cR, node == 0,
                      &gl, want, &pi, &vmix);
    if (best < 0) best = 0;      // (a root without a legal action: stay inside the node pool)
    ce = __shfl(cE, best, G);
    return true;
  }
  __device__ __forceinline__ void leave(const MzDescent &d) {
    const float *hp = t.hpool + ((size_t)b * (size_t)(t.sims + 1) + (size_t)d.slot) * MZ_HS;
    for (int k = lane; k < MZ_H; k += G) gz.hid[(size_t)b * MZ_H + k] = hp[k];
  }
};

// The descent of simulation `sim`.  Leaves what every descent leaves and the next inference's row: the parent's hidden state
// in gz.hid[b] (GzRule::leave), the action in gz.act[b].
template <int G>
__device__ __forceinline__ void mz_gz_select(const TreeView &t, const GzState &gz, int b, int lane, int sim) {
  const int A = t.A;
  const uint32_t legal = t.legal[b];
  const int want = gz.seq[(size_t)mz_gz_considered(gz.par, legal, A) * t.sims + sim];
  const double gl = lane < A ? gz.par.gumbel_scale * gz.G[(size_t)b * A + lane] + (double)t.root_logits[(size_t)b * A + lane] : 0.0;
  GzRule<G> rule = {t, gz, b, lane, t.mn[b], t.mx[b], legal, want, gl};
  const MzDescent d = mz_tree_descend<G>(t, b, lane, rule);
  if (lane == 0) gz.act[b] = d.act;
}

// ------------------------------------------------------------------ kernels
// k_gz_root (after k_tree_root without noise): v^ of slot 0 = the initial inference's root value; G = the caller's
// (given), or -log(-log u) with u from the counter RNG keyed (env, move, action) -- a game's draws do not depend on its
// batch --, or 0 with gumbel_scale 0 (nothing is drawn); then the first descent, by the root rule.  The move is move_val, or
// -- the self-play loop, whose captured graphs must draw afresh at every replay -- what move_ptr points to (as k_dirichlet).
template <int G>
__global__ void k_gz_root(TreeView t, GzState gz, const double *given, uint64_t seed, uint64_t move_val,
                          const unsigned long long *move_ptr, int env_offset) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  const uint64_t move = move_ptr ? (uint64_t)*move_ptr : move_val;
  if (lane < t.A) {
    double g = 0.0;
    if (gz.par.gumbel_scale != 0.0) {
      if (given) {
        g = given[(size_t)b * t.A + lane];
      } else {
        const mz_u4 r = mz_philox(seed, (uint32_t)(env_offset + b), (uint32_t)move, (uint32_t)(move >> 32),
                                  (MZ_RNG_GUMBEL << 24) | (uint32_t)lane);
        const double u = mz_u01(r.x, r.y);
        g = -log(-log(u > 0.0 ? u : 0x1p-54));
      }
    }
    gz.G[(size_t)b * t.A + lane] = g;
  }
  if (lane == 0) gz.vhat[(size_t)b * (size_t)(t.sims + 1)] = t.root_value[b];
  __threadfence_block();          // lane 0's v^ -> visible to the group's other lanes
  mz_gz_select<G>(t, gz, b, lane, 0);
}

template <int G>
__global__ void k_gz_select(TreeView t, GzState gz, int sim) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  mz_gz_select<G>(t, gz, b, lane, sim);
}

// expand + backup of a simulation (mz_tree_expand_backup, shared) with v^ of the new slot, and (do_select) the descent of
// simulation next_sim in the same launch, as k_tree_step.  hidden (may be null: the caller has stored it): [B][MZ_H], the
// new node's hidden state, into the slot this expansion takes.
template <int G>
__global__ void k_gz_step(TreeView t, GzState gz, const float *value, const float *reward, const float *logits,
                          const float *hidden, int do_select, int next_sim) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gt / G, lane = gt % G;
  if (b >= t.B) return;
  const int e = t.nexp[b];
  const float v = value[b];
  if (hidden) {
    float *hp = t.hpool + ((size_t)b * (size_t)(t.sims + 1) + (size_t)e) * MZ_HS;
    for (int k = lane; k < MZ_HS; k += G) hp[k] = k < MZ_H ? hidden[(size_t)b * MZ_H + k] : 0.f;
  }
  mz_tree_expand_backup<G>(t, b, lane, v, reward[b], logits + (size_t)b * t.A);
  if (lane == 0) gz.vhat[(size_t)b * (size_t)(t.sims + 1) + e] = v;
  if (do_select) {
    __threadfence_block();          // lane 0's node updates and v^, the hidden state -> visible to the group's other lanes
    mz_gz_select<G>(t, gz, b, lane, next_sim);
  }
}

// The end of the move at the root of tree b, by the G lanes of one group (lane = action): the action by the root rule among the
// most visited (-1: no legal action), this lane's pi'(a) (0 beyond A and on illegal actions), v_mix, and this lane's child's
// reward.  Shared by k_gz_pick and the self-play loop's end-of-move kernels (mz_gumbel_selfplay.hip.h).
template <int G>
__device__ __forceinline__ int mz_gz_root_pick(const TreeView &t, const GzState &gz, int b, int lane, double *pi, double *vmix,
                                               float *child_reward) {
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  const uint32_t legal = t.legal[b];
  const bool has = lane < A && ((legal >> lane) & 1u);
  const double gl = lane < A ? gz.par.gumbel_scale * gz.G[(size_t)b * A + lane] + (double)t.root_logits[(size_t)b * A + lane] : 0.0;
  double cP = 0.0, cW = 0.0;
  int cN = 0;
  float cR = 0.f;
  if (has) {
    const MzNode c = mz_node_load(t, o + 1 + lane);
    cP = c.P; cW = c.W; cN = c.N; cR = c.R;
  }
  *child_reward = cR;
  return mz_gz_node(GzLanes<G>{lane}, A, gz.par, t.two_players, t.discount, t.mn[b], t.mx[b],
                    (double)gz.vhat[(size_t)b * (size_t)(t.sims + 1)], &has, &cP, &cW, &cN, &cR, true, &gl, -1, pi, vmix);
}

// The end of the move, one 64-lane workgroup per tree (its 64 / G groups compute the same): the action by the root rule
// among the most visited, its child's reward, pi' and v_mix of the root -- and what k_eval_walk writes for one action per
// move: actions, pred_rewards, n_actions = 1 (0: a root without a legal action) and path_lengths (mz_walk_path_lengths).
// action / pred_reward / improved_policy / v_mix / path_lengths may be null.
template <int G>
__global__ __launch_bounds__(64) void k_gz_pick(TreeView t, GzState gz, int nexp, int32_t *actions, float *pred_rewards,
                                                int32_t *n_actions, int32_t *path_lengths, int32_t *action,
                                                float *pred_reward, double *improved_policy, double *v_mix) {
  extern __shared__ int32_t par[];            // [sims + 1] parent slot of every expansion slot
  const int b = blockIdx.x, wl = threadIdx.x, lane = wl % G;
  if (b >= t.B) return;
  const int A = t.A;
  const size_t o = mz_slab(t, b);
  if (path_lengths) mz_walk_path_lengths(t, o, b, wl, nexp, par, path_lengths);
  double pi, vmix;
  float cR;
  const int best = mz_gz_root_pick<G>(t, gz, b, lane, &pi, &vmix, &cR);
  const float r = __shfl(cR, best < 0 ? 0 : best, G);
  if (wl < A && improved_policy) improved_policy[(size_t)b * A + wl] = pi;
  if (wl == 0) {
    if (actions) actions[b] = best;
    if (pred_rewards) pred_rewards[b] = best < 0 ? 0.f : r;
    if (n_actions) n_actions[b] = best < 0 ? 0 : 1;
    if (action) action[b] = best;
    if (pred_reward) pred_reward[b] = best < 0 ? 0.f : r;
    if (v_mix) v_mix[b] = vmix;
  }
}
