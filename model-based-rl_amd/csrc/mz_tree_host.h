// mz_tree_host.h -- host only: n MCTS trees in mz_export_tree's layout as plain sequential C++, the part of a search that
// does not depend on its rule.  The host twins of the searches (mz_truemodel_host.inc, mz_gumbel_host.inc) are this plus
// their rule, as the device searches are mz_tree_descend / mz_tree_expand_backup plus theirs; mz_create takes its tables
// here.  Included by mz_truemodel.hip.h and mz_gumbel.hip.h, after mz_tree.hip.h (MzNode, mz_puct_score).  No device is touched.
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/mz_engine.h"

// mcts.py:116-117: lt[N] = math.log((N + base + 1) / base) + init and st[N] = math.sqrt(N) for every N a parent can have
// inside one search -- libm on the host, the values CPython computes
inline void mz_host_tables(const mz_config &cfg, std::vector<double> &lt, std::vector<double> &st) {
  const int T = cfg.num_simulations + 2;
  lt.resize(T); st.resize(T);
  for (int i = 0; i < T; ++i) {
    lt[i] = log(((double)i + cfg.pb_c_base + 1) / cfg.pb_c_base) + cfg.pb_c_init;
    st[i] = sqrt((double)i);
  }
}

struct MzHostTrees {
  const mz_config &cfg;
  const int n, A, NN;      // trees, actions, nodes per tree
  const bool two;
  std::vector<MzNode> pool;
  std::vector<double> mn, mx;                 // MinMaxStats
  std::vector<uint32_t> legal;                // root child masks
  std::vector<int> nexp, leaf_tp;             // expansions so far; to_play at the pending leaf
  std::vector<std::vector<int>> path;         // the pending descent's search path

  struct Leaf { int node, slot, act, tp; bool stopped; };      // as MzDescent

  MzHostTrees(const mz_config &c, int trees)
      : cfg(c), n(trees), A(c.action_space), NN(1 + (c.num_simulations + 1) * c.action_space), two(c.two_players != 0),
        pool((size_t)trees * NN), mn(trees), mx(trees), legal(trees), nexp(trees, 1), leaf_tp(trees), path(trees) {
    memset(pool.data(), 0, pool.size() * sizeof(MzNode));
    for (MzNode &c0 : pool) c0.E = -1;
  }
  MzNode *tree(int b) { return pool.data() + (size_t)b * NN; }

  // a fresh Node(prior) (mcts.py:30-40)
  static void fresh(MzNode &c, double prior, int tp) { memset(&c, 0, sizeof c); c.P = prior; c.E = -1; c.TP = (int8_t)tp; }

  // Node.expand (mcts.py:47-55) into slot e over the children in mask: exp(logit) in double over them in ascending order, no
  // max-shift, divided by their sum; a child that does not exist is marked TP = 0, prior 0
  void expand(int b, int e, uint32_t mask, const float *logits) {
    double sum = 0.0, p[MZ_MAX_ACTIONS];
    for (int a = 0; a < A; ++a) {
      p[a] = ((mask >> a) & 1u) ? exp((double)logits[a]) : 0.0;
      sum = sum + p[a];
    }
    for (int a = 0; a < A; ++a) {
      const bool ok = (mask >> a) & 1u;
      fresh(tree(b)[1 + e * A + a], ok ? p[a] / sum : 0.0, ok ? 1 : 0);
    }
  }

  // Node(0) + root.expand(mask) + add_exploration_noise (noise [A], may be null) + MinMaxStats.reset (mz_tree_root)
  void root(int b, int to_play, uint32_t mask, const float *logits, const double *noise) {
    const double frac = cfg.root_exploration_fraction;
    MzNode *t = tree(b);
    legal[b] = mask;
    expand(b, 0, mask, logits);
    for (int a = 0; a < A; ++a)
      if (((mask >> a) & 1u) && noise) t[1 + a].P = t[1 + a].P * (1 - frac) + noise[a] * frac;
    t[0].E = 0; t[0].TP = (int8_t)to_play;
    mn[b] = cfg.has_min_bound ? cfg.min_bound : __builtin_inf();
    mx[b] = cfg.has_max_bound ? cfg.max_bound : -__builtin_inf();
  }

  // the descent of MCTS.run (mz_tree_descend): choose(t, e, node) = the action taken at the node in expansion slot e, or -1:
  // it has no child and the descent stops at it.  Leaves path[b] and leaf_tp[b].
  template <class CHOOSE>
  Leaf descend(int b, CHOOSE choose) {
    const MzNode *t = tree(b);
    std::vector<int> &pa = path[b];
    pa.assign(1, 0);
    Leaf d = {0, 0, -1, t[0].TP, false};
    for (int e = t[0].E; e >= 0; e = t[d.node].E) {
      const int best = choose(t, e, d.node);
      if (best < 0) { d.stopped = true; break; }
      d.act = best;
      d.slot = e;
      d.node = 1 + e * A + best;
      pa.push_back(d.node);
      if (two) d.tp = -d.tp;
    }
    leaf_tp[b] = d.tp;
    return d;
  }

  // expand + backup of the pending leaf (mz_tree_expand_backup): Node.expand over mask into the next free slot -- unless
  // !grow: a revisit, nothing is expanded --, then MCTS.backpropagate (mcts.py:126-143) along path[b], leaf last: the leaf
  // takes `reward` and to_play leaf_tp[b], every node above it its stored ones.  Returns the slot.
  int expand_backup(int b, bool grow, uint32_t mask, const float *logits, double v, float reward) {
    MzNode *t = tree(b);
    const std::vector<int> &pa = path[b];
    const int len = (int)pa.size(), tp = leaf_tp[b], e = nexp[b];
    const double g = cfg.discount;
    if (grow) { expand(b, e, mask, logits); nexp[b] = e + 1; }
    for (int idx = 0; idx < len; ++idx) {
      MzNode &c = t[pa[len - 1 - idx]];
      const int ntp = idx == 0 ? tp : (int)c.TP;
      const double r_node = idx == 0 ? (double)reward : (double)c.R;
      c.W = c.W + ((ntp == tp) ? v : -v);
      c.N = c.N + 1;
      const double r = (two && ntp == tp) ? -r_node : r_node;
      if (idx < len - 1) {
        const double q = c.W / (double)c.N;
        const double new_q = two ? r_node - g * q : r_node + g * q;
        mn[b] = new_q < mn[b] ? new_q : mn[b];
        mx[b] = new_q > mx[b] ? new_q : mx[b];
      }
      v = r + g * v;
    }
    if (grow) { MzNode &leaf = t[pa[len - 1]]; leaf.E = e; leaf.TP = (int8_t)tp; leaf.R = reward; }
    return e;
  }

  // the trees as mz_export_tree gives them: six node arrays [n][NN], legal_mask [n], minmax [n][2]; any may be null
  void export_trees(int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP, uint32_t *legal_mask, double *minmax) const {
    for (size_t i = 0; i < pool.size(); ++i) {
      const MzNode &c = pool[i];
      if (N) N[i] = c.N;
      if (W) W[i] = c.W;
      if (P) P[i] = c.P;
      if (R) R[i] = c.R;
      if (E) E[i] = c.E;
      if (TP) TP[i] = c.TP;
    }
    for (int b = 0; b < n; ++b) {
      if (legal_mask) legal_mask[b] = legal[b];
      if (minmax) { minmax[2 * b] = mn[b]; minmax[2 * b + 1] = mx[b]; }
    }
  }
};
