// mz_gumbel_host.inc -- mz_gz_search_host, the host twin of the Gumbel search (DESIGN s7h; include/mz_engine_debug.h): the
// search of mz_gumbel.hip.h as plain sequential C++ over n trees in mz_export_tree's layout, through the same per-node body
// (mz_gz_node over GzSeq) and the same table (mz_gz_seq).  No device is touched.  Included inside extern "C" by
// mz_gumbel_abi.inc, and by tests/gumbel_host.cpp, a stand-alone program that runs it under the sanitizers; the includer
// provides fail(fmt, ...) -> -1, <math.h>, <string.h>, <vector>, mz_engine.h and mz_gumbel.hip.h.
int mz_gz_seq_host(int m, int n, int32_t *out) {
  if (!out || m < 0 || m > MZ_MAX_ACTIONS || n < 1) return fail("mz_gz_seq_host: m in 0 .. %d, n >= 1 and out are needed", MZ_MAX_ACTIONS);
  mz_gz_seq(m, n, out);
  return 0;
}

int mz_gz_search_host(const mz_config *cfg, int n, const int8_t *to_play, const uint8_t *legal, const float *root_value,
                      const float *root_logits, const double *gumbel, int max_considered, double c_visit, double c_scale,
                      double gumbel_scale, int num_simulations,
                      void (*eval)(void *ctx, int sim, const int32_t *parent_slot, const int32_t *action, int n, float *value,
                                   float *reward, float *logits),
                      void *ctx, int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP, uint32_t *legal_mask,
                      double *minmax, float *vhat_out, int32_t *sel_slot, int32_t *sel_action, int32_t *paths, int32_t *plens,
                      int32_t *action_out, float *pred_reward, double *improved_policy, double *v_mix, double *min_gap) {
  if (!cfg || !root_value || !root_logits || !eval) return fail("mz_gz_search_host: null argument");
  if (n < 1) return fail("mz_gz_search_host: n must be >= 1");
  const int A = cfg->action_space, sims = cfg->num_simulations;
  if (A < 1 || A > MZ_MAX_ACTIONS) return fail("mz_gz_search_host: action_space %d outside [1,%d]", A, MZ_MAX_ACTIONS);
  if (num_simulations < 1 || num_simulations > sims)
    return fail("mz_gz_search_host: %d simulations exceed the trees sized for num_simulations = %d", num_simulations, sims);
  if (max_considered < 2 || c_visit < 0 || !(c_scale > 0))
    return fail("mz_gz_search_host: max_considered >= 2, c_visit >= 0 and c_scale > 0 are needed");
  if (gumbel_scale != 0.0 && !gumbel) return fail("mz_gz_search_host: gumbel_scale %g needs the draws (the host twin draws none)", gumbel_scale);
  const int NN = 1 + (sims + 1) * A, S = sims + 1, PL = sims + 2;
  const double g = cfg->discount;
  const bool two = cfg->two_players != 0;
  const GzPar gp = {max_considered, c_visit, c_scale, gumbel_scale};
  std::vector<int32_t> seq((size_t)(A + 1) * sims);
  for (int m = 0; m <= A; ++m) mz_gz_seq(m, sims, seq.data() + (size_t)m * sims);
  std::vector<MzNode> pool((size_t)n * NN);
  std::vector<double> mn(n), mx(n), gl((size_t)n * A);
  std::vector<uint32_t> lmask(n);
  std::vector<int> nexp(n, 1), leaf_tp(n);
  std::vector<std::vector<int>> path(n);
  std::vector<float> vhat((size_t)n * S, 0.f), value(n), reward(n), logits((size_t)n * A);
  std::vector<int32_t> pslot(n), pact(n);
  double gap = __builtin_inf();
  const GzSeq x = {A, &gap};
  memset(pool.data(), 0, pool.size() * sizeof(MzNode));
  auto fresh = [](MzNode &c, double prior, int tp) { memset(&c, 0, sizeof c); c.P = prior; c.E = -1; c.TP = (int8_t)tp; };
  for (int b = 0; b < n; ++b) {      // Node(0) + root.expand(legal) + MinMaxStats.reset (mz_tree_root, no noise)
    MzNode *t = pool.data() + (size_t)b * NN;
    for (int k = 1; k < NN; ++k) t[k].E = -1;
    uint32_t mask = 0;
    for (int a = 0; a < A; ++a) mask |= ((legal ? legal[(size_t)b * A + a] : 1) ? 1u : 0u) << a;
    lmask[b] = mask;
    double sum = 0.0, p[MZ_MAX_ACTIONS];
    for (int a = 0; a < A; ++a) {
      p[a] = ((mask >> a) & 1u) ? exp((double)root_logits[(size_t)b * A + a]) : 0.0;
      sum = sum + p[a];
    }
    for (int a = 0; a < A; ++a) {
      const bool ok = (mask >> a) & 1u;
      fresh(t[1 + a], ok ? p[a] / sum : 0.0, ok ? 1 : 0);
      gl[(size_t)b * A + a] = (gumbel_scale != 0.0 ? gumbel_scale * gumbel[(size_t)b * A + a] : 0.0) + (double)root_logits[(size_t)b * A + a];
    }
    t[0].E = 0; t[0].TP = to_play ? to_play[b] : (int8_t)1;
    mn[b] = cfg->has_min_bound ? cfg->min_bound : __builtin_inf();
    mx[b] = cfg->has_max_bound ? cfg->max_bound : -__builtin_inf();
    vhat[(size_t)b * S] = root_value[b];
  }
  // the children of the node in slot e (node: its index) as mz_gz_node takes them
  bool has[MZ_MAX_ACTIONS];
  double cP[MZ_MAX_ACTIONS], cW[MZ_MAX_ACTIONS], pi[MZ_MAX_ACTIONS], vm = 0.0;
  int cN[MZ_MAX_ACTIONS];
  float cR[MZ_MAX_ACTIONS];
  auto children = [&](const MzNode *t, int node, int e, uint32_t mask) {
    for (int a = 0; a < A; ++a) {
      const MzNode &c = t[1 + e * A + a];
      has[a] = node != 0 || ((mask >> a) & 1u);
      cP[a] = has[a] ? c.P : 0.0; cW[a] = has[a] ? c.W : 0.0; cN[a] = has[a] ? c.N : 0; cR[a] = has[a] ? c.R : 0.f;
    }
  };
  for (int sim = 0; sim < num_simulations; ++sim) {
    for (int b = 0; b < n; ++b) {      // the descent (mz_gz_select)
      MzNode *t = pool.data() + (size_t)b * NN;
      std::vector<int> &pa = path[b];
      pa.assign(1, 0);
      const int want = seq[(size_t)mz_gz_considered(gp, lmask[b], A) * sims + sim];
      int node = 0, parent_e = 0, a_sel = 0, tp = t[0].TP, e = t[0].E;
      while (e >= 0) {
        children(t, node, e, lmask[b]);
        int best = mz_gz_node(x, A, gp, two ? 1 : 0, g, mn[b], mx[b], (double)vhat[(size_t)b * S + e], has, cP, cW, cN, cR,
                              node == 0, gl.data() + (size_t)b * A, want, pi, &vm);
        if (best < 0) best = 0;
        a_sel = best;
        parent_e = e;
        node = 1 + e * A + a_sel;
        pa.push_back(node);
        if (two) tp = -tp;
        e = t[node].E;
      }
      leaf_tp[b] = tp;
      pslot[b] = parent_e; pact[b] = a_sel;
      if (sel_slot) sel_slot[(size_t)b * sims + sim] = parent_e;
      if (sel_action) sel_action[(size_t)b * sims + sim] = a_sel;
      if (plens) plens[(size_t)b * sims + sim] = (int32_t)pa.size();
      if (paths)
        for (int k = 0; k < PL; ++k) paths[((size_t)b * sims + sim) * PL + k] = k < (int)pa.size() ? pa[k] : -1;
    }
    eval(ctx, sim, pslot.data(), pact.data(), n, value.data(), reward.data(), logits.data());
    for (int b = 0; b < n; ++b) {      // expand + backup (mz_tree_expand_backup), v^ of the new slot
      MzNode *t = pool.data() + (size_t)b * NN;
      const std::vector<int> &pa = path[b];
      const int len = (int)pa.size(), tp = leaf_tp[b], e = nexp[b], leafnode = pa[len - 1];
      double sum = 0.0, p[MZ_MAX_ACTIONS];
      for (int a = 0; a < A; ++a) {
        p[a] = exp((double)logits[(size_t)b * A + a]);
        sum = sum + p[a];
      }
      for (int a = 0; a < A; ++a) fresh(t[1 + e * A + a], p[a] / sum, 1);
      nexp[b] = e + 1;
      vhat[(size_t)b * S + e] = value[b];
      double v = (double)value[b];
      for (int idx = 0; idx < len; ++idx) {      // MCTS.backpropagate (mz_tree_backup_path)
        MzNode &c = t[pa[len - 1 - idx]];
        const int ntp = idx == 0 ? tp : (int)c.TP;
        const double r_node = idx == 0 ? (double)reward[b] : (double)c.R;
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
      t[leafnode].E = e; t[leafnode].TP = (int8_t)tp; t[leafnode].R = reward[b];
    }
  }
  for (int b = 0; b < n; ++b) {      // the end of the move (k_gz_pick) and the export
    const MzNode *t = pool.data() + (size_t)b * NN;
    children(t, 0, 0, lmask[b]);
    const int best = mz_gz_node(x, A, gp, two ? 1 : 0, g, mn[b], mx[b], (double)vhat[(size_t)b * S], has, cP, cW, cN, cR,
                                true, gl.data() + (size_t)b * A, -1, pi, &vm);
    if (action_out) action_out[b] = best;
    if (pred_reward) pred_reward[b] = best < 0 ? 0.f : t[1 + best].R;
    if (v_mix) v_mix[b] = vm;
    for (int a = 0; a < A; ++a)
      if (improved_policy) improved_policy[(size_t)b * A + a] = pi[a];
    for (int k = 0; k < NN; ++k) {
      const MzNode &c = t[k];
      const size_t i = (size_t)b * NN + k;
      if (N) N[i] = c.N;
      if (W) W[i] = c.W;
      if (P) P[i] = c.P;
      if (R) R[i] = c.R;
      if (E) E[i] = c.E;
      if (TP) TP[i] = c.TP;
    }
    if (legal_mask) legal_mask[b] = lmask[b];
    if (minmax) { minmax[2 * b] = mn[b]; minmax[2 * b + 1] = mx[b]; }
    for (int s = 0; s < S; ++s)
      if (vhat_out) vhat_out[(size_t)b * S + s] = vhat[(size_t)b * S + s];
  }
  if (min_gap) *min_gap = gap;
  return 0;
}
