// mz_gumbel_host.inc -- mz_gz_search_host, the host twin of the Gumbel search (DESIGN s7h; include/mz_engine_debug.h): the
// search of mz_gumbel.hip.h as plain sequential C++ over n trees in mz_export_tree's layout, through the same per-node body
// (mz_gz_node over GzSeq) and the same table (mz_gz_seq).  No device is touched.  Included inside extern "C" by
// mz_gumbel_abi.inc, and by tests/gumbel_host.cpp, a stand-alone program that runs it under the sanitizers; the includer
// provides fail(fmt, ...) -> -1, mz_engine.h, mz_gumbel.hip.h and mz_tree_host.h (the trees, their root, backup and export).
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
  const int S = sims + 1, PL = sims + 2;
  const int two = cfg->two_players != 0 ? 1 : 0;
  const GzPar gp = {max_considered, c_visit, c_scale, gumbel_scale};
  std::vector<int32_t> seq((size_t)(A + 1) * sims);
  for (int m = 0; m <= A; ++m) mz_gz_seq(m, sims, seq.data() + (size_t)m * sims);
  MzHostTrees tr(*cfg, n);
  std::vector<double> gl((size_t)n * A);
  std::vector<float> vhat((size_t)n * S, 0.f), value(n), reward(n), logits((size_t)n * A);
  std::vector<int32_t> pslot(n), pact(n);
  double gap = __builtin_inf();
  const GzSeq x = {A, &gap};
  for (int b = 0; b < n; ++b) {      // the root, without noise, and what k_gz_root adds: g + logit per action, v^ of slot 0
    uint32_t mask = 0;
    for (int a = 0; a < A; ++a) mask |= ((legal ? legal[(size_t)b * A + a] : 1) ? 1u : 0u) << a;
    tr.root(b, to_play ? to_play[b] : 1, mask, root_logits + (size_t)b * A, nullptr);
    for (int a = 0; a < A; ++a)
      gl[(size_t)b * A + a] = (gumbel_scale != 0.0 ? gumbel_scale * gumbel[(size_t)b * A + a] : 0.0) + (double)root_logits[(size_t)b * A + a];
    vhat[(size_t)b * S] = root_value[b];
  }
  // mz_gz_node on the children of the node in slot e (node: its index) of tree b
  double pi[MZ_MAX_ACTIONS], vm = 0.0;
  auto gz_node = [&](int b, const MzNode *t, int e, int node, int want) {
    bool has[MZ_MAX_ACTIONS];
    double cP[MZ_MAX_ACTIONS], cW[MZ_MAX_ACTIONS];
    int cN[MZ_MAX_ACTIONS];
    float cR[MZ_MAX_ACTIONS];
    for (int a = 0; a < A; ++a) {
      const MzNode &c = t[1 + e * A + a];
      has[a] = node != 0 || ((tr.legal[b] >> a) & 1u);
      cP[a] = has[a] ? c.P : 0.0; cW[a] = has[a] ? c.W : 0.0; cN[a] = has[a] ? c.N : 0; cR[a] = has[a] ? c.R : 0.f;
    }
    return mz_gz_node(x, A, gp, two, cfg->discount, tr.mn[b], tr.mx[b], (double)vhat[(size_t)b * S + e], has, cP, cW, cN, cR,
                      node == 0, gl.data() + (size_t)b * A, want, pi, &vm);
  };
  for (int sim = 0; sim < num_simulations; ++sim) {
    for (int b = 0; b < n; ++b) {      // the descent (mz_gz_select)
      const int want = seq[(size_t)mz_gz_considered(gp, tr.legal[b], A) * sims + sim];
      const MzHostTrees::Leaf d = tr.descend(b, [&](const MzNode *t, int e, int node) {
        const int best = gz_node(b, t, e, node, want);
        return best < 0 ? 0 : best;
      });
      const std::vector<int> &pa = tr.path[b];
      pslot[b] = d.slot; pact[b] = d.act;
      if (sel_slot) sel_slot[(size_t)b * sims + sim] = d.slot;
      if (sel_action) sel_action[(size_t)b * sims + sim] = d.act;
      if (plens) plens[(size_t)b * sims + sim] = (int32_t)pa.size();
      if (paths)
        for (int k = 0; k < PL; ++k) paths[((size_t)b * sims + sim) * PL + k] = k < (int)pa.size() ? pa[k] : -1;
    }
    eval(ctx, sim, pslot.data(), pact.data(), n, value.data(), reward.data(), logits.data());
    for (int b = 0; b < n; ++b) {      // expand + backup (mz_tree_expand_backup, every action), v^ of the new slot
      const int e = tr.expand_backup(b, true, 0xFFFFFFFFu, logits.data() + (size_t)b * A, (double)value[b], reward[b]);
      vhat[(size_t)b * S + e] = value[b];
    }
  }
  for (int b = 0; b < n; ++b) {      // the end of the move (k_gz_pick)
    const MzNode *t = tr.tree(b);
    const int best = gz_node(b, t, 0, 0, -1);
    if (action_out) action_out[b] = best;
    if (pred_reward) pred_reward[b] = best < 0 ? 0.f : t[1 + best].R;
    if (v_mix) v_mix[b] = vm;
    for (int a = 0; a < A; ++a)
      if (improved_policy) improved_policy[(size_t)b * A + a] = pi[a];
    for (int s = 0; s < S; ++s)
      if (vhat_out) vhat_out[(size_t)b * S + s] = vhat[(size_t)b * S + s];
  }
  tr.export_trees(N, W, P, R, E, TP, legal_mask, minmax);
  if (min_gap) *min_gap = gap;
  return 0;
}
