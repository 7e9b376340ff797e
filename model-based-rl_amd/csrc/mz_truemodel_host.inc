// mz_truemodel_host.inc -- mz_tm_search_host, the host twin of the true-rules search (DESIGN s7g; include/mz_engine_debug.h):
// the search of mz_truemodel.hip.h as plain sequential C++ over n trees in mz_export_tree's layout, on the same rules
// (mz_games.h) and the same leaf body (mz_tm_leaf).  No device is touched.  Included inside extern "C" by
// mz_truemodel_abi.inc, and by tests/truemodel_host.cpp, a stand-alone program that runs it under the sanitizers; the
// includer provides fail(fmt, ...) -> -1, <math.h>, <string.h>, <vector>, mz_engine.h and mz_truemodel.hip.h.
int mz_tm_search_host(const mz_config *cfg, int kind, int n, const int8_t *boards, const int8_t *turn, const int32_t *step,
                      const float *root_logits, const double *noise, int num_simulations,
                      void (*eval)(void *ctx, const float *obs, int n, float *value, float *logits), void *ctx,
                      int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP, uint32_t *legal_mask, double *minmax,
                      int32_t *nexp_out, int8_t *slot_boards, int8_t *slot_mover, int32_t *slot_step, uint32_t *slot_mask,
                      uint8_t *slot_finished, int32_t *leaf_depth) {
  if (!cfg || !boards || !turn || !step || !root_logits || !eval) return fail("mz_tm_search_host: null argument");
  if (kind != 1 && kind != 3) return fail("mz_tm_search_host: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", kind);
  char why[96];
  if (!mz_game_shape_ok(kind, cfg->obs_dim, cfg->action_space, cfg->two_players != 0, why, sizeof why))
    return fail("mz_tm_search_host: %s", why);
  if (n < 1) return fail("mz_tm_search_host: n must be >= 1");
  const int A = cfg->action_space, O = cfg->obs_dim, sims = cfg->num_simulations, cells = mz_game_info(kind).cells;
  if (num_simulations < 1 || num_simulations > sims)
    return fail("mz_tm_search_host: %d simulations exceed the trees sized for num_simulations = %d", num_simulations, sims);
  const int NN = 1 + (sims + 1) * A, S = sims + 1;
  const double g = cfg->discount, frac = cfg->root_exploration_fraction;
  const bool two = cfg->two_players != 0;
  std::vector<double> lt(sims + 2), st(sims + 2);      // mz_create's tables
  for (int i = 0; i < sims + 2; ++i) {
    lt[i] = log(((double)i + cfg->pb_c_base + 1) / cfg->pb_c_base) + cfg->pb_c_init;
    st[i] = sqrt((double)i);
  }
  std::vector<MzNode> pool((size_t)n * NN);
  std::vector<MzTmSlot> slots((size_t)n * S), pend(n);
  std::vector<double> mn(n), mx(n);
  std::vector<int> nexp(n, 1), leaf_tp(n);
  std::vector<std::vector<int>> path(n);
  std::vector<float> obs((size_t)n * O), value(n), logits((size_t)n * A);
  memset(pool.data(), 0, pool.size() * sizeof(MzNode));
  memset(slots.data(), 0, slots.size() * sizeof(MzTmSlot));
  auto fresh = [](MzNode &c, double prior, int tp) { memset(&c, 0, sizeof c); c.P = prior; c.E = -1; c.TP = (int8_t)tp; };
  for (int b = 0; b < n; ++b) {      // Node(0) + root.expand(legal) + add_exploration_noise + MinMaxStats.reset (mz_tree_root)
    MzNode *t = pool.data() + (size_t)b * NN;
    for (int k = 1; k < NN; ++k) t[k].E = -1;
    MzTmSlot &r = slots[(size_t)b * S];
    memcpy(r.bd, boards + (size_t)b * 42, cells);
    r.mask = mz_game_legal(kind, r.bd);
    r.step = step[b];
    r.mover = turn[b];
    double sum = 0.0, p[MZ_GAME_MAX_ACTIONS];
    for (int a = 0; a < A; ++a) {
      p[a] = ((r.mask >> a) & 1u) ? exp((double)root_logits[(size_t)b * A + a]) : 0.0;
      sum = sum + p[a];
    }
    for (int a = 0; a < A; ++a) {
      const bool ok = (r.mask >> a) & 1u;
      double prior = ok ? p[a] / sum : 0.0;
      if (ok && noise) prior = prior * (1 - frac) + noise[(size_t)b * A + a] * frac;
      fresh(t[1 + a], prior, ok ? 1 : 0);
    }
    t[0].E = 0; t[0].TP = turn[b];
    mn[b] = cfg->has_min_bound ? cfg->min_bound : __builtin_inf();
    mx[b] = cfg->has_max_bound ? cfg->max_bound : -__builtin_inf();
  }
  for (int sim = 0; sim < num_simulations; ++sim) {
    for (int b = 0; b < n; ++b) {      // the descent (mz_tm_select)
      MzNode *t = pool.data() + (size_t)b * NN;
      MzTmSlot *sl = slots.data() + (size_t)b * S;
      std::vector<int> &pa = path[b];
      pa.assign(1, 0);
      int node = 0, parent_e = 0, a_sel = -1, tp = t[0].TP, e = t[0].E, Np = t[0].N;
      bool revisit = false;
      while (e >= 0) {
        const uint32_t mask = sl[e].mask;
        if (mask == 0u) { revisit = true; break; }
        double bs = 0.0;
        int best = -1;
        for (int a = 0; a < A; ++a) {
          if (!((mask >> a) & 1u)) continue;
          const MzNode &c = t[1 + e * A + a];
          double score;
          if (Np == 0) {
            score = c.P;
          } else {
            const double pb_c = lt[Np] * (st[Np] / (double)(c.N + 1));
            const double prior_score = pb_c * c.P;
            double value_score;
            if (c.N > 0) {
              const double q = c.W / (double)c.N;
              const double v = two ? -q : q;
              const double x = (double)c.R + g * v;
              value_score = mx[b] > mn[b] ? (x - mn[b]) / (mx[b] - mn[b]) : (mx[b] == mn[b] ? 1.0 : x);
            } else {
              value_score = cfg->init_value_score;
            }
            score = prior_score + value_score;
          }
          if (best < 0 || score >= bs) { bs = score; best = a; }      // ties go to the largest action
        }
        a_sel = best;
        parent_e = e;
        node = 1 + e * A + a_sel;
        pa.push_back(node);
        if (two) tp = -tp;
        Np = t[node].N;
        e = t[node].E;
      }
      leaf_tp[b] = tp;
      if (leaf_depth) leaf_depth[(size_t)b * sims + sim] = (int)pa.size() - 1;
      MzTmSlot &u = pend[b];
      if (revisit) {
        memset(&u, 0, sizeof u);
        u.reward = t[node].R; u.mover = (int8_t)tp; u.fin = 1; u.revisit = 1;
        for (int k = 0; k < O; ++k) obs[(size_t)b * O + k] = 0.f;
      } else {
        u = sl[parent_e];
        mz_tm_leaf(kind, u, a_sel, O, A, obs.data() + (size_t)b * O);
      }
    }
    eval(ctx, obs.data(), n, value.data(), logits.data());
    for (int b = 0; b < n; ++b) {      // expand + backup (mz_tm_expand_backup)
      MzNode *t = pool.data() + (size_t)b * NN;
      const MzTmSlot &u = pend[b];
      const std::vector<int> &pa = path[b];
      const int len = (int)pa.size(), tp = leaf_tp[b], e = nexp[b], leafnode = pa[len - 1];
      if (!u.revisit) {
        double sum = 0.0, p[MZ_GAME_MAX_ACTIONS];
        for (int a = 0; a < A; ++a) {
          p[a] = ((u.mask >> a) & 1u) ? exp((double)logits[(size_t)b * A + a]) : 0.0;
          sum = sum + p[a];
        }
        for (int a = 0; a < A; ++a) {
          const bool ok = (u.mask >> a) & 1u;
          fresh(t[1 + e * A + a], ok ? p[a] / sum : 0.0, ok ? 1 : 0);
        }
        slots[(size_t)b * S + e] = u;
        nexp[b] = e + 1;
      }
      double v = u.fin ? 0.0 : (double)value[b];
      for (int idx = 0; idx < len; ++idx) {      // MCTS.backpropagate (mz_tree_backup_path)
        MzNode &c = t[pa[len - 1 - idx]];
        const int ntp = idx == 0 ? tp : (int)c.TP;
        const double r_node = idx == 0 ? (double)u.reward : (double)c.R;
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
      if (!u.revisit) { t[leafnode].E = e; t[leafnode].TP = (int8_t)tp; t[leafnode].R = u.reward; }
    }
  }
  for (int b = 0; b < n; ++b) {
    for (int k = 0; k < NN; ++k) {
      const MzNode &c = pool[(size_t)b * NN + k];
      const size_t i = (size_t)b * NN + k;
      if (N) N[i] = c.N;
      if (W) W[i] = c.W;
      if (P) P[i] = c.P;
      if (R) R[i] = c.R;
      if (E) E[i] = c.E;
      if (TP) TP[i] = c.TP;
    }
    if (legal_mask) legal_mask[b] = slots[(size_t)b * S].mask;
    if (minmax) { minmax[2 * b] = mn[b]; minmax[2 * b + 1] = mx[b]; }
    if (nexp_out) nexp_out[b] = nexp[b];
    for (int s = 0; s < S; ++s) {
      const MzTmSlot &u = slots[(size_t)b * S + s];
      const size_t i = (size_t)b * S + s;
      if (slot_boards) memcpy(slot_boards + i * 42, u.bd, 42);
      if (slot_mover) slot_mover[i] = u.mover;
      if (slot_step) slot_step[i] = u.step;
      if (slot_mask) slot_mask[i] = u.mask;
      if (slot_finished) slot_finished[i] = u.fin;
    }
  }
  return 0;
}
