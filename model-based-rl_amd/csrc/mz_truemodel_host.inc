// mz_truemodel_host.inc -- mz_tm_search_host, the host twin of the true-rules search (DESIGN s7g; include/mz_engine_debug.h):
// the search of mz_truemodel.hip.h as plain sequential C++ over n trees in mz_export_tree's layout, on the same rules
// (mz_games.h) and the same leaf body (mz_tm_leaf).  No device is touched.  Included inside extern "C" by
// mz_truemodel_abi.inc, and by tests/truemodel_host.cpp, a stand-alone program that runs it under the sanitizers; the
// includer provides fail(fmt, ...) -> -1, mz_engine.h, mz_truemodel.hip.h and mz_tree_host.h (the trees, their root, backup and
// export).
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
  const int S = sims + 1;
  std::vector<double> lt, st;
  mz_host_tables(*cfg, lt, st);
  MzHostTrees tr(*cfg, n);
  std::vector<MzTmSlot> slots((size_t)n * S), pend(n);
  std::vector<float> obs((size_t)n * O), value(n), logits((size_t)n * A);
  memset(slots.data(), 0, slots.size() * sizeof(MzTmSlot));
  for (int b = 0; b < n; ++b) {      // slot 0 = the root's position (k_tm_root), then the root
    MzTmSlot &r = slots[(size_t)b * S];
    memcpy(r.bd, boards + (size_t)b * 42, cells);
    r.mask = mz_game_legal(kind, r.bd);
    r.step = step[b];
    r.mover = turn[b];
    tr.root(b, turn[b], r.mask, root_logits + (size_t)b * A, noise ? noise + (size_t)b * A : nullptr);
  }
  for (int sim = 0; sim < num_simulations; ++sim) {
    for (int b = 0; b < n; ++b) {      // the descent (mz_tm_select): PUCT over the slots' child masks
      const MzTmSlot *sl = slots.data() + (size_t)b * S;
      const MzHostTrees::Leaf d = tr.descend(b, [&](const MzNode *t, int e, int node) {
        const uint32_t mask = sl[e].mask;
        const int Np = t[node].N;
        double bs = 0.0;
        int best = -1;      // (a finished node: no child)
        for (int a = 0; a < A; ++a) {
          if (!((mask >> a) & 1u)) continue;
          const MzNode &c = t[1 + e * A + a];
          const double score = mz_puct_score(Np, lt[Np], st[Np], c.P, c.W, c.N, c.R, cfg->two_players, cfg->discount,
                                             cfg->init_value_score, tr.mn[b], tr.mx[b]);
          if (best < 0 || score >= bs) { bs = score; best = a; }      // ties go to the largest action
        }
        return best;
      });
      if (leaf_depth) leaf_depth[(size_t)b * sims + sim] = (int)tr.path[b].size() - 1;
      MzTmSlot &u = pend[b];
      if (d.stopped) {
        memset(&u, 0, sizeof u);
        u.reward = tr.tree(b)[d.node].R; u.mover = (int8_t)d.tp; u.fin = 1; u.revisit = 1;
        for (int k = 0; k < O; ++k) obs[(size_t)b * O + k] = 0.f;
      } else {
        u = sl[d.slot];
        uint8_t legal[MZ_GAME_MAX_ACTIONS];
        mz_tm_leaf(kind, u, d.act, O, A, obs.data() + (size_t)b * O, legal);
      }
    }
    eval(ctx, obs.data(), n, value.data(), logits.data());
    for (int b = 0; b < n; ++b) {      // expand + backup (mz_tm_expand_backup)
      const MzTmSlot &u = pend[b];
      const int e = tr.expand_backup(b, !u.revisit, u.mask, logits.data() + (size_t)b * A, u.fin ? 0.0 : (double)value[b], u.reward);
      if (!u.revisit) slots[(size_t)b * S + e] = u;
    }
  }
  tr.export_trees(N, W, P, R, E, TP, legal_mask, minmax);
  for (int b = 0; b < n; ++b) {
    if (nexp_out) nexp_out[b] = tr.nexp[b];
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
