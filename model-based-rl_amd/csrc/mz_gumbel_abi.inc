// mz_gumbel_abi.inc -- C ABI of the Gumbel search (included inside extern "C" of mz_engine.hip; kernels and state:
// mz_gumbel.hip.h; DESIGN s7h); its host twin mz_gz_search_host is mz_gumbel_host.inc.

#define GZ_LAUNCH(kern, s, ...) TREE_LAUNCH(kern, s, e->tv, e->gz, __VA_ARGS__)

int mz_set_gumbel(mz_engine *e, int on, int max_considered, double c_visit, double c_scale, double gumbel_scale) {
  if (!e) return fail("mz_set_gumbel: null engine");
  MZ_ENTER(e);
  GzState &gz = e->gz;
  if (!on && e->sp_mode == MZ_SP_GUMBEL) return fail("mz_set_gumbel: the self-play loop searches with the Gumbel search on this engine (mz_selfplay_set_gumbel 0 first)");
  if (!on) { gz.on = 0; gz.root_set = false; return 0; }
  if (e->tm.kind) return fail("mz_set_gumbel: the true-rules search is set on this engine; an engine takes one of the two (mz_set_true_model 0 first)");
  if (max_considered < 2) return fail("mz_set_gumbel: max_considered must be >= 2, got %d", max_considered);
  if (!(c_visit >= 0)) return fail("mz_set_gumbel: c_visit must be >= 0, got %g", c_visit);
  if (!(c_scale > 0)) return fail("mz_set_gumbel: c_scale must be > 0, got %g", c_scale);
  if (!(gumbel_scale >= 0)) return fail("mz_set_gumbel: gumbel_scale must be >= 0, got %g", gumbel_scale);
  if (!gz.G) {
    const size_t nb = (size_t)e->Bp;
    int32_t *seq = nullptr;
    if (dmalloc(e, &gz.G, nb * e->A) || dmalloc(e, &gz.vhat, nb * (e->sims + 1)) || dmalloc(e, &seq, (size_t)(e->A + 1) * e->sims) ||
        dmalloc(e, &gz.hid, nb * MZ_H) || dmalloc(e, &gz.act, nb) || dmalloc(e, &gz.hout, nb * MZ_H)) return -1;
    std::vector<int32_t> tab((size_t)(e->A + 1) * e->sims);
    for (int m = 0; m <= e->A; ++m) mz_gz_seq(m, e->sims, tab.data() + (size_t)m * e->sims);
    HIPCHECK(hipMemcpy(seq, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    gz.seq = seq;
  }
  gz.par = GzPar{max_considered, c_visit, c_scale, gumbel_scale};
  if (e->sp_mode == MZ_SP_GUMBEL) drop_graphs(e, false);      // (captured self-play moves hold the parameters by value)
  gz.on = 1;
  gz.root_set = false;
  return 0;
}

int mz_gz_root(mz_engine *e, const double *gumbel, uint64_t move, void *stream) {
  if (!e) return fail("mz_gz_root: null engine");
  MZ_ENTER(e);
  if (!e->gz.on) return fail("mz_gz_root: no Gumbel search is set (call mz_set_gumbel)");
  if (!e->root_ready || e->sims_done != 0) return fail("mz_gz_root: call mz_root_prepare first, and before any simulation");
  if (e->root_noise) return fail("mz_gz_root: this root was prepared with exploration noise; the Gumbel draw replaces it (mz_root_prepare without noise)");
  hipStream_t s = (hipStream_t)stream;
  GZ_LAUNCH(k_gz_root, s, gumbel, (uint64_t)e->cfg.seed, move, (const unsigned long long *)nullptr, e->cfg.env_id_offset);
  HIPCHECK(hipGetLastError());
  e->gz.root_set = true;
  e->selection_valid = true;
  return 0;
}

// ---- the stepwise search: the step protocol of mz_engine.hip with this variant's readiness, kernels and leaf outputs
static bool gz_ready(const mz_engine *e) { return e->gz.on && e->gz.root_set; }

static int gz_pending(mz_engine *e, const char *fn, hipStream_t s) {
  return step_pending(e, fn, gz_ready(e), "mz_gz_root", [&] { GZ_LAUNCH(k_gz_select, s, e->sims_done); });
}

static int gz_step(mz_engine *e, const char *fn, const float *value, const float *reward, const float *logits, const float *hidden,
                   bool more, hipStream_t s) {
  return step_advance(e, fn, gz_ready(e), "mz_gz_select", more,
                      [&](bool m) { GZ_LAUNCH(k_gz_step, s, value, reward, logits, hidden, m ? 1 : 0, e->sims_done + 1); });
}

// n simulations behind a pending descent (mz_gz_search, and a self-play move of mz_selfplay_set_gumbel: launch_move_game): the recurrent
// inference on the rows the descent left (parent hidden state, action), then the tree step with the next descent
static int gz_simulations(mz_engine *e, const char *fn, int n, hipStream_t s) {
  const GzState &gz = e->gz;
  for (int i = 0; i < n; ++i) {
    NET_LAUNCH(k_net_recurrent_rows, (e->B + MZ_ROWS - 1) / MZ_ROWS, s, e->nv, (const float *)gz.hid, (const int32_t *)gz.act, e->B,
               gz.hout, e->tv.reward, e->tv.value, e->tv.logits);
    HIPCHECK(hipGetLastError());
    if (gz_step(e, fn, e->tv.value, e->tv.reward, e->tv.logits, gz.hout, step_more(e), s)) return -1;
  }
  return 0;
}

int mz_gz_select(mz_engine *e, int32_t *parent_slot, int32_t *action, void *stream) {
  if (!e) return fail("mz_gz_select: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (gz_pending(e, "mz_gz_select", s)) return -1;
  return export_selection(e, nullptr, parent_slot, action, nullptr, s);
}

int mz_gz_expand_backup(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                        void *stream) {
  if (!e || !value || !reward || !logits) return fail("mz_gz_expand_backup: null argument");
  MZ_ENTER(e);
  return gz_step(e, "mz_gz_expand_backup", value, reward, logits, hidden, false, (hipStream_t)stream);
}

int mz_gz_expand_backup_select(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                               int32_t *parent_slot, int32_t *action, void *stream) {
  if (!e || !value || !reward || !logits) return fail("mz_gz_expand_backup_select: null argument");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  const bool more = step_more(e);
  if (gz_step(e, "mz_gz_expand_backup_select", value, reward, logits, hidden, more, s)) return -1;
  return more ? export_selection(e, nullptr, parent_slot, action, nullptr, s) : 0;
}

int mz_gz_search(mz_engine *e, int num_simulations, void *stream) {
  if (!e) return fail("mz_gz_search: null engine");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_gz_search: weights not set (call mz_set_weights)");
  if (!gz_ready(e)) return fail("mz_gz_search: call mz_gz_root first");
  if (num_simulations < 1 || e->sims_done + num_simulations > e->sims)
    return fail("mz_gz_search: %d + %d simulations exceed the pool sized for num_simulations = %d", e->sims_done,
                num_simulations, e->sims);
  hipStream_t s = (hipStream_t)stream;
  if (gz_pending(e, "mz_gz_search", s)) return -1;
  return gz_simulations(e, "mz_gz_search", num_simulations, s);
}

// k_gz_pick with the walk's outputs (ply_search) or without them (mz_gz_pick)
static int gz_pick(mz_engine *e, const char *fn, int32_t *actions, float *pred_rewards, int32_t *n_actions, int32_t *path_lengths,
                   int32_t *action, float *pred_reward, double *improved_policy, double *v_mix, hipStream_t s) {
  if (!e->gz.on || !e->gz.root_set) return fail("%s: call mz_gz_root first", fn);
  if (e->sims_done < 1) return fail("%s: no simulation was run (call mz_gz_search first)", fn);
  const size_t lds = (size_t)(e->sims + 1) * sizeof(int32_t);
  if (lds > 48 * 1024) return fail("%s: num_simulations = %d exceeds the LDS map of the path lengths", fn, e->sims);
#define GZ_PICK(G_)                                                                                                      \
  hipLaunchKernelGGL(k_gz_pick<G_>, dim3(e->B), dim3(64), lds, s, e->tv, e->gz, e->sims_done + 1, actions, pred_rewards, \
                     n_actions, path_lengths, action, pred_reward, improved_policy, v_mix)
  switch (e->G) {
    case 4: GZ_PICK(4); break;
    case 8: GZ_PICK(8); break;
    case 16: GZ_PICK(16); break;
    default: GZ_PICK(32); break;
  }
#undef GZ_PICK
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_gz_pick(mz_engine *e, int32_t *action, float *pred_reward, double *improved_policy, double *v_mix, void *stream) {
  if (!e) return fail("mz_gz_pick: null engine");
  MZ_ENTER(e);
  return gz_pick(e, "mz_gz_pick", nullptr, nullptr, nullptr, nullptr, action, pred_reward, improved_policy, v_mix, (hipStream_t)stream);
}

int mz_gz_export(mz_engine *e, double *gumbel, float *vhat) {
  if (!e) return fail("mz_gz_export: null engine");
  MZ_ENTER(e);
  if (!e->gz.G) return fail("mz_gz_export: no Gumbel search was set (mz_set_gumbel)");
  HIPCHECK(hipDeviceSynchronize());
  if (gumbel) HIPCHECK(hipMemcpy(gumbel, e->gz.G, (size_t)e->B * e->A * sizeof(double), hipMemcpyDeviceToHost));
  if (vhat) HIPCHECK(hipMemcpy(vhat, e->gz.vhat, (size_t)e->B * (e->sims + 1) * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
#undef GZ_LAUNCH

// the host twin mz_gz_search_host: its own file, so that a stand-alone host program can compile it (tests/gumbel_host.cpp)
#include "mz_gumbel_host.inc"
