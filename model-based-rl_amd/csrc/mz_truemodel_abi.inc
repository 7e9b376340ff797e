// mz_truemodel_abi.inc -- C ABI of the true-rules search (included inside extern "C" of mz_engine.hip; kernels and state:
// mz_truemodel.hip.h; DESIGN s7g); its host twin mz_tm_search_host is mz_truemodel_host.inc.

#define TM_LAUNCH(kern, s, ...) TREE_LAUNCH(kern, s, e->tv, e->tm, e->O, __VA_ARGS__)

int mz_set_true_model(mz_engine *e, int kind) {
  if (!e) return fail("mz_set_true_model: null engine");
  MZ_ENTER(e);
  if (kind != 0 && kind != 1 && kind != 3)
    return fail("mz_set_true_model: kind must be 0 (off), 1 (TicTacToe) or 3 (Connect Four), got %d", kind);
  if (kind != 0 && game_shape(e, "mz_set_true_model", kind)) return -1;
  if (kind != e->tm.kind && e->sp_mode == MZ_SP_TRUE_RULES)
    return fail("mz_set_true_model: the self-play loop searches the true rules of the current game on this engine (mz_selfplay_set_true_model 0 first)");
  if (kind != 0 && e->gz.on) return fail("mz_set_true_model: the Gumbel search is set on this engine; an engine takes one of the two (mz_set_gumbel off first)");
  TmState &tm = e->tm;
  if (kind != 0 && !tm.slots) {
    const size_t nb = (size_t)e->Bp;
    if (dmalloc(e, &tm.slots, nb * (e->sims + 1)) || dmalloc(e, &tm.pend, nb) || dmalloc(e, &tm.obs, nb * e->O) ||
        dmalloc(e, &tm.leaf_fin, nb) || dmalloc(e, &tm.value, nb) || dmalloc(e, &tm.logits, nb * e->A)) return -1;
  }
  tm.kind = kind;
  tm.root_set = false;
  return 0;
}

int mz_tm_root(mz_engine *e, const int8_t *boards, const int8_t *turn, const int32_t *step, void *stream) {
  if (!e || !boards || !turn || !step) return fail("mz_tm_root: null argument");
  MZ_ENTER(e);
  if (!e->tm.kind) return fail("mz_tm_root: no true-rules search is set (call mz_set_true_model)");
  if (!e->root_ready || e->sims_done != 0) return fail("mz_tm_root: call mz_root_prepare first, and before any simulation");
  hipStream_t s = (hipStream_t)stream;
  TM_LAUNCH(k_tm_root, s, boards, turn, step);
  HIPCHECK(hipGetLastError());
  e->tm.root_set = true;
  e->selection_valid = true;
  return 0;
}

// ---- the stepwise search: the step protocol of mz_engine.hip with this variant's readiness, kernels and leaf outputs
static bool tm_ready(const mz_engine *e) { return e->tm.kind && e->tm.root_set; }

static int tm_pending(mz_engine *e, const char *fn, hipStream_t s) {
  return step_pending(e, fn, tm_ready(e), "mz_tm_root", [&] { TREE_LAUNCH(k_tm_select, s, e->tv, e->tm, e->O); });
}

static int tm_step(mz_engine *e, const char *fn, const float *value, const float *logits, bool more, hipStream_t s) {
  return step_advance(e, fn, tm_ready(e), "mz_tm_select", more, [&](bool m) { TM_LAUNCH(k_tm_step, s, value, logits, m ? 1 : 0); });
}

static int tm_leaf_out(mz_engine *e, float *obs_out, uint8_t *finished_out, hipStream_t s) {
  if (obs_out) HIPCHECK(hipMemcpyAsync(obs_out, e->tm.obs, (size_t)e->B * e->O * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (finished_out) HIPCHECK(hipMemcpyAsync(finished_out, e->tm.leaf_fin, (size_t)e->B, hipMemcpyDeviceToDevice, s));
  return 0;
}

int mz_tm_select(mz_engine *e, float *obs_out, uint8_t *finished_out, void *stream) {
  if (!e) return fail("mz_tm_select: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (tm_pending(e, "mz_tm_select", s)) return -1;
  return tm_leaf_out(e, obs_out, finished_out, s);
}

int mz_tm_expand_backup(mz_engine *e, const float *value, const float *logits, void *stream) {
  if (!e || !value || !logits) return fail("mz_tm_expand_backup: null argument");
  MZ_ENTER(e);
  return tm_step(e, "mz_tm_expand_backup", value, logits, false, (hipStream_t)stream);
}

int mz_tm_expand_backup_select(mz_engine *e, const float *value, const float *logits, float *obs_out, uint8_t *finished_out,
                               void *stream) {
  if (!e || !value || !logits) return fail("mz_tm_expand_backup_select: null argument");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  const bool more = step_more(e);
  if (tm_step(e, "mz_tm_expand_backup_select", value, logits, more, s)) return -1;
  return more ? tm_leaf_out(e, obs_out, finished_out, s) : 0;
}

// what mz_tm_search and mz_tm_search_fused ask before they launch, in fn's name; leaves the pending descent on the stream
static int tm_search_begin(mz_engine *e, const char *fn, int num_simulations, hipStream_t s) {
  if (!e->weights_set) return fail("%s: weights not set (call mz_set_weights)", fn);
  if (!tm_ready(e)) return fail("%s: call mz_tm_root first", fn);
  if (num_simulations < 1 || e->sims_done + num_simulations > e->sims)
    return fail("%s: %d + %d simulations exceed the pool sized for num_simulations = %d", fn, e->sims_done, num_simulations, e->sims);
  return tm_pending(e, fn, s);
}

// the two-launch loop: per simulation the root kernel on the leaves' observations, then k_tm_step
static int tm_simulations(mz_engine *e, const char *fn, int n, hipStream_t s) {
  // the leaf inference is the root kernel on the leaves' observations; its outputs land in the true-model state, so the
  // move's own root value and logits stay (k_eval_apply, k_match_apply and mz_finalize's error read them after the search)
  TreeView leaf_tv = e->tv;
  leaf_tv.root_value = e->tm.value;
  leaf_tv.root_logits = e->tm.logits;
  for (int i = 0; i < n; ++i) {
    if (launch_root(e, leaf_tv, e->tm.obs, false, s)) return -1;
    if (tm_step(e, fn, e->tm.value, e->tm.logits, step_more(e), s)) return -1;
  }
  return 0;
}

// the same n simulations in one launch of k_tm_search (DESIGN s7k); the two board games' lane groups are instantiated
static int tm_simulations_fused(mz_engine *e, const char *fn, int n, hipStream_t s) {
  if (!tm_ready(e) || !e->selection_valid) return fail("%s: call mz_tm_select first", fn);
  const int sel_last = e->sims_done + n < e->sims ? 1 : 0;
  const dim3 grid(e->Bp / MZ_ROWS), block(256);
#define TM_FUSED(JTP_, G_) \
  hipLaunchKernelGGL((k_tm_search<JTP_, G_>), grid, block, 0, s, e->nv, e->tv, e->tm, e->istream, e->nst0, n, sel_last)
  if (e->G == 16) { if (e->jtp == 1) TM_FUSED(1, 16); else TM_FUSED(2, 16); }
  else if (e->G == 8) { if (e->jtp == 1) TM_FUSED(1, 8); else TM_FUSED(2, 8); }
  else return fail("%s: internal: no k_tm_search for lane groups of %d", fn, e->G);
#undef TM_FUSED
  HIPCHECK(hipGetLastError());
  e->sims_done += n;
  e->selection_valid = sel_last != 0;
  return 0;
}

int mz_tm_search(mz_engine *e, int num_simulations, void *stream) {
  if (!e) return fail("mz_tm_search: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (tm_search_begin(e, "mz_tm_search", num_simulations, s)) return -1;
  return tm_simulations(e, "mz_tm_search", num_simulations, s);
}

int mz_tm_search_fused(mz_engine *e, int num_simulations, void *stream) {
  if (!e) return fail("mz_tm_search_fused: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (tm_search_begin(e, "mz_tm_search_fused", num_simulations, s)) return -1;
  return tm_simulations_fused(e, "mz_tm_search_fused", num_simulations, s);
}

int mz_tm_export(mz_engine *e, int8_t *boards, int8_t *mover, int32_t *step, uint32_t *mask, uint8_t *finished, int32_t *nexp) {
  if (!e) return fail("mz_tm_export: null engine");
  MZ_ENTER(e);
  if (!e->tm.slots) return fail("mz_tm_export: no true-rules search was set (mz_set_true_model)");
  HIPCHECK(hipDeviceSynchronize());
  const size_t S = (size_t)e->sims + 1, n = (size_t)e->B * S;
  std::vector<MzTmSlot> sl(n);
  HIPCHECK(hipMemcpy(sl.data(), e->tm.slots, n * sizeof(MzTmSlot), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    if (boards) memcpy(boards + i * 42, sl[i].bd, 42);
    if (mover) mover[i] = sl[i].mover;
    if (step) step[i] = sl[i].step;
    if (mask) mask[i] = sl[i].mask;
    if (finished) finished[i] = sl[i].fin;
  }
  if (nexp) HIPCHECK(hipMemcpy(nexp, e->tv.nexp, (size_t)e->B * 4, hipMemcpyDeviceToHost));
  return 0;
}

#undef TM_LAUNCH

// the host twin mz_tm_search_host: its own file, so that a stand-alone host program can compile it (tests/truemodel_host.cpp)
#include "mz_truemodel_host.inc"
