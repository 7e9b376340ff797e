// mz_reanalyse_abi.inc -- C ABI of MuZero Reanalyse on the device (included inside extern "C" of mz_engine.hip; kernels and
// state: mz_reanalyse.hip.h).  Stored rows of the replay (mzr_reanalyse_pick, include/mz_replay.h) are searched again under the
// engine's current weights, chunk by chunk, and the fresh child_visits / root_value come back in the layout mzr_reanalyse_write
// takes.  Like mz_eval_env_moves / mz_match_plies: whole chunks are enqueued, the host touches nothing in between.

int mz_reanalyse(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                 int num_simulations, void *stream) {
  if (!e) return fail("mz_reanalyse: null engine");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_reanalyse: weights not set (call mz_set_weights)");
  if (rec_floats != MZ_REC_FLOATS(e->O, e->A, 0))
    return fail("mz_reanalyse: rec_floats %d != obs_dim + action_space + %d = %d", rec_floats, MZ_REC_EXTRA, MZ_REC_FLOATS(e->O, e->A, 0));
  if (kind < 0 || kind > 3)
    return fail("mz_reanalyse: kind must be 0 (synthetic), 1 (TicTacToe), 2 (CartPole) or 3 (Connect Four), got %d", kind);
  if (kind != 0 && game_shape(e, "mz_reanalyse", kind)) return -1;
  if (n_rows < 0) return fail("mz_reanalyse: n_rows must be >= 0, got %d", n_rows);
  if (num_simulations < 1 || num_simulations > e->sims)
    return fail("mz_reanalyse: num_simulations must be in 1 .. %d (the engine's pool), got %d", e->sims, num_simulations);
  if (n_rows == 0) return 0;
  if (!rows_host || !fresh_host) return fail("mz_reanalyse: null buffer");
  const float *rows_dev = nullptr;
  float *fresh_dev = nullptr;
  if (hipHostGetDevicePointer((void **)&rows_dev, (void *)rows_host, 0) != hipSuccess || !rows_dev ||
      hipHostGetDevicePointer((void **)&fresh_dev, (void *)fresh_host, 0) != hipSuccess || !fresh_dev) {
    (void)hipGetLastError();
    return fail("mz_reanalyse: rows and fresh must be page-locked (pinned) host memory");
  }
  ReanalyseState &rs = e->ra;
  const int B = e->B, O = e->O, A = e->A;
  if (!rs.to_play) {      // allocated on the first call (which therefore synchronises: hipMalloc + hipMemset); to_play is the last one
    rs = ReanalyseState{};      // (an earlier call that failed half-way starts over: what it got stays with the engine's allocations)
    if (dmalloc(e, &rs.obs, (size_t)e->Bp * O) || dmalloc(e, &rs.legal, (size_t)B * A) || dmalloc(e, &rs.to_play, (size_t)B)) {
      rs = ReanalyseState{};
      return -1;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(128), grid_obs(((size_t)B * O + 127) / 128), grid_store(((size_t)B * (A + 2) + 127) / 128);
  int rc = 0;
  for (int at = 0; at < n_rows && !rc; at += B) {
    const int n = n_rows - at < B ? n_rows - at : B;
    hipLaunchKernelGGL(k_reanalyse_observe, grid_obs, block, 0, s, rs, rows_dev + (size_t)at * rec_floats, n, rec_floats, kind, B, O, A);
    if (hipGetLastError() != hipSuccess) { rc = fail("mz_reanalyse: k_reanalyse_observe did not launch"); break; }
    rc = mz_initial_inference(e, rs.obs, s) || mz_root_prepare(e, rs.to_play, rs.legal, nullptr, 0, 0, s) ||
         mz_search(e, num_simulations, s);
    if (rc) break;
    hipLaunchKernelGGL(k_reanalyse_store, grid_store, block, 0, s, e->tv, fresh_dev + (size_t)at * (A + 2), n);
    if (hipGetLastError() != hipSuccess) rc = fail("mz_reanalyse: k_reanalyse_store did not launch");
  }
  if (rc) {      // what was enqueued still reads / writes the caller's buffers: let it end before they are handed back
    (void)hipStreamSynchronize(s);
    return -1;
  }
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

// Reanalyse with the Gumbel search (DESIGN s7j): mz_reanalyse's buffers, kinds and chunks, searched as a self-play move of
// mz_selfplay_set_gumbel is (launch_move_gumbel, mz_gumbel_abi.inc) and stored as pi' and the root's mean value (value_kind 0)
// or its v_mix (1).  A row's Gumbel draws are keyed (engine seed, the row's index in the pass, draw_key, action): k_gz_root takes
// the chunk's first row as its environment offset, so a pass does not depend on the engine's B.  The host side of the step
// protocol starts over at every chunk and ends where mz_gz_search leaves it.
int mz_reanalyse_gumbel(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                        int num_simulations, int value_kind, uint64_t draw_key, void *stream) {
  if (!e) return fail("mz_reanalyse_gumbel: null engine");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_reanalyse_gumbel: weights not set (call mz_set_weights)");
  if (!e->gz.on) return fail("mz_reanalyse_gumbel: no Gumbel search is set on this engine (call mz_set_gumbel first)");
  if (value_kind != 0 && value_kind != 1)
    return fail("mz_reanalyse_gumbel: value_kind %d (0 the root's mean value, 1 its v_mix)", value_kind);
  if (rec_floats != MZ_REC_FLOATS(e->O, e->A, 0))
    return fail("mz_reanalyse_gumbel: rec_floats %d != obs_dim + action_space + %d = %d", rec_floats, MZ_REC_EXTRA, MZ_REC_FLOATS(e->O, e->A, 0));
  if (kind < 0 || kind > 3)
    return fail("mz_reanalyse_gumbel: kind must be 0 (synthetic), 1 (TicTacToe), 2 (CartPole) or 3 (Connect Four), got %d", kind);
  if (kind != 0 && game_shape(e, "mz_reanalyse_gumbel", kind)) return -1;
  if (n_rows < 0) return fail("mz_reanalyse_gumbel: n_rows must be >= 0, got %d", n_rows);
  if (num_simulations < 1 || num_simulations > e->sims)
    return fail("mz_reanalyse_gumbel: num_simulations must be in 1 .. %d (the engine's pool), got %d", e->sims, num_simulations);
  if (n_rows == 0) return 0;
  if (!rows_host || !fresh_host) return fail("mz_reanalyse_gumbel: null buffer");
  const float *rows_dev = nullptr;
  float *fresh_dev = nullptr;
  if (hipHostGetDevicePointer((void **)&rows_dev, (void *)rows_host, 0) != hipSuccess || !rows_dev ||
      hipHostGetDevicePointer((void **)&fresh_dev, (void *)fresh_host, 0) != hipSuccess || !fresh_dev) {
    (void)hipGetLastError();
    return fail("mz_reanalyse_gumbel: rows and fresh must be page-locked (pinned) host memory");
  }
  ReanalyseState &rs = e->ra;
  const int B = e->B, O = e->O, A = e->A;
  if (!rs.to_play) {      // (as mz_reanalyse: allocated on the first call of either)
    rs = ReanalyseState{};
    if (dmalloc(e, &rs.obs, (size_t)e->Bp * O) || dmalloc(e, &rs.legal, (size_t)B * A) || dmalloc(e, &rs.to_play, (size_t)B)) {
      rs = ReanalyseState{};
      return -1;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(128), grid_obs(((size_t)B * O + 127) / 128);
  // one chunk; a launch that fails leaves rc set, and what it had enqueued is waited for below
  auto chunk = [&](int at, int n) -> int {
    hipLaunchKernelGGL(k_reanalyse_observe, grid_obs, block, 0, s, rs, rows_dev + (size_t)at * rec_floats, n, rec_floats, kind, B, O, A);
    if (hipGetLastError() != hipSuccess) return fail("mz_reanalyse_gumbel: k_reanalyse_observe did not launch");
    if (mz_initial_inference(e, rs.obs, s)) return -1;
    TREE_LAUNCH(k_tree_root, s, e->tv, (const int8_t *)rs.to_play, (const uint8_t *)rs.legal, (const double *)nullptr,
                e->cfg.root_exploration_fraction, 0);
    TREE_LAUNCH(k_gz_root, s, e->tv, e->gz, (const double *)nullptr, (uint64_t)e->cfg.seed, draw_key,
                (const unsigned long long *)nullptr, at);
    HIPCHECK(hipGetLastError());
    step_restart(e, false, MZ_SP_GUMBEL);
    if (gz_simulations(e, "mz_reanalyse_gumbel", num_simulations, s)) return -1;
#define RA_STORE(G_)                                                                                                     \
  hipLaunchKernelGGL(k_reanalyse_store_gumbel<G_>, dim3(B), dim3(64), 0, s, e->tv, e->gz, fresh_dev + (size_t)at * (A + 2), n, \
                     value_kind)
    switch (e->G) {
      case 4: RA_STORE(4); break;
      case 8: RA_STORE(8); break;
      case 16: RA_STORE(16); break;
      default: RA_STORE(32); break;
    }
#undef RA_STORE
    if (hipGetLastError() != hipSuccess) return fail("mz_reanalyse_gumbel: k_reanalyse_store_gumbel did not launch");
    return 0;
  };
  int rc = 0;
  for (int at = 0; at < n_rows && !rc; at += B) rc = chunk(at, n_rows - at < B ? n_rows - at : B);
  if (rc) {      // what was enqueued still reads / writes the caller's buffers: let it end before they are handed back
    (void)hipStreamSynchronize(s);
    return -1;
  }
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

// Reanalyse on the true rules (DESIGN s7n): mz_reanalyse's buffers, chunks and stored fields -- visit shares and the root's mean
// value, what a record of mz_selfplay_set_true_model holds --, searched as a self-play move of that mode is (launch_move_game,
// mz_selfplay_abi.inc): the root without noise, slot 0 from the stored observation and the record's mover (k_tm_root_reanalyse),
// then all simulations in one launch of k_tm_search (fused) or the two-launch loop.  k_tree_root leaves the first descent to
// k_tm_root_reanalyse, which makes it with the leaf's position: the descent writes nothing but the selection.  The host side of
// the step protocol starts over at every chunk and ends where the search leaves it.
int mz_reanalyse_true_model(mz_engine *e, int kind, const float *rows_host, int rec_floats, int n_rows, float *fresh_host,
                            int num_simulations, int fused, void *stream) {
  if (!e) return fail("mz_reanalyse_true_model: null engine");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_reanalyse_true_model: weights not set (call mz_set_weights)");
  if (!e->tm.kind) return fail("mz_reanalyse_true_model: no true-rules search is set on this engine (call mz_set_true_model first)");
  if (kind != 1 && kind != 3)
    return fail("mz_reanalyse_true_model: kind must be 1 (TicTacToe) or 3 (Connect Four), the games with true rules, got %d", kind);
  if (kind != e->tm.kind)
    return fail("mz_reanalyse_true_model: kind %d is not the game of the engine's true-rules search (mz_set_true_model %d)", kind, e->tm.kind);
  if (rec_floats != MZ_REC_FLOATS(e->O, e->A, 0))
    return fail("mz_reanalyse_true_model: rec_floats %d != obs_dim + action_space + %d = %d", rec_floats, MZ_REC_EXTRA, MZ_REC_FLOATS(e->O, e->A, 0));
  if (n_rows < 0) return fail("mz_reanalyse_true_model: n_rows must be >= 0, got %d", n_rows);
  if (num_simulations < 1 || num_simulations > e->sims)
    return fail("mz_reanalyse_true_model: num_simulations must be in 1 .. %d (the engine's pool), got %d", e->sims, num_simulations);
  if (n_rows == 0) return 0;
  if (!rows_host || !fresh_host) return fail("mz_reanalyse_true_model: null buffer");
  const float *rows_dev = nullptr;
  float *fresh_dev = nullptr;
  if (hipHostGetDevicePointer((void **)&rows_dev, (void *)rows_host, 0) != hipSuccess || !rows_dev ||
      hipHostGetDevicePointer((void **)&fresh_dev, (void *)fresh_host, 0) != hipSuccess || !fresh_dev) {
    (void)hipGetLastError();
    return fail("mz_reanalyse_true_model: rows and fresh must be page-locked (pinned) host memory");
  }
  ReanalyseState &rs = e->ra;
  const int B = e->B, O = e->O, A = e->A;
  if (!rs.to_play) {      // (as mz_reanalyse: allocated on the first call of any of the three)
    rs = ReanalyseState{};
    if (dmalloc(e, &rs.obs, (size_t)e->Bp * O) || dmalloc(e, &rs.legal, (size_t)B * A) || dmalloc(e, &rs.to_play, (size_t)B)) {
      rs = ReanalyseState{};
      return -1;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(128), grid_obs(((size_t)B * O + 127) / 128), grid_store(((size_t)B * (A + 2) + 127) / 128);
  // one chunk; a launch that fails leaves rc set, and what it had enqueued is waited for below
  auto chunk = [&](int at, int n) -> int {
    hipLaunchKernelGGL(k_reanalyse_observe, grid_obs, block, 0, s, rs, rows_dev + (size_t)at * rec_floats, n, rec_floats, kind, B, O, A);
    if (hipGetLastError() != hipSuccess) return fail("mz_reanalyse_true_model: k_reanalyse_observe did not launch");
    if (mz_initial_inference(e, rs.obs, s)) return -1;
    TREE_LAUNCH(k_tree_root, s, e->tv, (const int8_t *)rs.to_play, (const uint8_t *)rs.legal, (const double *)nullptr,
                e->cfg.root_exploration_fraction, 0);
    step_restart(e, false, MZ_SP_TRUE_RULES);
    TREE_LAUNCH(k_tm_root_reanalyse, s, e->tv, e->tm, O, rs);
    HIPCHECK(hipGetLastError());
    if (fused ? tm_simulations_fused(e, "mz_reanalyse_true_model", num_simulations, s)
              : tm_simulations(e, "mz_reanalyse_true_model", num_simulations, s)) return -1;
    hipLaunchKernelGGL(k_reanalyse_store, grid_store, block, 0, s, e->tv, fresh_dev + (size_t)at * (A + 2), n);
    if (hipGetLastError() != hipSuccess) return fail("mz_reanalyse_true_model: k_reanalyse_store did not launch");
    return 0;
  };
  int rc = 0;
  for (int at = 0; at < n_rows && !rc; at += B) rc = chunk(at, n_rows - at < B ? n_rows - at : B);
  if (rc) {      // what was enqueued still reads / writes the caller's buffers: let it end before they are handed back
    (void)hipStreamSynchronize(s);
    return -1;
  }
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}
