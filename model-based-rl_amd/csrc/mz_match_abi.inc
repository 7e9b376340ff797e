// mz_match_abi.inc -- C ABI of a match between two networks on the device games (included inside extern "C" of
// mz_engine.hip; kernels and state: mz_match.hip.h).  Replaces the per-ply host loop a match driven from Python would
// need: two Evaluator._play_batch loops interleaved by hand, one engine call sequence and one host environment step per ply.

static int match_alloc(mz_match *m, void **p, size_t bytes) {
  void *q = nullptr;
  HIPCHECK(hipMalloc(&q, bytes + 64));
  HIPCHECK(hipMemset(q, 0, bytes + 64));
  m->allocs.push_back(q);
  *p = q;
  return 0;
}

int mz_match_destroy(mz_match *m) {
  if (!m) return 0;
  hipSetDevice(m->device);
  hipDeviceSynchronize();
  for (void *p : m->allocs) hipFree(p);
  delete m;
  return 0;
}

int mz_match_create(mz_engine *e0, mz_engine *e1, int kind, int max_steps, int keep_history, mz_match **out) {
  if (!e0 || !e1 || !out) return fail("mz_match_create: null argument");
  *out = nullptr;
  if (kind == 2) return fail("mz_match_create: CartPole (kind 2) has a single player; a match is played on TicTacToe (1) or Connect Four (3)");
  if (kind != 1 && kind != 3) return fail("mz_match_create: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", kind);
  if (!e0->cfg.two_players || !e1->cfg.two_players) return fail("mz_match_create: a single-player engine cannot play a match");
  if (e0->device != e1->device) return fail("mz_match_create: the two engines live on different devices (%d and %d)", e0->device, e1->device);
  if (e0->B != e1->B) return fail("mz_match_create: the two engines hold different numbers of games (%d and %d)", e0->B, e1->B);
  if (e0->O != e1->O || e0->A != e1->A)
    return fail("mz_match_create: the two engines have different shapes (obs_dim %d / %d, action_space %d / %d)", e0->O, e1->O, e0->A, e1->A);
  if (e0->cfg.seed != e1->cfg.seed || e0->cfg.env_id_offset != e1->cfg.env_id_offset)
    return fail("mz_match_create: the two engines key their draws differently (seed and env_id_offset must be equal)");
  if (game_shape(e0, "mz_match_create", kind)) return -1;
  if (max_steps < 1) return fail("mz_match_create: max_steps must be >= 1");
  MZ_ENTER(e0);
  mz_match *m = new mz_match();
  m->e[0] = e0; m->e[1] = e1;
  m->device = e0->device; m->B = e0->B; m->A = e0->A; m->O = e0->O;
  m->keep = keep_history != 0;
  MatchState &ms = m->ms;
  memset(&ms, 0, sizeof ms);
  const int longest = mz_game_info(kind).longest;
  ms.kind = kind; ms.max_steps = max_steps; ms.cap = max_steps < longest ? max_steps : longest;
  ms.S = e0->sims > e1->sims ? e0->sims : e1->sims;
  const size_t nb = (size_t)m->B, A = (size_t)m->A, S = (size_t)ms.S;
#define DM(p, n) if (match_alloc(m, (void **)&(p), (n) * sizeof(*(p)))) { mz_match_destroy(m); return -1; }
  DM(ms.board, nb * 42) DM(ms.turn, nb) DM(ms.step, nb) DM(ms.terminal, nb) DM(ms.live, 1) DM(ms.result, nb)
  DM(ms.acc, 8 * nb) DM(ms.n_searched, 2 * nb) DM(ms.depth_max, 2 * nb * S)
  DM(ms.obs, (size_t)e0->Bp * m->O) DM(ms.legal, nb * A) DM(ms.to_play, nb) DM(ms.noise, nb * A) DM(ms.walk_u, nb)
  DM(ms.temp, 2 * nb) DM(ms.actions, nb) DM(ms.pred_rewards, nb) DM(ms.n_actions, nb) DM(ms.path_lengths, nb * S)
  DM(ms.child_visits, nb * A) DM(ms.root_value, nb)
  if (m->keep) {
    const size_t L = nb * ms.cap;
    DM(ms.log_action, L) DM(ms.log_mover, L) DM(ms.log_net, L) DM(ms.log_reward, L) DM(ms.log_pred_reward, L)
    DM(ms.log_pred_value, L) DM(ms.log_root_value, L) DM(ms.log_child_visits, L * A) DM(ms.log_depths, L * S)
  }
#undef DM
  *out = m;
  return 0;
}

int mz_match_reset(mz_match *m, int first_net, int opening_plies, void *stream) {
  if (!m) return fail("mz_match_reset: null match");
  MZ_ENTER(m);
  MatchState &ms = m->ms;
  if (first_net != 0 && first_net != 1) return fail("mz_match_reset: first_net must be 0 or 1, got %d", first_net);
  if (opening_plies < 0 || opening_plies >= ms.max_steps)
    return fail("mz_match_reset: opening_plies %d outside [0, max_steps = %d)", opening_plies, ms.max_steps);
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = (size_t)m->B, A = (size_t)m->A, S = (size_t)ms.S;
  ms.opening = opening_plies;
  ms.d_walk = nullptr; ms.d_noise = nullptr; ms.d_open = nullptr;
  ms.d_walk_plies = ms.d_noise_plies = ms.d_open_n = 0;
  HIPCHECK(hipMemsetAsync(ms.board, 0, nb * 42, s));
  HIPCHECK(hipMemsetAsync(ms.turn, 1, nb, s));
  HIPCHECK(hipMemsetAsync(ms.step, 0, nb * 4, s));
  HIPCHECK(hipMemsetAsync(ms.terminal, 0, nb, s));
  HIPCHECK(hipMemsetAsync(ms.result, 0, nb, s));
  HIPCHECK(hipMemsetAsync(ms.acc, 0, 8 * nb * 8, s));
  HIPCHECK(hipMemsetAsync(ms.n_searched, 0, 2 * nb * 4, s));
  HIPCHECK(hipMemsetAsync(ms.depth_max, 0, 2 * nb * S * 4, s));
  if (m->keep) {
    const size_t L = nb * ms.cap;
    HIPCHECK(hipMemsetAsync(ms.log_action, 0, L * 4, s));
    HIPCHECK(hipMemsetAsync(ms.log_mover, 0, L, s));
    HIPCHECK(hipMemsetAsync(ms.log_net, 0, L, s));
    HIPCHECK(hipMemsetAsync(ms.log_reward, 0, L * 8, s));
    HIPCHECK(hipMemsetAsync(ms.log_pred_reward, 0, L * 4, s));
    HIPCHECK(hipMemsetAsync(ms.log_pred_value, 0, L * 4, s));
    HIPCHECK(hipMemsetAsync(ms.log_root_value, 0, L * 8, s));
    HIPCHECK(hipMemsetAsync(ms.log_child_visits, 0, L * A * 8, s));
    HIPCHECK(hipMemsetAsync(ms.log_depths, 0, L * S * 4, s));
  }
  const int32_t live = m->B;
  HIPCHECK(hipMemcpyAsync(ms.live, &live, 4, hipMemcpyHostToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  m->first_net = first_net;
  m->plies = 0;
  m->opened = false;
  m->ready = true;
  return 0;
}

int mz_match_set_draws(mz_match *m, const double *walk, int walk_plies, const double *noise, int noise_plies,
                       const int32_t *opening, int opening_n, void *stream) {
  (void)stream;
  if (!m) return fail("mz_match_set_draws: null match");
  MatchState &ms = m->ms;
  if (!m->ready) return fail("mz_match_set_draws: call mz_match_reset first");
  if (m->opened || m->plies) return fail("mz_match_set_draws: the games have started; draws are given before the first ply");
  if ((walk && walk_plies < 1) || (noise && noise_plies < 1) || (opening && opening_n < 1))
    return fail("mz_match_set_draws: a given array needs its size (>= 1)");
  ms.d_walk = walk; ms.d_walk_plies = walk ? walk_plies : 0;
  ms.d_noise = noise; ms.d_noise_plies = noise ? noise_plies : 0;
  ms.d_open = opening; ms.d_open_n = opening ? opening_n : 0;
  return 0;
}

int mz_match_plies(mz_match *m, int n, const int *mode, const double *temperature, const int *noise_on, int *live_out,
                   void *stream) {
  if (!m || !mode || !temperature || !noise_on || !live_out) return fail("mz_match_plies: null argument");
  MZ_ENTER(m);
  MatchState &ms = m->ms;
  if (!m->ready) return fail("mz_match_plies: call mz_match_reset first");
  if (n < 0) return fail("mz_match_plies: n must be >= 0");
  for (int k = 0; k < 2; ++k) {
    if (!m->e[k]->weights_set) return fail("mz_match_plies: network %d has no weights (call mz_set_weights on its engine)", k);
    if (mode[k] < 0 || mode[k] > 2)
      return fail("mz_match_plies: mode must be 0 (search), 1 (only_prior) or 2 (only_value), got %d for network %d", mode[k], k);
  }
  hipStream_t s = (hipStream_t)stream;
  const int B = m->B, A = m->A;
  const dim3 grid((B + 127) / 128), block(128);
  if (!m->temp_set || m->temp[0] != temperature[0] || m->temp[1] != temperature[1]) {
    hipLaunchKernelGGL(k_match_temperature, grid, block, 0, s, ms.temp, B, temperature[0], temperature[1]);
    HIPCHECK(hipGetLastError());
    m->temp[0] = temperature[0]; m->temp[1] = temperature[1]; m->temp_set = true;
  }
  if (!m->opened) {
    if (ms.opening > 0) {
      hipLaunchKernelGGL(k_match_open, grid, block, 0, s, ms, B, A, (uint64_t)m->e[0]->cfg.seed, m->e[0]->cfg.env_id_offset);
      HIPCHECK(hipGetLastError());
    }
    m->plies = (unsigned long long)ms.opening;
    m->opened = true;
  }
  for (int i = 0; i < n; ++i) {
    const int ply = (int)m->plies;
    const int net = ((ply - ms.opening) % 2 == 0) ? m->first_net : 1 - m->first_net;
    mz_engine *e = m->e[net];
    const int md = mode[net];
    hipLaunchKernelGGL(k_match_observe, grid, block, 0, s, ms, B, m->O, A, ply);
    HIPCHECK(hipGetLastError());
    if (ply_search(e, ms, md, 1, ms.temp + (size_t)net * B, noise_on[net] != 0, ms.d_noise != nullptr, ms.d_walk != nullptr,
                   (uint64_t)ply, s)) return -1;
    hipLaunchKernelGGL(k_match_apply, grid, block, 0, s, ms, (const float *)e->tv.root_value, B, A, net, md, e->sims);
    HIPCHECK(hipGetLastError());
    m->plies += 1;
  }
  int32_t live = 0;
  HIPCHECK(hipMemcpyAsync(&live, ms.live, 4, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *live_out = live;
  return 0;
}

int mz_match_results(mz_match *m, int8_t *result, int32_t *length, int32_t *n_searched, double *acc, int32_t *depth_max,
                     int32_t *actions, int8_t *mover, int8_t *net, double *rewards, float *pred_rewards, float *pred_values,
                     double *root_values, double *child_visits, int32_t *depths, void *stream) {
  if (!m) return fail("mz_match_results: null match");
  MZ_ENTER(m);
  MatchState &ms = m->ms;
  if (!m->ready) return fail("mz_match_results: call mz_match_reset first");
  const bool want_logs = actions || mover || net || rewards || pred_rewards || pred_values || root_values || child_visits || depths;
  if (want_logs && !m->keep) return fail("mz_match_results: no logs were kept (mz_match_create's keep_history)");
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  const size_t nb = (size_t)m->B, L = nb * ms.cap;
#define OUT(dst, src, n) if (dst) HIPCHECK(hipMemcpy((dst), (src), (n) * sizeof(*(dst)), hipMemcpyDeviceToHost));
  OUT(result, ms.result, nb) OUT(length, ms.step, nb) OUT(n_searched, ms.n_searched, 2 * nb) OUT(acc, ms.acc, 8 * nb)
  OUT(depth_max, ms.depth_max, 2 * nb * ms.S)
  OUT(actions, ms.log_action, L) OUT(mover, ms.log_mover, L) OUT(net, ms.log_net, L) OUT(rewards, ms.log_reward, L)
  OUT(pred_rewards, ms.log_pred_reward, L) OUT(pred_values, ms.log_pred_value, L) OUT(root_values, ms.log_root_value, L)
  OUT(child_visits, ms.log_child_visits, L * m->A) OUT(depths, ms.log_depths, L * ms.S)
#undef OUT
  return 0;
}

int mz_match_log_capacity(const mz_match *m) {
  if (!m) return fail("mz_match_log_capacity: null match");
  return m->ms.cap;
}
