// mz_eval_abi.inc -- C ABI of the evaluation games that live on the device environments (included inside extern "C" of
// mz_engine.hip; kernels and state: mz_eval_env.hip.h).  Replaces the host loop between two moves of Evaluator._play_batch
// (reference evaluate.py:331-374) for TicTacToe, CartPole and Connect Four.

// One searched move of engine e on the inputs laid out in io: initial inference, root preparation with the given draws
// (have_noise: io.noise holds them), the device's, or none, then the search with its walk of M actions and finalize (mode
// 0) or the lookahead (mode 1 only_prior, 2 only_value).  temp [B]; have_walk: io.walk_u holds the walk's uniforms.
// An engine whose true-rules search is set (mz_set_true_model) searches the games' real positions instead: mz_tm_root +
// mz_tm_search in place of mz_search, everything around it as it is.  An engine whose Gumbel search is set (mz_set_gumbel)
// runs mz_gz_root + mz_gz_search + the pick in place of mz_search + mz_eval_walk: the pick writes what the walk writes for
// one action per move; mz_finalize still gives the visit fractions and the root value.
static int ply_search(mz_engine *e, const PlyIO &io, int mode, int M, const double *temp, bool noise_on, bool have_noise,
                      bool have_walk, uint64_t move, hipStream_t s) {
  const int tmk = e->tm.kind;
  if (tmk && io.kind == 2) return fail("true_model: CartPole has no true-rules search (TicTacToe and Connect Four have)");
  if (tmk && tmk != io.kind) return fail("true_model: the engine's true-rules search is set for kind %d, the games are of kind %d", tmk, io.kind);
  if (tmk && mode != 0) return fail("true_model: only_prior / only_value (mode %d) run no search; unset the true-rules search for them", mode);
  if (tmk && M != 1) return fail("true_model: the true-rules search takes one action per move (max_actions 1), got %d", M);
  const bool gzo = e->gz.on != 0;
  if (gzo && mode != 0) return fail("gumbel: only_prior / only_value (mode %d) run no search; unset the Gumbel search for them", mode);
  if (gzo && M != 1) return fail("gumbel: the Gumbel search takes one action per move (max_actions 1), got %d", M);
  if (gzo && noise_on) return fail("gumbel: the Gumbel draw replaces the exploration noise at the root (gumbel_scale is the stochastic setting); run without noise");
  if (mz_initial_inference(e, io.obs, s)) return -1;
  const bool given = noise_on && have_noise;
  if (mz_root_prepare(e, io.to_play, io.legal, given ? io.noise : nullptr, noise_on && !given ? 1 : 0, move, s)) return -1;
  if (mode != 0) return mz_eval_lookahead(e, mode, io.actions, io.pred_rewards, io.child_visits, nullptr, nullptr, s);
  if (gzo) {
    if (mz_gz_root(e, nullptr, move, s) || mz_gz_search(e, e->sims, s)) return -1;
    if (gz_pick(e, "gumbel", io.actions, io.pred_rewards, io.n_actions, io.path_lengths, nullptr, nullptr, nullptr, nullptr, s)) return -1;
    return mz_finalize(e, nullptr, nullptr, move, nullptr, io.child_visits, io.root_value, nullptr, nullptr, s);
  }
  if (tmk ? (mz_tm_root(e, io.board, io.turn, io.step, s) || mz_tm_search(e, e->sims, s)) : mz_search(e, e->sims, s)) return -1;
  if (mz_eval_walk(e, M, temp, have_walk ? io.walk_u : nullptr, move, io.actions, io.pred_rewards, io.n_actions,
                   io.path_lengths, s)) return -1;
  return mz_finalize(e, nullptr, nullptr, move, nullptr, io.child_visits, io.root_value, nullptr, nullptr, s);
}

int mz_eval_env_reset(mz_engine *e, int kind, int max_steps, int time_limit, int random_opp, int keep_history, void *stream) {
  if (!e) return fail("mz_eval_env_reset: null engine");
  MZ_ENTER(e);
  if (kind < 1 || kind > 3) return fail("mz_eval_env_reset: kind must be 1 (TicTacToe), 2 (CartPole) or 3 (Connect Four), got %d", kind);
  if (game_shape(e, "mz_eval_env_reset", kind)) return -1;
  if (max_steps < 1) return fail("mz_eval_env_reset: max_steps must be >= 1");
  if (kind == 2 && time_limit < 1) return fail("mz_eval_env_reset: CartPole needs its time limit (>= 1)");
  if (random_opp < -1 || random_opp > 1) return fail("mz_eval_env_reset: random_opp must be -1, 0 (none) or +1");
  EvalState &es = e->ev;
  const int longest = kind == 2 ? time_limit : mz_game_info(kind).longest;
  const int cap = max_steps < longest ? max_steps : longest;
  const size_t nb = (size_t)e->B, A = (size_t)e->A, sims = (size_t)e->sims;
  hipStream_t s = (hipStream_t)stream;
  if (es.board && (es.kind != kind || es.cap != cap || (keep_history && !es.log_action)))
    return fail("mz_eval_env_reset: this engine's evaluation state was sized for another game; create a new engine");
#define DM(p, n) if (dmalloc(e, &(p), (n))) return -1;
  if (!es.board) {
    DM(es.board, nb * 42) DM(es.turn, nb) DM(es.cart, nb * 4) DM(es.step, nb) DM(es.terminal, nb) DM(es.live, 1)
    DM(es.acc, 5 * nb) DM(es.n_moves, nb) DM(es.depth_max, nb * sims)
    DM(es.obs, (size_t)e->Bp * e->O) DM(es.legal, nb * A) DM(es.to_play, nb) DM(es.noise, nb * A) DM(es.temp, nb)
    DM(es.n_actions, nb) DM(es.path_lengths, nb * sims) DM(es.child_visits, nb * A) DM(es.root_value, nb) DM(es.opp_pos, nb)
    if (keep_history) {
      const size_t L = nb * cap;
      DM(es.log_action, L) DM(es.log_reward, L) DM(es.log_mover, L) DM(es.log_pred_reward, L) DM(es.log_pred_value, L)
      DM(es.log_root_value, L) DM(es.log_child_visits, L * A) DM(es.log_n_actions, L) DM(es.log_depths, L * sims)
    }
  }
#undef DM
  es.kind = kind; es.max_steps = max_steps; es.time_limit = time_limit; es.random_opp = random_opp;
  es.two_players = e->cfg.two_players != 0; es.cap = cap; es.sims = e->sims;
  es.d_walk = nullptr; es.d_noise = nullptr; es.d_opp = nullptr;
  es.d_walk_moves = es.d_walk_m = es.d_noise_moves = es.d_opp_n = 0;
  es.opp_playouts = 0; es.opp_action = nullptr;      // the random mover, until mz_eval_env_set_opponent says otherwise
  HIPCHECK(hipMemsetAsync(es.board, 0, nb * 42, s));
  HIPCHECK(hipMemsetAsync(es.turn, 1, nb, s));
  HIPCHECK(hipMemsetAsync(es.step, 0, nb * 4, s));
  HIPCHECK(hipMemsetAsync(es.terminal, 0, nb, s));
  HIPCHECK(hipMemsetAsync(es.acc, 0, 5 * nb * 8, s));
  HIPCHECK(hipMemsetAsync(es.n_moves, 0, nb * 4, s));
  HIPCHECK(hipMemsetAsync(es.depth_max, 0, nb * sims * 4, s));
  HIPCHECK(hipMemsetAsync(es.opp_pos, 0, nb * 4, s));
  const int32_t live = e->B;
  HIPCHECK(hipMemcpyAsync(es.live, &live, 4, hipMemcpyHostToDevice, s));
  if (kind == 2) {      // env.reset(): the counter RNG's start state of (game's seed, episode 0), as the self-play CartPole's
    std::vector<double> st(nb * 4, 0.0);
    for (int b = 0; b < e->B; ++b)
      mz_cartpole_reset_state(e->cfg.seed, (uint32_t)(e->cfg.env_id_offset + b), 0u, st.data() + (size_t)b * 4);
    HIPCHECK(hipMemcpyAsync(es.cart, st.data(), st.size() * 8, hipMemcpyHostToDevice, s));
  }
  HIPCHECK(hipStreamSynchronize(s));
  e->ev_moves = 0;
  es.ready = true;
  return 0;
}

int mz_eval_env_set_draws(mz_engine *e, const double *walk, int walk_moves, int walk_m, const double *noise, int noise_moves,
                          const int32_t *opp, int opp_n, const double *start_states, void *stream) {
  if (!e) return fail("mz_eval_env_set_draws: null engine");
  MZ_ENTER(e);
  EvalState &es = e->ev;
  if (!es.ready) return fail("mz_eval_env_set_draws: call mz_eval_env_reset first");
  if (e->ev_moves) return fail("mz_eval_env_set_draws: the games have started; draws are given before the first move");
  if ((walk && (walk_moves < 1 || walk_m < 1)) || (noise && noise_moves < 1) || (opp && opp_n < 1))
    return fail("mz_eval_env_set_draws: a given array needs its sizes (>= 1)");
  if (start_states && es.kind != 2) return fail("mz_eval_env_set_draws: start states are CartPole's");
  es.d_walk = walk; es.d_walk_moves = walk ? walk_moves : 0; es.d_walk_m = walk ? walk_m : 0;
  es.d_noise = noise; es.d_noise_moves = noise ? noise_moves : 0;
  es.d_opp = opp; es.d_opp_n = opp ? opp_n : 0;
  if (start_states)
    HIPCHECK(hipMemcpyAsync(es.cart, start_states, (size_t)e->B * 4 * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int mz_eval_env_moves(mz_engine *e, int n, int mode, int max_actions, double temperature, int noise_on, int *live_out,
                      void *stream) {
  if (!e || !live_out) return fail("mz_eval_env_moves: null argument");
  MZ_ENTER(e);
  EvalState &es = e->ev;
  if (!es.ready) return fail("mz_eval_env_moves: call mz_eval_env_reset first");
  if (!e->weights_set) return fail("mz_eval_env_moves: weights not set (call mz_set_weights)");
  if (n < 0) return fail("mz_eval_env_moves: n must be >= 0");
  if (mode < 0 || mode > 2) return fail("mz_eval_env_moves: mode must be 0 (search), 1 (only_prior) or 2 (only_value), got %d", mode);
  const int M = mode == 0 ? max_actions : 1;
  if (M < 1) return fail("mz_eval_env_moves: max_actions must be >= 1");
  if (es.kind == 3 && M != 1)
    return fail("mz_eval_env_moves: Connect Four takes one action per move (below the root the walk offers full columns)");
  if (es.opp_playouts > 0 && M != 1)
    return fail("mz_eval_env_moves: the playout opponent takes one action per move (max_actions 1), got %d", M);
  if (es.d_walk && mode == 0 && es.d_walk_m != M)
    return fail("mz_eval_env_moves: the given walk uniforms are [B][moves][%d], the walk takes %d actions", es.d_walk_m, M);
  hipStream_t s = (hipStream_t)stream;
  const int B = e->B, A = e->A;
  if (es.walk_cap < M) {      // the walk's buffers, sized on the first call (which therefore synchronises)
    if (es.walk_cap) return fail("mz_eval_env_moves: max_actions changed from %d to %d within one engine", es.walk_cap, M);
    if (dmalloc(e, &es.actions, (size_t)B * M) || dmalloc(e, &es.pred_rewards, (size_t)B * M) ||
        dmalloc(e, &es.walk_u, (size_t)B * M)) return -1;
    es.walk_cap = M;
  }
  if (e->ev_temp != temperature || !e->ev_temp_set) {
    std::vector<double> t((size_t)B, temperature);
    HIPCHECK(hipMemcpyAsync(es.temp, t.data(), t.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    e->ev_temp = temperature; e->ev_temp_set = true;
  }
  const dim3 grid((B + 127) / 128), block(128);
  for (int i = 0; i < n; ++i) {
    const int move = (int)e->ev_moves;
    hipLaunchKernelGGL(k_eval_observe, grid, block, 0, s, es, B, e->O, A, M, move);
    HIPCHECK(hipGetLastError());
    if (ply_search(e, es, mode, M, es.temp, noise_on != 0, es.d_noise != nullptr, es.d_walk != nullptr, (uint64_t)move, s))
      return -1;
    if (es.opp_playouts > 0 &&      // the opponent's move in the live games that are its to move, keyed by this move
        playout_launch(e, "mz_eval_env_moves", es.kind, es.board, es.turn, es.step, es.terminal, es.random_opp, B,
                       es.opp_playouts, (uint64_t)move, es.opp_action, nullptr, nullptr, s)) return -1;
    hipLaunchKernelGGL(k_eval_apply, grid, block, 0, s, es, (const float *)e->tv.root_value, B, A, M, mode, move,
                       (uint64_t)e->cfg.seed, e->cfg.env_id_offset);
    HIPCHECK(hipGetLastError());
    e->ev_moves += 1;
  }
  int32_t live = 0;
  HIPCHECK(hipMemcpyAsync(&live, es.live, 4, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *live_out = live;
  return 0;
}

int mz_eval_env_results(mz_engine *e, int32_t *step, int32_t *n_moves, double *acc, int32_t *depth_max, int32_t *actions,
                        double *rewards, int8_t *mover, float *pred_rewards, float *pred_values, double *root_values,
                        double *child_visits, int32_t *n_actions, int32_t *depths, void *stream) {
  if (!e) return fail("mz_eval_env_results: null engine");
  MZ_ENTER(e);
  EvalState &es = e->ev;
  if (!es.ready) return fail("mz_eval_env_results: call mz_eval_env_reset first");
  const bool want_logs = actions || rewards || mover || pred_rewards || pred_values || root_values || child_visits ||
                         n_actions || depths;
  if (want_logs && !es.log_action) return fail("mz_eval_env_results: no logs were kept (mz_eval_env_reset's keep_history)");
  hipStream_t s = (hipStream_t)stream;
  HIPCHECK(hipStreamSynchronize(s));
  const size_t nb = (size_t)e->B, L = nb * es.cap;
#define OUT(dst, src, n) if (dst) HIPCHECK(hipMemcpy((dst), (src), (n) * sizeof(*(dst)), hipMemcpyDeviceToHost));
  OUT(step, es.step, nb) OUT(n_moves, es.n_moves, nb) OUT(acc, es.acc, 5 * nb) OUT(depth_max, es.depth_max, nb * e->sims)
  OUT(actions, es.log_action, L) OUT(rewards, es.log_reward, L) OUT(mover, es.log_mover, L)
  OUT(pred_rewards, es.log_pred_reward, L) OUT(pred_values, es.log_pred_value, L) OUT(root_values, es.log_root_value, L)
  OUT(child_visits, es.log_child_visits, L * e->A) OUT(n_actions, es.log_n_actions, L) OUT(depths, es.log_depths, L * e->sims)
#undef OUT
  return 0;
}

int mz_eval_env_log_capacity(const mz_engine *e) {
  if (!e || !e->ev.ready) return fail("mz_eval_env_log_capacity: call mz_eval_env_reset first");
  return e->ev.cap;
}
