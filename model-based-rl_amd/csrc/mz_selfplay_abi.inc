// mz_selfplay_abi.inc -- C ABI of the on-device self-play loop (included inside extern "C" of
// mz_engine.hip).  Replaces the per-move body of Actor.play_game (reference actors.py:131-173) for B
// synthetic environments; the history hand-off to the replay buffer (actors.py:160-169) is the drain.

// while the moves are not searched with PUCT on the learned model (mz_selfplay_mode.inc), fn refuses: the one sentence of the mode
static int refuse_searched(const mz_engine *e, const char *fn, const char *why) {
  char buf[256];
  return e->sp_mode == MZ_SP_PUCT ? 0 : fail("%s", mz_sp_refusal(buf, sizeof buf, fn, e->sp_mode, why));
}

static int selfplay_alloc(mz_engine *e) {
  SelfplayState &sp = e->sp;
  if (sp.t) return 0;
  const size_t nb = (size_t)e->Bp;
#define DM(p, n) if (dmalloc(e, &(p), (n))) return -1;
  DM(sp.t, nb) DM(sp.episode, nb) DM(sp.obs, nb * e->O) DM(sp.temp, nb) DM(sp.temp_next, 1) DM(sp.action, nb)
  DM(sp.child_visits, nb * e->A) DM(sp.root_value, nb) DM(sp.error, nb) DM(sp.movecnt, nb)
  sp.obs_slots = MZ_REC_OBS_SLOTS(e->O, sp.obs_u8 == 2);
  sp.rec_floats = MZ_REC_FLOATS(e->O, e->A, 0);      // (the ring is sized for unpacked observations; set_obs may shrink the record)
  sp.ring_moves = e->ring.capacity = RecordRing::capacity_for((size_t)e->B * sp.rec_floats * sizeof(float));
  DM(sp.ring, (size_t)sp.ring_moves * e->B * sp.rec_floats)
#undef DM
  sp.env_offset = e->cfg.env_id_offset;
  return 0;
}

int mz_selfplay_reset(mz_engine *e, int episode_len, double temperature, int stagger, void *stream) {
  if (!e) return fail("mz_selfplay_reset: null engine");
  MZ_ENTER(e);
  if (episode_len < 1) return fail("mz_selfplay_reset: episode_len must be >= 1");
  if (selfplay_alloc(e)) return -1;
  hipStream_t s = (hipStream_t)stream;
  SelfplayState &sp = e->sp;
  sp.episode_len = episode_len;
  {
    // stagger: env i starts its first episode at t0 = hash(global env id) % episode_len, so episodes end
    // (and histories reach the replay buffer) at a uniform rate, as they do with real variable-length envs
    std::vector<int32_t> t0(e->Bp, 0);
    if (stagger)
      for (int b = 0; b < e->B; ++b)
        t0[b] = (int32_t)(((uint32_t)(e->cfg.env_id_offset + b) * 2654435761u >> 8) % (uint32_t)episode_len);
    HIPCHECK(hipMemcpyAsync(sp.t, t0.data(), t0.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  if (sp.env_kind == 1 || sp.env_kind == 3) {      // a board game: env.reset() everywhere (tic_tac_toe.py:20-25); real games end by themselves
    const MzGameInfo g = mz_game_info(sp.env_kind);
    sp.episode_len = g.longest;
    HIPCHECK(hipMemsetAsync(sp.t, 0, (size_t)e->Bp * 4, s));
    HIPCHECK(hipMemsetAsync(sp.board, 0, (size_t)e->Bp * g.cells, s));
    HIPCHECK(hipMemsetAsync(sp.turn, 1, (size_t)e->Bp, s));
  }
  if (sp.env_kind == 2) {      // CartPole: episode_len is the time limit; every environment starts episode 0 at step 0
    std::vector<double> st((size_t)e->Bp * 4, 0.0);
    for (int b = 0; b < e->B; ++b)
      mz_cartpole_reset_state(e->cfg.seed, (uint32_t)(e->cfg.env_id_offset + b), 0u, st.data() + (size_t)b * 4);
    HIPCHECK(hipMemsetAsync(sp.t, 0, (size_t)e->Bp * 4, s));
    HIPCHECK(hipMemcpyAsync(sp.cart, st.data(), st.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  HIPCHECK(hipMemsetAsync(sp.episode, 0, (size_t)e->Bp * 4, s));
  HIPCHECK(hipMemsetAsync(sp.movecnt, 0, (size_t)e->Bp * 8, s));
  std::vector<double> temp(e->Bp, temperature);
  HIPCHECK(hipMemcpyAsync(sp.temp, temp.data(), temp.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(sp.temp_next, temp.data(), 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  // drains issued on COPY streams may still be reading the ring (only the compute stream was synchronised above): wait
  // for the latest one -- drains are chained, so it covers every earlier copy -- before the ordering state is dropped
  // and the next moves may overwrite any slot
  if (e->ring.latest()) HIPCHECK(hipEventSynchronize((hipEvent_t)e->ring.latest()));
  e->ring.forget(0);
  sp.ready = true;
  drop_graphs(e, false);
  return 0;
}

// One move of a game environment (mz_selfplay_set_env), the only statement of it (DESIGN s7l): every step of actors.py:131-158 is its own
// launch here -- observe, initial inference on that observation, the root with its noise, the search of the loop's mode, end of move with the
// real env.step --, on the stream, no host round trip, the same arguments at every move; up to 16 moves per hipGraph like every other configuration.
static int launch_move_game(mz_engine *e, const SearchOpts &o, hipStream_t s) {
  SelfplayState &sp = e->sp;
  const int B = e->B, A = e->A;
  const MzSpMode mode = e->sp_mode;
  const dim3 per_env((B + 127) / 128), threads(128);
  hipLaunchKernelGGL(k_game_observe, per_env, threads, 0, s, sp, B, e->O, A);
  if (launch_root(e, sp.obs, false, s)) return -1;
  // the root's noise: the Dirichlet draw over the legal actions, keyed by the environments' move counter -- a record does not depend on its batch, a
  // captured graph draws afresh at every replay --, or the host's draw (PUCT only); none, and no first PUCT descent, at the Gumbel root: k_gz_root's
  const bool noise = mode != MZ_SP_GUMBEL;
  if (noise && !e->draws_noise)
    hipLaunchKernelGGL(k_dirichlet, per_env, threads, 0, s, e->tv, (const uint8_t *)sp.legal, e->cfg.root_dirichlet_alpha, e->cfg.seed, 0ull,
                       (const unsigned long long *)sp.movecnt, sp.env_offset);
  // (a timed run clocks the search kernel's dispatch, not the root's)
  TREE_LAUNCH(k_tree_root, s, e->tv, (const int8_t *)sp.to_play, (const uint8_t *)sp.legal, noise ? (const double *)e->tv.noise : nullptr,
              e->cfg.root_exploration_fraction, noise ? 1 : 0);
  // the mode's own root and its simulations; the step protocol's host side starts over at every move: k moves follow one another in a chunk or a capture
  if (mode != MZ_SP_PUCT) step_restart(e, noise, mode);
  if (mode == MZ_SP_GUMBEL) {      // G drawn under the move read from the environments' counter, what keys a PUCT move's Dirichlet draw
    TREE_LAUNCH(k_gz_root, s, e->tv, e->gz, (const double *)nullptr, (uint64_t)e->cfg.seed, (uint64_t)0, (const unsigned long long *)sp.movecnt,
                sp.env_offset);
    if (gz_simulations(e, "mz_selfplay_steps", e->sims, s)) return -1;
  } else if (mode == MZ_SP_TRUE_RULES) {      // the root's position from the environment itself; one launch of k_tm_search, or the two-launch loop
    TREE_LAUNCH(k_tm_root_selfplay, s, e->tv, e->tm, e->O, sp);
    if (e->sp_tm_fused ? tm_simulations_fused(e, "mz_selfplay_steps", e->sims, s) : tm_simulations(e, "mz_selfplay_steps", e->sims, s)) return -1;
  } else if (launch_search(e, o, true, s)) return -1;      // PUCT on the learned model: the search kernel
  // the end of the move.  Gumbel: pick, pi' in the policy slots and env.step in one launch (mz_gumbel_selfplay.hip.h); else the PUCT move's (the true-rules tree is in the engine's own node records)
#define GZ_MOVE(G_, KIND_) \
  hipLaunchKernelGGL((k_gz_move_record<G_, KIND_>), dim3(B), dim3(64), 0, s, e->tv, e->gz, sp, e->sp_gumbel_value, (uint64_t)e->cfg.seed)
#define GZ_MOVE_G(KIND_)                    \
  switch (e->G) {                           \
    case 4: GZ_MOVE(4, KIND_); break;       \
    case 8: GZ_MOVE(8, KIND_); break;       \
    case 16: GZ_MOVE(16, KIND_); break;     \
    default: GZ_MOVE(32, KIND_); break;     \
  }
  if (mode == MZ_SP_GUMBEL && sp.env_kind == 2) { GZ_MOVE_G(2) }
  else if (mode == MZ_SP_GUMBEL && sp.env_kind == 3) { GZ_MOVE_G(3) }
  else if (mode == MZ_SP_GUMBEL) { GZ_MOVE_G(1) }
  else if (sp.env_kind == 2) hipLaunchKernelGGL(k_cartpole_step_record, per_env, threads, 0, s, e->tv, sp, B, A, e->cfg.seed);
  else if (sp.env_kind == 3) hipLaunchKernelGGL(k_board_step_record<3>, per_env, threads, 0, s, e->tv, sp, B, A, e->cfg.seed);
  else hipLaunchKernelGGL(k_board_step_record<1>, per_env, threads, 0, s, e->tv, sp, B, A, e->cfg.seed);
#undef GZ_MOVE_G
#undef GZ_MOVE
  HIPCHECK(hipGetLastError());
  return 0;
}

// o: the move's search (all simulations; mz_selfplay_steps_timed adds events around its dispatch)
static int launch_move(mz_engine *e, SearchOpts o, hipStream_t s) {
  SelfplayState &sp = e->sp;
  const int B = e->B, O = e->O, A = e->A;
  if (sp.env_kind) return launch_move_game(e, o, s);
  // observation + initial inference + root expansion with Dirichlet noise + first descent: one launch
  if (launch_root(e, nullptr, true, s)) return -1;
  // search; the fused kernel also finalizes the move (action, visit distribution, env step, record) in its tail
  const bool fused = fused_usable(e);
  o.record = fused;
  if (launch_search(e, o, true, s)) return -1;
  if (!fused)
    hipLaunchKernelGGL(k_env_step_record, dim3((B + 127) / 128), dim3(128), 0, s, e->tv, sp, B, O, A, e->cfg.seed);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The temperature every environment's NEXT game starts with (actors.py:128-129 evaluates
// config.visit_softmax_temperature(training_step) at the top of play_game; config.py:41-49).  Games in progress keep
// theirs.  Read from device memory by the kernels, so captured graphs stay valid.
int mz_selfplay_set_temperature(mz_engine *e, double temperature, void *stream) {
  if (!e) return fail("mz_selfplay_set_temperature: null engine");
  MZ_ENTER(e);
  if (!e->sp.ready) return fail("mz_selfplay_set_temperature: call mz_selfplay_reset first");
  if (!(temperature >= 0.0)) return fail("mz_selfplay_set_temperature: temperature must be >= 0");
  hipLaunchKernelGGL(k_store_double, dim3(1), dim3(1), 0, (hipStream_t)stream, e->sp.temp_next, temperature);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The move counter of every environment (what keys the device RNG and places the records): a caller may continue a resumed run's
// count, and the tests start close to 2^30 and 2^32 to cross the places where the counter's low words wrap.
// The device ring must be empty (drained); synchronous.
int mz_selfplay_set_moves(mz_engine *e, unsigned long long moves) {
  if (!e) return fail("mz_selfplay_set_moves: null engine");
  MZ_ENTER(e);
  SelfplayState &sp = e->sp;
  if (!sp.ready) return fail("mz_selfplay_set_moves: call mz_selfplay_reset first");
  if (e->ring.undrained()) return fail("mz_selfplay_set_moves: %llu moves wait in the device ring; drain them first", e->ring.undrained());
  HIPCHECK(hipDeviceSynchronize());        // (moves in flight still read the counters; drains still read the ring)
  std::vector<unsigned long long> m((size_t)e->Bp, moves);
  HIPCHECK(hipMemcpy(sp.movecnt, m.data(), m.size() * 8, hipMemcpyHostToDevice));
  e->ring.forget(moves);
  return 0;
}

// Observation format of the synthetic env: uint8_obs != 0 = byte-valued observations (the -ram- shapes); obs_min /
// obs_range [host][obs_dim] or NULL = --norm_obs (actors.py:55-58: min = obs_range[::2], range = max - min): the
// network sees (obs - min) / range, the experience record keeps the raw observation (the learner normalises its
// batches itself, learners.py:167-168).  Call before mz_selfplay_reset / between drains; synchronous.
int mz_selfplay_set_obs(mz_engine *e, int uint8_obs, const float *obs_min, const float *obs_range) {
  if (!e) return fail("mz_selfplay_set_obs: null engine");
  MZ_ENTER(e);
  if ((obs_min == nullptr) != (obs_range == nullptr)) return fail("mz_selfplay_set_obs: give both obs_min and obs_range or neither");
  HIPCHECK(hipDeviceSynchronize());
  SelfplayState &sp = e->sp;
  if (uint8_obs < 0 || uint8_obs > 2) return fail("mz_selfplay_set_obs: uint8_obs %d (0 float, 1 byte-valued, 2 byte-valued and packed in the record)", uint8_obs);
  if (uint8_obs == 2 && sp.env_kind) return fail("mz_selfplay_set_obs: packed byte observations are for the synthetic -ram- environments");
  if ((sp.env_kind == 2 || sp.env_kind == 3) && (uint8_obs || obs_min))
    return fail("mz_selfplay_set_obs: the %s environment has neither byte observations nor --norm_obs", mz_game_info(sp.env_kind).name);
  if (selfplay_alloc(e)) return -1;
  if (e->ring.undrained()) return fail("mz_selfplay_set_obs: drain the ring first (the record layout may change)");
  sp.obs_u8 = uint8_obs;
  sp.obs_slots = MZ_REC_OBS_SLOTS(e->O, uint8_obs == 2);
  sp.rec_floats = MZ_REC_FLOATS(e->O, e->A, uint8_obs == 2);
  if (obs_min) {
    for (int k = 0; k < e->O; ++k)
      if (!(obs_range[k] != 0.f)) return fail("mz_selfplay_set_obs: obs_range[%d] is zero", k);
    if (!e->obs_norm) { if (dmalloc(e, &e->obs_norm, (size_t)2 * e->O)) return -1; }
    HIPCHECK(hipMemcpy(e->obs_norm, obs_min, (size_t)e->O * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(e->obs_norm + e->O, obs_range, (size_t)e->O * 4, hipMemcpyHostToDevice));
    e->obs_norm_host.assign(obs_min, obs_min + e->O);
    e->obs_norm_host.insert(e->obs_norm_host.end(), obs_range, obs_range + e->O);
    sp.obs_min = e->obs_norm; sp.obs_rng = e->obs_norm + e->O;
  } else {
    sp.obs_min = sp.obs_rng = nullptr;
  }
  drop_graphs(e, false);
  return 0;
}

// keep != 0: every move writes its searched tree back to the global pool (mz_export_tree after mz_selfplay_steps);
// the self-play loop itself never reads it (default 0).
int mz_selfplay_export_trees(mz_engine *e, int keep) {
  if (!e) return fail("mz_selfplay_export_trees: null engine");
  MZ_ENTER(e);
  HIPCHECK(hipDeviceSynchronize());
  e->sp.export_trees = keep ? 1 : 0;
  drop_graphs(e, false);
  return 0;
}

// The environment of the self-play loop.  kind 0: the synthetic fixed-length episodes (default).  kind 1: TicTacToe with
// the reference's rules (custom_environments/tic_tac_toe.py:5-76) -- needs obs_dim 9, action_space 9 and a two-player
// engine; observations, legal moves, wins, draws and the alternating to_play all live on the device.  kind 2: CartPole
// (envs.CartPole: CartPole-v1 / -v0) -- needs obs_dim 4, action_space 2 and a single-player engine; the float64 state,
// termination and the time limit (mz_selfplay_reset's episode_len) live on the device.  kind 3: Connect Four
// (envs.ConnectFour) -- needs obs_dim 42, action_space 7 and a two-player engine; board, turn, full columns, lines of four
// and draws live on the device.  Call before mz_selfplay_reset.
int mz_selfplay_set_env(mz_engine *e, int kind) {
  if (!e) return fail("mz_selfplay_set_env: null engine");
  MZ_ENTER(e);
  if (kind < 0 || kind > 3) return fail("mz_selfplay_set_env: unknown environment %d (0 synthetic, 1 TicTacToe, 2 CartPole, 3 Connect Four)", kind);
  if (refuse_searched(e, "mz_selfplay_set_env", "set for the current game")) return -1;
  if (kind != 0 && game_shape(e, "mz_selfplay_set_env", kind)) return -1;
  if (kind == 3 && e->sp.obs_u8 == 2)
    return fail("mz_selfplay_set_env: packed byte observations are for the synthetic -ram- environments");
  if ((kind == 2 || kind == 3) && (e->sp.obs_u8 || e->sp.obs_min))
    return fail("mz_selfplay_set_env: the %s environment has neither byte observations nor --norm_obs", mz_game_info(kind).name);
  if (selfplay_alloc(e)) return -1;
  HIPCHECK(hipDeviceSynchronize());
  SelfplayState &sp = e->sp;
  if ((kind == 1 || kind == 3) && !sp.board) {      // (the two board games differ in obs_dim: an engine plays one of them)
    if (dmalloc(e, &sp.board, (size_t)e->Bp * mz_game_info(kind).cells) || dmalloc(e, &sp.turn, (size_t)e->Bp) ||
        dmalloc(e, &sp.legal, (size_t)e->Bp * e->A) || dmalloc(e, &sp.to_play, (size_t)e->Bp) ||
        dmalloc(e, &e->draw_uniform, (size_t)e->Bp))
      return -1;
  }
  if (kind == 2 && !sp.cart) {
    if (dmalloc(e, &sp.cart, (size_t)e->Bp * 4)) return -1;
    if (!sp.legal && (dmalloc(e, &sp.legal, (size_t)e->Bp * e->A) || dmalloc(e, &sp.to_play, (size_t)e->Bp))) return -1;
  }
  sp.env_kind = kind;
  sp.ready = false;                // the environment state is (re)made by mz_selfplay_reset
  drop_graphs(e, false);
  return 0;
}

// Parity runs of a game environment: the Dirichlet draw (noise [dev][B][A] float64, scattered to the legal positions;
// mcts.py:59) and the uniform of select_action (uniform [dev][B] float64; config.py:77) of the NEXT moves come from the
// caller (numpy's stream in the reference's order) instead of the device RNG.  Either may be NULL (= device RNG); both
// NULL switches back.  The values are copied at the call.
int mz_selfplay_set_draws(mz_engine *e, const double *noise, const double *uniform, void *stream) {
  if (!e) return fail("mz_selfplay_set_draws: null engine");
  MZ_ENTER(e);
  if (e->sp.env_kind != 1) return fail("mz_selfplay_set_draws: only for the TicTacToe environment (mz_selfplay_set_env)");
  if (refuse_searched(e, "mz_selfplay_set_draws", "a mode that draws its noise on the device")) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (noise) HIPCHECK(hipMemcpyAsync(e->tv.noise, noise, (size_t)e->B * e->A * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (uniform) HIPCHECK(hipMemcpyAsync(e->draw_uniform, uniform, (size_t)e->B * sizeof(double), hipMemcpyDeviceToDevice, s));
  e->draws_noise = noise != nullptr;
  e->sp.draws_noise = noise != nullptr ? 1 : 0;
  e->sp.draw_uniform = uniform ? e->draw_uniform : nullptr;
  e->draws_set = noise || uniform;
  return 0;
}

// ---- how the moves are searched (mz_selfplay_mode.inc; DESIGN s7l).  Both switches: the facts, mz_sp_switch_ok's sentence, then the new mode and its parameter par
static int selfplay_set_mode(mz_engine *e, const char *fn, MzSpMode which, int on, int par) {
  if (!e) return fail("%s: null engine", fn);
  MZ_ENTER(e);
  const MzSpFacts facts = {e->sp_mode, e->sp.env_kind, e->gz.on != 0, e->tm.kind, e->draws_set, e->tv.sim_io != nullptr, e->ring.undrained()};
  char why[256];
  MzSpMode next = e->sp_mode;
  if (!mz_sp_switch_ok(facts, fn, which, on != 0, par, &next, why, sizeof why)) return fail("%s", why);
  HIPCHECK(hipDeviceSynchronize());      // (moves in flight were launched under the other plan)
  e->sp_mode = next;
  if (which == MZ_SP_GUMBEL) { e->sp_gumbel_value = on ? par : 0; e->gz.root_set = false; }
  else { e->sp_tm_fused = on != 0 && par != 0; e->tm.root_set = false; }
  drop_graphs(e, false);
  return 0;
}
int mz_selfplay_set_gumbel(mz_engine *e, int on, int value_kind) { return selfplay_set_mode(e, "mz_selfplay_set_gumbel", MZ_SP_GUMBEL, on, value_kind); }
int mz_selfplay_set_true_model(mz_engine *e, int on, int fused) { return selfplay_set_mode(e, "mz_selfplay_set_true_model", MZ_SP_TRUE_RULES, on, fused); }

// keep != 0: every move of the self-play loop also stores its Dirichlet draw in a per-move log (as many moves as the
// experience ring holds); mz_selfplay_read_noise fetches the draw of one move.  Test instrumentation: a move played in the
// middle of a whole-moves launch can then be replayed on the CPU by the parity tests with the draw the device itself used.
int mz_selfplay_noise_log(mz_engine *e, int keep) {
  if (!e) return fail("mz_selfplay_noise_log: null engine");
  MZ_ENTER(e);
  if (selfplay_alloc(e)) return -1;
  HIPCHECK(hipDeviceSynchronize());
  SelfplayState &sp = e->sp;
  if (keep && !e->noise_log) {
    if (dmalloc(e, &e->noise_log, (size_t)e->ring.capacity * e->B * e->A)) return -1;
  }
  sp.noise_log = keep ? e->noise_log : nullptr;
  drop_graphs(e, false);
  return 0;
}

// Test instrumentation of the fused search kernels (k_search_fused / k_search_h2; the stand-alone kernels take their
// network outputs through mz_expand_backup anyway).  buf [dev][keep_moves][B][num_simulations + 1][2 + A] float32, owned
// by the caller, must outlive the mode.  mode 1 (log): every simulation of every tree stores the three things its tree
// step consumed -- value, reward, the A policy logits -- in slot 1 + s of row (move % keep_moves, tree); the root of a
// self-play move stores (value, 0, logits) in slot 0; mz_search uses row 0.  mode 2 (inject): mz_search's simulations
// READ slot 1 + s instead of using their own network outputs (keep_moves = 1): recorded network outputs -- the goldens'
// -- reach the fused kernels' own tree code.  mode 0: off (buf ignored) -- the production state, a null pointer in the
// kernels' arguments.
int mz_sim_io(mz_engine *e, int mode, float *buf, int keep_moves) {
  if (!e) return fail("mz_sim_io: null engine");
  MZ_ENTER(e);
  if (mode < 0 || mode > 2) return fail("mz_sim_io: mode %d (0 off, 1 log, 2 inject)", mode);
  if (mode && (!buf || keep_moves < 1)) return fail("mz_sim_io: a buffer of keep_moves >= 1 moves is required");
  if (mode && refuse_searched(e, "mz_sim_io", "which the fused kernels do not run")) return -1;
  HIPCHECK(hipDeviceSynchronize());
  e->tv.sim_io = mode ? buf : nullptr;
  e->tv.sim_io_keep = mode == 2 ? -keep_moves : (mode == 1 ? keep_moves : 0);
  drop_graphs(e, true);
  return 0;
}

// out [host][B][A] float64: the Dirichlet draw of move `move` (0 = the first move after mz_selfplay_reset); the move
// must be one of the last ring_moves moves played.  Synchronous.
int mz_selfplay_read_noise(mz_engine *e, uint64_t move, double *out) {
  if (!e || !out) return fail("mz_selfplay_read_noise: null argument");
  MZ_ENTER(e);
  SelfplayState &sp = e->sp;
  if (!sp.noise_log) return fail("mz_selfplay_read_noise: the noise log is off (mz_selfplay_noise_log)");
  const RecordRing &ring = e->ring;
  if (move >= ring.produced || ring.produced - move > (unsigned long long)ring.capacity)
    return fail("mz_selfplay_read_noise: move %llu is not among the last %d of %llu moves played", (unsigned long long)move,
                ring.capacity, ring.produced);
  HIPCHECK(hipDeviceSynchronize());
  if (move >> 32) return fail("mz_selfplay_read_noise: the log is indexed by the low 32 bits of the move counter");
  HIPCHECK(hipMemcpy(out, sp.noise_log + (size_t)ring.slot(move) * e->B * e->A, (size_t)e->B * e->A * sizeof(double),
                     hipMemcpyDeviceToHost));
  return 0;
}

// ---- producing moves.  mz_selfplay_steps, mz_selfplay_steps_into, mz_selfplay_steps_timed and mz_selfplay_phase_profile all go
// produce_begin -> launch_moves under a ProduceGuard (mz_selfplay_ring.inc) -> produce_finish.

// The preconditions the producers share, in fn's name -- reset, weights, `own` (the caller's own refusal, or null), 1 <= moves <=
// most and, for moves into the device ring (into_ring), the ring's room -- then the stream is ordered behind the drains whose
// copies still read the slots about to be written.  < 0: failed; PRODUCE_RANGE / PRODUCE_FULL: refused in the caller's words
// (the sentences differ).
enum { PRODUCE_RANGE = 1, PRODUCE_FULL = 2 };
static int produce_begin(mz_engine *e, const char *fn, const char *own, int moves, int most, bool into_ring, hipStream_t s) {
  if (!e->sp.ready) return fail("%s: call mz_selfplay_reset first", fn);
  if (!e->weights_set) return fail("%s: weights not set (call mz_set_weights)", fn);
  if (own) return fail("%s: %s", fn, own);
  if (moves < 1 || moves > most) return PRODUCE_RANGE;
  if (!into_ring) return 0;
  if (!e->ring.fits(moves)) return PRODUCE_FULL;
  if (void *ev = e->ring.order_behind_drains(moves)) HIPCHECK(hipStreamWaitEvent(s, (hipEvent_t)ev, 0));
  return 0;
}

// k moves on stream s (or into a capture): ONE launch of the search kernel where the loop runs as whole moves (no root kernel),
// else k times a move's kernels.  o: each launch's search (the timed and profiled runs add events / counters)
static int launch_moves(mz_engine *e, int k, SearchOpts o, hipStream_t s) {
  if (search_plan(e).persist) {
    o.moves = k;
    return launch_search(e, o, true, s);
  }
  for (int i = 0; i < k; ++i)
    if (launch_move(e, o, s)) return -1;
  return 0;
}

static int produce_finish(mz_engine *e, int moves, ProduceGuard &guard) {
  guard.ok = true;
  e->ring.produced += (unsigned long long)moves;
  e->root_ready = true;
  e->sims_done = e->sims;
  e->selection_valid = false;
  return 0;
}

// direct: device mapping of the caller's pinned record buffer (mz_selfplay_steps_into), or null (the device ring)
static int selfplay_steps_impl(mz_engine *e, int moves, void *stream, float *direct) {
  SelfplayState &sp = e->sp;
  hipStream_t s = (hipStream_t)stream;
  const char *inject = e->tv.sim_io_keep < 0 ? "mz_sim_io's inject mode applies to mz_search only (switch it off or to log mode)" : nullptr;
  const int rc = produce_begin(e, "mz_selfplay_steps", inject, moves, INT_MAX, !direct, s);
  if (rc == PRODUCE_RANGE) return fail("mz_selfplay_steps: moves must be >= 1");
  if (rc == PRODUCE_FULL)
    return fail("mz_selfplay_steps: experience ring holds %d moves; drain before producing %d more", e->ring.capacity, moves);
  if (rc) return -1;
  ProduceGuard guard{sp.ready};
  // up to MZ_GRAPH_MOVES moves go out as ONE launch: whole moves inside the search kernel, else a hipGraph of the moves' kernels
  // (one graph per distinct count, built on first use): back-to-back nodes inside a graph start without a gap, between graph
  // launches the GPU idles ~9 us.  No graph for a direct launch (a captured one holds the device ring's address)
  const bool graph = !direct && e->use_graph && !e->draws_set && !search_plan(e).persist;
  for (int done = 0, k; done < moves; done += k) {
    k = moves - done < MZ_GRAPH_MOVES ? moves - done : MZ_GRAPH_MOVES;
    if (direct) {      // the kernels' "ring": RecordRing::direct_origin
      const size_t bytes = (size_t)e->B * sp.rec_floats * sizeof(float);
      const DirectOrigin at = RecordRing::direct_origin(e->ring.produced + (unsigned long long)done, k, bytes);
      // (an address computed in integers: the origin itself is never dereferenced, slot first_move % R is the buffer again)
      sp.ring = (float *)((uintptr_t)direct + (uintptr_t)((size_t)done * bytes) - (uintptr_t)at.back_bytes);
      sp.ring_moves = at.R;
    }
    if (graph && !e->move_graph[k]) {
      hipGraph_t g = nullptr;
      HIPCHECK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
      const int lrc = launch_moves(e, k, {e->sims}, e->cap_stream);
      hipError_t ce = hipStreamEndCapture(e->cap_stream, &g);
      if (lrc || ce != hipSuccess) return fail("mz_selfplay_steps: graph capture failed");
      HIPCHECK(hipGraphInstantiate(&e->move_graph[k], g, nullptr, nullptr, 0));
      hipGraphDestroy(g);
    }
    guard.attempted += k;
    if (graph) HIPCHECK(hipGraphLaunch(e->move_graph[k], s));
    else if (launch_moves(e, k, {e->sims}, s)) return -1;
  }
  return produce_finish(e, moves, guard);
}

int mz_selfplay_steps(mz_engine *e, int moves, void *stream) {
  if (!e) return fail("mz_selfplay_steps: null engine");
  MZ_ENTER(e);
  return selfplay_steps_impl(e, moves, stream, nullptr);
}

// The moves' records straight into the caller's pinned buffer: host_records [moves][B][rec_floats] is page-locked host
// memory (hipHostMalloc / torch pin_memory), the kernels store each record through its device mapping -- 1 KB per
// environment and move at LunarLander shapes, 0.6 GB/s of posted PCIe writes at the benched rate -- and the buffer is
// complete when work recorded on `stream` behind this call is.  No ring slot, no D2H copy, no copy stream: the copy
// engine's cross-stream dependency cost the host most of a core per rank (profiles/r05_host_threads.txt).  The device
// ring must be empty (moves produced by mz_selfplay_steps are drained first); these moves count as drained.
// The kernels stay untouched (k_search_fused's register allocation is tuned to the last scratch byte: a slot argument cost it
// 1 % of the headline): the host points their ring at the buffer (selfplay_steps_impl) and back.
int mz_selfplay_steps_into(mz_engine *e, int moves, float *host_records, void *stream) {
  if (!e || !host_records) return fail("mz_selfplay_steps_into: null argument");
  MZ_ENTER(e);
  if (!e->sp.ready) return fail("mz_selfplay_steps_into: call mz_selfplay_reset first");
  SelfplayState &sp = e->sp;
  if (e->ring.undrained())
    return fail("mz_selfplay_steps_into: %llu moves wait in the device ring; drain them first", e->ring.undrained());
  if (moves < 1) return fail("mz_selfplay_steps_into: moves must be >= 1");
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, host_records, 0) != hipSuccess || !dev) {
    (void)hipGetLastError();
    return fail("mz_selfplay_steps_into: host_records is not page-locked host memory");
  }
  if (sp.noise_log) return fail("mz_selfplay_steps_into: the Dirichlet log is indexed by ring slot (mz_selfplay_steps + mz_selfplay_drain)");
  float *ring = sp.ring;
  const int rc = selfplay_steps_impl(e, moves, stream, (float *)dev);
  sp.ring = ring; sp.ring_moves = e->ring.capacity;
  if (rc) return rc;
  e->ring.drained = e->ring.produced;
  return 0;
}

int mz_selfplay_moves_per_launch(const mz_engine *e) {
  if (!e) return -1;
  return search_plan(e).persist ? MZ_GRAPH_MOVES : 0;
}
int mz_selfplay_rec_floats(const mz_engine *e) { return e ? (e->sp.t ? e->sp.rec_floats : MZ_REC_FLOATS(e->O, e->A, 0)) : -1; }
int mz_selfplay_ring_moves(const mz_engine *e) { return (e && e->sp.t) ? e->ring.capacity : -1; }

int mz_selfplay_steps_timed(mz_engine *e, int k, float *ms_out, void *stream) {
  if (!e || !ms_out) return fail("mz_selfplay_steps_timed: null argument");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  char searched[256];      // (produce_begin puts the name in front)
  const char *own = e->sp_mode != MZ_SP_PUCT ? mz_sp_refusal(searched, sizeof searched, nullptr, e->sp_mode, "a search without a clocked dispatch", "the moves") :
                    fused_usable(e) ? nullptr : "fused kernel not in use";
  const int brc = produce_begin(e, "mz_selfplay_steps_timed", own, k, INT_MAX, true, s);
  if (brc > 0) return fail("mz_selfplay_steps_timed: %d moves do not fit the undrained ring", k);
  if (brc) return -1;
  // eager launches, back to back, no synchronisation in between, events around every search dispatch; where the loop runs as
  // whole moves one dispatch holds up to MZ_GRAPH_MOVES moves, every move of it reported as its share of the dispatch's duration
  const int per = search_plan(e).persist ? MZ_GRAPH_MOVES : 1, nl = (k + per - 1) / per;
  std::vector<hipEvent_t> ev(2 * (size_t)nl, nullptr);
  for (auto &x : ev) HIPCHECK(hipEventCreate(&x));
  ProduceGuard guard{e->sp.ready};
  int rc = 0;
  for (int i = 0; i < nl && !rc; ++i) {
    SearchOpts o = {e->sims};
    o.ev_start = ev[2 * i]; o.ev_stop = ev[2 * i + 1];
    ++guard.attempted;
    rc = launch_moves(e, k - i * per < per ? k - i * per : per, o, s);
  }
  hipError_t se = hipStreamSynchronize(s);
  if (!rc && se == hipSuccess)
    for (int i = 0; i < nl; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) { rc = fail("mz_selfplay_steps_timed: event timing failed"); break; }
      const int m0 = i * per, m1 = m0 + per < k ? m0 + per : k;
      for (int m = m0; m < m1; ++m) ms_out[m] = ms / (float)(m1 - m0);
    }
  for (auto &x : ev) hipEventDestroy(x);
  if (rc) return -1;
  if (se != hipSuccess) return fail("mz_selfplay_steps_timed: %s", hipGetErrorString(se));
  return produce_finish(e, k, guard);
}

int mz_selfplay_phase_profile(mz_engine *e, int moves, double *cycles_out, void *stream) {
  if (!e || !cycles_out) return fail("mz_selfplay_phase_profile: null argument");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  const char *own = search_plan(e).persist && !e->split_f16 ? nullptr :
      "the self-play loop of this configuration does not run as whole moves in one launch of the exact-f32 kernel";
  const int brc = produce_begin(e, "mz_selfplay_phase_profile", own, moves, MZ_GRAPH_MOVES, true, s);
  if (brc > 0)
    return fail("mz_selfplay_phase_profile: %d moves: at most %d per launch, and they must fit the undrained ring", moves, MZ_GRAPH_MOVES);
  if (brc) return -1;
  const size_t n = (size_t)(e->Bp / MZ_ROWS) * 4 * 8;
  unsigned long long *buf = nullptr;
  HIPCHECK(hipMalloc((void **)&buf, n * 8));
  ProduceGuard guard{e->sp.ready};
  SearchOpts o = {e->sims};
  o.prof = buf;
  ++guard.attempted;
  const int rc = launch_moves(e, moves, o, s);
  hipError_t se = hipStreamSynchronize(s);
  std::vector<unsigned long long> h(n);
  if (!rc && se == hipSuccess) se = hipMemcpy(h.data(), buf, n * 8, hipMemcpyDeviceToHost);
  hipFree(buf);
  if (rc) return -1;
  if (se != hipSuccess) return fail("mz_selfplay_phase_profile: %s", hipGetErrorString(se));
  // kernel order of the counters: 0 root's tree part, 1 ring + barrier, 2 simulations, 3 end of move, 4 root first stage,
  // 5 representation + LayerNorm, 6 prediction, 7 resident steps + tree set-up  ->  the order of a move
  static const int order[8] = {4, 5, 6, 0, 7, 1, 2, 3};
  for (int p = 0; p < 8; ++p) {
    double sum = 0;
    for (size_t i = 0; i < n / 8; ++i) sum += (double)h[i * 8 + order[p]];
    cycles_out[p] = sum / (double)(n / 8) / (double)moves;
  }
  return produce_finish(e, moves, guard);
}

int mz_selfplay_drain(mz_engine *e, float *out, int max_moves, int *n_moves, void *stream) {
  if (!e || !out || !n_moves) return fail("mz_selfplay_drain: null argument");
  MZ_ENTER(e);
  SelfplayState &sp = e->sp;
  if (!sp.ready) return fail("mz_selfplay_drain: call mz_selfplay_reset first");
  hipStream_t s = (hipStream_t)stream;
  const RingDrain d = e->ring.plan_drain(max_moves, stream);
  // drains on different streams: chained, so that the one event recorded below covers every copy issued so far
  if (d.chain) HIPCHECK(hipStreamWaitEvent(s, (hipEvent_t)d.chain, 0));
  const size_t per_move = (size_t)e->B * sp.rec_floats;
  for (int r = 0; r < d.runs; ++r) {
    HIPCHECK(hipMemcpyAsync(out, sp.ring + (size_t)d.run[r].slot * per_move, (size_t)d.run[r].moves * per_move * sizeof(float),
                            hipMemcpyDeviceToHost, s));
    out += (size_t)d.run[r].moves * per_move;
  }
  if (d.moves > 0) {
    // the event marks the point where the copies have read their slots: mz_selfplay_steps waits for it before it launches
    // moves into slots not yet covered (RecordRing::note_drain, order_behind_drains)
    hipEvent_t ev = (hipEvent_t)e->ring.take_token();
    if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(ev, s));
    e->ring.note_drain(d.moves, ev, stream);
  }
  *n_moves = d.moves;
  return 0;
}

// ---- the CartPole environment's state (include/mz_engine_debug.h)
int mz_cartpole_reset_state(const mz_engine *e, int env, int episode, double *out) {
  if (!e || !out) return fail("mz_cartpole_reset_state: null argument");
  mz_cartpole_reset_state(e->cfg.seed, (uint32_t)env, (uint32_t)episode, out);
  return 0;
}
int mz_selfplay_env_state(mz_engine *e, double *out) {
  if (!e || !out) return fail("mz_selfplay_env_state: null argument");
  MZ_ENTER(e);
  if (e->sp.env_kind != 2 || !e->sp.ready) return fail("mz_selfplay_env_state: the CartPole environment is not set up (mz_selfplay_set_env, mz_selfplay_reset)");
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(out, e->sp.cart, (size_t)e->B * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
int mz_selfplay_set_env_state(mz_engine *e, int env, const double *state) {
  if (!e || !state) return fail("mz_selfplay_set_env_state: null argument");
  MZ_ENTER(e);
  if (e->sp.env_kind != 2 || !e->sp.ready) return fail("mz_selfplay_set_env_state: the CartPole environment is not set up (mz_selfplay_set_env, mz_selfplay_reset)");
  if (env < 0 || env >= e->B) return fail("mz_selfplay_set_env_state: environment %d outside [0, %d)", env, e->B);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(e->sp.cart + (size_t)env * 4, state, 4 * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// ---- the Connect Four environment's state (include/mz_engine_debug.h)
int mz_selfplay_board_state(mz_engine *e, int8_t *out) {
  if (!e || !out) return fail("mz_selfplay_board_state: null argument");
  MZ_ENTER(e);
  if (e->sp.env_kind != 3 || !e->sp.ready) return fail("mz_selfplay_board_state: the Connect Four environment is not set up (mz_selfplay_set_env, mz_selfplay_reset)");
  HIPCHECK(hipDeviceSynchronize());
  const size_t B = (size_t)e->B;
  std::vector<int8_t> bd(B * 42), turn(B);
  std::vector<int32_t> t(B);
  HIPCHECK(hipMemcpy(bd.data(), e->sp.board, B * 42, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(turn.data(), e->sp.turn, B, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(t.data(), e->sp.t, B * 4, hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; ++b) {
    for (int k = 0; k < 42; ++k) out[b * 44 + k] = bd[b * 42 + k];
    out[b * 44 + 42] = turn[b];
    out[b * 44 + 43] = (int8_t)t[b];
  }
  return 0;
}
int mz_selfplay_set_board_state(mz_engine *e, int env, const int8_t *cells42, int turn) {
  if (!e || !cells42) return fail("mz_selfplay_set_board_state: null argument");
  MZ_ENTER(e);
  if (e->sp.env_kind != 3 || !e->sp.ready) return fail("mz_selfplay_set_board_state: the Connect Four environment is not set up (mz_selfplay_set_env, mz_selfplay_reset)");
  if (env < 0 || env >= e->B) return fail("mz_selfplay_set_board_state: environment %d outside [0, %d)", env, e->B);
  if (turn != 1 && turn != -1) return fail("mz_selfplay_set_board_state: turn %d (+1 or -1)", turn);
  int32_t stones = 0;
  bool open = false;
  for (int k = 0; k < 42; ++k) {
    if (cells42[k] < -1 || cells42[k] > 1) return fail("mz_selfplay_set_board_state: cell %d holds %d (0, +1 or -1)", k, (int)cells42[k]);
    stones += cells42[k] != 0;
    open = open || (k >= 35 && cells42[k] == 0);
  }
  if (!open) return fail("mz_selfplay_set_board_state: every column is full, the position has no move");
  const int8_t tn = (int8_t)turn;
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(e->sp.board + (size_t)env * 42, cells42, 42, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(e->sp.turn + env, &tn, 1, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(e->sp.t + env, &stones, 4, hipMemcpyHostToDevice));
  return 0;
}

int mz_synth_obs(const mz_engine *e, int env, int episode, int t, float *out_obs, float *out_reward) {
  if (!e) return fail("mz_synth_obs: null engine");
  if (out_obs)
    for (int k = 0; k < e->O; ++k)
      out_obs[k] = e->sp.obs_u8 ? mz_synth_obs_u8(e->cfg.seed, (uint32_t)env, (uint32_t)episode, (uint32_t)t, (uint32_t)k)
                                : mz_synth_obs_elem(e->cfg.seed, (uint32_t)env, (uint32_t)episode, (uint32_t)t, (uint32_t)k);
  if (out_reward) *out_reward = mz_synth_reward(e->cfg.seed, (uint32_t)env, (uint32_t)episode, (uint32_t)t);
  return 0;
}
