// mz_playout_abi.inc -- C ABI of the playout-search opponent (included inside extern "C" of mz_engine.hip before
// mz_eval_abi.inc, whose moves launch the planner; bodies, kernel and state: mz_playout.hip.h).

// the budget and the positions, checked alike for the device entry and the host hook
static int playout_check(const char *fn, int kind, int A, int playouts, const int8_t *boards, const int8_t *turn,
                         const int32_t *step, int n_games) {
  if (kind != 1 && kind != 3) return fail("%s: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", fn, kind);
  const MzGameInfo g = mz_game_info(kind);
  if (A != g.actions) return fail("%s: %s has %d actions, got %d", fn, g.name, g.actions, A);
  if (playouts < MZ_PO_MIN_PLAYOUTS || playouts > MZ_PO_MAX_PLAYOUTS || playouts % MZ_PO_LANES)
    return fail("%s: playouts must be a multiple of 64 in 64 .. 65536, got %d", fn, playouts);
  if (n_games < 0) return fail("%s: n_games must be >= 0, got %d", fn, n_games);
  if (n_games && (!boards || !turn || !step)) return fail("%s: null position array", fn);
  for (int i = 0; i < n_games; ++i) {
    const int8_t *bd = boards + (size_t)i * 42;
    int stones = 0;
    for (int k = 0; k < 42; ++k) {
      if (bd[k] < -1 || bd[k] > 1 || (k >= g.cells && bd[k] != 0))
        return fail("%s: position %d is not a board of the game (cell %d holds %d)", fn, i, k, (int)bd[k]);
      stones += bd[k] != 0 ? 1 : 0;
    }
    if (turn[i] != 1 && turn[i] != -1) return fail("%s: position %d has turn %d, not +1 or -1", fn, i, (int)turn[i]);
    if (step[i] != stones) return fail("%s: position %d has step %d but %d stones", fn, i, step[i], stones);
    if (po_legal(kind, bd) == 0) return fail("%s: position %d has no legal action", fn, i);
  }
  return 0;
}

// LN[v] = log(64 v): computed here, on the host, for the device kernel and the host hook alike
static void playout_ln_table(std::vector<double> &ln) {
  ln.assign((size_t)MZ_PO_MAX_ITERS + 1, 0.0);
  for (int v = 1; v <= MZ_PO_MAX_ITERS; ++v) ln[v] = std::log(64.0 * (double)v);
}

static int playout_ready(mz_engine *e, hipStream_t s) {
  PlayoutState &ps = e->po;
  if (ps.wins) return 0;      // (the last one allocated)
  ps = PlayoutState{};
  const size_t nb = (size_t)e->B, A = (size_t)e->A;
  if (dmalloc(e, &ps.ln, (size_t)MZ_PO_MAX_ITERS + 1) || dmalloc(e, &ps.boards, nb * 42) || dmalloc(e, &ps.turn, nb) ||
      dmalloc(e, &ps.step, nb) || dmalloc(e, &ps.action, nb) || dmalloc(e, &ps.visits, nb * A)) {
    ps = PlayoutState{};
    return -1;
  }
  std::vector<double> ln;
  playout_ln_table(ln);
  HIPCHECK(hipMemcpyAsync(ps.ln, ln.data(), ln.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));      // (ln is this call's)
  if (dmalloc(e, &ps.wins, nb * A)) return -1;
  return 0;
}

// enqueue the planner over n games (device arrays); terminal (or null) and only_mover (or 0) say which games are planned
static int playout_launch(mz_engine *e, const char *fn, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step,
                          const uint8_t *terminal, int only_mover, int n, int playouts, uint64_t move, int32_t *action,
                          int32_t *visits, int32_t *wins, hipStream_t s) {
  const int iters = playouts / MZ_PO_LANES, A = mz_game_info(kind).actions;
  const size_t per_wave = po_wave_bytes(iters + 1, A);
  if (per_wave > (size_t)MZ_LDS_BYTES) return fail("%s: a tree of %d nodes does not fit the LDS", fn, iters + 1);
  const int waves = 4 * per_wave <= 65536 ? 4 : (2 * per_wave <= 65536 ? 2 : 1);      // per block; no more LDS than one wave needs above 64 KiB
  const size_t lds = (size_t)waves * per_wave;
  const void *kfn = (const void *)k_playout_plan;
  if (lds > 65536 && std::find(e->lds_attr_done.begin(), e->lds_attr_done.end(), kfn) == e->lds_attr_done.end()) {
    HIPCHECK(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MZ_LDS_BYTES));
    e->lds_attr_done.push_back(kfn);
  }
  hipLaunchKernelGGL(k_playout_plan, dim3((n + waves - 1) / waves), dim3(64 * waves), lds, s, kind, A, boards, turn, step,
                     terminal, only_mover, n, iters, (const double *)e->po.ln, (uint64_t)e->cfg.seed, e->cfg.env_id_offset,
                     (uint32_t)move, (int)per_wave, action, visits, wins);
  if (hipGetLastError() != hipSuccess) return fail("%s: k_playout_plan did not launch", fn);
  return 0;
}

int mz_playout_plan(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n_games,
                    int playouts, uint64_t move, int32_t *action_out, int32_t *visits_out, int32_t *wins_out, void *stream) {
  if (!e) return fail("mz_playout_plan: null engine");
  MZ_ENTER(e);
  if (kind != 1 && kind != 3) return fail("mz_playout_plan: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", kind);
  if (game_shape(e, "mz_playout_plan", kind)) return -1;
  if (n_games > e->B) return fail("mz_playout_plan: n_games %d exceeds the engine's num_envs %d", n_games, e->B);
  if (playout_check("mz_playout_plan", kind, e->A, playouts, boards, turn, step, n_games)) return -1;
  if (n_games == 0) return 0;
  if (!action_out) return fail("mz_playout_plan: null action_out");
  hipStream_t s = (hipStream_t)stream;
  if (playout_ready(e, s)) return -1;
  PlayoutState &ps = e->po;
  const size_t n = (size_t)n_games, A = (size_t)e->A;
  HIPCHECK(hipMemcpyAsync(ps.boards, boards, n * 42, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(ps.turn, turn, n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(ps.step, step, n * 4, hipMemcpyHostToDevice, s));
  if (playout_launch(e, "mz_playout_plan", kind, ps.boards, ps.turn, ps.step, nullptr, 0, n_games, playouts, move, ps.action,
                     ps.visits, ps.wins, s)) return -1;
  HIPCHECK(hipMemcpyAsync(action_out, ps.action, n * 4, hipMemcpyDeviceToHost, s));
  if (visits_out) HIPCHECK(hipMemcpyAsync(visits_out, ps.visits, n * A * 4, hipMemcpyDeviceToHost, s));
  if (wins_out) HIPCHECK(hipMemcpyAsync(wins_out, ps.wins, n * A * 4, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

int mz_playout_plan_host(int kind, int A, uint64_t seed, int env_id_offset, const int8_t *boards, const int8_t *turn,
                         const int32_t *step, int n_games, int playouts, uint64_t move, int32_t *action_out,
                         int32_t *visits_out, int32_t *wins_out) {
  if (playout_check("mz_playout_plan_host", kind, A, playouts, boards, turn, step, n_games)) return -1;
  if (n_games == 0) return 0;
  if (!action_out) return fail("mz_playout_plan_host: null action_out");
  const int iters = playouts / MZ_PO_LANES;
  std::vector<double> ln;
  playout_ln_table(ln);
  std::vector<uint64_t> mem((po_wave_bytes(iters + 1, A) + 7) / 8);
  PoTree t;
  int8_t *lane_boards, *root;
  po_carve((unsigned char *)mem.data(), iters + 1, A, &t, &lane_boards, &root);
  for (int i = 0; i < n_games; ++i) {
    memcpy(root, boards + (size_t)i * 42, 42);
    po_plan(kind, t, lane_boards, root, (int)turn[i], step[i], iters, ln.data(), seed, (uint32_t)(env_id_offset + i),
            (uint32_t)move, 0, action_out + i, visits_out ? visits_out + (size_t)i * A : nullptr,
            wins_out ? wins_out + (size_t)i * A : nullptr);
  }
  return 0;
}

int mz_eval_env_set_opponent(mz_engine *e, int playouts, void *stream) {
  if (!e) return fail("mz_eval_env_set_opponent: null engine");
  MZ_ENTER(e);
  EvalState &es = e->ev;
  if (!es.ready) return fail("mz_eval_env_set_opponent: call mz_eval_env_reset first");
  if (e->ev_moves) return fail("mz_eval_env_set_opponent: the games have started; the opponent is set before the first move");
  if (playouts == 0) { es.opp_playouts = 0; es.opp_action = nullptr; return 0; }
  if (es.kind != 1 && es.kind != 3)
    return fail("mz_eval_env_set_opponent: the playout opponent plays TicTacToe (kind 1) or Connect Four (kind 3), the games are of kind %d", es.kind);
  if (playouts < MZ_PO_MIN_PLAYOUTS || playouts > MZ_PO_MAX_PLAYOUTS || playouts % MZ_PO_LANES)
    return fail("mz_eval_env_set_opponent: playouts must be 0 or a multiple of 64 in 64 .. 65536, got %d", playouts);
  if (!es.random_opp) return fail("mz_eval_env_set_opponent: the games were reset without an opponent's seat (random_opp 0)");
  if (playout_ready(e, (hipStream_t)stream)) return -1;
  if (!es.opp_action_buf && dmalloc(e, &es.opp_action_buf, (size_t)e->B)) return -1;
  es.opp_playouts = playouts;
  es.opp_action = es.opp_action_buf;
  return 0;
}
