// mz_solve_abi.inc -- C ABI of the exact game solver (included inside extern "C" of mz_engine.hip after
// mz_playout_abi.inc, whose position checks it shares; bodies, kernels and state: mz_solve.hip.h).

// the budget and the positions, checked alike for the device entry and the host hook: playout_check's checks, and no side
// has a line yet
static int solve_check(const char *fn, int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step, int n,
                       int max_nodes) {
  if (playout_check(fn, kind, A, MZ_PO_MIN_PLAYOUTS, boards, turn, step, n)) return -1;
  if (max_nodes < 1 || max_nodes > MZ_SV_MAX_NODES) return fail("%s: max_nodes must be in 1 .. %d, got %d", fn, MZ_SV_MAX_NODES, max_nodes);
  for (int i = 0; i < n; ++i) {
    uint64_t cur, mask;
    bool over;
    if (kind == 3) { sv_pack<3>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask); over = sv_finished<3>(cur, mask); }
    else { sv_pack<1>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask); over = sv_finished<1>(cur, mask); }
    if (over) return fail("%s: position %d already holds a finished line, so the game was over before it", fn, i);
  }
  return 0;
}

static int solve_ready(mz_engine *e) {
  SolveState &ss = e->sv;
  if (ss.nodes) return 0;      // (the last one allocated)
  ss = SolveState{};
  const size_t nb = (size_t)e->B, A = (size_t)e->A;
  if (dmalloc(e, &ss.boards, nb * 42) || dmalloc(e, &ss.turn, nb) || dmalloc(e, &ss.step, nb) || dmalloc(e, &ss.bits, 2 * nb) ||
      dmalloc(e, &ss.values, nb * A)) {
    ss = SolveState{};
    return -1;
  }
  if (dmalloc(e, &ss.nodes, nb * A)) return -1;
  return 0;
}

// the units of one launch share out as 64 * k per wave, k the smallest that keeps the launch within 1024 waves (one unit a
// lane while the device has lanes to spare, several a lane, pulled as the lanes come free, beyond that)
static int solve_per_wave(int n_units) {
  int k = (n_units + 64 * 1024 - 1) / (64 * 1024);
  if (k < 1) k = 1;
  if (k > MZ_SV_MAX_UNITS_PER_LANE) k = MZ_SV_MAX_UNITS_PER_LANE;
  return 64 * k;
}

// the table search's tables and counters, sized for the waves one chunk of num_envs positions can launch
static int solve_tt_ready(mz_engine *e) {
  SolveTableState &st = e->svt;
  if (st.gens) return 0;      // (the last one allocated)
  st = SolveTableState{};
  int waves = (e->B * e->A + 63) / 64;
  if (waves > MZ_SVT_MAX_WAVES) waves = MZ_SVT_MAX_WAVES;
  if (dmalloc(e, &st.tables, ((size_t)waves * 64) << MZ_SVT_BITS)) { st = SolveTableState{}; return -1; }
  st.waves = waves;
  if (dmalloc(e, &st.gens, (size_t)waves * 64)) return -1;
  return 0;
}

// mz_solve and mz_solve_tt: the checks, the chunks of num_envs positions through the one staging in stream order, one
// synchronisation at the end.  table: k_solve_tt on the engine's SolveTableState, else k_solve.
static int solve_run(const char *fn, bool table, mz_engine *e, int kind, const int8_t *boards, const int8_t *turn,
                     const int32_t *step, int n, int max_nodes, int8_t *values_out, uint32_t *nodes_out, void *stream) {
  if (!e) return fail("%s: null engine", fn);
  MZ_ENTER(e);
  if (kind != 1 && kind != 3) return fail("%s: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", fn, kind);
  if (game_shape(e, fn, kind)) return -1;
  if (solve_check(fn, kind, e->A, boards, turn, step, n, max_nodes)) return -1;
  if (n == 0) return 0;
  if (!values_out) return fail("%s: null values_out", fn);
  hipStream_t s = (hipStream_t)stream;
  if (solve_ready(e) || (table && solve_tt_ready(e))) return -1;
  SolveState &ss = e->sv;
  const SolveTableState &st = e->svt;
  const size_t A = (size_t)e->A;
  for (int lo = 0; lo < n; lo += e->B) {      // chunks of num_envs positions through the one staging, in stream order
    const int m = n - lo < e->B ? n - lo : e->B;
    const int units = m * e->A;
    int per_wave = solve_per_wave(units);
    if (table && (units + per_wave - 1) / per_wave > st.waves)      // (more than 2^20 units a chunk: the tables bound the waves)
      per_wave = 64 * ((units + 64 * st.waves - 1) / (64 * st.waves));
    HIPCHECK(hipMemcpyAsync(ss.boards, boards + (size_t)lo * 42, (size_t)m * 42, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ss.turn, turn + lo, (size_t)m, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ss.step, step + lo, (size_t)m * 4, hipMemcpyHostToDevice, s));
    const dim3 pg((m + 255) / 256), g((units + per_wave - 1) / per_wave);
    if (kind == 3) {
      hipLaunchKernelGGL(k_solve_pack<3>, pg, dim3(256), 0, s, (const int8_t *)ss.boards, (const int8_t *)ss.turn, m, ss.bits);
      if (table)
        hipLaunchKernelGGL(k_solve_tt<3>, g, dim3(64), 0, s, e->A, (const uint64_t *)ss.bits, (const int32_t *)ss.step, units, per_wave,
                           (uint32_t)max_nodes, st.tables, st.gens, ss.values, ss.nodes);
      else
        hipLaunchKernelGGL(k_solve<3>, g, dim3(64), 0, s, e->A, (const uint64_t *)ss.bits, (const int32_t *)ss.step, units, per_wave,
                           (uint32_t)max_nodes, ss.values, ss.nodes);
    } else {
      hipLaunchKernelGGL(k_solve_pack<1>, pg, dim3(256), 0, s, (const int8_t *)ss.boards, (const int8_t *)ss.turn, m, ss.bits);
      if (table)
        hipLaunchKernelGGL(k_solve_tt<1>, g, dim3(64), 0, s, e->A, (const uint64_t *)ss.bits, (const int32_t *)ss.step, units, per_wave,
                           (uint32_t)max_nodes, st.tables, st.gens, ss.values, ss.nodes);
      else
        hipLaunchKernelGGL(k_solve<1>, g, dim3(64), 0, s, e->A, (const uint64_t *)ss.bits, (const int32_t *)ss.step, units, per_wave,
                           (uint32_t)max_nodes, ss.values, ss.nodes);
    }
    if (hipGetLastError() != hipSuccess) return fail("%s: %s did not launch", fn, table ? "k_solve_tt" : "k_solve");
    HIPCHECK(hipMemcpyAsync(values_out + (size_t)lo * A, ss.values, (size_t)m * A, hipMemcpyDeviceToHost, s));
    if (nodes_out) HIPCHECK(hipMemcpyAsync(nodes_out + (size_t)lo * A, ss.nodes, (size_t)m * A * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

int mz_solve(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
             int8_t *values_out, uint32_t *nodes_out, void *stream) {
  return solve_run("mz_solve", false, e, kind, boards, turn, step, n, max_nodes, values_out, nodes_out, stream);
}

int mz_solve_tt(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                int8_t *values_out, uint32_t *nodes_out, void *stream) {
  return solve_run("mz_solve_tt", true, e, kind, boards, turn, step, n, max_nodes, values_out, nodes_out, stream);
}

int mz_solve_tt_set_generation(mz_engine *e, int generation) {
  if (!e) return fail("mz_solve_tt_set_generation: null engine");
  MZ_ENTER(e);
  if (generation < 0 || generation >= MZ_SVT_GEN_WRAP)
    return fail("mz_solve_tt_set_generation: generation must be in 0 .. %d, got %d", MZ_SVT_GEN_WRAP - 1, generation);
  if (solve_tt_ready(e)) return -1;
  const std::vector<uint32_t> g((size_t)e->svt.waves * 64, (uint32_t)generation);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(e->svt.gens, g.data(), g.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

int mz_solve_host(int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                  int8_t *values_out, uint32_t *nodes_out) {
  if (solve_check("mz_solve_host", kind, A, boards, turn, step, n, max_nodes)) return -1;
  if (n == 0) return 0;
  if (!values_out) return fail("mz_solve_host: null values_out");
  uint8_t stack[MZ_SV_STACK_STRIDE];
  for (int i = 0; i < n; ++i) {
    uint64_t cur, mask;
    if (kind == 3) sv_pack<3>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask);
    else sv_pack<1>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask);
    for (int a = 0; a < A; ++a) {
      uint32_t spent;
      const int v = kind == 3 ? sv_unit<3>(cur, mask, step[i], a, (uint32_t)max_nodes, stack, &spent)
                              : sv_unit<1>(cur, mask, step[i], a, (uint32_t)max_nodes, stack, &spent);
      values_out[(size_t)i * A + a] = (int8_t)v;
      if (nodes_out) nodes_out[(size_t)i * A + a] = spent;
    }
  }
  return 0;
}

int mz_solve_tt_host(int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step, int n, int max_nodes,
                     int8_t *values_out, uint32_t *nodes_out) {
  if (solve_check("mz_solve_tt_host", kind, A, boards, turn, step, n, max_nodes)) return -1;
  if (n == 0) return 0;
  if (!values_out) return fail("mz_solve_tt_host: null values_out");
  std::vector<uint64_t> tab((size_t)1 << MZ_SVT_BITS, 0);      // one lane's table and counter, as a lane of k_solve_tt has them
  uint32_t gen = 0;
  SvRules<3>::level_t stack3[SvRules<3>::LEVELS];
  SvRules<1>::level_t stack1[SvRules<1>::LEVELS];
  for (int i = 0; i < n; ++i) {
    uint64_t cur, mask;
    if (kind == 3) sv_pack<3>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask);
    else sv_pack<1>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask);
    for (int a = 0; a < A; ++a) {
      uint32_t spent;
      gen = svt_next_gen(tab.data(), gen);
      const int v = kind == 3 ? sv_unit_tt<3>(cur, mask, step[i], a, (uint32_t)max_nodes, stack3, tab.data(), gen, &spent)
                              : sv_unit_tt<1>(cur, mask, step[i], a, (uint32_t)max_nodes, stack1, tab.data(), gen, &spent);
      values_out[(size_t)i * A + a] = (int8_t)v;
      if (nodes_out) nodes_out[(size_t)i * A + a] = spent;
    }
  }
  return 0;
}
