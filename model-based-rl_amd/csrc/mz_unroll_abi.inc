// mz_unroll_abi.inc -- C ABI of the unroll diagnostic (included inside extern "C" of mz_engine.hip after mz_solve_abi.inc,
// whose position checks it shares; bodies, kernels and state: mz_unroll.hip.h).

// what the device entry and the lines hook check alike: the kind, K, n and the start positions (mz_solve's checks)
static int unroll_check(const char *fn, int kind, int A, const int8_t *boards, const int8_t *turn, const int32_t *step,
                        const int32_t *actions, int n, int K) {
  if (kind != 1 && kind != 3) return fail("%s: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", fn, kind);
  if (A != mz_game_info(kind).actions) return fail("%s: %s has %d actions, got %d", fn, mz_game_info(kind).name, mz_game_info(kind).actions, A);
  if (K < 0 || K > MZ_UR_MAXK) return fail("%s: K must be in 0 .. %d, got %d", fn, MZ_UR_MAXK, K);
  if (n < 1) return fail("%s: n must be >= 1, got %d", fn, n);
  if (!boards || !turn || !step || (K > 0 && !actions)) return fail("%s: null argument", fn);
  return solve_check(fn, kind, A, boards, turn, step, n, 1);
}

static int unroll_ready(mz_engine *e) {
  UnrollState &u = e->ur;
  if (u.raw_meta) return 0;      // (the last one allocated)
  u = UnrollState{};
  const size_t nb = (size_t)e->B, A = (size_t)e->A, O = (size_t)e->O, D = MZ_UR_MAXK + 1;
  if (dmalloc(e, &u.start, nb * 42) || dmalloc(e, &u.turn, nb) || dmalloc(e, &u.step, nb) || dmalloc(e, &u.actions, nb * MZ_UR_MAXK) ||
      dmalloc(e, &u.truth, nb * D * A) || dmalloc(e, &u.boards, nb * D * 42) || dmalloc(e, &u.obs, D * nb * O) ||
      dmalloc(e, &u.legal, D * nb) || dmalloc(e, &u.terminal, D * nb) || dmalloc(e, &u.rtrue, D * nb) || dmalloc(e, &u.act, D * nb) ||
      dmalloc(e, &u.depth, nb) || dmalloc(e, &u.flags, nb) || dmalloc(e, &u.hid_u, D * nb * MZ_H) || dmalloc(e, &u.rew_u, D * nb) ||
      dmalloc(e, &u.val_u, D * nb) || dmalloc(e, &u.val_f, D * nb) || dmalloc(e, &u.lg_u, D * nb * A) || dmalloc(e, &u.lg_f, D * nb * A) ||
      dmalloc(e, &u.terms, nb * D * MZ_UR_NT) || dmalloc(e, &u.raw, nb * D * (O + MZ_H + 2 * A + 4))) {
    u = UnrollState{};
    return -1;
  }
  if (dmalloc(e, &u.raw_meta, nb * D * 2)) return -1;
  return 0;
}

int mz_unroll_raw_floats(const mz_engine *e) { return e ? e->O + MZ_H + 2 * e->A + 4 : -1; }
int mz_unroll_num_terms(void) { return MZ_UR_NT; }

int mz_unroll(mz_engine *e, int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, const int32_t *actions, int n,
              int K, const int8_t *truth, double *terms_out, int32_t *depth_out, int32_t *flags_out, float *raw_out,
              int32_t *raw_meta_out, void *stream) {
  if (!e || !terms_out || !depth_out || !flags_out) return fail("mz_unroll: null argument");
  MZ_ENTER(e);
  if (kind != 1 && kind != 3) return fail("mz_unroll: kind must be 1 (TicTacToe) or 3 (Connect Four), got %d", kind);
  if (game_shape(e, "mz_unroll", kind)) return -1;
  if (unroll_check("mz_unroll", kind, e->A, boards, turn, step, actions, n, K)) return -1;
  if (!e->weights_set) return fail("mz_unroll: weights not set (call mz_set_weights)");
  if ((raw_out == nullptr) != (raw_meta_out == nullptr)) return fail("mz_unroll: raw_out and raw_meta_out go together");
  if (unroll_ready(e)) return -1;
  hipStream_t s = (hipStream_t)stream;
  UnrollState &u = e->ur;
  const int B = e->B, A = e->A, O = e->O, K1 = K + 1;
  const size_t W = (size_t)O + MZ_H + 2 * (size_t)A + 4;
  for (int lo = 0; lo < n; lo += B) {      // chunks of num_envs rows through the one staging, in stream order
    const int m = n - lo < B ? n - lo : B;
    HIPCHECK(hipMemcpyAsync(u.start, boards + (size_t)lo * 42, (size_t)m * 42, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(u.turn, turn + lo, (size_t)m, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(u.step, step + lo, (size_t)m * 4, hipMemcpyHostToDevice, s));
    if (K > 0) HIPCHECK(hipMemcpyAsync(u.actions, actions + (size_t)lo * K, (size_t)m * K * 4, hipMemcpyHostToDevice, s));
    if (truth) HIPCHECK(hipMemcpyAsync(u.truth, truth + (size_t)lo * K1 * A, (size_t)m * K1 * A, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_unroll_lines, dim3((B + 63) / 64), dim3(64), 0, s, kind, O, A, K, m, B, u);
    if (hipGetLastError() != hipSuccess) return fail("mz_unroll: k_unroll_lines did not launch");
    // h_0, v_0, logits_0 of p_0; then the unrolled outputs along the actions; then the fresh outputs of every real p_k
    if (mz_initial_inference(e, u.obs, stream)) return -1;
    hipLaunchKernelGGL(k_unroll_take_root, dim3(B), dim3(64), 0, s, e->tv, 0, B, A, u);
    for (int k = 1; k <= K; ++k) {
      const size_t at = (size_t)k * B, from = (size_t)(k - 1) * B;
      if (mz_recurrent_inference(e, u.hid_u + from * MZ_H, u.act + from, m, u.hid_u + at * MZ_H, u.rew_u + at, u.val_u + at,
                                 u.lg_u + at * A, stream)) return -1;
      hipLaunchKernelGGL(k_unroll_mask, dim3(B), dim3(64), 0, s, k, B, A, u);
    }
    for (int k = 1; k <= K; ++k) {
      if (mz_initial_inference(e, u.obs + (size_t)k * B * O, stream)) return -1;
      hipLaunchKernelGGL(k_unroll_take_root, dim3(B), dim3(64), 0, s, e->tv, k, B, A, u);
    }
    hipLaunchKernelGGL(k_unroll_terms, dim3((m * K1 + 15) / 16), dim3(256), 0, s, A, K1, m, B, truth ? 1 : 0, u);
    if (raw_out) hipLaunchKernelGGL(k_unroll_export, dim3(m * K1), dim3(64), 0, s, O, A, K1, m, B, u);
    if (hipGetLastError() != hipSuccess) return fail("mz_unroll: a kernel did not launch");
    HIPCHECK(hipMemcpyAsync(terms_out + (size_t)lo * K1 * MZ_UR_NT, u.terms, (size_t)m * K1 * MZ_UR_NT * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(depth_out + lo, u.depth, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(flags_out + lo, u.flags, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    if (raw_out) {
      HIPCHECK(hipMemcpyAsync(raw_out + (size_t)lo * K1 * W, u.raw, (size_t)m * K1 * W * 4, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipMemcpyAsync(raw_meta_out + (size_t)lo * K1 * 2, u.raw_meta, (size_t)m * K1 * 2 * 4, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHECK(hipStreamSynchronize(s));
  return 0;
}

int mz_unroll_lines_host(int kind, const int8_t *boards, const int8_t *turn, const int32_t *step, const int32_t *actions, int n, int K,
                         float *obs_out, uint32_t *legal_out, uint8_t *terminal_out, float *reward_true_out, int32_t *depth_out,
                         int32_t *flags_out) {
  const MzGameInfo g = mz_game_info(kind);
  if (unroll_check("mz_unroll_lines_host", kind, g.actions, boards, turn, step, actions, n, K)) return -1;
  if (!obs_out || !legal_out || !terminal_out || !reward_true_out || !depth_out || !flags_out)
    return fail("mz_unroll_lines_host: null argument");
  const int K1 = K + 1;
  int8_t bd[(MZ_UR_MAXK + 1) * 42];
  int32_t act[MZ_UR_MAXK + 1];
  for (int i = 0; i < n; ++i) {
    const size_t it = (size_t)i * K1;
    ur_line(kind, g.obs_dim, g.actions, K, boards + (size_t)i * 42, (int)turn[i], step[i], actions + (size_t)i * K, bd, 1,
            obs_out + it * g.obs_dim, legal_out + it, terminal_out + it, reward_true_out + it, act, depth_out + i, flags_out + i);
  }
  return 0;
}

int mz_unroll_terms_host(int A, int items, const float *logits_u, const float *logits_f, const uint32_t *legal, const uint8_t *terminal,
                         const uint8_t *live, const int32_t *k, const float *reward_true, const float *reward_u, const float *value_u,
                         const float *value_f, const int8_t *truth, double *terms_out) {
  if (A < 1 || A > 16) return fail("mz_unroll_terms_host: A must be in 1 .. 16, got %d", A);
  if (items < 0) return fail("mz_unroll_terms_host: items must be >= 0, got %d", items);
  if (items && (!logits_u || !logits_f || !legal || !terminal || !live || !k || !reward_true || !reward_u || !value_u || !value_f ||
                !terms_out))
    return fail("mz_unroll_terms_host: null argument");
  double eu[16], ef[16];
  for (int i = 0; i < items; ++i) {
    const float *lu = logits_u + (size_t)i * A, *lf = logits_f + (size_t)i * A;
    for (int a = 0; a < A; ++a) { eu[a] = std::exp(ur_exp_arg(lu, A, a)); ef[a] = std::exp(ur_exp_arg(lf, A, a)); }
    ur_terms(A, lu, lf, eu, ef, legal[i], terminal[i] != 0, live[i] != 0, k[i], reward_true[i], reward_u[i], value_u[i], value_f[i],
             truth ? truth + (size_t)i * A : nullptr, terms_out + (size_t)i * MZ_UR_NT);
  }
  return 0;
}
