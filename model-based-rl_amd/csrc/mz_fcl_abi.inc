// mz_fcl_abi.inc -- host side of the FCNetwork learner step (mz_fcl.hip.h; include/mz_engine.h "learner step").
// Included inside mz_engine.hip's extern "C" block.

extern "C++" {
// staging slots of mz_fcl_update / mz_fcl_run: an update's batch stays in its slot until the update has run.  With n slots the host
// runs n - 1 updates ahead of the GPU: launch and completion latencies hide behind whole updates, and the Python the learner's loop
// runs between two mz_fcl_run calls (logging, send_weights: ~0.6 ms per 100 updates) hides behind the updates still queued.
// FCL_SLOTS: the most a handle can have; mz_fcl.nslots: what it uses (6; MZ_FCL_SLOTS=2..8 for A/B runs)
#define FCL_SLOTS 8
struct mz_fcl {
  int device = 0;
  int bs = 0, K = 0, O = 0, A = 0, nwg = 0, njobs = 0, njobs_heads = 0, nblk = 0, nsteps = 0;
  // weight-gradient jobs [0, njobs_heads) read only what k_fcl_heads wrote (they run beside the backward chain, in its launch), the
  // rest needs the backward chain's deltas; S = row slabs per job (1 up to batch 512: the fused dW + Adam path)
  int S = 1;
  int G = 1;            // groups of four samples per chain workgroup (2 from batch 2048, 4 from 4096: more than one chain workgroup per CU otherwise)
  int nln = 0;          // rows of lnpart: batch / 4 (one per group)
  // batch <= 512: the forward pass as ONE launch (k_fcl_fwd: chain workgroups + heads units gated by arrival counters)
  bool fb_jobs = true;
  bool fuse_fwd = false, fuse_fb = false;      // (fuse_fb: forward chain + heads + backward chain as ONE launch, k_fcl_fb)
  unsigned *flags = nullptr, *wedge_h = nullptr, *wedge_hd = nullptr;      // (wedge: the pinned word a unit's bounded wait sets when it gives up)
  size_t nflat = 0, npk = 0, lds_bytes = 0, lds_bwd_dw = 0, tape_floats = 0;
  FlatLayout L;
  FclView view;
  float *pk = nullptr, *tapes = nullptr, *part = nullptr, *grad = nullptr, *bsq = nullptr, *lnpart = nullptr, *lngrad = nullptr;
  int32_t *posA = nullptr, *posB = nullptr;
  FclJob *jobs = nullptr;
  float *P = nullptr, *m = nullptr, *v = nullptr, *steps = nullptr;
  const float *lr = nullptr;
  // mz_fcl_set_optimizer: FCL_ADAM (the default) / FCL_SGD / FCL_RMSPROP, momentum and RMSprop's alpha
  int opt_kind = FCL_ADAM;
  double opt_mom = 0.0, opt_alpha = 0.0;
  int scalar_loss = 0;                     // mz_fcl_set_scalar_loss: 0 categorical (the default), 1 MSE, 2 Huber
  // mz_fcl_update: FCL_SLOTS pinned staging slots for a batch, its device copy, the new errors' way back
  char *stage_h[FCL_SLOTS] = {}, *stage_d = nullptr;
  size_t stage_bytes = 0, soff[6] = {0, 0, 0, 0, 0, 0};
  float *err_h[FCL_SLOTS] = {}, *err_d = nullptr;
  hipEvent_t ev[FCL_SLOTS] = {};
  bool ev_pending[FCL_SLOTS] = {};
  // mz_fcl_run: the update's completion word instead of an event (k_fcl_dwa's last workgroup stores the slot's sequence number into
  // pinned host memory): done_h [FCL_SLOTS][16] words, done_seq the number the slot's update in flight will store
  unsigned *done_h = nullptr, *done_hd = nullptr, *done_ctr = nullptr;
  unsigned done_seq[FCL_SLOTS] = {};
  bool done_pending[FCL_SLOTS] = {};
  int slot = 0, nslots = 6;
  // mz_fcl_run: the batch indices of the update in each staging slot whose priority refresh is still owed, per-update learning rates
  std::vector<int64_t> run_idx[FCL_SLOTS];
  bool run_owed[FCL_SLOTS] = {};
  // ... the five launches READ THE BATCH FROM THE SLOT'S PINNED STAGING (device-visible host memory: 50 KB per update, no copy
  // engine, no blit kernel; the update's learning rate rides at its end) and write the new errors into the slot's pinned error
  // buffer; optionally as one captured graph per slot (MZ_FCL_RUN_GRAPH=1: measured out)
  char *stage_hd[FCL_SLOTS] = {};          // device addresses of stage_h / err_h (hipHostGetDevicePointer)
  float *err_hd[FCL_SLOTS] = {};
  hipGraphExec_t run_graph[FCL_SLOTS] = {};
  double run_key[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double run_stats[6] = {0, 0, 0, 0, 0, 0};      // host seconds in: waiting for a slot, refresh, sampling, launching, the whole call; updates
  hipStream_t run_cap = nullptr;
  size_t soff_lr = 0;
  // mz_fcl_set_symmetry: the game kind (0: off), the draw's seed, the counter of the handle's updates (the draw's `update`) and the
  // device buffer the images of a batch's observations, actions and policies are written into (sections at soff[0], soff[1], soff[4])
  int sym_kind = 0;
  uint64_t sym_seed = 0;
  uint32_t sym_update = 0;
  char *sym_d = nullptr;
  std::vector<void *> allocs;
};

static int fcl_even(int x) { return (x + 1) & ~1; }

template <typename T>
static int fcl_alloc(mz_fcl *c, T **p, size_t n) {
  void *q = nullptr;
  HIPCHECK(hipMalloc(&q, n * sizeof(T) + 64));
  HIPCHECK(hipMemset(q, 0, n * sizeof(T) + 64));
  c->allocs.push_back(q);
  *p = (T *)q;
  return 0;
}

// gather map of P(W; M, K) (mz_fcl.hip.h): packed element (tg, s, lane, i) <- flat index of W[64 tg + 16 i + m16][4 s + g4]
static size_t fcl_pack_map(std::vector<int64_t> &gm, int TG, int ks_alloc, const std::function<int64_t(int, int)> &fetch) {
  const size_t pos0 = gm.size();
  gm.resize(pos0 + (size_t)TG * ks_alloc * 256, -1);
  for (int tg = 0; tg < TG; ++tg)
    for (int s = 0; s < ks_alloc; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i)
          gm[pos0 + (((size_t)tg * ks_alloc + s) * 64 + lane) * 4 + i] = fetch(64 * tg + 16 * i + (lane & 15), 4 * s + (lane >> 4));
  return pos0;
}

// the four packed copies of one Linear(kin, 512) -> ReLU -> Linear(512, mout) block (b1: the d-input pack, rows < 50)
static FclPack fcl_pack_block(std::vector<int64_t> &gm, size_t w1, int kin, size_t w2, int mout, bool b1) {
  FclPack p;
  p.ks1 = fcl_even((kin + 3) / 4);
  p.ks2 = fcl_even((mout + 3) / 4);
  p.mout = mout;
  p.nt = (mout + 15) / 16;
  if (p.nt == 3) p.nt = 4;
  const int64_t W1 = (int64_t)w1, W2 = (int64_t)w2;
  p.F1 = fcl_pack_map(gm, 8, FCL_KSA(p.ks1), [=](int m, int k) { return k < kin ? W1 + (int64_t)m * kin + k : (int64_t)-1; });
  p.F2 = fcl_pack_map(gm, 1, 128, [=](int m, int k) { return m < mout ? W2 + (int64_t)m * MZ_F + k : (int64_t)-1; });
  p.B2 = fcl_pack_map(gm, 8, FCL_KSA(p.ks2), [=](int m, int k) { return k < mout ? W2 + (int64_t)k * MZ_F + m : (int64_t)-1; });
  p.B1 = b1 ? fcl_pack_map(gm, 1, 128, [=](int m, int k) { return m < MZ_H ? W1 + (int64_t)k * kin + m : (int64_t)-1; }) : 0;
  return p;
}

// quad copies Q(W; M, K) for the 4-sample chain kernels (mz_fcl.hip.h): [groups][K][64 lanes] floats
static size_t fcl_quad_map(std::vector<int64_t> &gm, int groups, int K, const std::function<int64_t(int, int, int)> &fetch) {
  const size_t pos0 = gm.size();
  gm.resize(pos0 + (size_t)groups * K * 64, -1);
  for (int g = 0; g < groups; ++g)
    for (int k = 0; k < K; ++k)
      for (int lane = 0; lane < 64; ++lane) gm[pos0 + ((size_t)g * K + k) * 64 + lane] = fetch(g, k, lane);
  return pos0;
}

// Linear(kin, 512) -> ReLU -> Linear(512, 50) of the chain: F1 [8 waves][kpad][64] (row 64 w + lane, input k), F2 [512][64]
// (row = lane < 50, input k; wave w reads k in [64 w, 64 w + 64)), B2 [8][50][64] (W2^T: a1 feature 64 w + lane, output k),
// B1 [512][64] (W1^T: hidden input lane < 50, a1 feature k)
static FclPack fcl_pack_quad_block(std::vector<int64_t> &gm, size_t w1, int kin, int kpad, size_t w2, bool b1) {
  FclPack p;
  p.ks1 = kpad; p.ks2 = MZ_H; p.mout = MZ_H; p.nt = 4;
  const int64_t W1 = (int64_t)w1, W2 = (int64_t)w2;
  p.F1 = fcl_quad_map(gm, 8, kpad, [=](int g, int k, int lane) { return k < kin ? W1 + (int64_t)(64 * g + lane) * kin + k : (int64_t)-1; });
  p.F2 = fcl_quad_map(gm, 1, MZ_F, [=](int, int k, int lane) { return lane < MZ_H ? W2 + (int64_t)lane * MZ_F + k : (int64_t)-1; });
  p.B2 = fcl_quad_map(gm, 8, MZ_H, [=](int g, int k, int lane) { return W2 + (int64_t)k * MZ_F + 64 * g + lane; });
  p.B1 = b1 ? fcl_quad_map(gm, 1, MZ_F, [=](int, int k, int lane) { return lane < MZ_H ? W1 + (int64_t)k * kin + lane : (int64_t)-1; }) : 0;
  return p;
}
}  // extern "C++"

int mz_fcl_create(int batch, int unroll_steps, int obs_dim, int action_space, int value_support_min, int value_support_max,
                  int reward_support_min, int reward_support_max, int no_target_transform, mz_fcl **out) {
  if (!out) return fail("mz_fcl_create: null argument");
  const int Sv = value_support_max - value_support_min + 1, Sr = reward_support_max - reward_support_min + 1;
  if (batch < 16 || batch % 16) return fail("mz_fcl_create: the batch size must be a multiple of 16 (got %d)", batch);
  if (unroll_steps < 1 || unroll_steps + 1 > FCL_MAXP) return fail("mz_fcl_create: 1..%d unroll steps (got %d)", FCL_MAXP - 1, unroll_steps);
  if (action_space < 1 || MZ_H + action_space > 64) return fail("mz_fcl_create: 1..%d actions (got %d)", 64 - MZ_H, action_space);
  if (Sv < 1 || Sv > 64 || Sr < 1 || Sr > 64) return fail("mz_fcl_create: supports of 1..64 bins (got %d, %d)", Sv, Sr);
  if (obs_dim < 1 || obs_dim > 1024) return fail("mz_fcl_create: 1..1024 observation features (got %d; the input tile lives in LDS)", obs_dim);
  mz_fcl *c = new mz_fcl();
  auto bail = [&](int rc) {
    for (int k = 0; k < c->nslots; ++k) {
      if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
      if (c->stage_h[k]) (void)hipHostFree(c->stage_h[k]);
      if (c->err_h[k]) (void)hipHostFree(c->err_h[k]);
    }
    for (void *q : c->allocs) (void)hipFree(q);
    if (c->wedge_h) (void)hipHostFree(c->wedge_h);
    if (c->done_h) (void)hipHostFree(c->done_h);
    delete c;
    return rc;
  };
  if (hipGetDevice(&c->device) != hipSuccess) return bail(fail("mz_fcl_create: no HIP device"));
  if (const char *ns = getenv("MZ_FCL_SLOTS")) {
    const int n = atoi(ns);
    if (n >= 2 && n <= FCL_SLOTS) c->nslots = n;
  }
  c->bs = batch; c->K = unroll_steps; c->O = obs_dim; c->A = action_space;
  {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    if (cus < 1) cus = 256;
    c->G = batch / 4 >= 4 * cus ? 4 : (batch / 4 >= 2 * cus ? 2 : 1);
    if (const char *gs = getenv("MZ_FCL_GROUPS")) {            // (kernel development: 1, 2 or 4)
      const int g = atoi(gs);
      if ((g == 1 || g == 2 || g == 4) && batch % (4 * g) == 0) c->G = g;
    }
    while (batch % (4 * c->G)) c->G >>= 1;
    // row slabs of the weight-gradient jobs: 1 up to batch 512 (the fused dW + Adam path: its backward launch carries the chain as
    // ONE group per workgroup), else batch / 128 up to 16
    c->S = batch <= 512 ? 1 : (batch / 128 < 16 ? batch / 128 : 16);      // (16 slabs of >= 8 row chunks: 1280 workgroups; measured against 8 / 32 / 64 at batch 2048 and 4096)
    if (const char *ss = getenv("MZ_FCL_SLABS")) {            // (kernel development: force the slab count; > 1 = the unfused path)
      const int n = atoi(ss);
      if (n >= 1 && n <= batch / 16) c->S = n;
    }
    if (c->S == 1) c->G = 1;
  }
  c->nwg = batch / (4 * c->G);
  c->nln = batch / 4;
  c->L = flat_layout(obs_dim, action_space, Sv, Sr);
  c->nflat = c->L.total;
  const FlatLayout &L = c->L;
  const int KD = MZ_H + action_space, K1 = unroll_steps + 1, R = batch;
  FclView &v = c->view;
  memset(&v, 0, sizeof v);
  v.bs = batch; v.K = unroll_steps; v.O = obs_dim; v.A = action_space; v.KD = KD; v.Sv = Sv; v.Sr = Sr;
  v.vmin = value_support_min; v.rmin = reward_support_min; v.ntt = no_target_transform ? 1 : 0; v.R = R;
  v.XR = 64 * ((obs_dim + 63) / 64);
  v.xks = 16;
  v.xq = obs_dim > 64 ? ((obs_dim + 3) & ~3) : 64;            // input features held in LDS by the chain kernels
  v.rep_b1 = L.rep_b1; v.rep_b2 = L.rep_b2; v.tr_b1 = L.tr_b1; v.tr_b2 = L.tr_b2; v.ln_w = L.ln_w; v.ln_b = L.ln_b;
  v.hb1[0] = L.val_b1; v.hb2[0] = L.val_b2; v.hb1[1] = L.pol_b1; v.hb2[1] = L.pol_b2; v.hb1[2] = L.rew_b1; v.hb2[2] = L.rew_b2;
  // packed copies + the scatter maps flat index -> (at most two) packed positions
  std::vector<int64_t> gm;
  const int KP = KD <= 56 ? 56 : 64;                 // the transition's input features as the chain kernels are instantiated
  v.rep = fcl_pack_quad_block(gm, L.rep_w1, obs_dim, obs_dim, L.rep_w2, false);
  v.tr = fcl_pack_quad_block(gm, L.tr_w1, KD, KP, L.tr_w2, true);
  v.head[0] = fcl_pack_block(gm, L.val_w1, MZ_H, L.val_w2, Sv, true);
  v.head[1] = fcl_pack_block(gm, L.pol_w1, MZ_H, L.pol_w2, action_space, true);
  v.head[2] = fcl_pack_block(gm, L.rew_w1, KD, L.rew_w2, Sr, true);
  c->npk = gm.size();
  std::vector<int32_t> posA(c->nflat, -1), posB(c->nflat, -1);
  for (size_t pos = 0; pos < gm.size(); ++pos) {
    const int64_t g = gm[pos];
    if (g < 0) continue;
    if (posA[g] < 0) posA[g] = (int32_t)pos;
    else if (posB[g] < 0) posB[g] = (int32_t)pos;
    else return bail(fail("mz_fcl_create: a weight with three packed copies (internal)"));
  }
  if (fcl_alloc(c, &c->pk, c->npk) || fcl_alloc(c, &c->posA, c->nflat) || fcl_alloc(c, &c->posB, c->nflat)) return bail(-1);
  if (hipMemcpy(c->posA, posA.data(), c->nflat * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->posB, posB.data(), c->nflat * 4, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail("mz_fcl_create: upload of the pack maps failed"));
  // tapes
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += (n + 15) & ~(size_t)15; return o; };
  const size_t o_xin = take((size_t)K1 * v.XR * R), o_a1c = take((size_t)K1 * 512 * R), o_xhat = take((size_t)K1 * 64 * R),
               o_rstd = take((size_t)K1 * R), o_h = take((size_t)K1 * 64 * R), o_d2c = take((size_t)K1 * 64 * R),
               o_d1c = take((size_t)K1 * 512 * R), o_a1h = take((size_t)3 * K1 * 512 * R), o_d2h = take((size_t)3 * K1 * 64 * R),
               o_d1h = take((size_t)3 * K1 * 512 * R), o_dH = take((size_t)3 * K1 * 64 * R), o_lossb = take((size_t)3 * K1 * R);
  if (fcl_alloc(c, &c->tapes, off)) return bail(-1);
  c->tape_floats = off;
  if (off * 4 > 0x7fffffffull) { c->tape_floats = 0; }      // (buffer descriptors address 2 GB: larger tapes never take the one-launch path)
  float *T = c->tapes;
  v.xin = T + o_xin; v.a1c = T + o_a1c; v.xhat = T + o_xhat; v.rstd = T + o_rstd; v.h = T + o_h; v.d2c = T + o_d2c; v.d1c = T + o_d1c;
  v.a1h = T + o_a1h; v.d2h = T + o_d2h; v.d1h = T + o_d1h; v.dH = T + o_dH; v.lossb = T + o_lossb;
  if (fcl_alloc(c, &c->lnpart, (size_t)c->nln * 128) || fcl_alloc(c, &c->lngrad, (size_t)128)) return bail(-1);
  v.lnpart = c->lnpart;
  // weight-gradient jobs: one tile of a layer's dW over every position the layer is applied at (their tapes lie one stride
  // apart); the heads' jobs first: [0, njobs_heads) only read what k_fcl_heads wrote, the rest needs the backward chain's deltas
  const size_t T64 = (size_t)64 * R, T512 = (size_t)512 * R, TX = (size_t)v.XR * R;
  // tiles: batch <= 512 (one slab, fused with Adam): many small jobs -- the heads' layers as 16 x 64 strips (beside the backward
  // chain), the chain's layers as 16 x 32 (the last launch, alone on the chip); larger batches: 16 na x 64 with na = 4 / 2 / 1 by the
  // layer's output rows (k_fcl_dwt)
  std::vector<FclJob> jobs, jobs_chain;
  auto layer = [&](size_t d_off, int M, size_t x_off, int N, size_t w_off, size_t b_off, int npos) {
    const bool chain = d_off >= o_d2c && d_off < o_a1h;                 // delta tape d2c / d1c: a chain layer
    const bool x_is_xin = x_off >= o_xin && x_off < o_a1c;
    std::vector<FclJob> &dst = chain ? jobs_chain : jobs;
    const int Mp = M == MZ_F ? 512 : 64, Np = x_is_xin ? v.XR : (N == MZ_F ? 512 : 64);      // features per row chunk
    const int na = c->S == 1 ? 1 : (M > 32 ? 4 : (M > 16 ? 2 : 1)), ni = (c->S == 1 && chain) ? 2 : 4;
    for (int tm = 0; tm < (M + 16 * na - 1) / (16 * na); ++tm)
      for (int ng = 0; ng < (N + 16 * ni - 1) / (16 * ni); ++ng) {
        FclJob j;
        memset(&j, 0, sizeof j);
        j.d_off = d_off; j.x_off = x_off; j.d_ps = Mp == 512 ? T512 : T64; j.x_ps = x_is_xin ? TX : (Np == 512 ? T512 : T64);
        j.w_off = w_off; j.b_off = b_off; j.M = M; j.N = N; j.Mp = Mp; j.Np = Np; j.tm = tm; j.ng = ng; j.npos = npos; j.na = na;
        j.hd = chain ? -1 : (w_off == L.val_w1 || w_off == L.val_w2 ? 0 : (w_off == L.pol_w1 || w_off == L.pol_w2 ? 1 : 2));
        dst.push_back(j);
      }
  };
  const int Kn = unroll_steps;
  layer(o_d1c, MZ_F, o_xin, obs_dim, L.rep_w1, L.rep_b1, 1);
  layer(o_d2c, MZ_H, o_a1c, MZ_F, L.rep_w2, L.rep_b2, 1);
  layer(o_d1c + T512, MZ_F, o_xin + TX, KD, L.tr_w1, L.tr_b1, Kn);
  layer(o_d2c + T64, MZ_H, o_a1c + T512, MZ_F, L.tr_w2, L.tr_b2, Kn);
  layer(o_d1h + ((size_t)2 * K1 + 1) * T512, MZ_F, o_xin + TX, KD, L.rew_w1, L.rew_b1, Kn);
  layer(o_d2h + ((size_t)2 * K1 + 1) * T64, Sr, o_a1h + ((size_t)2 * K1 + 1) * T512, MZ_F, L.rew_w2, L.rew_b2, Kn);
  layer(o_d1h, MZ_F, o_h, MZ_H, L.val_w1, L.val_b1, K1);
  layer(o_d2h, Sv, o_a1h, MZ_F, L.val_w2, L.val_b2, K1);
  layer(o_d1h + (size_t)K1 * T512, MZ_F, o_h, MZ_H, L.pol_w1, L.pol_b1, K1);
  layer(o_d2h + (size_t)K1 * T64, action_space, o_a1h + (size_t)K1 * T512, MZ_F, L.pol_w2, L.pol_b2, K1);
  c->njobs_heads = (int)jobs.size();
  jobs.insert(jobs.end(), jobs_chain.begin(), jobs_chain.end());
  c->njobs = (int)jobs.size();
  if (fcl_alloc(c, &c->jobs, jobs.size())) return bail(-1);
  if (hipMemcpy(c->jobs, jobs.data(), jobs.size() * sizeof(FclJob), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail("mz_fcl_create: upload of the job list failed"));
  c->nblk = (int)((c->nflat + 255) / 256);
  if (fcl_alloc(c, &c->part, (size_t)c->S * c->nflat) || fcl_alloc(c, &c->grad, c->nflat) || fcl_alloc(c, &c->bsq, (size_t)c->nblk)) return bail(-1);
  c->lds_bytes = (size_t)FCL_LDS4_FLOATS(v.xq, c->G) * 4;
  if (c->lds_bytes > 160 * 1024) return bail(fail("mz_fcl_create: %d observation features x %d samples per chain workgroup do not fit the LDS", obs_dim, 4 * c->G));
  if (c->lds_bytes > 64 * 1024) {
    const void *fn[9] = {(const void *)k_fcl_chain_fwd4<56, 1>, (const void *)k_fcl_chain_fwd4<64, 1>, (const void *)k_fcl_chain_fwd4<56, 2>,
                         (const void *)k_fcl_chain_fwd4<64, 2>, (const void *)k_fcl_chain_fwd4<56, 4>, (const void *)k_fcl_chain_fwd4<64, 4>,
                         (const void *)k_fcl_chain_bwd4<1>, (const void *)k_fcl_chain_bwd4<2>, (const void *)k_fcl_chain_bwd4<4>};
    for (int i = 0; i < 9; ++i)
      if (hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_bytes) != hipSuccess)
        return bail(fail("mz_fcl_create: %zu bytes of LDS per workgroup refused", c->lds_bytes));
  }
  c->lds_bwd_dw = c->lds_bytes > (size_t)FCL_DW_LDS(FCL_NW, 1, 4) ? c->lds_bytes : (size_t)FCL_DW_LDS(FCL_NW, 1, 4);
  if (hipFuncSetAttribute((const void *)k_fcl_dwt, hipFuncAttributeMaxDynamicSharedMemorySize, FCL_DW_LDS(4, 4, 4)) != hipSuccess)
    return bail(fail("mz_fcl_create: %d bytes of LDS per workgroup refused", FCL_DW_LDS(4, 4, 4)));
  if (c->lds_bwd_dw > 64 * 1024) {
    const void *fn[5] = {(const void *)k_fcl_bwd_dw<FCL_ADAM>, (const void *)k_fcl_bwd_dw<FCL_SGD>, (const void *)k_fcl_bwd_dw<FCL_SGD | FCL_MOM>,
                         (const void *)k_fcl_bwd_dw<FCL_RMSPROP>, (const void *)k_fcl_bwd_dw<FCL_RMSPROP | FCL_MOM>};
    for (int i = 0; i < 5; ++i)
      if (hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_bwd_dw) != hipSuccess)
        return bail(fail("mz_fcl_create: %zu bytes of LDS per workgroup refused", c->lds_bwd_dw));
  }
  if (hipFuncSetAttribute((const void *)k_fcl_heads, hipFuncAttributeMaxDynamicSharedMemorySize, FCL_LDS_HEADS * 4) != hipSuccess ||
      hipFuncSetAttribute((const void *)k_fcl_heads_scalar, hipFuncAttributeMaxDynamicSharedMemorySize, FCL_LDS_HEADS * 4) != hipSuccess)
    return bail(fail("mz_fcl_create: %d bytes of LDS per workgroup refused", FCL_LDS_HEADS * 4));
  {
    // the fused forward launch: where the chain leaves at least half of the chip idle (batch <= 512 on 256 CUs: 107 against 115 us per
    // update at batch 512) and its LDS fits beside the heads' (MZ_FCL_FUSE_FWD=0 / 1: off / on at any batch up to 1024, kernel
    // development); with the backward chain in the same launch (k_fcl_fb) up to batch 256 (at 512 the units' share of the chip is too
    // small for it: 110.5 us)
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    c->fuse_fwd = c->S == 1 && c->G == 1 && batch <= 512 && cus >= 2 * c->nwg && c->lds_bytes <= (size_t)FCL_LDS_HEADS * 4;
    if (const char *ff = getenv("MZ_FCL_FUSE_FWD")) c->fuse_fwd = ff[0] == '1' && c->S == 1 && c->G == 1 && cus >= c->nwg && c->lds_bytes <= (size_t)FCL_LDS_HEADS * 4;
    c->fuse_fb = c->fuse_fwd && batch <= 256 && cus >= 2 * c->nwg && c->tape_floats > 0;      // (every chain workgroup resident beside the units it waits for)
    if (const char *tp = getenv("MZ_FCL_FB_JOBS")) c->fb_jobs = tp[0] == '1';
    if (const char *fb = getenv("MZ_FCL_FUSE_FB")) c->fuse_fb = c->fuse_fb && fb[0] == '1';      // (0: the three-launch step, A/B)
    if (fcl_alloc(c, &c->flags, (size_t)2 * (batch / 16) * K1 + 192)) return bail(-1);
    if (hipHostMalloc((void **)&c->wedge_h, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->wedge_hd, c->wedge_h, 0) != hipSuccess)
      return bail(fail("mz_fcl_create: pinned error word refused"));
    *c->wedge_h = 0u;
    if (hipHostMalloc((void **)&c->done_h, FCL_SLOTS * 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->done_hd, c->done_h, 0) != hipSuccess || fcl_alloc(c, &c->done_ctr, (size_t)16))
      return bail(fail("mz_fcl_create: pinned completion words refused"));
    memset(c->done_h, 0, FCL_SLOTS * 64);
    const void *fn[24] = {(const void *)k_fcl_fwd<56>, (const void *)k_fcl_fwd<64>, (const void *)k_fcl_fb<56, FCL_ADAM>, (const void *)k_fcl_fb<64, FCL_ADAM>,
                          (const void *)k_fcl_fb<56, FCL_SGD>, (const void *)k_fcl_fb<64, FCL_SGD>, (const void *)k_fcl_fb<56, FCL_SGD | FCL_MOM>,
                          (const void *)k_fcl_fb<64, FCL_SGD | FCL_MOM>, (const void *)k_fcl_fb<56, FCL_RMSPROP>, (const void *)k_fcl_fb<64, FCL_RMSPROP>,
                          (const void *)k_fcl_fb<56, FCL_RMSPROP | FCL_MOM>, (const void *)k_fcl_fb<64, FCL_RMSPROP | FCL_MOM>,
                          // (their scalar-loss siblings: mz_fcl_set_scalar_loss)
                          (const void *)k_fcl_fwd<56, true>, (const void *)k_fcl_fwd<64, true>, (const void *)k_fcl_fb<56, FCL_ADAM, true>,
                          (const void *)k_fcl_fb<64, FCL_ADAM, true>, (const void *)k_fcl_fb<56, FCL_SGD, true>, (const void *)k_fcl_fb<64, FCL_SGD, true>,
                          (const void *)k_fcl_fb<56, FCL_SGD | FCL_MOM, true>, (const void *)k_fcl_fb<64, FCL_SGD | FCL_MOM, true>,
                          (const void *)k_fcl_fb<56, FCL_RMSPROP, true>, (const void *)k_fcl_fb<64, FCL_RMSPROP, true>,
                          (const void *)k_fcl_fb<56, FCL_RMSPROP | FCL_MOM, true>, (const void *)k_fcl_fb<64, FCL_RMSPROP | FCL_MOM, true>};
    for (int i = 0; i < 24; ++i)
      if (hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, FCL_LDS_HEADS * 4) != hipSuccess)
        return bail(fail("mz_fcl_create: %d bytes of LDS per workgroup refused", FCL_LDS_HEADS * 4));
  }
  {
    const size_t sz[6] = {(size_t)batch * obs_dim * 4, (size_t)batch * unroll_steps * 8, (size_t)batch * K1 * 4, (size_t)batch * K1 * 4,
                          (size_t)batch * K1 * action_space * 4, (size_t)batch * 8};
    size_t o = 0;
    for (int i = 0; i < 6; ++i) { c->soff[i] = o; o += (sz[i] + 15) & ~(size_t)15; }
    c->soff_lr = o;                          // (mz_fcl_run: the update's learning rate, one float)
    o += 16;
    c->stage_bytes = o;
    if (fcl_alloc(c, &c->stage_d, o) || fcl_alloc(c, &c->err_d, (size_t)batch)) return bail(-1);
    for (int k = 0; k < c->nslots; ++k) {
      if (hipHostMalloc((void **)&c->stage_h[k], o, hipHostMallocDefault) != hipSuccess ||
          hipHostMalloc((void **)&c->err_h[k], (size_t)batch * 4, hipHostMallocDefault) != hipSuccess ||
          hipEventCreateWithFlags(&c->ev[k], hipEventDisableTiming) != hipSuccess)
        return bail(fail("mz_fcl_create: pinned staging of %zu bytes refused", o));
    }
  }
  *out = c;
  return 0;
}

// slot k's update of mz_fcl_run that announces its end through the pinned completion word: wait for it (bounded)
static int fcl_wait_done_word(mz_fcl *c, int k) {
  if (!c->done_pending[k]) return 0;
  const volatile unsigned *word = c->done_h + 16 * k;
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(word, __ATOMIC_ACQUIRE) != c->done_seq[k]) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 30.0)
      return fail("mz_fcl: the update in staging slot %d did not finish in 30 s", k);
    if (*c->wedge_h) return fail("mz_fcl: a wait inside the update's launch ran into its bound (device wedged or oversubscribed)");
    __builtin_ia32_pause();
  }
  c->done_pending[k] = false;
  return 0;
}

static void fcl_drop_run_graphs(mz_fcl *c) {
  for (int k = 0; k < c->nslots; ++k)
    if (c->run_graph[k]) { (void)hipGraphExecDestroy(c->run_graph[k]); c->run_graph[k] = nullptr; }
}

int mz_fcl_destroy(mz_fcl *c) {
  if (!c) return 0;
  fcl_drop_run_graphs(c);
  if (c->run_cap) (void)hipStreamDestroy(c->run_cap);
  for (int k = 0; k < c->nslots; ++k) {
    if (c->ev[k]) { (void)hipEventSynchronize(c->ev[k]); (void)hipEventDestroy(c->ev[k]); }
    (void)fcl_wait_done_word(c, k);
    if (c->stage_h[k]) (void)hipHostFree(c->stage_h[k]);
    if (c->err_h[k]) (void)hipHostFree(c->err_h[k]);
  }
  for (void *q : c->allocs) (void)hipFree(q);
  if (c->wedge_h) (void)hipHostFree(c->wedge_h);
  if (c->done_h) (void)hipHostFree(c->done_h);
  delete c;
  return 0;
}

size_t mz_fcl_num_params(mz_fcl *c) { return c ? c->nflat : 0; }
int mz_fcl_slots(mz_fcl *c) { return c ? c->nslots : -1; }

#define FCL_ENTER(c)                                                                        \
  MzDeviceGuard fcl_guard_;                                                                 \
  if (fcl_guard_.enter((c)->device)) return fail("hipSetDevice(%d) failed", (c)->device)

int mz_fcl_set_optimizer(mz_fcl *c, int kind, double momentum, double alpha) {
  if (!c) return fail("mz_fcl_set_optimizer: null argument");
  if (kind != FCL_ADAM && kind != FCL_SGD && kind != FCL_RMSPROP)
    return fail("mz_fcl_set_optimizer: unknown optimiser kind %d (0 Adam / AdamW, 1 SGD, 2 RMSprop)", kind);
  if (!(momentum >= 0.0) || !std::isfinite(momentum)) return fail("mz_fcl_set_optimizer: momentum %g must be finite and >= 0", momentum);
  if (!(alpha >= 0.0 && alpha < 1.0)) return fail("mz_fcl_set_optimizer: alpha %g outside [0, 1)", alpha);
  c->opt_kind = kind;
  c->opt_mom = kind == FCL_ADAM ? 0.0 : momentum;
  c->opt_alpha = kind == FCL_RMSPROP ? alpha : 0.0;
  fcl_drop_run_graphs(c);
  return 0;
}

int mz_fcl_set_scalar_loss(mz_fcl *c, int kind) {
  if (!c) return fail("mz_fcl_set_scalar_loss: null argument");
  if (kind < 0 || kind > 2) return fail("mz_fcl_set_scalar_loss: unknown loss kind %d (0 categorical, 1 MSE, 2 Huber)", kind);
  if (kind != 0 && (c->view.Sv != 1 || c->view.Sr != 1))
    return fail("mz_fcl_set_scalar_loss: a scalar loss needs a handle created with one output per head (value_support_min == value_support_max, "
                "reward_support_min == reward_support_max); this one has %d value and %d reward bins", c->view.Sv, c->view.Sr);
  c->scalar_loss = kind;
  fcl_drop_run_graphs(c);
  return 0;
}

int mz_fcl_set_symmetry(mz_fcl *c, int kind, uint64_t seed, uint32_t first_update) {
  if (!c) return fail("mz_fcl_set_symmetry: null argument");
  if (kind != 0 && sym_elements(kind) == 0) return fail("mz_fcl_set_symmetry: unknown kind %d (0 off, 1 TicTacToe, 3 Connect Four)", kind);
  if (kind != 0 && (c->O != sym_cells(kind) || c->A != sym_actions(kind)))
    return fail("mz_fcl_set_symmetry: %s has obs_dim %d and action_space %d, the handle was created with %d and %d",
                mz_game_info(kind).name, sym_cells(kind), sym_actions(kind), c->O, c->A);
  if (kind != 0 && !c->sym_d) {
    // ONE buffer for every update of the handle, however many mz_fcl_run keeps in flight: an update's symmetry kernel and the step
    // kernels that read its output are enqueued on the same stream, and so are the next update's, so the next image is written only
    // after every reader of this one has finished (stream order); the staging slots exist because the HOST writes them ahead
    FCL_ENTER(c);
    if (fcl_alloc(c, &c->sym_d, c->soff[5])) return -1;
  }
  c->sym_kind = kind; c->sym_seed = seed; c->sym_update = first_update;
  return 0;
}

// the symmetry kernel over one batch on `s`
static int fcl_symmetry_launch(const SymBatch &b, hipStream_t s) {
  const size_t total = sym_total(b);
  hipLaunchKernelGGL(k_fcl_symmetry, dim3((unsigned)((total + MZ_SYM_THREADS - 1) / MZ_SYM_THREADS)), dim3(MZ_SYM_THREADS), 0, s, b);
  if (hipGetLastError() != hipSuccess) return fail("mz_fcl: k_fcl_symmetry did not launch");
  return 0;
}

// the address the device reads `p` at: mapped pinned host memory (hipHostMalloc, torch's pin_memory) by its device address, device
// memory as it is
static const void *fcl_device_address(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return p; }
  return (at.type == hipMemoryTypeHost && at.devicePointer) ? (const void *)at.devicePointer : p;
}

// test hook (include/mz_engine_debug.h): the kernel alone on given device arrays, with the handle's kind and seed
int mz_fcl_symmetry_apply(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_policies,
                          uint32_t update, float *obs_out, void *actions_out, float *policies_out, int32_t *elements_out, void *stream) {
  if (!c || !obs || !actions || !target_policies || !obs_out || !actions_out || !policies_out)
    return fail("mz_fcl_symmetry_apply: null argument");
  if (!c->sym_kind) return fail("mz_fcl_symmetry_apply: the handle has no symmetry set (mz_fcl_set_symmetry)");
  if ((const void *)obs == (const void *)obs_out || actions == (const void *)actions_out || (const void *)target_policies == (const void *)policies_out)
    return fail("mz_fcl_symmetry_apply: the images cannot be written over their sources");
  FCL_ENTER(c);
  SymBatch b = {(const float *)fcl_device_address(obs), fcl_device_address(actions), (const float *)fcl_device_address(target_policies), obs_out,
                actions_out, policies_out, elements_out, c->sym_seed, update, c->sym_kind, c->bs, c->K, actions_are_i32 ? 1 : 0};
  return fcl_symmetry_launch(b, (hipStream_t)stream);
}

// test hook: the same bodies looped on the host; no handle, no device
int mz_fcl_symmetry_host(int kind, uint64_t seed, uint32_t update, int batch, int K, const float *obs, const void *actions,
                         int actions_are_i32, const float *target_policies, float *obs_out, void *actions_out, float *policies_out,
                         int32_t *elements_out) {
  if (sym_elements(kind) == 0) return fail("mz_fcl_symmetry_host: unknown kind %d (1 TicTacToe, 3 Connect Four)", kind);
  if (batch < 0 || K < 1) return fail("mz_fcl_symmetry_host: batch %d and %d unroll steps", batch, K);
  if (batch && (!obs || !actions || !target_policies || !obs_out || !actions_out || !policies_out))
    return fail("mz_fcl_symmetry_host: null argument");
  if (batch && ((const void *)obs == (const void *)obs_out || actions == (const void *)actions_out || (const void *)target_policies == (const void *)policies_out))
    return fail("mz_fcl_symmetry_host: the images cannot be written over their sources");
  SymBatch b = {obs, actions, target_policies, obs_out, actions_out, policies_out, elements_out, seed, update, kind, batch, K,
                actions_are_i32 ? 1 : 0};
  const size_t total = sym_total(b);
  for (size_t t = 0; t < total; ++t) sym_element(b, t);
  return 0;
}

int mz_fcl_repack(mz_fcl *c, void *stream) {
  if (!c || !c->P) return fail("mz_fcl_repack: no parameters bound");
  FCL_ENTER(c);
  hipLaunchKernelGGL(k_fcl_repack, dim3(c->nblk), dim3(256), 0, (hipStream_t)stream, (const float *)c->P, c->pk,
                     (const int32_t *)c->posA, (const int32_t *)c->posB, c->nflat);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_fcl_bind(mz_fcl *c, float *params, float *exp_avg, float *exp_avg_sq, float *steps, int nsteps, const float *lr,
                void *stream) {
  if (!c || !params || !exp_avg || !exp_avg_sq || !steps || !lr || nsteps < 1 || nsteps > 64) return fail("mz_fcl_bind: bad argument");
  c->P = params; c->m = exp_avg; c->v = exp_avg_sq; c->steps = steps; c->nsteps = nsteps; c->lr = lr;
  fcl_drop_run_graphs(c);                  // (they hold the old addresses)
  return mz_fcl_repack(c, stream);
}

static int fcl_step_lr(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards, const float *target_values,
                       const float *target_policies, const void *is_weights, int weights_are_f64, double beta1, double beta2, double eps,
                       double weight_decay, double clip_grad, int adamw, int no_update, float *new_errors, double *loss_sums, void *stream,
                       const float *lr, unsigned *done_flag = nullptr, unsigned seq = 0u, bool *flag_used = nullptr);

int mz_fcl_step(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards, const float *target_values,
                const float *target_policies, const void *is_weights, int weights_are_f64, double beta1, double beta2, double eps,
                double weight_decay, double clip_grad, int adamw, int no_update, float *new_errors, double *loss_sums, void *stream) {
  return fcl_step_lr(c, obs, actions, actions_are_i32, target_rewards, target_values, target_policies, is_weights, weights_are_f64, beta1, beta2,
                     eps, weight_decay, clip_grad, adamw, no_update, new_errors, loss_sums, stream, nullptr);
}

// lr: the device float the optimiser reads its rate from (null: the one bound by mz_fcl_bind)
// done_flag / seq: the pinned word the step's LAST launch stores `seq` into when its last workgroup ends (k_fcl_dwa: the fused paths of
// batches up to 512); *flag_used says whether this step's structure does -- otherwise the caller records an event
static int fcl_step_lr(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards, const float *target_values,
                       const float *target_policies, const void *is_weights, int weights_are_f64, double beta1, double beta2, double eps,
                       double weight_decay, double clip_grad, int adamw, int no_update, float *new_errors, double *loss_sums, void *stream,
                       const float *lr, unsigned *done_flag, unsigned seq, bool *flag_used) {
  if (!c || !obs || !actions || !target_rewards || !target_values || !target_policies || !is_weights || !new_errors || !loss_sums)
    return fail("mz_fcl_step: null argument");
  if (!c->P) return fail("mz_fcl_step: no parameters bound (mz_fcl_bind)");
  FCL_ENTER(c);
  hipStream_t s = (hipStream_t)stream;
  if (c->sym_kind && !no_update) {
    // the batch's images into sym_d, ahead of the step on its stream; the step reads them in the batch's place
    char *d = c->sym_d;
    SymBatch b = {obs, actions, target_policies, (float *)(d + c->soff[0]), (void *)(d + c->soff[1]), (float *)(d + c->soff[4]), nullptr,
                  c->sym_seed, c->sym_update, c->sym_kind, c->bs, c->K, actions_are_i32 ? 1 : 0};
    if (fcl_symmetry_launch(b, s)) return -1;
    c->sym_update += 1u;
    obs = b.obs_out; actions = b.act_out; target_policies = b.pol_out;
  }
  FclView v = c->view;
  v.P = c->P; v.pk = c->pk;
  v.obs = obs; v.act = actions; v.act_i32 = actions_are_i32 ? 1 : 0; v.t_rew = target_rewards; v.t_val = target_values; v.t_pol = target_policies;
  v.w = is_weights; v.w_f64 = weights_are_f64 ? 1 : 0; v.new_errors = new_errors;
  const int K1 = c->K + 1;
  const bool clip = clip_grad > 0.0;
  v.steps = c->steps; v.nsteps = no_update ? 0 : c->nsteps;
  v.sloss = c->scalar_loss;
  FclOpt o;
  o.beta1 = beta1; o.beta2 = beta2; o.eps = eps; o.wd = weight_decay; o.clip = (float)clip_grad;
  o.adamw = adamw ? 1 : 0; o.no_update = no_update ? 1 : 0;
  o.kind = c->opt_kind; o.mom = (float)c->opt_mom; o.alpha = (float)c->opt_alpha; o.alpha_c = (float)(1.0 - c->opt_alpha);
  o.eps_f = (float)eps; o.wd_f = (float)weight_decay;
  FclDw a;
  a.tapes = c->tapes; a.tape_bytes = (unsigned)(c->tape_floats * 4); a.R = c->bs; a.S = c->S; a.part = c->part; a.nflat = c->nflat; a.grad = c->grad;
  a.fuse = (c->S == 1 && !clip && !no_update) ? 1 : 0;
  a.P = c->P; a.pk = c->pk; a.posA = c->posA; a.posB = c->posB; a.m = c->m; a.vv = c->v; a.steps = c->steps; a.lr_p = lr ? lr : c->lr; a.o = o;
  if (*c->wedge_h) return fail("mz_fcl_step: a heads unit of an earlier step gave up waiting for its chain workgroups (k_fcl_fwd's bounded wait): "
                            "the device is wedged or oversubscribed; the handle's updates since then are void");
  const bool dwa_last = c->S == 1 && !clip && !no_update;      // (k_fcl_dwa is the step's last launch)
  unsigned *dflag = (done_flag && dwa_last) ? done_flag : nullptr;
  if (flag_used) *flag_used = dflag != nullptr;
  v.flags = c->flags; v.nflags = 2 * (c->bs / 16) * K1 + 192; v.err = c->wedge_hd;
  const int nchain_jobs = c->njobs - c->njobs_heads;
  const int lds_dwa = FCL_DW_LDS(FCL_NW, 1, 4) > 3 * 256 * 8 ? FCL_DW_LDS(FCL_NW, 1, 4) : 3 * 256 * 8;
  // the launches, with the optimiser kind's instantiation of every kernel that updates weights
  // and, for a handle in scalar-loss mode, the scalar instantiation of every kernel that runs heads units
  auto launches = [&](auto kind, auto scalar) {
  constexpr int OK = decltype(kind)::value;
  constexpr bool SC = decltype(scalar)::value;
  if (c->fuse_fb) {
    // batch <= 256: TWO launches -- forward chain, heads and backward chain (k_fcl_fb); every weight-gradient job with Adam in its
    // workgroup, the LayerNorm parameters and the loss sums (k_fcl_dwa)
    const int units = (c->bs / 16) * (3 * c->K - 1);      // (position K's units run in the chain workgroups)
    const int inl = c->fb_jobs ? c->njobs_heads : 0;        // the heads' jobs inside k_fcl_fb (MZ_FCL_FB_JOBS=0: in the last launch, A/B)
    if (v.tr.ks1 == 56) hipLaunchKernelGGL((k_fcl_fb<56, OK, SC>), dim3(c->nwg + units + inl), dim3(FCL_THREADS), FCL_LDS_HEADS * 4, s, v, c->nwg, (const FclJob *)c->jobs, a);
    else hipLaunchKernelGGL((k_fcl_fb<64, OK, SC>), dim3(c->nwg + units + inl), dim3(FCL_THREADS), FCL_LDS_HEADS * 4, s, v, c->nwg, (const FclJob *)c->jobs, a);
    hipLaunchKernelGGL((k_fcl_dwa<10, 2, OK>), dim3(c->njobs - inl + (a.fuse ? 2 : 0)), dim3(FCL_THREADS), lds_dwa, s, (const FclJob *)c->jobs + inl, c->njobs - inl, a, a.fuse,
                       (const float *)c->lnpart, c->nln, c->L.ln_w, (const float *)v.lossb, is_weights, v.w_f64, c->bs, K1, loss_sums,
                       c->njobs_heads - inl, c->flags, v.nflags, c->done_ctr, dflag, seq);
  } else if (c->fuse_fwd) {
    const int units = (c->bs / 16) * (3 * K1 - 1);
    if (v.tr.ks1 == 56) hipLaunchKernelGGL((k_fcl_fwd<56, SC>), dim3(c->nwg + units), dim3(FCL_THREADS), FCL_LDS_HEADS * 4, s, v, c->nwg);
    else hipLaunchKernelGGL((k_fcl_fwd<64, SC>), dim3(c->nwg + units), dim3(FCL_THREADS), FCL_LDS_HEADS * 4, s, v, c->nwg);
  } else {
    const bool k56 = v.tr.ks1 == 56;
    if (c->G == 1) { if (k56) hipLaunchKernelGGL((k_fcl_chain_fwd4<56, 1>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
                     else hipLaunchKernelGGL((k_fcl_chain_fwd4<64, 1>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v); }
    else if (c->G == 2) { if (k56) hipLaunchKernelGGL((k_fcl_chain_fwd4<56, 2>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
                          else hipLaunchKernelGGL((k_fcl_chain_fwd4<64, 2>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v); }
    else { if (k56) hipLaunchKernelGGL((k_fcl_chain_fwd4<56, 4>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
           else hipLaunchKernelGGL((k_fcl_chain_fwd4<64, 4>), dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v); }
    hipLaunchKernelGGL(SC ? k_fcl_heads_scalar : k_fcl_heads, dim3(c->bs / 16, K1, 3), dim3(FCL_THREADS), FCL_LDS_HEADS * 4, s, v);
  }
  if (c->fuse_fb) {
  } else if (c->S == 1) {
    // batch <= 512: FOUR launches -- the heads' weight-gradient jobs run beside the backward chain in its launch, the chain's
    // in the last one; every job covers all unroll positions, so its strip is the gradient and (no clipping) Adam follows in
    // the same workgroup; the last launch also carries the LayerNorm parameters and the loss sums
    hipLaunchKernelGGL(k_fcl_bwd_dw<OK>, dim3(c->nwg + c->njobs_heads), dim3(FCL_THREADS), c->lds_bwd_dw, s, v, c->nwg, (const FclJob *)c->jobs, a);
    hipLaunchKernelGGL((k_fcl_dwa<4, 2, OK>), dim3(nchain_jobs + (a.fuse ? 2 : 0)), dim3(FCL_THREADS), lds_dwa, s,
                       (const FclJob *)c->jobs + c->njobs_heads, nchain_jobs, a, a.fuse, (const float *)c->lnpart, c->nln, c->L.ln_w,
                       (const float *)v.lossb, is_weights, v.w_f64, c->bs, K1, loss_sums, 0, (unsigned *)nullptr, 0, c->done_ctr, dflag, seq);
  } else {
    // larger batches: the backward chain fills the chip by itself; every job x row slab is a workgroup of four waves, the
    // slabs' strips are added up by the optimiser kernel
    if (c->G == 1) hipLaunchKernelGGL(k_fcl_chain_bwd4<1>, dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
    else if (c->G == 2) hipLaunchKernelGGL(k_fcl_chain_bwd4<2>, dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
    else hipLaunchKernelGGL(k_fcl_chain_bwd4<4>, dim3(c->nwg), dim3(FCL_THREADS), c->lds_bytes, s, v);
    hipLaunchKernelGGL(k_fcl_dwt, dim3(c->njobs * c->S + 1), dim3(256), FCL_DW_LDS(4, 4, 4), s, (const FclJob *)c->jobs, c->njobs, a,
                       (const float *)c->lnpart, c->nln, c->lngrad);
  }
  if (!a.fuse) {
    // (S > 1: the LayerNorm gradients were reduced by k_fcl_dwt's last workgroup -- lngrad, flagged by nwg = -1)
    const float *lnp = c->S > 1 ? (const float *)c->lngrad : (const float *)c->lnpart;
    const int lnn = c->S > 1 ? -1 : c->nln;
    if (clip)
      hipLaunchKernelGGL(k_fcl_grad, dim3(c->nblk), dim3(256), 0, s, (const float *)c->part, c->S, lnp, lnn,
                         c->L.ln_w, c->nflat, c->grad, c->bsq);
    hipLaunchKernelGGL(k_fcl_adam<OK>, dim3(c->nblk + 1), dim3(256), 0, s, c->P, c->pk, (const int32_t *)c->posA, (const int32_t *)c->posB,
                       c->grad, clip ? (const float *)nullptr : (const float *)c->part, c->S, lnp, lnn, c->L.ln_w,
                       (const float *)c->bsq, c->nblk, c->m, c->v, (const float *)c->steps, lr ? lr : c->lr, o, c->nflat,
                       (const float *)v.lossb, is_weights, v.w_f64, c->bs, K1, loss_sums);
  }
  };
  const bool mom = c->opt_mom != 0.0;
  auto by_loss = [&](auto kind) {
    if (c->scalar_loss) launches(kind, std::true_type{});
    else launches(kind, std::false_type{});
  };
  if (c->opt_kind == FCL_SGD && mom) by_loss(std::integral_constant<int, FCL_SGD | FCL_MOM>{});
  else if (c->opt_kind == FCL_SGD) by_loss(std::integral_constant<int, FCL_SGD>{});
  else if (c->opt_kind == FCL_RMSPROP && mom) by_loss(std::integral_constant<int, FCL_RMSPROP | FCL_MOM>{});
  else if (c->opt_kind == FCL_RMSPROP) by_loss(std::integral_constant<int, FCL_RMSPROP>{});
  else by_loss(std::integral_constant<int, FCL_ADAM>{});
  HIPCHECK(hipGetLastError());
  return 0;
}

// One update from HOST arrays (what replay_buffer.sample_batch returns): stage into pinned memory, one copy to the device,
// mz_fcl_step, the new errors on their way back -- nothing waited for except the staging slot's own previous use (two
// updates ago).  *slot_out names the slot whose errors mz_fcl_errors hands over once they have arrived.
int mz_fcl_update(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards,
                  const float *target_values, const float *target_policies, const void *is_weights, int weights_are_f64, double beta1,
                  double beta2, double eps, double weight_decay, double clip_grad, int adamw, double *loss_sums, void *stream,
                  int *slot_out) {
  if (!c || !obs || !actions || !target_rewards || !target_values || !target_policies || !is_weights || !loss_sums || !slot_out)
    return fail("mz_fcl_update: null argument");
  FCL_ENTER(c);
  const int k = c->slot;
  c->slot = (c->slot + 1) % c->nslots;
  if (c->ev_pending[k]) { HIPCHECK(hipEventSynchronize(c->ev[k])); c->ev_pending[k] = false; }
  if (fcl_wait_done_word(c, k)) return -1;
  if (c->run_owed[k]) return fail("mz_fcl_update: a priority refresh of mz_fcl_run is still owed on this slot (internal)");
  const int K1 = c->K + 1;
  const size_t bs = (size_t)c->bs;
  char *h = c->stage_h[k];
  memcpy(h + c->soff[0], obs, bs * c->O * 4);
  memcpy(h + c->soff[1], actions, bs * c->K * (actions_are_i32 ? 4 : 8));
  memcpy(h + c->soff[2], target_rewards, bs * K1 * 4);
  memcpy(h + c->soff[3], target_values, bs * K1 * 4);
  memcpy(h + c->soff[4], target_policies, bs * K1 * c->A * 4);
  memcpy(h + c->soff[5], is_weights, bs * (weights_are_f64 ? 8 : 4));
  hipStream_t s = (hipStream_t)stream;
  HIPCHECK(hipMemcpyAsync(c->stage_d, h, c->stage_bytes, hipMemcpyHostToDevice, s));
  const char *d = c->stage_d;
  if (mz_fcl_step(c, (const float *)(d + c->soff[0]), d + c->soff[1], actions_are_i32, (const float *)(d + c->soff[2]),
                  (const float *)(d + c->soff[3]), (const float *)(d + c->soff[4]), d + c->soff[5], weights_are_f64, beta1, beta2, eps,
                  weight_decay, clip_grad, adamw, 0, c->err_d, loss_sums, stream))
    return -1;
  HIPCHECK(hipMemcpyAsync(c->err_h[k], c->err_d, bs * 4, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipEventRecord(c->ev[k], s));
  c->ev_pending[k] = true;
  *slot_out = k;
  return 0;
}

// the new errors (priority refresh, learners.py:181-182) of the update that used `slot`: waits for their copy, host_out [batch]
int mz_fcl_errors(mz_fcl *c, int slot, float *host_out) {
  if (!c || !host_out || slot < 0 || slot >= c->nslots) return fail("mz_fcl_errors: bad argument");
  FCL_ENTER(c);
  HIPCHECK(hipEventSynchronize(c->ev[slot]));
  if (fcl_wait_done_word(c, slot)) return -1;
  memcpy(host_out, c->err_h[slot], (size_t)c->bs * 4);
  return 0;
}

// Learner.learn's loop body (learners.py:118-131: sample_batch -> update_weights -> replay_buffer.update) for n_updates training
// steps without a line of Python in between.  Per update: the slot's previous occupant (nslots = 6 updates ago) has finished -> its
// priority refresh goes to the replay (src->refresh on its float32 errors); the next batch is sampled STRAIGHT INTO the slot's
// pinned staging (src->sample = mzr_sample_batches_full: stratified draws from words [2 bs i, 2 bs (i + 1)), action padding
// from numpy's generator state, beta schedule, importance weights); --norm_obs applied in place ((obs - min) / range in
// float32, learners.py:170-171); then the five launches of the step, which read the batch from the pinned staging itself and
// write the new errors into pinned memory (no copies).  The GPU works on updates i - 2 and i - 1 while the
// host samples batch i.  Returns with up to nslots updates still in flight (their refreshes are handed over by the next
// call as their slots come up); n_updates = 0 is the flush: waits for them and hands their refreshes over.
int mz_fcl_run(mz_fcl *c, const mz_fcl_source *src, int n_updates, const uint32_t *words, uint32_t *np_key, int32_t *np_pos,
               double *beta_inout, const float *obs_min, const float *obs_range, double beta1, double beta2, double eps,
               double weight_decay, double clip_grad, int adamw, const float *lrs, double *loss_sums, void *stream,
               int64_t *pads_out, uint32_t *py_key, int32_t *py_pos) {
  if (!c || !src || !src->replay || !src->sample || !src->refresh || (!words && (!py_key || !py_pos)) || !np_key || !np_pos || !beta_inout ||
      !loss_sums)
    return fail("mz_fcl_run: null argument");
  if (n_updates < 0) return fail("mz_fcl_run: n_updates must be >= 0");
  if (!c->P) return fail("mz_fcl_run: no parameters bound (mz_fcl_bind)");
  FCL_ENTER(c);
  hipStream_t s = (hipStream_t)stream;
  const int K1 = c->K + 1;
  const size_t bs = (size_t)c->bs;
  // MZ_FCL_RUN_GRAPH=1: the five launches of an update as one captured graph per slot.  Measured out (one box, A/B): kernels run
  // without gaps inside a graph, but consecutive graph launches start ~15 us apart -- 105 us per update against 96.5 us for the
  // five direct launches (8.4 k against 9.0 k updates/s); profiles/r05_kernel_experiments.txt
  static const bool use_graph = getenv("MZ_FCL_RUN_GRAPH") && getenv("MZ_FCL_RUN_GRAPH")[0] == '1';
  if (use_graph && c->sym_kind) return fail("mz_fcl_run: MZ_FCL_RUN_GRAPH=1 captures an update once and cannot carry the symmetry counter of mz_fcl_set_symmetry");
  const char *ev_env = getenv("MZ_FCL_RUN_EVENTS");      // (1: an event behind every update instead of the completion word; A/B and tests)
  const bool use_flag = !(ev_env && ev_env[0] == '1');
  // the captured update of each slot (rebuilt when a hyper-parameter or an address it holds changes)
  const double key[11] = {beta1, beta2, eps, weight_decay, clip_grad, (double)(adamw ? 1 : 0) + (lrs ? 2 : 0), (double)(uintptr_t)loss_sums,
                          (double)(uintptr_t)c->lr, (double)c->opt_kind, c->opt_mom, c->opt_alpha};
  if (memcmp(key, c->run_key, sizeof key)) { fcl_drop_run_graphs(c); memcpy(c->run_key, key, sizeof key); }
  if (!c->run_cap) HIPCHECK(hipStreamCreateWithFlags(&c->run_cap, hipStreamNonBlocking));
  for (int k = 0; k < c->nslots; ++k) {
    if (!c->stage_hd[k]) {
      HIPCHECK(hipHostGetDevicePointer((void **)&c->stage_hd[k], c->stage_h[k], 0));
      HIPCHECK(hipHostGetDevicePointer((void **)&c->err_hd[k], c->err_h[k], 0));
    }
    if (c->run_graph[k] || !use_graph) continue;
    const char *d = c->stage_hd[k];
    hipGraph_t g = nullptr;
    HIPCHECK(hipStreamBeginCapture(c->run_cap, hipStreamCaptureModeThreadLocal));
    int rc = fcl_step_lr(c, (const float *)(d + c->soff[0]), d + c->soff[1], 1, (const float *)(d + c->soff[2]), (const float *)(d + c->soff[3]),
                         (const float *)(d + c->soff[4]), d + c->soff[5], 1, beta1, beta2, eps, weight_decay, clip_grad, adamw, 0,
                         c->err_hd[k], loss_sums, (void *)c->run_cap, lrs ? (const float *)(d + c->soff_lr) : nullptr);
    const hipError_t ce = hipStreamEndCapture(c->run_cap, &g);
    if (rc || ce != hipSuccess) { if (g) (void)hipGraphDestroy(g); return fail("mz_fcl_run: capture of the update failed"); }
    const hipError_t ie = hipGraphInstantiate(&c->run_graph[k], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) return fail("mz_fcl_run: hipGraphInstantiate failed (%s)", hipGetErrorString(ie));
  }
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_call = now();
  auto settle = [&](int k) -> int {         // slot k's previous update: wait for it, hand its refresh over
    double t0 = now();
    if (c->ev_pending[k]) { HIPCHECK(hipEventSynchronize(c->ev[k])); c->ev_pending[k] = false; }
    if (fcl_wait_done_word(c, k)) return -1;      // (the update's last workgroup stores the slot's sequence number: k_fcl_dwa)
    double t1 = now();
    c->run_stats[0] += t1 - t0;
    if (c->run_owed[k]) {
      c->run_owed[k] = false;
      if (src->refresh(src->replay, c->run_idx[k].data(), c->err_h[k], (int64_t)bs))
        return fail("mz_fcl_run: priority refresh failed: %s", src->last_error ? src->last_error() : "?");
      c->run_stats[1] += now() - t1;
    }
    return 0;
  };
  int64_t pads_total = 0;
  for (int i = 0; i < n_updates; ++i) {
    const int k = c->slot;
    c->slot = (c->slot + 1) % c->nslots;
    if (settle(k)) return -1;
    char *h = c->stage_h[k];
    c->run_idx[k].resize(bs);
    int64_t pads = 0;
    const double t_s = now();
    if (src->sample(src->replay, words ? words + 2 * bs * (size_t)i : nullptr, 1, (int)bs, (float *)(h + c->soff[0]), (int32_t *)(h + c->soff[1]),
                    (float *)(h + c->soff[2]), (float *)(h + c->soff[3]), (float *)(h + c->soff[4]), c->run_idx[k].data(),
                    (double *)(h + c->soff[5]), np_key, np_pos, beta_inout, &pads, py_key, py_pos))
      return fail("mz_fcl_run: sampling failed: %s", src->last_error ? src->last_error() : "?");
    pads_total += pads;
    if (obs_min && obs_range) {
      float *o = (float *)(h + c->soff[0]);
      for (size_t r = 0; r < bs; ++r)
        for (int j = 0; j < c->O; ++j) o[r * c->O + j] = (o[r * c->O + j] - obs_min[j]) / obs_range[j];
    }
    if (lrs) *(float *)(h + c->soff_lr) = lrs[i];
    const double t_l = now();
    c->run_stats[2] += t_l - t_s;
    bool by_flag = false;
    if (use_graph) {
      HIPCHECK(hipGraphLaunch(c->run_graph[k], s));    // the five launches, reading this slot's staging
    } else {
      const char *d = c->stage_hd[k];
      if (fcl_step_lr(c, (const float *)(d + c->soff[0]), d + c->soff[1], 1, (const float *)(d + c->soff[2]), (const float *)(d + c->soff[3]),
                      (const float *)(d + c->soff[4]), d + c->soff[5], 1, beta1, beta2, eps, weight_decay, clip_grad, adamw, 0, c->err_hd[k],
                      loss_sums, stream, lrs ? (const float *)(d + c->soff_lr) : nullptr, use_flag ? c->done_hd + 16 * k : nullptr,
                      c->done_seq[k] + 1u, &by_flag))
        return -1;
    }
    if (by_flag) { c->done_seq[k] += 1u; c->done_pending[k] = true; }
    else { HIPCHECK(hipEventRecord(c->ev[k], s)); c->ev_pending[k] = true; }
    c->run_stats[3] += now() - t_l;
    c->run_owed[k] = true;
  }
  if (n_updates == 0)                       // the flush: every update in flight finishes, the oldest first (refreshes in update order)
    for (int j = 0; j < c->nslots; ++j)
      if (settle((c->slot + j) % c->nslots)) return -1;
  if (pads_out) *pads_out = pads_total;
  c->run_stats[4] += now() - t_call;
  c->run_stats[5] += (double)n_updates;
  return 0;
}

// development hook: where mz_fcl_run's host time went since the handle was created (or the last reset): out [host][6] = seconds
// waiting for a staging slot's previous update, in priority refreshes, in sampling (+ normalisation), in launching, in the calls as a
// whole; and the number of updates
int mz_fcl_run_stats(mz_fcl *c, double *out6, int reset) {
  if (!c || !out6) return fail("mz_fcl_run_stats: null argument");
  memcpy(out6, c->run_stats, sizeof c->run_stats);
  if (reset) memset(c->run_stats, 0, sizeof c->run_stats);
  return 0;
}

// test hook: the assembled gradient of the last step (flat, engine.WEIGHT_ORDER) to the host; waits for the device
int mz_fcl_read_grad(mz_fcl *c, float *host_out, size_t n) {
  if (!c || !host_out || n != c->nflat) return fail("mz_fcl_read_grad: bad argument");
  FCL_ENTER(c);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(host_out, c->grad, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// test hook: one of the tapes of the last step to the host (which: 0 xin, 1 a1c, 2 xhat, 3 rstd, 4 h, 5 d2c, 6 d1c, 7 a1h,
// 8 d2h, 9 d1h, 10 dH, 11 lossb -- layouts in mz_fcl.hip.h); n = its float count, returned when host_out is null
long long mz_fcl_read_tape(mz_fcl *c, int which, float *host_out, size_t n) {
  if (!c) return fail("mz_fcl_read_tape: null argument");
  const FclView &v = c->view;
  const size_t K1 = (size_t)c->K + 1, R = (size_t)c->bs;
  const float *ptr[12] = {v.xin, v.a1c, v.xhat, v.rstd, v.h, v.d2c, v.d1c, v.a1h, v.d2h, v.d1h, v.dH, v.lossb};
  const size_t cnt[12] = {K1 * v.XR * R, K1 * 512 * R, K1 * 64 * R, K1 * R, K1 * 64 * R, K1 * 64 * R, K1 * 512 * R, 3 * K1 * 512 * R,
                          3 * K1 * 64 * R, 3 * K1 * 512 * R, 3 * K1 * 64 * R, 3 * K1 * R};
  if (which < 0 || which >= 12) return fail("mz_fcl_read_tape: tape %d", which);
  if (!host_out) return (long long)cnt[which];
  if (n != cnt[which]) return fail("mz_fcl_read_tape: tape %d has %zu floats (got %zu)", which, cnt[which], n);
  FCL_ENTER(c);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(host_out, ptr[which], n * sizeof(float), hipMemcpyDeviceToHost));
  return (long long)n;
}

// development hook: shader-clock stamps of k_fcl_heads' phases in the LAST mz_fcl_step after this call (workgroup 0 of each
// head at position 1; slots 48..53: k_fcl_chain_fwd4's position 2 in workgroup 0): enable = 1 arms it, enable = 0 reads the
// stamps of the last step to host_out [64].  Shader-clock ticks.
int mz_fcl_heads_profile(mz_fcl *c, int enable, unsigned long long *host_out) {
  if (!c) return fail("mz_fcl_heads_profile: null argument");
  FCL_ENTER(c);
  if (enable) {
    if (!c->view.prof && fcl_alloc(c, &c->view.prof, (size_t)96)) return -1;
    return 0;
  }
  if (!c->view.prof || !host_out) return fail("mz_fcl_heads_profile: not armed");
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(host_out, c->view.prof, 96 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemset(c->view.prof + 64, 0, 32 * sizeof(unsigned long long)));      // (the running maxima start over)
  return 0;
}
