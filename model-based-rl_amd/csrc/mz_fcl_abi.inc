// mz_fcl_abi.inc -- host side of the FCNetwork learner step (mz_fcl.hip.h; include/mz_engine.h "learner step").
// Included inside mz_engine.hip's extern "C" block.

extern "C++" {
// staging slots of mz_fcl_update / mz_fcl_run: an update's batch stays in its slot until the update has run.  With n slots the host
// runs n - 1 updates ahead of the GPU: launch and completion latencies hide behind whole updates, and the Python the learner's loop
// runs between two mz_fcl_run calls (logging, send_weights: ~0.6 ms per 100 updates) hides behind the updates still queued.
// FCL_SLOTS: the most a handle can have; mz_fcl.nslots: what it uses (6; MZ_FCL_SLOTS=2..8 for A/B runs)
#define FCL_SLOTS 8
// a launch of the step: the kernel's address, the dynamic LDS it is launched with and its name with its template arguments
template <class F>
struct FclKernel { F fn = nullptr; size_t lds = 0; std::string name; };
// every launch a step can make (fcl_kernels); null where the plan's forms do not have it
struct FclKernels {
  FclKernel<decltype(&k_fcl_fb<56, FCL_ADAM, false>)> fb;
  FclKernel<decltype(&k_fcl_fwd<56, false>)> fwd;
  FclKernel<decltype(&k_fcl_chain_fwd4<56, 1>)> chain_fwd;
  FclKernel<decltype(&k_fcl_heads)> heads;
  FclKernel<decltype(&k_fcl_bwd_dw<FCL_ADAM>)> bwd_dw;
  FclKernel<decltype(&k_fcl_dwa<4, 2, FCL_ADAM>)> dwa;
  FclKernel<decltype(&k_fcl_chain_bwd4<1>)> chain_bwd;
  FclKernel<decltype(&k_fcl_dwt)> dwt;
  FclKernel<decltype(&k_fcl_grad)> grad;
  FclKernel<decltype(&k_fcl_adam<FCL_ADAM>)> adam;
};
template <class V>
static void fcl_each_kernel(const FclKernels &k, V &&visit) {
  visit(k.fb); visit(k.fwd); visit(k.chain_fwd); visit(k.heads); visit(k.bwd_dw); visit(k.dwa); visit(k.chain_bwd); visit(k.dwt);
  visit(k.grad); visit(k.adam);
}

struct mz_fcl {
  int device = 0;
  FclPlan plan;                            // the step's shape (mz_fcl_plan.inc), decided once by mz_fcl_create
  FclKernels kern;                         // ... and its launches for the handle's optimiser kind and loss form (fcl_resolve)
  int nblk = 0, nsteps = 0;
  unsigned *flags = nullptr, *wedge_h = nullptr, *wedge_hd = nullptr;      // (wedge: the pinned word a unit's bounded wait sets when it gives up)
  size_t nflat = 0, npk = 0;
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
  // mz_fcl_set_symmetry: the game kind (0: off), the draw's seed, the counter of the handle's updates (the draw's `update`) and the
  // device buffer the images of a batch's observations, actions and policies are written into (a staging slot's sections 0, 1 and 4)
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
// ---- the step's kernels.  fcl_kernels(plan, optimiser kind with its momentum bit, scalar loss): every launch a step of that plan can
// make, with the LDS the plan launches it with.  The ONLY place a k_fcl_* template argument list is written: mz_fcl_create raises the
// LDS limits of what it returns, the step launches what it returns.
static std::string fcl_kname(const char *base, std::initializer_list<int> args) {
  std::string s = std::string(base) + "<";
  for (int a : args) s += (s.back() == '<' ? "" : ",") + std::to_string(a);
  return s + ">";
}

template <int G>
static void fcl_chain_kernels(const FclPlan &p, FclKernels &k) {
  if (p.fwd == FCL_FWD_CHAIN) {
    if (p.KP == 56) k.chain_fwd.fn = k_fcl_chain_fwd4<56, G>;
    else k.chain_fwd.fn = k_fcl_chain_fwd4<64, G>;
    k.chain_fwd.lds = p.lds_bytes; k.chain_fwd.name = fcl_kname("k_fcl_chain_fwd4", {p.KP, G});
  }
  if (p.bwd == FCL_BWD_SLABS) k.chain_bwd = {k_fcl_chain_bwd4<G>, p.lds_bytes, fcl_kname("k_fcl_chain_bwd4", {G})};
}

// OK: the optimiser kind's instantiation of every kernel that updates weights; SC: the scalar-loss one of every kernel that runs heads units
template <int OK, bool SC>
static FclKernels fcl_kernels_of(const FclPlan &p) {
  FclKernels k;
  const size_t lds_heads = (size_t)FCL_LDS_HEADS * 4;
  if (p.fwd == FCL_FWD_FB) {
    if (p.KP == 56) k.fb.fn = k_fcl_fb<56, OK, SC>;
    else k.fb.fn = k_fcl_fb<64, OK, SC>;
    k.fb.lds = lds_heads; k.fb.name = fcl_kname("k_fcl_fb", {p.KP, OK, SC});
    k.dwa = {k_fcl_dwa<10, 2, OK>, (size_t)p.lds_dwa, fcl_kname("k_fcl_dwa", {10, 2, OK})};
  } else if (p.fwd == FCL_FWD_FUSED) {
    if (p.KP == 56) k.fwd.fn = k_fcl_fwd<56, SC>;
    else k.fwd.fn = k_fcl_fwd<64, SC>;
    k.fwd.lds = lds_heads; k.fwd.name = fcl_kname("k_fcl_fwd", {p.KP, SC});
  } else {
    k.heads = {SC ? k_fcl_heads_scalar : k_fcl_heads, lds_heads, SC ? "k_fcl_heads_scalar" : "k_fcl_heads"};
  }
  if (p.bwd == FCL_BWD_DW) {
    k.bwd_dw = {k_fcl_bwd_dw<OK>, p.lds_bwd_dw, fcl_kname("k_fcl_bwd_dw", {OK})};
    k.dwa = {k_fcl_dwa<4, 2, OK>, (size_t)p.lds_dwa, fcl_kname("k_fcl_dwa", {4, 2, OK})};
  } else if (p.bwd == FCL_BWD_SLABS) {
    k.dwt = {k_fcl_dwt, (size_t)FCL_DW_LDS(4, 4, 4), "k_fcl_dwt"};
  }
  if (p.G == 1) fcl_chain_kernels<1>(p, k);
  else if (p.G == 2) fcl_chain_kernels<2>(p, k);
  else fcl_chain_kernels<4>(p, k);
  // (where the update is not fused into the weight-gradient jobs: row slabs, gradient clipping, a step without an update)
  k.grad = {k_fcl_grad, 0, "k_fcl_grad"};
  k.adam = {k_fcl_adam<OK>, 0, fcl_kname("k_fcl_adam", {OK})};
  return k;
}

template <int OK>
static FclKernels fcl_kernels_by_loss(const FclPlan &p, bool scalar) { return scalar ? fcl_kernels_of<OK, true>(p) : fcl_kernels_of<OK, false>(p); }

static const int fcl_opt_kinds[5] = {FCL_ADAM, FCL_SGD, FCL_SGD | FCL_MOM, FCL_RMSPROP, FCL_RMSPROP | FCL_MOM};
static FclKernels fcl_kernels(const FclPlan &p, int ok, bool scalar) {
  switch (ok) {
    case FCL_SGD: return fcl_kernels_by_loss<FCL_SGD>(p, scalar);
    case FCL_SGD | FCL_MOM: return fcl_kernels_by_loss<FCL_SGD | FCL_MOM>(p, scalar);
    case FCL_RMSPROP: return fcl_kernels_by_loss<FCL_RMSPROP>(p, scalar);
    case FCL_RMSPROP | FCL_MOM: return fcl_kernels_by_loss<FCL_RMSPROP | FCL_MOM>(p, scalar);
    default: return fcl_kernels_by_loss<FCL_ADAM>(p, scalar);
  }
}

// the handle's launches follow its optimiser kind and loss form (mz_fcl_set_optimizer, mz_fcl_set_scalar_loss)
static void fcl_resolve(mz_fcl *c) {
  const int ok = c->opt_kind == FCL_ADAM ? FCL_ADAM : (c->opt_kind | (c->opt_mom != 0.0 ? FCL_MOM : 0));
  c->kern = fcl_kernels(c->plan, ok, c->scalar_loss != 0);
}

static float *FclView::*const fcl_tape_of[FCL_NTAPES] = {&FclView::xin, &FclView::a1c, &FclView::xhat, &FclView::rstd, &FclView::h, &FclView::d2c, &FclView::d1c,
                                                         &FclView::a1h, &FclView::d2h, &FclView::d1h, &FclView::dH, &FclView::lossb};

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

// everything the handle holds, and the handle (a failed mz_fcl_create; mz_fcl_destroy once nothing of it is in flight)
static void fcl_release(mz_fcl *c) {
  fcl_drop_run_graphs(c);
  if (c->run_cap) (void)hipStreamDestroy(c->run_cap);
  for (int k = 0; k < c->nslots; ++k) {
    if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
    if (c->stage_h[k]) (void)hipHostFree(c->stage_h[k]);
    if (c->err_h[k]) (void)hipHostFree(c->err_h[k]);
  }
  for (void *q : c->allocs) (void)hipFree(q);
  if (c->wedge_h) (void)hipHostFree(c->wedge_h);
  if (c->done_h) (void)hipHostFree(c->done_h);
  delete c;
}

static FclKnobs fcl_knobs_from_env() {
  FclKnobs kn;
  auto number = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : -1; };
  auto is_one = [](const char *name) { const char *e = getenv(name); return e ? (e[0] == '1' ? 1 : 0) : -1; };
  kn.groups = number("MZ_FCL_GROUPS"); kn.slabs = number("MZ_FCL_SLABS");
  kn.fuse_fwd = is_one("MZ_FCL_FUSE_FWD"); kn.fuse_fb = is_one("MZ_FCL_FUSE_FB"); kn.fb_jobs = is_one("MZ_FCL_FB_JOBS");
  return kn;
}

// the shapes mz_fcl_create takes (Sv, Sr: the supports' bins)
static int fcl_refuse_shape(int batch, int unroll_steps, int obs_dim, int action_space, int Sv, int Sr) {
  if (batch < 16 || batch % 16) return fail("mz_fcl_create: the batch size must be a multiple of 16 (got %d)", batch);
  if (unroll_steps < 1 || unroll_steps + 1 > FCL_MAXP) return fail("mz_fcl_create: 1..%d unroll steps (got %d)", FCL_MAXP - 1, unroll_steps);
  if (action_space < 1 || MZ_H + action_space > 64) return fail("mz_fcl_create: 1..%d actions (got %d)", 64 - MZ_H, action_space);
  if (Sv < 1 || Sv > 64 || Sr < 1 || Sr > 64) return fail("mz_fcl_create: supports of 1..64 bins (got %d, %d)", Sv, Sr);
  if (obs_dim < 1 || obs_dim > 1024) return fail("mz_fcl_create: 1..1024 observation features (got %d; the input tile lives in LDS)", obs_dim);
  return 0;
}
static int fcl_refuse_plan(const FclPlan &p) {
  if (!fcl_plan_fits(p)) return fail("mz_fcl_create: %d observation features x %d samples per chain workgroup do not fit the LDS", p.O, 4 * p.G);
  return 0;
}
}  // extern "C++"

int mz_fcl_create(int batch, int unroll_steps, int obs_dim, int action_space, int value_support_min, int value_support_max,
                  int reward_support_min, int reward_support_max, int no_target_transform, mz_fcl **out) {
  if (!out) return fail("mz_fcl_create: null argument");
  const int Sv = value_support_max - value_support_min + 1, Sr = reward_support_max - reward_support_min + 1;
  if (fcl_refuse_shape(batch, unroll_steps, obs_dim, action_space, Sv, Sr)) return -1;
  mz_fcl *c = new mz_fcl();
  auto bail = [&](int rc) { fcl_release(c); return rc; };
  if (hipGetDevice(&c->device) != hipSuccess) return bail(fail("mz_fcl_create: no HIP device"));
  if (const char *ns = getenv("MZ_FCL_SLOTS")) {
    const int n = atoi(ns);
    if (n >= 2 && n <= FCL_SLOTS) c->nslots = n;
  }
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
  if (cus < 1) cus = 256;
  c->plan = fcl_plan(batch, unroll_steps, obs_dim, action_space, Sv, Sr, cus, fcl_knobs_from_env());
  const FclPlan &p = c->plan;
  if (fcl_refuse_plan(p)) return bail(-1);
  c->L = flat_layout(obs_dim, action_space, Sv, Sr);
  c->nflat = c->L.total;
  const FlatLayout &L = c->L;
  const int KD = p.KD, K1 = unroll_steps + 1, R = batch;
  FclView &v = c->view;
  memset(&v, 0, sizeof v);
  v.bs = batch; v.K = unroll_steps; v.O = obs_dim; v.A = action_space; v.KD = KD; v.Sv = Sv; v.Sr = Sr;
  v.vmin = value_support_min; v.rmin = reward_support_min; v.ntt = no_target_transform ? 1 : 0; v.R = R;
  v.XR = p.XR;
  v.xks = 16;
  v.xq = p.xq;
  v.rep_b1 = L.rep_b1; v.rep_b2 = L.rep_b2; v.tr_b1 = L.tr_b1; v.tr_b2 = L.tr_b2; v.ln_w = L.ln_w; v.ln_b = L.ln_b;
  v.hb1[0] = L.val_b1; v.hb2[0] = L.val_b2; v.hb1[1] = L.pol_b1; v.hb2[1] = L.pol_b2; v.hb1[2] = L.rew_b1; v.hb2[2] = L.rew_b2;
  // packed copies + the scatter maps flat index -> (at most two) packed positions
  std::vector<int64_t> gm;
  v.rep = fcl_pack_quad_block(gm, L.rep_w1, obs_dim, obs_dim, L.rep_w2, false);
  v.tr = fcl_pack_quad_block(gm, L.tr_w1, KD, p.KP, L.tr_w2, true);
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
  if (fcl_alloc(c, &c->tapes, p.tape_floats)) return bail(-1);
  for (int i = 0; i < FCL_NTAPES; ++i) v.*fcl_tape_of[i] = c->tapes + p.tape[i].off;
  if (fcl_alloc(c, &c->lnpart, (size_t)p.nln * 128) || fcl_alloc(c, &c->lngrad, (size_t)128)) return bail(-1);
  v.lnpart = c->lnpart;
  // weight-gradient jobs: one tile (fcl_tiles) of a layer's dW over every position the layer is applied at (their tapes lie one
  // stride apart); the heads' jobs first: [0, njobs_heads) only read what k_fcl_heads wrote, the rest needs the backward chain's deltas
  const size_t T64 = (size_t)64 * R, T512 = (size_t)512 * R, TX = (size_t)v.XR * R;
  const size_t o_xin = p.tape[FCL_T_XIN].off, o_a1c = p.tape[FCL_T_A1C].off, o_h = p.tape[FCL_T_H].off, o_d2c = p.tape[FCL_T_D2C].off,
               o_d1c = p.tape[FCL_T_D1C].off, o_a1h = p.tape[FCL_T_A1H].off, o_d2h = p.tape[FCL_T_D2H].off, o_d1h = p.tape[FCL_T_D1H].off;
  std::vector<FclJob> jobs, jobs_chain;
  auto layer = [&](size_t d_off, int M, size_t x_off, int N, size_t w_off, size_t b_off, int npos) {
    const bool chain = d_off >= o_d2c && d_off < o_a1h;                 // delta tape d2c / d1c: a chain layer
    const bool x_is_xin = x_off >= o_xin && x_off < o_a1c;
    std::vector<FclJob> &dst = chain ? jobs_chain : jobs;
    const int Mp = M == MZ_F ? 512 : 64, Np = x_is_xin ? v.XR : (N == MZ_F ? 512 : 64);      // features per row chunk
    const FclTiles t = fcl_tiles(p.S, chain, M, N);
    for (int tm = 0; tm < t.tm; ++tm)
      for (int ng = 0; ng < t.ng; ++ng) {
        FclJob j;
        memset(&j, 0, sizeof j);
        j.d_off = d_off; j.x_off = x_off; j.d_ps = Mp == 512 ? T512 : T64; j.x_ps = x_is_xin ? TX : (Np == 512 ? T512 : T64);
        j.w_off = w_off; j.b_off = b_off; j.M = M; j.N = N; j.Mp = Mp; j.Np = Np; j.tm = tm; j.ng = ng; j.npos = npos; j.na = t.na;
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
  if ((int)jobs.size() != p.njobs_heads || (int)(jobs.size() + jobs_chain.size()) != p.njobs)
    return bail(fail("mz_fcl_create: the job list and the plan disagree (internal)"));
  jobs.insert(jobs.end(), jobs_chain.begin(), jobs_chain.end());
  if (fcl_alloc(c, &c->jobs, jobs.size())) return bail(-1);
  if (hipMemcpy(c->jobs, jobs.data(), jobs.size() * sizeof(FclJob), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail("mz_fcl_create: upload of the job list failed"));
  c->nblk = (int)((c->nflat + 255) / 256);
  if (fcl_alloc(c, &c->part, (size_t)p.S * c->nflat) || fcl_alloc(c, &c->grad, c->nflat) || fcl_alloc(c, &c->bsq, (size_t)c->nblk)) return bail(-1);
  // every kernel a step of this plan can launch, under any optimiser and loss form, with more than the default 64 KB of LDS: raise its limit
  std::vector<const void *> raised;
  for (int ok : fcl_opt_kinds)
    for (int sc = 0; sc < 2; ++sc) {
      int rc = 0;
      fcl_each_kernel(fcl_kernels(p, ok, sc != 0), [&](const auto &k) {
        const void *fn = (const void *)k.fn;
        if (rc || !fn || k.lds <= 64 * 1024 || std::find(raised.begin(), raised.end(), fn) != raised.end()) return;
        raised.push_back(fn);
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) != hipSuccess)
          rc = fail("mz_fcl_create: %zu bytes of LDS per workgroup refused (%s)", k.lds, k.name.c_str());
      });
      if (rc) return bail(rc);
    }
  fcl_resolve(c);
  if (fcl_alloc(c, &c->flags, (size_t)p.nflags)) return bail(-1);
  if (hipHostMalloc((void **)&c->wedge_h, 64, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void **)&c->wedge_hd, c->wedge_h, 0) != hipSuccess)
    return bail(fail("mz_fcl_create: pinned error word refused"));
  *c->wedge_h = 0u;
  if (hipHostMalloc((void **)&c->done_h, FCL_SLOTS * 64, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void **)&c->done_hd, c->done_h, 0) != hipSuccess || fcl_alloc(c, &c->done_ctr, (size_t)16))
    return bail(fail("mz_fcl_create: pinned completion words refused"));
  memset(c->done_h, 0, FCL_SLOTS * 64);
  if (fcl_alloc(c, &c->stage_d, p.stage_bytes) || fcl_alloc(c, &c->err_d, (size_t)batch)) return bail(-1);
  for (int k = 0; k < c->nslots; ++k) {
    if (hipHostMalloc((void **)&c->stage_h[k], p.stage_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&c->err_h[k], (size_t)batch * 4, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev[k], hipEventDisableTiming) != hipSuccess)
      return bail(fail("mz_fcl_create: pinned staging of %zu bytes refused", p.stage_bytes));
  }
  *out = c;
  return 0;
}

int mz_fcl_destroy(mz_fcl *c) {
  if (!c) return 0;
  for (int k = 0; k < c->nslots; ++k) {
    if (c->ev[k]) (void)hipEventSynchronize(c->ev[k]);
    (void)fcl_wait_done_word(c, k);
  }
  fcl_release(c);
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
  fcl_resolve(c);
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
  fcl_resolve(c);
  fcl_drop_run_graphs(c);
  return 0;
}

int mz_fcl_set_symmetry(mz_fcl *c, int kind, uint64_t seed, uint32_t first_update) {
  if (!c) return fail("mz_fcl_set_symmetry: null argument");
  if (kind != 0 && sym_elements(kind) == 0) return fail("mz_fcl_set_symmetry: unknown kind %d (0 off, 1 TicTacToe, 3 Connect Four)", kind);
  if (kind != 0 && (c->plan.O != sym_cells(kind) || c->plan.A != sym_actions(kind)))
    return fail("mz_fcl_set_symmetry: %s has obs_dim %d and action_space %d, the handle was created with %d and %d",
                mz_game_info(kind).name, sym_cells(kind), sym_actions(kind), c->plan.O, c->plan.A);
  if (kind != 0 && !c->sym_d) {
    // ONE buffer for every update of the handle, however many mz_fcl_run keeps in flight: an update's symmetry kernel and the step
    // kernels that read its output are enqueued on the same stream, and so are the next update's, so the next image is written only
    // after every reader of this one has finished (stream order); the staging slots exist because the HOST writes them ahead
    FCL_ENTER(c);
    if (fcl_alloc(c, &c->sym_d, c->plan.soff[5])) return -1;
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
                actions_out, policies_out, elements_out, c->sym_seed, update, c->sym_kind, c->plan.batch, c->plan.K, actions_are_i32 ? 1 : 0};
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

extern "C++" {
// a batch as the step reads it, and the hyper-parameters of one update
struct FclBatch {
  const float *obs; const void *actions; const float *target_rewards, *target_values, *target_policies; const void *is_weights;
  int actions_are_i32, weights_are_f64;
};
struct FclHyper { double beta1, beta2, eps, weight_decay, clip_grad; int adamw; };
// the pinned word the step's LAST launch stores `seq` into when its last workgroup ends (k_fcl_dwa: the fused paths of batches up to
// 512); used says whether this step's structure does -- otherwise the caller records an event
struct FclDone { unsigned *flag; unsigned seq; bool used; };

// the six sections of a staging slot (mz_fcl_update's device copy, mz_fcl_run's pinned slots, the symmetry buffer) at `base`
static FclBatch fcl_batch_at(const mz_fcl *c, const char *base, int actions_are_i32, int weights_are_f64) {
  const size_t *o = c->plan.soff;
  return {(const float *)(base + o[0]), base + o[1], (const float *)(base + o[2]), (const float *)(base + o[3]), (const float *)(base + o[4]),
          base + o[5], actions_are_i32, weights_are_f64};
}

// one launch of the step; the arguments convert to the kernel's parameter types
template <class... P>
static int fcl_launch(const FclKernel<void (*)(P...)> &k, dim3 grid, unsigned threads, hipStream_t s, const std::common_type_t<P> &...args) {
  if (!k.fn) return fail("mz_fcl_step: a launch the handle's plan has no kernel for (internal)");
  void *argv[] = {(void *)&args...};
  const hipError_t e = hipLaunchKernel((const void *)k.fn, grid, dim3(threads), argv, k.lds, s);
  if (e != hipSuccess) return fail("mz_fcl_step: %s did not launch: %s", k.name.c_str(), hipGetErrorString(e));
  return 0;
}
#define FCL_LAUNCH(...) do { if (fcl_launch(__VA_ARGS__)) return -1; } while (0)

// lr: the device float the optimiser reads its rate from (null: the one bound by mz_fcl_bind); done: null, or the completion word
static int fcl_step(mz_fcl *c, FclBatch b, const FclHyper &hy, int no_update, float *new_errors, double *loss_sums, hipStream_t s,
                    const float *lr, FclDone *done) {
  if (!c || !b.obs || !b.actions || !b.target_rewards || !b.target_values || !b.target_policies || !b.is_weights || !new_errors || !loss_sums)
    return fail("mz_fcl_step: null argument");
  if (!c->P) return fail("mz_fcl_step: no parameters bound (mz_fcl_bind)");
  FCL_ENTER(c);
  const FclPlan &p = c->plan;
  const FclKernels &k = c->kern;
  if (c->sym_kind && !no_update) {
    // the batch's images into sym_d, ahead of the step on its stream; the step reads them in the batch's place
    const FclBatch img = fcl_batch_at(c, c->sym_d, b.actions_are_i32, b.weights_are_f64);
    SymBatch sb = {b.obs, b.actions, b.target_policies, (float *)img.obs, (void *)img.actions, (float *)img.target_policies, nullptr,
                   c->sym_seed, c->sym_update, c->sym_kind, p.batch, p.K, b.actions_are_i32 ? 1 : 0};
    if (fcl_symmetry_launch(sb, s)) return -1;
    c->sym_update += 1u;
    b.obs = img.obs; b.actions = img.actions; b.target_policies = img.target_policies;
  }
  FclView v = c->view;
  v.P = c->P; v.pk = c->pk;
  v.obs = b.obs; v.act = b.actions; v.act_i32 = b.actions_are_i32 ? 1 : 0; v.t_rew = b.target_rewards; v.t_val = b.target_values; v.t_pol = b.target_policies;
  v.w = b.is_weights; v.w_f64 = b.weights_are_f64 ? 1 : 0; v.new_errors = new_errors;
  const int K1 = p.K + 1;
  const bool clip = hy.clip_grad > 0.0;
  v.steps = c->steps; v.nsteps = no_update ? 0 : c->nsteps;
  v.sloss = c->scalar_loss;
  FclOpt o;
  o.beta1 = hy.beta1; o.beta2 = hy.beta2; o.eps = hy.eps; o.wd = hy.weight_decay; o.clip = (float)hy.clip_grad;
  o.adamw = hy.adamw ? 1 : 0; o.no_update = no_update ? 1 : 0;
  o.kind = c->opt_kind; o.mom = (float)c->opt_mom; o.alpha = (float)c->opt_alpha; o.alpha_c = (float)(1.0 - c->opt_alpha);
  o.eps_f = (float)hy.eps; o.wd_f = (float)hy.weight_decay;
  FclDw a;
  a.tapes = c->tapes; a.tape_bytes = p.tapes_fit ? (unsigned)(p.tape_floats * 4) : 0u; a.R = p.batch; a.S = p.S; a.part = c->part; a.nflat = c->nflat; a.grad = c->grad;
  a.fuse = (p.S == 1 && !clip && !no_update) ? 1 : 0;      // the update in the jobs' workgroups: k_fcl_dwa is the step's last launch
  a.P = c->P; a.pk = c->pk; a.posA = c->posA; a.posB = c->posB; a.m = c->m; a.vv = c->v; a.steps = c->steps; a.lr_p = lr ? lr : c->lr; a.o = o;
  if (*c->wedge_h) return fail("mz_fcl_step: a heads unit of an earlier step gave up waiting for its chain workgroups (k_fcl_fwd's bounded wait): "
                            "the device is wedged or oversubscribed; the handle's updates since then are void");
  unsigned *dflag = (done && a.fuse) ? done->flag : nullptr;
  if (done) done->used = dflag != nullptr;
  const unsigned seq = done ? done->seq : 0u;
  v.flags = c->flags; v.nflags = p.nflags; v.err = c->wedge_hd;
  const int tail = a.fuse ? 2 : 0;      // k_fcl_dwa's two more workgroups: the LayerNorm parameters and the loss sums
  if (p.fwd == FCL_FWD_FB) {
    // batch <= 256: TWO launches -- forward chain, heads and backward chain (k_fcl_fb); every weight-gradient job with the update in its
    // workgroup, the LayerNorm parameters and the loss sums (k_fcl_dwa)
    const int units = (p.batch / 16) * (3 * p.K - 1);      // (position K's units run in the chain workgroups)
    const int inl = p.fb_jobs ? p.njobs_heads : 0;           // the heads' jobs inside k_fcl_fb
    FCL_LAUNCH(k.fb, p.nwg + units + inl, FCL_THREADS, s, v, p.nwg, c->jobs, a);
    FCL_LAUNCH(k.dwa, p.njobs - inl + tail, FCL_THREADS, s, c->jobs + inl, p.njobs - inl, a, a.fuse, c->lnpart, p.nln, c->L.ln_w, v.lossb,
               b.is_weights, v.w_f64, p.batch, K1, loss_sums, p.njobs_heads - inl, c->flags, v.nflags, c->done_ctr, dflag, seq);
  } else if (p.fwd == FCL_FWD_FUSED) {
    FCL_LAUNCH(k.fwd, p.nwg + (p.batch / 16) * (3 * K1 - 1), FCL_THREADS, s, v, p.nwg);
  } else {
    FCL_LAUNCH(k.chain_fwd, p.nwg, FCL_THREADS, s, v);
    FCL_LAUNCH(k.heads, dim3(p.batch / 16, K1, 3), FCL_THREADS, s, v);
  }
  if (p.bwd == FCL_BWD_DW) {
    // batch <= 512: the heads' weight-gradient jobs run beside the backward chain in its launch, the chain's in the last one; every
    // job covers all unroll positions, so its strip is the gradient and (no clipping) the update follows in the same workgroup; the
    // last launch also carries the LayerNorm parameters and the loss sums
    const int nchain_jobs = p.njobs - p.njobs_heads;
    FCL_LAUNCH(k.bwd_dw, p.nwg + p.njobs_heads, FCL_THREADS, s, v, p.nwg, c->jobs, a);
    FCL_LAUNCH(k.dwa, nchain_jobs + tail, FCL_THREADS, s, c->jobs + p.njobs_heads, nchain_jobs, a, a.fuse, c->lnpart, p.nln, c->L.ln_w, v.lossb,
               b.is_weights, v.w_f64, p.batch, K1, loss_sums, 0, nullptr, 0, c->done_ctr, dflag, seq);
  } else if (p.bwd == FCL_BWD_SLABS) {
    // larger batches: the backward chain fills the chip by itself; every job x row slab is a workgroup of four waves, the
    // slabs' strips are added up by the optimiser kernel
    FCL_LAUNCH(k.chain_bwd, p.nwg, FCL_THREADS, s, v);
    FCL_LAUNCH(k.dwt, p.njobs * p.S + 1, 256, s, c->jobs, p.njobs, a, c->lnpart, p.nln, c->lngrad);
  }
  if (!a.fuse) {
    // (S > 1: the LayerNorm gradients were reduced by k_fcl_dwt's last workgroup -- lngrad, flagged by nwg = -1)
    const float *lnp = p.S > 1 ? c->lngrad : c->lnpart;
    const int lnn = p.S > 1 ? -1 : p.nln;
    if (clip) FCL_LAUNCH(k.grad, c->nblk, 256, s, c->part, p.S, lnp, lnn, c->L.ln_w, c->nflat, c->grad, c->bsq);
    FCL_LAUNCH(k.adam, c->nblk + 1, 256, s, c->P, c->pk, c->posA, c->posB, c->grad, clip ? nullptr : c->part, p.S, lnp, lnn, c->L.ln_w, c->bsq,
               c->nblk, c->m, c->v, c->steps, lr ? lr : c->lr, o, c->nflat, v.lossb, b.is_weights, v.w_f64, p.batch, K1, loss_sums);
  }
  HIPCHECK(hipGetLastError());
  return 0;
}
}  // extern "C++"

int mz_fcl_step(mz_fcl *c, const float *obs, const void *actions, int actions_are_i32, const float *target_rewards, const float *target_values,
                const float *target_policies, const void *is_weights, int weights_are_f64, double beta1, double beta2, double eps,
                double weight_decay, double clip_grad, int adamw, int no_update, float *new_errors, double *loss_sums, void *stream) {
  return fcl_step(c, {obs, actions, target_rewards, target_values, target_policies, is_weights, actions_are_i32, weights_are_f64},
                  {beta1, beta2, eps, weight_decay, clip_grad, adamw}, no_update, new_errors, loss_sums, (hipStream_t)stream, nullptr, nullptr);
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
  const FclPlan &p = c->plan;
  const int K1 = p.K + 1;
  const size_t bs = (size_t)p.batch;
  char *h = c->stage_h[k];
  memcpy(h + p.soff[0], obs, bs * p.O * 4);
  memcpy(h + p.soff[1], actions, bs * p.K * (actions_are_i32 ? 4 : 8));
  memcpy(h + p.soff[2], target_rewards, bs * K1 * 4);
  memcpy(h + p.soff[3], target_values, bs * K1 * 4);
  memcpy(h + p.soff[4], target_policies, bs * K1 * p.A * 4);
  memcpy(h + p.soff[5], is_weights, bs * (weights_are_f64 ? 8 : 4));
  hipStream_t s = (hipStream_t)stream;
  HIPCHECK(hipMemcpyAsync(c->stage_d, h, p.stage_bytes, hipMemcpyHostToDevice, s));
  if (fcl_step(c, fcl_batch_at(c, c->stage_d, actions_are_i32, weights_are_f64), {beta1, beta2, eps, weight_decay, clip_grad, adamw}, 0, c->err_d,
               loss_sums, s, nullptr, nullptr))
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
  memcpy(host_out, c->err_h[slot], (size_t)c->plan.batch * 4);
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
  const FclPlan &p = c->plan;
  const size_t bs = (size_t)p.batch;
  const FclHyper hy = {beta1, beta2, eps, weight_decay, clip_grad, adamw};
  // slot k's pinned staging as the device reads it, and its rate
  auto staged = [&](int k) { return fcl_batch_at(c, c->stage_hd[k], 1, 1); };
  auto staged_lr = [&](int k) { return lrs ? (const float *)(c->stage_hd[k] + p.soff_lr) : nullptr; };
  // MZ_FCL_RUN_GRAPH=1: the five launches of an update as one captured graph per slot.  Measured out (one box, A/B): kernels run
  // without gaps inside a graph, but consecutive graph launches start ~15 us apart -- 105 us per update against 96.5 us for the
  // five direct launches (8.4 k against 9.0 k updates/s); profiles/r05_kernel_experiments.txt
  static const bool use_graph = getenv("MZ_FCL_RUN_GRAPH") && getenv("MZ_FCL_RUN_GRAPH")[0] == '1';
  if (use_graph && c->sym_kind) return fail("mz_fcl_run: MZ_FCL_RUN_GRAPH=1 captures an update once and cannot carry the symmetry counter of mz_fcl_set_symmetry");
  const char *ev_env = getenv("MZ_FCL_RUN_EVENTS");      // (1: an event behind every update instead of the completion word; A/B and tests)
  const bool use_flag = !(ev_env && ev_env[0] == '1');
  // the captured update of each slot (rebuilt when a hyper-parameter or an address it holds changes)
  const double key[11] = {hy.beta1, hy.beta2, hy.eps, hy.weight_decay, hy.clip_grad, (double)(hy.adamw ? 1 : 0) + (lrs ? 2 : 0), (double)(uintptr_t)loss_sums,
                          (double)(uintptr_t)c->lr, (double)c->opt_kind, c->opt_mom, c->opt_alpha};
  if (memcmp(key, c->run_key, sizeof key)) { fcl_drop_run_graphs(c); memcpy(c->run_key, key, sizeof key); }
  if (!c->run_cap) HIPCHECK(hipStreamCreateWithFlags(&c->run_cap, hipStreamNonBlocking));
  for (int k = 0; k < c->nslots; ++k) {
    if (!c->stage_hd[k]) {
      HIPCHECK(hipHostGetDevicePointer((void **)&c->stage_hd[k], c->stage_h[k], 0));
      HIPCHECK(hipHostGetDevicePointer((void **)&c->err_hd[k], c->err_h[k], 0));
    }
    if (c->run_graph[k] || !use_graph) continue;
    hipGraph_t g = nullptr;
    HIPCHECK(hipStreamBeginCapture(c->run_cap, hipStreamCaptureModeThreadLocal));
    int rc = fcl_step(c, staged(k), hy, 0, c->err_hd[k], loss_sums, c->run_cap, staged_lr(k), nullptr);
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
    if (src->sample(src->replay, words ? words + 2 * bs * (size_t)i : nullptr, 1, (int)bs, (float *)(h + p.soff[0]), (int32_t *)(h + p.soff[1]),
                    (float *)(h + p.soff[2]), (float *)(h + p.soff[3]), (float *)(h + p.soff[4]), c->run_idx[k].data(),
                    (double *)(h + p.soff[5]), np_key, np_pos, beta_inout, &pads, py_key, py_pos))
      return fail("mz_fcl_run: sampling failed: %s", src->last_error ? src->last_error() : "?");
    pads_total += pads;
    if (obs_min && obs_range) {
      float *o = (float *)(h + p.soff[0]);
      for (size_t r = 0; r < bs; ++r)
        for (int j = 0; j < p.O; ++j) o[r * p.O + j] = (o[r * p.O + j] - obs_min[j]) / obs_range[j];
    }
    if (lrs) *(float *)(h + p.soff_lr) = lrs[i];
    const double t_l = now();
    c->run_stats[2] += t_l - t_s;
    FclDone done = {use_flag ? c->done_hd + 16 * k : nullptr, c->done_seq[k] + 1u, false};
    if (use_graph) {
      HIPCHECK(hipGraphLaunch(c->run_graph[k], s));    // the five launches, reading this slot's staging
    } else if (fcl_step(c, staged(k), hy, 0, c->err_hd[k], loss_sums, s, staged_lr(k), &done)) {
      return -1;
    }
    const bool by_flag = done.used;
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
  if (which < 0 || which >= FCL_NTAPES) return fail("mz_fcl_read_tape: tape %d", which);
  const size_t cnt = c->plan.tape[which].floats;
  if (!host_out) return (long long)cnt;
  if (n != cnt) return fail("mz_fcl_read_tape: tape %d has %zu floats (got %zu)", which, cnt, n);
  FCL_ENTER(c);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(host_out, c->view.*fcl_tape_of[which], n * sizeof(float), hipMemcpyDeviceToHost));
  return (long long)n;
}

extern "C++" {
// the record of mz_fcl_plan / mz_fcl_plan_host (include/mz_engine_debug.h), and the names fcl_kernels returns for (opt_kind, scalar_loss)
static int fcl_plan_record(const FclPlan &p, int opt_kind, int scalar_loss, long long *out, char *names, size_t names_cap) {
  if (std::find(fcl_opt_kinds, fcl_opt_kinds + 5, opt_kind) == fcl_opt_kinds + 5)
    return fail("mz_fcl_plan: optimiser kind %d (0 Adam, 1 SGD, 2 RMSprop; + 4 with a momentum buffer)", opt_kind);
  const long long rec[MZ_FCL_PLAN_FIELDS] = {p.G, p.S, p.nwg, p.nln, fcl_fuse_fwd(p), fcl_fuse_fb(p), p.fb_jobs, p.KP, (long long)p.lds_bytes,
                                             (long long)p.lds_bwd_dw, p.njobs, p.njobs_heads, (long long)p.stage_bytes, p.fwd, p.bwd, p.lds_dwa,
                                             p.cus, (long long)p.tape_floats, p.tapes_fit, p.nflags};
  memcpy(out, rec, sizeof rec);
  if (names) {
    std::string all;
    fcl_each_kernel(fcl_kernels(p, opt_kind, scalar_loss != 0), [&](const auto &k) { if (k.fn) all += k.name + "\n"; });
    if (all.size() + 1 > names_cap) return fail("mz_fcl_plan: %zu bytes of kernel names (room for %zu)", all.size() + 1, names_cap);
    memcpy(names, all.c_str(), all.size() + 1);
  }
  return 0;
}
}  // extern "C++"

int mz_fcl_plan_host(int batch, int unroll_steps, int obs_dim, int action_space, int value_bins, int reward_bins, int cus, const int *knobs5,
                     int opt_kind, int scalar_loss, long long *out, char *names, size_t names_cap) {
  if (!out || cus < 1) return fail("mz_fcl_plan_host: bad argument");
  if (fcl_refuse_shape(batch, unroll_steps, obs_dim, action_space, value_bins, reward_bins)) return -1;
  FclKnobs kn;
  if (knobs5) { kn.groups = knobs5[0]; kn.slabs = knobs5[1]; kn.fuse_fwd = knobs5[2]; kn.fuse_fb = knobs5[3]; kn.fb_jobs = knobs5[4]; }
  const FclPlan p = fcl_plan(batch, unroll_steps, obs_dim, action_space, value_bins, reward_bins, cus, kn);
  if (fcl_refuse_plan(p)) return -1;
  return fcl_plan_record(p, opt_kind, scalar_loss, out, names, names_cap);
}

int mz_fcl_plan(mz_fcl *c, int opt_kind, int scalar_loss, long long *out, char *names, size_t names_cap) {
  if (!c || !out) return fail("mz_fcl_plan: null argument");
  return fcl_plan_record(c->plan, opt_kind, scalar_loss, out, names, names_cap);
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
