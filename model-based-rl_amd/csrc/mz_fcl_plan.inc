// mz_fcl_plan.inc -- the shape of one FCNetwork learner step (mz_fcl.hip.h), decided in ONE pure function: which launches make the
// step, how many workgroups, how much LDS, how many weight-gradient jobs, where the tapes and the staging sections lie.  No HIP
// call, no getenv: mz_fcl_create (mz_fcl_abi.inc) reads the MZ_FCL_* knobs and the device's CU count once and hands them in; a
// stand-alone host program can include this file after mz_common.h and mz_fcl_sizes.h (tests/fcl_plan_host.cpp).  C++ linkage.

// forward: ONE launch with the backward chain (k_fcl_fb) / one launch (k_fcl_fwd) / the chain and the heads as launches of their own
enum FclFwd { FCL_FWD_FB = 0, FCL_FWD_FUSED = 1, FCL_FWD_CHAIN = 2 };
// backward: inside k_fcl_fb / k_fcl_bwd_dw + k_fcl_dwa (one row slab: the update in the jobs' workgroups) / k_fcl_chain_bwd4 + k_fcl_dwt
enum FclBwd { FCL_BWD_FB = 0, FCL_BWD_DW = 1, FCL_BWD_SLABS = 2 };

// kernel development knobs (MZ_FCL_GROUPS, MZ_FCL_SLABS: atoi of the variable; MZ_FCL_FUSE_FWD, MZ_FCL_FUSE_FB, MZ_FCL_FB_JOBS: 1 where its
// value starts with '1', else 0); -1: not set
struct FclKnobs { int groups = -1, slabs = -1, fuse_fwd = -1, fuse_fb = -1, fb_jobs = -1; };

struct FclTape { const char *name; size_t floats, off; };      // off: floats from the start of the tapes' allocation
// the tapes in the order of FclPlan::tape (and of mz_fcl_read_tape's `which`); layouts in mz_fcl.hip.h
enum { FCL_T_XIN, FCL_T_A1C, FCL_T_XHAT, FCL_T_RSTD, FCL_T_H, FCL_T_D2C, FCL_T_D1C, FCL_T_A1H, FCL_T_D2H, FCL_T_D1H, FCL_T_DH, FCL_T_LOSSB, FCL_NTAPES };
#define FCL_LDS_MAX (160 * 1024)

struct FclPlan {
  int batch, K, O, A, Sv, Sr, cus;
  int KD, KP;            // the transition's input features, and as the chain kernels are instantiated (56 / 64)
  int XR, xq;            // the input tile's rows on tape, the input features the chain kernels hold in LDS
  int G;                 // groups of four samples per chain workgroup (2 from batch 2048, 4 from 4096: more than one chain workgroup per CU otherwise)
  int S;                 // row slabs per weight-gradient job (1 up to batch 512: the fused dW + update path)
  int nwg, nln;          // chain workgroups; rows of lnpart: batch / 4 (one per group)
  FclFwd fwd;
  FclBwd bwd;
  bool fb_jobs;          // the heads' jobs inside k_fcl_fb (MZ_FCL_FB_JOBS=0: in the last launch, A/B)
  size_t lds_bytes, lds_bwd_dw;      // dynamic LDS of the chain kernels, of k_fcl_bwd_dw
  int lds_dwa;                       // ... of k_fcl_dwa
  int njobs, njobs_heads;            // weight-gradient jobs; [0, njobs_heads) read only what the heads wrote
  int nflags;                        // arrival / finished-unit counters
  FclTape tape[FCL_NTAPES];
  size_t tape_floats;                // the allocation
  bool tapes_fit;                    // (buffer descriptors address 2 GB: larger tapes never take the one-launch path)
  size_t soff[6], soff_lr, stage_bytes;      // a staging slot: obs, actions, target rewards / values / policies, weights; the update's rate
};

static bool fcl_fuse_fwd(const FclPlan &p) { return p.fwd != FCL_FWD_CHAIN; }
static bool fcl_fuse_fb(const FclPlan &p) { return p.fwd == FCL_FWD_FB; }
static bool fcl_plan_fits(const FclPlan &p) { return p.lds_bytes <= FCL_LDS_MAX; }

// tiles of one layer's dW (M outputs x N inputs): batch <= 512 (one slab, fused with the update): many small jobs -- the heads' layers
// as 16 x 64 strips (beside the backward chain), the chain's layers as 16 x 32 (the last launch, alone on the chip); larger batches:
// 16 na x 64 with na = 4 / 2 / 1 by the layer's output rows (k_fcl_dwt)
struct FclTiles { int na, ni, tm, ng; };
static FclTiles fcl_tiles(int S, bool chain, int M, int N) {
  FclTiles t;
  t.na = S == 1 ? 1 : (M > 32 ? 4 : (M > 16 ? 2 : 1));
  t.ni = (S == 1 && chain) ? 2 : 4;
  t.tm = (M + 16 * t.na - 1) / (16 * t.na);
  t.ng = (N + 16 * t.ni - 1) / (16 * t.ni);
  return t;
}

static FclPlan fcl_plan(int batch, int unroll_steps, int obs_dim, int action_space, int Sv, int Sr, int cus, const FclKnobs &kn) {
  FclPlan p;
  p.batch = batch; p.K = unroll_steps; p.O = obs_dim; p.A = action_space; p.Sv = Sv; p.Sr = Sr; p.cus = cus;
  const int K1 = unroll_steps + 1, R = batch;
  p.KD = MZ_H + action_space;
  p.KP = p.KD <= 56 ? 56 : 64;
  p.XR = 64 * ((obs_dim + 63) / 64);
  p.xq = obs_dim > 64 ? ((obs_dim + 3) & ~3) : 64;
  p.G = batch / 4 >= 4 * cus ? 4 : (batch / 4 >= 2 * cus ? 2 : 1);
  if ((kn.groups == 1 || kn.groups == 2 || kn.groups == 4) && batch % (4 * kn.groups) == 0) p.G = kn.groups;
  while (batch % (4 * p.G)) p.G >>= 1;
  // row slabs: 1 up to batch 512 (its backward launch carries the chain as ONE group per workgroup), else batch / 128 up to 16
  p.S = batch <= 512 ? 1 : (batch / 128 < 16 ? batch / 128 : 16);      // (16 slabs of >= 8 row chunks: 1280 workgroups; measured against 8 / 32 / 64 at batch 2048 and 4096)
  if (kn.slabs >= 1 && kn.slabs <= batch / 16) p.S = kn.slabs;      // (> 1 = the unfused path)
  if (p.S == 1) p.G = 1;
  p.nwg = batch / (4 * p.G);
  p.nln = batch / 4;
  p.lds_bytes = (size_t)FCL_LDS4_FLOATS(p.xq, p.G) * 4;
  p.lds_bwd_dw = p.lds_bytes > (size_t)FCL_DW_LDS(FCL_NW, 1, 4) ? p.lds_bytes : (size_t)FCL_DW_LDS(FCL_NW, 1, 4);
  p.lds_dwa = FCL_DW_LDS(FCL_NW, 1, 4) > 3 * 256 * 8 ? FCL_DW_LDS(FCL_NW, 1, 4) : 3 * 256 * 8;
  p.nflags = 2 * (batch / 16) * K1 + 192;
  // tapes
  const size_t KR = (size_t)K1 * R;
  const FclTape tapes[FCL_NTAPES] = {{"xin", KR * p.XR, 0}, {"a1c", KR * 512, 0}, {"xhat", KR * 64, 0}, {"rstd", KR, 0}, {"h", KR * 64, 0},
                                     {"d2c", KR * 64, 0}, {"d1c", KR * 512, 0}, {"a1h", 3 * KR * 512, 0}, {"d2h", 3 * KR * 64, 0},
                                     {"d1h", 3 * KR * 512, 0}, {"dH", 3 * KR * 64, 0}, {"lossb", 3 * KR, 0}};
  p.tape_floats = 0;
  for (int i = 0; i < FCL_NTAPES; ++i) {
    p.tape[i] = tapes[i];
    p.tape[i].off = p.tape_floats;
    p.tape_floats += (tapes[i].floats + 15) & ~(size_t)15;
  }
  p.tapes_fit = p.tape_floats * 4 <= 0x7fffffffull;
  // the fused forward launch: where the chain leaves at least half of the chip idle (batch <= 512 on 256 CUs: 107 against 115 us per
  // update at batch 512) and its LDS fits beside the heads' (MZ_FCL_FUSE_FWD=0 / 1: off / on at any batch up to 1024, kernel
  // development); with the backward chain in the same launch (k_fcl_fb) up to batch 256 (at 512 the units' share of the chip is too
  // small for it: 110.5 us)
  const bool one_group = p.S == 1 && p.G == 1 && p.lds_bytes <= (size_t)FCL_LDS_HEADS * 4;
  bool fuse_fwd = one_group && batch <= 512 && cus >= 2 * p.nwg;
  if (kn.fuse_fwd >= 0) fuse_fwd = kn.fuse_fwd == 1 && one_group && cus >= p.nwg;
  bool fuse_fb = fuse_fwd && batch <= 256 && cus >= 2 * p.nwg && p.tapes_fit;      // (every chain workgroup resident beside the units it waits for)
  if (kn.fuse_fb >= 0) fuse_fb = fuse_fb && kn.fuse_fb == 1;      // (0: the three-launch step, A/B)
  p.fb_jobs = kn.fb_jobs >= 0 ? kn.fb_jobs == 1 : true;
  p.fwd = fuse_fb ? FCL_FWD_FB : (fuse_fwd ? FCL_FWD_FUSED : FCL_FWD_CHAIN);
  p.bwd = fuse_fb ? FCL_BWD_FB : (p.S == 1 ? FCL_BWD_DW : FCL_BWD_SLABS);
  // weight-gradient jobs: one per tile of the ten layers' dW; the heads' six layers first
  const int layers[10][3] = {{MZ_F, obs_dim, 1}, {MZ_H, MZ_F, 1}, {MZ_F, p.KD, 1}, {MZ_H, MZ_F, 1}, {MZ_F, p.KD, 0}, {Sr, MZ_F, 0},
                             {MZ_F, MZ_H, 0}, {Sv, MZ_F, 0}, {MZ_F, MZ_H, 0}, {action_space, MZ_F, 0}};
  p.njobs = p.njobs_heads = 0;
  for (const auto &l : layers) {
    const FclTiles t = fcl_tiles(p.S, l[2] != 0, l[0], l[1]);
    p.njobs += t.tm * t.ng;
    if (!l[2]) p.njobs_heads += t.tm * t.ng;
  }
  // a staging slot
  const size_t sz[6] = {(size_t)batch * obs_dim * 4, (size_t)batch * unroll_steps * 8, (size_t)batch * K1 * 4, (size_t)batch * K1 * 4,
                        (size_t)batch * K1 * action_space * 4, (size_t)batch * 8};
  size_t o = 0;
  for (int i = 0; i < 6; ++i) { p.soff[i] = o; o += (sz[i] + 15) & ~(size_t)15; }
  p.soff_lr = o;                          // (mz_fcl_run: the update's learning rate, one float)
  p.stage_bytes = o + 16;
  return p;
}
