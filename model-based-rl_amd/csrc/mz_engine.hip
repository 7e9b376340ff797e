// mz_engine.hip -- host side of libmz_hip.so: the C ABI of include/mz_engine.h over the gfx950
// kernels in mz_tree.hip.h / mz_net.hip.h / mz_selfplay.hip.h.  No torch types, no CPU fallback:
// every entry point launches HIP kernels on the stream it is given.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mz_engine.h"
#include "../../include/mz_engine_debug.h"      // instrumentation / test hooks (not the boundary)

#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS
#include "mz_common.h"
#include "mz_net.hip.h"
#include "mz_rng.h"
#include "mz_tree.hip.h"
#include "mz_selfplay.hip.h"
#include "mz_selfplay_ring.inc"   // MZ_GRAPH_MOVES, RecordRing
#include "mz_selfplay_mode.inc"   // MzSpMode, mz_sp_refusal, mz_sp_switch_ok
#include "mz_fused.hip.h"
#include "mz_root.hip.h"
#include "mz_fused_h2.hip.h"
#include "mz_learner.hip.h"
#include "mz_fcl.hip.h"
#include "mz_fcl_plan.inc"
#include "mz_pack.inc"            // FlatLayout, pack_plan
#include "mz_eval.hip.h"
#include "mz_eval_env.hip.h"
#include "mz_match.hip.h"
#include "mz_reanalyse.hip.h"
#include "mz_playout.hip.h"
#include "mz_solve.hip.h"
#include "mz_unroll.hip.h"
#include "mz_symmetry.hip.h"
#include "mz_truemodel.hip.h"
#include "mz_gumbel.hip.h"
#include "mz_gumbel_selfplay.hip.h"
// the search kernels are compiled in their own translation units, one per shape (mz_inst.hip); here they are declared,
// tabled and launched -- all three from the lists of mz_kernels.inc
#include "mz_kernels.inc"
#define MZ_KF(S, ...) extern template __global__ void k_search_fused<MZ_UNPACK S, __VA_ARGS__> MZ_KARGS;
#define MZ_KG MZ_KF
#define MZ_KH(S, ...) extern template __global__ void k_search_h2<MZ_UNPACK S, __VA_ARGS__> MZ_KARGS;
MZ_ALL_KERNELS
#undef MZ_KF
#undef MZ_KG
#undef MZ_KH

// a row of the shape lists (k_search_h2: ks1 = jtp = 0); an engine runs the first row with amax >= its action count
struct SearchShape { int amax, ks1, jtp, g; };
#define MZ_ROW_F(AMAX, KS1, JTP, G) {AMAX, KS1, JTP, G},
#define MZ_ROW_H(AMAX, G) {AMAX, 0, 0, G},
static constexpr SearchShape g_fused_shapes[] = {MZ_FUSED_ROWS(MZ_ROW_F)};
static constexpr SearchShape g_h2_shapes[] = {MZ_H2_ROWS(MZ_ROW_H)};
static_assert(g_fused_shapes[sizeof g_fused_shapes / sizeof *g_fused_shapes - 1].amax == MZ_MAX_ACTIONS &&
              g_h2_shapes[sizeof g_h2_shapes / sizeof *g_h2_shapes - 1].amax == MZ_H2_MAXA, "the last row covers every action count");
template <size_t N>
static const SearchShape *shape_for(const SearchShape (&rows)[N], int A) {
  for (const SearchShape &r : rows) if (A <= r.amax) return &r;
  return nullptr;
}

// every compiled search kernel: its address beside the template arguments it was instantiated with (kind 1
// k_search_fused, 2 k_search_h2).  Kernels are found by those arguments, never by position.
struct SearchKernel { int kind; SearchShape shape; int lt; bool prof, sp, head, game; const void *fn; };
#define MZ_KF(S, LT, PROF, SP, HEAD) {1, {0, MZ_UNPACK S}, LT, PROF, SP, HEAD, false, (const void *)k_search_fused<MZ_UNPACK S, LT, PROF, SP, HEAD>},
#define MZ_KG(S, LT, PROF, SP, HEAD, GAME) {1, {0, MZ_UNPACK S}, LT, PROF, SP, HEAD, GAME, (const void *)k_search_fused<MZ_UNPACK S, LT, PROF, SP, HEAD, GAME>},
#define MZ_KH(S, LT, PROF, SP, HEAD) {2, {0, 0, 0, MZ_UNPACK S}, LT, PROF, SP, HEAD, false, (const void *)k_search_h2<MZ_UNPACK S, LT, PROF, SP, HEAD>},
static const SearchKernel g_search_kernels[] = {MZ_ALL_KERNELS};
static const void *find_kernel(int kind, const SearchShape &sh, int lt, bool prof, bool sp, bool head, bool game) {
  for (const SearchKernel &k : g_search_kernels)
    if (k.kind == kind && k.shape.ks1 == sh.ks1 && k.shape.jtp == sh.jtp && k.shape.g == sh.g && k.lt == lt &&
        k.prof == prof && k.sp == sp && k.head == head && k.game == game)
      return k.fn;
  return nullptr;
}

static thread_local std::string g_err;

static int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

#define HIPCHECK(x)                                                                        \
  do {                                                                                     \
    hipError_t err_ = (x);                                                                 \
    if (err_ != hipSuccess) return fail("%s: %s (%s:%d)", #x, hipGetErrorString(err_), __FILE__, __LINE__); \
  } while (0)

struct mz_engine {
  mz_config cfg;
  int device = 0;                   // HIP device the engine's pools live on (the current device at mz_create)
  int B, Bp, A, O, sims, NN, PL, G, jtp;
  int NS = 0;                       // records per tree slab of the node pool
  MzNode *nodes = nullptr;          // the node pool [Bp][NS]
  TreeView tv;
  NetView nv;
  std::vector<void *> allocs;
  float *flat_dev = nullptr;
  int32_t *pack_idx = nullptr;
  int32_t *pack_idx2 = nullptr;     // a second source element per packed weight (-1: none), added before scaling
  float *packed = nullptr;
  size_t n_flat = 0, n_packed = 0;
  bool weights_set = false;
  int sims_done = 0;
  bool selection_valid = false;
  bool root_ready = false;
  hipStream_t cap_stream = nullptr;
  hipGraphExec_t search_graph = nullptr;
  int search_graph_sims = 0;
  bool use_graph = true;
  SelfplayState sp;
  hipGraphExec_t move_graph[MZ_GRAPH_MOVES + 1] = {};   // [k] = hipGraph of k consecutive self-play moves
  const f32x4 *wstream = nullptr;   // per-wave cyclic weight stream for the fused search kernel
  const f32x4 *istream = nullptr;   // per-wave weight stream of the root kernel (initial inference)
  int nst0 = 0;                     // its run-time first-stage steps (obs_dim + 1 columns, two k-steps per step)
  const SearchShape *shape = nullptr, *shape_h2 = nullptr;   // this A's rows of the shape lists (shape_h2: split_f16 only)
  bool use_fused = true;
  bool use_lds_trees = true;
  bool use_lds_hybrid = true;
  std::vector<const void *> lds_attr_done;   // kernels whose hipFuncAttributeMaxDynamicSharedMemorySize is set (per device: once per engine)
  bool use_persist = true;          // self-play loop: whole moves inside ONE launch of the search kernel (its HEAD instantiation)
  // the experience ring's counters and the drains that read it (mz_selfplay_ring.inc; its tokens are hipEvent_t).  Of sp the
  // kernels read ring, ring_moves and rec_floats; sp.moves_host, sp.drained and sp.host_ring are unused (the layout stays)
  RecordRing ring;
  double prof_spread[3] = {0, 0, 0};   // mean / min / max over workgroups of the last phase profile's total cycles
  bool split_f16 = false;           // FCNetwork GEMMs as float16 high/low splits (mz_fused_h2.hip.h)
  int32_t *pack_idx_h2 = nullptr;   // gather table of the split-f16 weight stream (bit 30: low part)
  uint16_t *packed_h2 = nullptr;    // [4 waves][NGROUPS][8 pieces][64 lanes][8] float16
  size_t n_packed_h2 = 0;
  float *obs_norm = nullptr;        // [2][O] --norm_obs minimum and range (device)
  double *noise_log = nullptr;      // [ring_moves][B][A] per-move Dirichlet draws (mz_selfplay_noise_log), allocated on first use
  FlatLayout layout;
  float relu_scale_host[4] = {1.f, 1.f, 1.f, 0.f};
  bool scale_host_valid = true;     // relu_scale_host mirrors relu_scale_dev (not after mz_set_weights_async: read back on demand)
  float *wstage[2] = {nullptr, nullptr};      // pinned staging of mz_set_weights_async's host source, used alternately
  hipEvent_t wstage_ev[2] = {nullptr, nullptr};
  int wstage_next = 0;
  bool stream_scaled = false;       // the last weight set admitted a scale: the fused search kernels may run
  float *relu_scale_dev = nullptr;     // {1, 2^-k, 2^k, flag} of the current weight set (k_relu_scale)
  unsigned *relu_bound_dev = nullptr;  // k_relu_bound's two maxima
  bool root_hidden_external = false;  // the root's hidden state came in through mz_root_load: no bound on it is known
  unsigned *absmax_dev = nullptr;   // scratch of the split_f16 weight-range check (mz_set_weights)
  double *draw_uniform = nullptr;   // [B] host-given uniforms of a game environment's parity run (mz_selfplay_set_draws)
  bool draws_noise = false, draws_set = false;
  std::vector<float> obs_norm_host;
  float *eval_rows = nullptr;       // mz_eval_lookahead's scratch [B*A][50 + A + 2] (hidden, logits, reward, value), first use
  EvalState ev;                     // evaluation games on the device environments (mz_eval_env_*; mz_eval_env.hip.h)
  unsigned long long ev_moves = 0;  // moves enqueued since mz_eval_env_reset: keys the device draws, indexes the given ones
  double ev_temp = 0.0;             // the temperature es.temp holds
  bool ev_temp_set = false;
  ReanalyseState ra = {};           // Reanalyse of stored replay rows (mz_reanalyse; mz_reanalyse.hip.h), allocated on first use
  PlayoutState po = {};             // the playout-search opponent (mz_playout_plan, mz_eval_env_set_opponent; mz_playout.hip.h), allocated on first use
  SolveState sv = {};               // the exact game solver (mz_solve; mz_solve.hip.h), allocated on first use
  SolveTableState svt = {};         // its table search's tables and counters (mz_solve_tt), allocated on its first use
  UnrollState ur = {};              // the unroll diagnostic (mz_unroll; mz_unroll.hip.h), allocated on first use
  TmState tm = {};                  // the true-rules search (mz_set_true_model, mz_tm_*; mz_truemodel.hip.h), allocated when set
  GzState gz = {};                  // the Gumbel search (mz_set_gumbel, mz_gz_*; mz_gumbel.hip.h), allocated when set
  bool root_noise = false;          // the last mz_root_prepare mixed exploration noise into the root's priors
  MzSpMode sp_mode = MZ_SP_PUCT;    // how the self-play loop's moves are searched (mz_selfplay_mode.inc; DESIGN s7l)
  int sp_gumbel_value = 0;          // MZ_SP_GUMBEL: the records' root_value, 0 the root's mean value, 1 its v_mix
  bool sp_tm_fused = false;         // MZ_SP_TRUE_RULES: all simulations of a move in one launch of k_tm_search (else the two-launch loop)
};

// Every ABI entry runs on the engine's own device, whatever the calling thread's current device is (an engine may be
// driven from a worker thread: rayshim actors, a replay/drain thread).
// every entry runs on the handle's own device and leaves the calling thread's current device as it found it
struct MzDeviceGuard {
  int prev = -1;
  bool switched = false;
  int enter(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) {
      if (hipSetDevice(device) != hipSuccess) return -1;
      switched = true;
    }
    return 0;
  }
  ~MzDeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};
#define MZ_ENTER(e)                                                                          \
  MzDeviceGuard mz_guard_;                                                                   \
  if (mz_guard_.enter((e)->device)) return fail("hipSetDevice(%d) failed", (e)->device)

__global__ void k_store_double(double *dst, double v) { *dst = v; }

// what mz_select hands back, in one launch: any of the four outputs may be null
__global__ void k_export_selection(TreeView t, int32_t *leaf, int32_t *slot, int32_t *act, int32_t *depth) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  if (leaf) leaf[b] = t.leaf[b];
  if (slot) slot[b] = t.slot[b];
  if (act) act[b] = t.act[b];
  if (depth) depth[b] = t.depth[b];
}

// y = relu(y * scale[c] + shift[c] (+ residual)) in place over an NCHW float32 tensor, HW a multiple of 4: one 16-byte
// access per thread and operand (a float4 never straddles a channel), grid-stride.  HBM-bound: 2 or 3 tensor passes.
template <bool RES>
__global__ __launch_bounds__(256) void k_affine_relu(float4 *__restrict__ y, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, const float4 *__restrict__ res,
                                                      size_t n4, int C, int hw4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int c = (int)((i / (size_t)hw4) % (size_t)C);
    const float a = scale[c], b = shift[c];
    float4 v = y[i];
    v.x = v.x * a + b; v.y = v.y * a + b; v.z = v.z * a + b; v.w = v.w * a + b;
    if constexpr (RES) { const float4 r = res[i]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    y[i] = v;
  }
}

// the fused search kernels (mz_fused.hip.h, mz_fused_h2.hip.h) can run: trees fit their path buffer, and the exact-f32
// kernel's weight stream could be scaled for its clamp ReLU (mz_set_weights; the split-f16 kernel has its own stream)
static inline bool fused_usable(const mz_engine *e) {
  return e->use_fused && e->sims + 2 <= MZ_FUSED_MAXPL && (e->split_f16 || e->stream_scaled || !e->weights_set);
}

// captured graphs hold kernel arguments and the launches of one kernel set: whatever changes either drops them
static void drop_graphs(mz_engine *e, bool also_search) {
  if (also_search && e->search_graph) { hipGraphExecDestroy(e->search_graph); e->search_graph = nullptr; }
  for (auto &g : e->move_graph) if (g) { hipGraphExecDestroy(g); g = nullptr; }
}

template <typename T>
static int dmalloc(mz_engine *e, T **p, size_t n) {
  void *q = nullptr;
  HIPCHECK(hipMalloc(&q, n * sizeof(T) + 64));
  HIPCHECK(hipMemset(q, 0, n * sizeof(T) + 64));
  e->allocs.push_back(q);
  *p = (T *)q;
  return 0;
}

// ---------------------------------------------------------------- weight layout (mz_pack.inc)

// the split-f16 weight stream (mz_fused_h2.hip.h) from its gather table: bit 30 of an index asks for the low part
__global__ void k_pack_weights_h2(const float *flat, const int32_t *idx, _Float16 *packed, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t s = idx[i];
  float v = 0.f;
  if (s >= 0) v = flat[s & 0x3fffffff];
  const _Float16 h = (_Float16)v;                                  // round to nearest
  packed[i] = (s >= 0 && (s & 0x40000000)) ? (_Float16)(v - (float)h) : h;
}

// max |w| over the flat weights, or +inf if any is not finite (bit pattern compare: non-negative floats order like uints)
__global__ void k_absmax(const float *w, size_t n, unsigned *out) {
  unsigned m = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned u = __float_as_uint(w[i]) & 0x7fffffffu;
    m = u > m ? u : m;
  }
  atomicMax(out, m);
}

// The power of two the search kernel's weight stream is scaled by (mz_fused.hip.h, "ReLU as a clamp"): 2^k above an upper
// bound of every output of the four 512-wide fc1 layers the search runs (reward, transition: input [hidden | one-hot];
// value, policy: input hidden), given that the hidden state is relu(LayerNorm(.)) -- |(x_i - mean) / std| <= sqrt(49)
// for 50 features, so 0 <= hidden_i <= 7 |gamma_i| + |beta_i| -- and a one-hot row holds a single 1:
//   |out_n| <= sum_i |W[n][i]| hb_i + max_a |W[n][50 + a]| + |b_n|       (every partial sum obeys the same bound).
// k_relu_bound: 64 workgroups, 8 lanes per fc1 row; the largest row bound and the largest |w| of the layers that consume
// the activations (they are multiplied by 2^k) land in mx[0], mx[1] as bit patterns (non-negative floats order like
// unsigned integers, and every NaN pattern lies above +inf: a NaN sticks).
__global__ void k_relu_bound(const float *flat, FlatLayout L, int A, int Sr, int Sv, unsigned *mx) {
  __shared__ float hb[MZ_H];
  const int tid = threadIdx.x;
  if (tid < MZ_H) hb[tid] = 7.01f * fabsf(flat[L.ln_w + tid]) + fabsf(flat[L.ln_b + tid]);
  __syncthreads();
  const size_t w1[4] = {L.rew_w1, L.tr_w1, L.val_w1, L.pol_w1}, b1[4] = {L.rew_b1, L.tr_b1, L.val_b1, L.pol_b1};
  const int row = blockIdx.x * 32 + (tid >> 3), q = tid & 7;       // 2048 rows = 4 heads x 512
  const int h = row >> 9, n = row & 511;
  const int K = h < 2 ? MZ_H + A : MZ_H;
  const float *r = flat + w1[h] + (size_t)n * K;
  float s = 0.f, oh = 0.f;
  for (int i = q; i < MZ_H; i += 8) s += fabsf(r[i]) * hb[i];
  for (int a = MZ_H + q; a < K; a += 8) oh = fmaxf(oh, fabsf(r[a]));
  unsigned nanbit = (s != s || oh != oh) ? 1u : 0u;
  for (int o = 1; o < 8; o <<= 1) {
    s += __shfl_xor(s, o); oh = fmaxf(oh, __shfl_xor(oh, o)); nanbit |= __shfl_xor(nanbit, o);
  }
  s += oh + fabsf(flat[b1[h] + n]);
  unsigned m = __float_as_uint(s) & 0x7fffffffu;
  if (nanbit) m = 0x7fc00000u;
  // largest |w| of the consuming layers, grid-strided
  const size_t w2[4] = {L.rew_w2, L.tr_w2, L.val_w2, L.pol_w2};
  const int J[4] = {Sr, MZ_H, Sv, A};
  unsigned m2 = 0;
  for (int hh = 0; hh < 4; ++hh)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + tid; i < (size_t)J[hh] * MZ_F; i += (size_t)gridDim.x * blockDim.x) {
      const unsigned u = __float_as_uint(flat[w2[hh] + i]) & 0x7fffffffu;
      m2 = u > m2 ? u : m2;
    }
  __shared__ unsigned red[2];
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  if (q == 0) atomicMax(&red[0], m);
  atomicMax(&red[1], m2);
  __syncthreads();
  if (tid < 2) atomicMax(&mx[tid], red[tid]);
}

// scale = {1, 2^-k, 2^k, 1}; {1, 1, 1, 0} when the bound is not finite, k would exceed 40, or 2^k times the largest
// weight of a consuming layer would leave the float32 range: the host then routes the engine to the stand-alone kernels.
// force < 0: decided here; force = 0 / 1: the HOST's decision (mz_weights_scale_ok on a host copy of the same weights,
// mz_set_weights_async) -- its limits are tighter than the ones below, so a 1 it hands over is one this kernel agrees with;
// should it ever not, scale[3] = NaN poisons the packed stream (k_pack_weights multiplies by it): every value the search
// computes is NaN, loudly, instead of a clamp applied to an unscaled stream.
__global__ void k_relu_scale(const unsigned *mx, float *scale, int force) {
  const float bound = __uint_as_float(mx[0]) * 1.01f;     // (rounding of the sums above and of the kernel's own accumulation)
  const float w2max = __uint_as_float(mx[1]);
  int k = 0;
  if (bound > 1.f) (void)frexpf(bound, &k);               // bound = f 2^k, 0.5 <= f < 1: bound < 2^k
  const bool own = bound == bound && bound < 0x1p40f && w2max == w2max && w2max < ldexpf(1.f, 100 - k);
  const bool ok = own && force != 0;
  if (force > 0 && !own) {
    scale[0] = scale[1] = scale[2] = scale[3] = __uint_as_float(0x7fc00000u);
    return;
  }
#ifdef MZ_RELU_VMAX
  k = 0;
#endif
  scale[0] = 1.f;
  scale[1] = ok ? ldexpf(1.f, -k) : 1.f;
  scale[2] = ok ? ldexpf(1.f, k) : 1.f;
  scale[3] = ok ? 1.f : 0.f;
}

// the shape an engine's tables are built for
static PackShape pack_shape(const mz_config &cfg, const SearchShape &row, bool split_f16) {
  const int Sv = cfg.no_support ? 1 : cfg.value_support_max - cfg.value_support_min + 1;   // networks.py:135-136
  const int Sr = cfg.no_support ? 1 : cfg.reward_support_max - cfg.reward_support_min + 1;
  return PackShape{cfg.obs_dim, cfg.action_space, Sv, Sr, row.ks1, row.jtp, row.g, split_f16};
}

static int build_packing(mz_engine *e) {
  const PackShape sh = pack_shape(e->cfg, *e->shape, e->split_f16);
  PackPlan p;
  std::string err;
  if (pack_plan(sh, p, err)) return fail("%s", err.c_str());
  e->layout = p.L;
  e->n_flat = p.L.total;
  e->n_packed = p.n_packed;
  e->n_packed_h2 = p.n_packed_h2;
  if (dmalloc(e, &e->pack_idx, p.n_packed)) return -1;
  if (dmalloc(e, &e->pack_idx2, p.n_packed)) return -1;
  if (dmalloc(e, &e->packed, p.n_packed)) return -1;
  if (dmalloc(e, &e->relu_scale_dev, (size_t)4)) return -1;
  if (dmalloc(e, &e->relu_bound_dev, (size_t)2)) return -1;
  if (dmalloc(e, &e->flat_dev, p.L.total)) return -1;
  HIPCHECK(hipMemcpy(e->pack_idx, p.idx.data(), p.n_packed * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(e->pack_idx2, p.idx2.data(), p.n_packed * sizeof(int32_t), hipMemcpyHostToDevice));
  if (e->split_f16) {
    if (dmalloc(e, &e->pack_idx_h2, p.n_packed_h2)) return -1;
    if (dmalloc(e, &e->packed_h2, p.n_packed_h2)) return -1;
    HIPCHECK(hipMemcpy(e->pack_idx_h2, p.idx_h2.data(), p.n_packed_h2 * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  NetView &n = e->nv;
  const float *P = e->packed;
  n.w0o = (const f32x4 *)(P + p.w0o); n.b0o = P + p.b0o;
  n.w1 = (const f32x4 *)(P + p.w1); n.b1 = (const f32x4 *)(P + p.b1); n.w2 = (const f32x4 *)(P + p.w2); n.b2 = P + p.b2;
  n.w3 = (const f32x4 *)(P + p.w3); n.b3 = (const f32x4 *)(P + p.b3); n.w4 = (const f32x4 *)(P + p.w4); n.b4 = P + p.b4;
  n.lnw = P + p.lnw; n.lnb = P + p.lnb;
  e->wstream = (const f32x4 *)(P + p.ws);
  e->istream = (const f32x4 *)(P + p.is);
  e->nst0 = p.nst0;
  n.ks0 = p.ks0; n.ks1 = p.ks1; n.ks3 = p.ks3; n.O = sh.O; n.A = sh.A; n.jtp = sh.jtp;
  n.Sr = sh.Sr; n.Sv = sh.Sv;
  n.rmin = e->cfg.no_support ? 0 : e->cfg.reward_support_min;   // (0: mz_support_to_scalar_q adds the raw output to it)
  n.vmin = e->cfg.no_support ? 0 : e->cfg.value_support_min;
  n.no_transform = e->cfg.no_support ? 2 : (e->cfg.no_target_transform ? 1 : 0);
  return 0;
}

// What every weight set enqueues on s, from the flat weights at src [dev]: the power of two the search kernel's stream is scaled by (its
// ReLU is a [0, 1] clamp, mz_fused.hip.h) from a bound of this weight set's activations, then the packed vector and, for a split-f16
// engine, its stream.  force: k_relu_scale's (< 0 the device decides, 0 / 1 the caller has)
static int enqueue_pack(mz_engine *e, const float *src, int force, hipStream_t s) {
  const int threads = 256;
  const unsigned blocks = (unsigned)((e->n_packed + threads - 1) / threads);
  HIPCHECK(hipMemsetAsync(e->relu_bound_dev, 0, 2 * sizeof(unsigned), s));
  hipLaunchKernelGGL(k_relu_bound, dim3(64), dim3(256), 0, s, src, e->layout, e->A, e->nv.Sr, e->nv.Sv, e->relu_bound_dev);
  hipLaunchKernelGGL(k_relu_scale, dim3(1), dim3(1), 0, s, (const unsigned *)e->relu_bound_dev, e->relu_scale_dev, force);
  hipLaunchKernelGGL(k_pack_weights, dim3(blocks), dim3(threads), 0, s, src, e->pack_idx, (const int32_t *)e->pack_idx2,
                     e->packed, e->n_packed, (const float *)e->relu_scale_dev);
  if (e->split_f16)
    hipLaunchKernelGGL(k_pack_weights_h2, dim3((unsigned)((e->n_packed_h2 + threads - 1) / threads)), dim3(threads), 0, s, src,
                       e->pack_idx_h2, (_Float16 *)e->packed_h2, e->n_packed_h2);
  HIPCHECK(hipGetLastError());
  return 0;
}

#define NET_LAUNCH(kern, grid, s, ...)                                                        \
  do {                                                                                        \
    if (e->jtp == 1) hipLaunchKernelGGL(kern<1>, dim3(grid), dim3(256), 0, s, __VA_ARGS__);    \
    else hipLaunchKernelGGL(kern<2>, dim3(grid), dim3(256), 0, s, __VA_ARGS__);                \
  } while (0)

// (ev0 set: the dispatch carries start / stop events -- mz_tree_pair_timed, the clock of bench.py --workload tree)
#define TREE_GO_(kern, G_, s, ...)                                                                                \
  do {                                                                                                            \
    if (ev0_) hipExtLaunchKernelGGL(kern<G_>, dim3(blocks_), dim3(threads_), 0, s, ev0_, ev1_, 0, __VA_ARGS__);     \
    else hipLaunchKernelGGL(kern<G_>, dim3(blocks_), dim3(threads_), 0, s, __VA_ARGS__);                          \
  } while (0)
#define TREE_LAUNCH_EV(kern, s, ev0, ev1, ...)                                                \
  do {                                                                                        \
    const int threads_ = 256;                                                                 \
    const int total_ = e->B * e->G;                                                           \
    const int blocks_ = (total_ + threads_ - 1) / threads_;                                   \
    const hipEvent_t ev0_ = (ev0), ev1_ = (ev1);                                              \
    switch (e->G) {                                                                           \
      case 4: TREE_GO_(kern, 4, s, __VA_ARGS__); break;                                       \
      case 8: TREE_GO_(kern, 8, s, __VA_ARGS__); break;                                       \
      case 16: TREE_GO_(kern, 16, s, __VA_ARGS__); break;                                     \
      default: TREE_GO_(kern, 32, s, __VA_ARGS__); break;                                     \
    }                                                                                         \
  } while (0)
#define TREE_LAUNCH(kern, s, ...) TREE_LAUNCH_EV(kern, s, nullptr, nullptr, __VA_ARGS__)

// BaseNetwork.initial_inference for all B rows; selfplay: + synthetic observation, root expansion, Dirichlet
// noise and first descent (mz_root.hip.h)
// (tv: the engine's own view, or a copy whose root_value / root_logits aim elsewhere -- the leaf inference of the true-rules
// search, mz_tm_search; the view goes to the kernel by value)
template <int JTP>
static int launch_root_j(mz_engine *e, const TreeView &tv, const float *obs, bool selfplay, hipStream_t s) {
  const dim3 grid(e->Bp / MZ_ROWS), block(256);
  const double alpha = e->cfg.root_dirichlet_alpha, frac = e->cfg.root_exploration_fraction;
#define MZ_ROOT_GO(G_, SP_)                                                                                     \
  hipLaunchKernelGGL((k_root<JTP, G_, SP_>), grid, block, 0, s, e->nv, tv, obs, e->istream, e->nst0, e->sp, \
                     (uint64_t)e->cfg.seed, alpha, frac)
  if (!selfplay) MZ_ROOT_GO(4, false);
  else switch (e->G) {
    case 4: MZ_ROOT_GO(4, true); break;
    case 8: MZ_ROOT_GO(8, true); break;
    case 16: MZ_ROOT_GO(16, true); break;
    default: MZ_ROOT_GO(32, true); break;
  }
#undef MZ_ROOT_GO
  HIPCHECK(hipGetLastError());
  return 0;
}
static int launch_root(mz_engine *e, const TreeView &tv, const float *obs, bool selfplay, hipStream_t s) {
  return e->jtp == 1 ? launch_root_j<1>(e, tv, obs, selfplay, s) : launch_root_j<2>(e, tv, obs, selfplay, s);
}
static int launch_root(mz_engine *e, const float *obs, bool selfplay, hipStream_t s) { return launch_root(e, e->tv, obs, selfplay, s); }

// dynamic LDS of a HEAD launch: the root's working set (mz_root_body) lies over the trees, behind the pb_c table
static size_t fused_head_dyn_lds(int sims, int NN, int lt) {
  const size_t table = ((size_t)(sims + 2) * (lt == 2 ? sims + 2 : 64) * 8 + 15) & ~(size_t)15;
  const size_t root = table + sizeof(float) * MZ_ROOT_LDS_FLOATS, trees = mz_fused_dyn_lds(sims, NN, lt);
  return root > trees ? root : trees;
}

// The LDS of a CU: a search kernel's static LDS and the dynamic LDS of a launch have to fit it together
static const size_t MZ_LDS_BYTES = 160 * 1024;
static bool lds_fits(size_t static_bytes, size_t dyn_bytes) { return static_bytes + dyn_bytes <= MZ_LDS_BYTES; }

// Which search kernel this engine runs right now, and on how much LDS: read by the launch, the self-play loop,
// mz_selfplay_moves_per_launch and mz_search_kernel_info alike.  Computed on demand (sp.env_kind, stream_scaled and
// root_hidden_external change after mz_create).
struct SearchPlan {
  int kind;                      // what launch_search runs now: 0 the stand-alone kernels, else fkind
  int fkind;                     // the engine's fused kernel: 2 k_search_h2 where split_f16 applies, else 1 k_search_fused
  const SearchShape *shape;      // its row of the shape list
  int lt;                        // its tree placement: 1 whole trees in LDS, 2 compact, 0 global pool
  bool sp;                       // its single-player instantiation
  size_t lds_static, dyn, dyn_head;   // bytes: static LDS, dynamic LDS of a plain launch / of a whole-moves (HEAD) launch
  int game;                      // != 0: whole moves are those of this device game environment (its kind; the game kernels)
  bool persist;                  // the self-play loop runs as whole moves inside one launch
};
static SearchPlan search_plan(const mz_engine *e) {
  SearchPlan p = {};
  auto lds_static = [](int kind, int lt) { return sizeof(float) * (size_t)(kind == 2 ? mz_h2_lds_floats(lt) : mz_fused_lds_floats(lt)); };
  // trees in LDS when 16 of them fit beside the kernel's static LDS; if not, at least the fields the descent reads
  // (N, E, P, reward + discount * Q); else (0) in the global pool
  // (k_search_fused, rows with an action table: the table shares the dynamic LDS with whole trees, and with the pool
  // placement's pb_c table; beside compact trees it stays in global memory -- mz_fused_atab_lds)
  auto atab_lds = [&](int kind, int lt) {
    return kind == 1 ? mz_fused_atab_lds(mz_fused_atab(e->shape->ks1, e->shape->jtp, e->shape->g), e->A, lt) : (size_t)0;
  };
  auto place = [&](int kind) {
    for (int lt = 1; lt <= (!e->use_lds_trees ? 0 : (e->use_lds_hybrid ? 2 : 1)); ++lt)
      if (lds_fits(lds_static(kind, lt), mz_fused_dyn_lds(e->sims, e->NN, lt) + atab_lds(kind, lt))) return lt;
    return 0;
  };
  p.fkind = 2;
  p.lt = e->split_f16 ? place(2) : 0;
  if (p.lt == 0) { p.fkind = 1; p.lt = place(1); }      // (the split-f16 kernel has no global-pool placement: the exact one)
  p.shape = p.fkind == 2 ? e->shape_h2 : e->shape;
  p.sp = !e->cfg.two_players;       // single-player games (every reference environment but TicTacToe): no to_play handling
  p.lds_static = lds_static(p.fkind, p.lt);
  p.dyn = mz_fused_dyn_lds(e->sims, e->NN, p.lt) + atab_lds(p.fkind, p.lt);
  p.dyn_head = fused_head_dyn_lds(e->sims, e->NN, p.lt) + atab_lds(p.fkind, p.lt);
  p.kind = fused_usable(e) && !e->root_hidden_external ? p.fkind : 0;
  p.game = e->sp.env_kind;
  // whole moves: LDS trees and a HEAD kernel -- single player on the synthetic environment, or the device TicTacToe
  // environment on the exact-f32 game kernel (host-given uniforms / draws work there too), or the device CartPole
  // environment on the single-player game kernel, or the device Connect Four environment on its two game kernels (whole
  // trees, compact placement); a game environment without such an instantiation for its shape and
  // placement, or with split_f16, plays in the launch-per-step form (launch_move_game), and so does every move searched with
  // the Gumbel search (mz_selfplay_set_gumbel) or on the true rules (mz_selfplay_set_true_model)
  p.persist = e->sp_mode == MZ_SP_PUCT && e->use_persist && fused_usable(e) && p.lt != 0 && lds_fits(p.lds_static, p.dyn_head) &&
              (p.game ? !e->split_f16 && !!e->cfg.two_players == (p.game != 2) &&
                            find_kernel(1, *p.shape, p.lt, false, p.sp, true, true) != nullptr
                      : p.sp && !e->sp.env_kind);
  return p;
}

// arguments of one search launch
struct SearchOpts {
  int sims;                              // simulations to run
  int sims_done = 0;                     // simulations the trees already hold
  int moves = 0;                         // > 0: that many whole self-play moves inside the launch (HEAD); 0: one search
  bool record = false;                   // self-play: finalize the move and write its record in the kernel tail
  unsigned long long *prof = nullptr;    // phase-cycle counters (mz_search_phase_profile, mz_selfplay_phase_profile)
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // bracket the dispatch itself (what rocprofv3's kernel trace reports)
};

static int launch_fused(mz_engine *e, const SearchPlan &p, const SearchOpts &o, hipStream_t s) {
  const bool head = o.moves > 0;
  const void *fn = find_kernel(p.fkind, *p.shape, p.lt, !head && o.prof, p.sp, head, head && p.game != 0);
  if (!fn) {
#ifdef MZ_DEV_ONLY      // kernel development: only the two bench shapes are instantiated
    if (!find_kernel(p.fkind, *p.shape, p.lt, false, p.sp, false, false))
      return fail("MZ_DEV_ONLY build: action_space %d not instantiated", e->A);
#endif
    return fail("internal: no HEAD instantiation for this configuration");
  }
  if (std::find(e->lds_attr_done.begin(), e->lds_attr_done.end(), fn) == e->lds_attr_done.end()) {
    HIPCHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MZ_LDS_BYTES - p.lds_static)));
    e->lds_attr_done.push_back(fn);
  }
  // MZ_KARGS; a HEAD launch plays its moves from the root on (mz_root_body, on the LDS the trees are about to occupy)
  const f32x4 *ws = p.fkind == 2 ? (const f32x4 *)e->packed_h2 : e->wstream;
  int nsims = o.sims, slot0 = head ? 0 : o.sims_done, record = head || o.record ? 1 : 0;
  unsigned long long *prof = o.prof;
  uint64_t seed = e->cfg.seed;
  MzRootArgs ra = {nullptr, 0, 1, 0.0, 0.0};
  if (head) ra = {e->istream, e->nst0, o.moves, e->cfg.root_dirichlet_alpha, e->cfg.root_exploration_fraction};
  void *args[] = {&e->nv, &e->tv, &ws, &nsims, &slot0, &prof, &e->sp, &record, &seed, &ra};
  const dim3 grid(e->Bp / MZ_ROWS), block(256);
  const size_t dyn = head ? p.dyn_head : p.dyn;
  if (o.ev_start) (void)hipExtLaunchKernel(fn, grid, block, args, dyn, s, o.ev_start, o.ev_stop, 0);
  else (void)hipLaunchKernel(fn, grid, block, args, dyn, s);
  HIPCHECK(hipGetLastError());      // (this launch, or a k_tree_select issued just before it)
  return 0;
}

static int launch_root_priors(mz_engine *e, const int8_t *to_play, const uint8_t *legal, const double *priors,
                              hipStream_t s) {
  TREE_LAUNCH(k_tree_root_priors, s, e->tv, to_play, legal, priors);
  HIPCHECK(hipGetLastError());
  return 0;
}

// (o.ev_start / o.ev_stop also ride on the tree kernels' dispatches here, as they do on the fused kernel's)
static int launch_search(mz_engine *e, const SearchOpts &o, bool selection_valid, hipStream_t s) {
  const SearchPlan p = search_plan(e);
  if (p.kind) {
    if (!selection_valid) TREE_LAUNCH_EV(k_tree_select, s, o.ev_start, o.ev_stop, e->tv);
    return launch_fused(e, p, o, s);
  }
  for (int i = 0; i < o.sims; ++i) {
    if (!selection_valid) TREE_LAUNCH_EV(k_tree_select, s, o.ev_start, o.ev_stop, e->tv);
    NET_LAUNCH(k_net_recurrent_tree, e->Bp / MZ_ROWS, s, e->nv, e->tv, o.sims_done + i + 1);
    const int more = (i + 1 < o.sims) ? 1 : 0;
    TREE_LAUNCH_EV(k_tree_step, s, o.ev_start, o.ev_stop, e->tv, more);
    selection_valid = more;
  }
  HIPCHECK(hipGetLastError());
  return 0;
}


// ---------------------------------------------------------------- ABI
// ---- the step protocol of the stepwise searches (the plain entry points below, mz_tm_* in mz_truemodel_abi.inc, mz_gz_* in
// mz_gumbel_abi.inc) over selection_valid (a descent is pending) and sims_done.  A variant brings its readiness condition
// (`ready`; `first`: the call its message asks for), its kernels (`launch`) and its leaf outputs.
// the pending descent, launched if there is none
template <class LAUNCH>
static int step_pending(mz_engine *e, const char *fn, bool ready, const char *first, LAUNCH launch) {
  if (!ready) return fail("%s: call %s first", fn, first);
  if (e->sims_done >= e->sims) return fail("%s: all %d simulations already done", fn, e->sims);
  if (!e->selection_valid) {
    launch();
    HIPCHECK(hipGetLastError());
    e->selection_valid = true;
  }
  return 0;
}
// does a descent follow this simulation?  (the move's last simulation: nothing to descend for)
static bool step_more(const mz_engine *e) { return e->sims_done + 1 < e->sims; }
// one simulation's expand + backup of the pending descent: launch(more), more = the same launch makes the next descent
template <class LAUNCH>
static int step_advance(mz_engine *e, const char *fn, bool ready, const char *select, bool more, LAUNCH launch) {
  if (!ready || !e->selection_valid) return fail("%s: call %s first", fn, select);
  if (e->sims_done >= e->sims) return fail("%s: all %d simulations already done", fn, e->sims);
  launch(more);
  HIPCHECK(hipGetLastError());
  e->sims_done += 1;
  e->selection_valid = more;
  return 0;
}
// a new root: the protocol starts over, no simulation done and the root's first descent pending.  noise: exploration noise is in the
// root's priors; variant: the search whose own root kernel the caller launched as well (a self-play move; MZ_SP_PUCT: none yet)
static void step_restart(mz_engine *e, bool noise, MzSpMode variant = MZ_SP_PUCT) {
  e->sims_done = 0;
  e->selection_valid = e->root_ready = true;
  e->root_noise = noise;
  e->gz.root_set = variant == MZ_SP_GUMBEL;
  e->tm.root_set = variant == MZ_SP_TRUE_RULES;
}

// what the last descent left, for the caller; any may be null (one launch: four D2D blits cost 4 x 4 us per simulation)
static int export_selection(mz_engine *e, int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth, hipStream_t s) {
  if (leaf_node || parent_slot || action || depth) {
    hipLaunchKernelGGL(k_export_selection, dim3((e->B + 255) / 256), dim3(256), 0, s, e->tv, leaf_node, parent_slot, action, depth);
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

extern "C" {

const char *mz_last_error(void) { return g_err.c_str(); }
int mz_version(void) { return 1; }

int mz_create(const mz_config *cfg, mz_engine **out) {
  if (!cfg || !out) return fail("mz_create: null argument");
  *out = nullptr;
  if (cfg->num_envs <= 0) return fail("mz_create: num_envs must be > 0");
  if (cfg->action_space < 1 || cfg->action_space > MZ_MAX_ACTIONS)
    return fail("mz_create: action_space %d outside [1,%d]", cfg->action_space, MZ_MAX_ACTIONS);
  if (cfg->obs_dim < 1) return fail("mz_create: obs_dim must be >= 1");
  if (cfg->num_simulations < 1 || cfg->num_simulations > 4096) return fail("mz_create: num_simulations out of range");
  const int Sv = cfg->no_support ? 1 : cfg->value_support_max - cfg->value_support_min + 1;
  const int Sr = cfg->no_support ? 1 : cfg->reward_support_max - cfg->reward_support_min + 1;
  if (Sv < 1 || Sv > MZ_MAX_SUPPORT || Sr < 1 || Sr > MZ_MAX_SUPPORT)
    return fail("mz_create: support size must be in [1,%d] (value %d, reward %d)", MZ_MAX_SUPPORT, Sv, Sr);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("mz_create: no HIP device visible (this engine has no CPU path)");
  mz_engine *e = new mz_engine();
  if (hipGetDevice(&e->device) != hipSuccess) { delete e; return fail("mz_create: hipGetDevice failed"); }
  e->cfg = *cfg;
  e->B = cfg->num_envs;
  e->Bp = (cfg->num_envs + MZ_ROWS - 1) / MZ_ROWS * MZ_ROWS;
  e->A = cfg->action_space;
  e->O = cfg->obs_dim;
  e->sims = cfg->num_simulations;
  e->NN = 1 + (e->sims + 1) * e->A;
  e->PL = e->sims + 2;
  e->shape = shape_for(g_fused_shapes, e->A);
  e->G = e->shape->g;
  e->jtp = e->shape->jtp;
  e->use_graph = getenv("MZ_NO_GRAPH") == nullptr;
  e->use_fused = getenv("MZ_NO_FUSED") == nullptr;
  e->use_persist = getenv("MZ_NO_PERSIST") == nullptr;
  e->use_lds_trees = getenv("MZ_NO_LDS_TREES") == nullptr;
  e->use_lds_hybrid = getenv("MZ_NO_LDS_HYBRID") == nullptr;
  {
    const char *sf = getenv("MZ_SPLIT_F16");
    const bool want = cfg->split_f16 != 0 || (sf && sf[0] == '1');
    if (cfg->split_f16 != 0 && cfg->action_space > MZ_H2_MAXA) {
      delete e;
      return fail("mz_create: split_f16 supports action_space <= %d (got %d)", MZ_H2_MAXA, cfg->action_space);
    }
    e->split_f16 = want && cfg->action_space <= MZ_H2_MAXA;
    if (e->split_f16) e->shape_h2 = shape_for(g_h2_shapes, e->A);
  }
  TreeView &t = e->tv;
  memset(&t, 0, sizeof t);
  const size_t nb = (size_t)e->Bp;
#define DM(p, n) if (dmalloc(e, &(p), (n))) { mz_destroy(e); return -1; }
  // the node pool: 32-byte records, NS per tree (mz_common.h: MzNode)
  e->NS = (e->NN + MZ_NODE_OFF + 3) & ~3;
  MzNode *nodes;
  DM(nodes, nb * e->NS)
  e->nodes = nodes;
  t.N.base = t.W.base = t.P.base = t.R.base = t.E.base = t.TP.base = nodes;
  t.NS = e->NS;
  DM(t.legal, nb) DM(t.mn, nb) DM(t.mx, nb) DM(t.nexp, nb) DM(t.path, nb * e->PL) DM(t.plen, nb) DM(t.leaf_tp, nb)
  DM(t.leaf, nb) DM(t.slot, nb) DM(t.act, nb) DM(t.depth, nb)
  DM(t.hpool, nb * (e->sims + 1) * MZ_HS)
  DM(t.value, nb) DM(t.reward, nb) DM(t.logits, nb * e->A) DM(t.root_value, nb) DM(t.root_logits, nb * e->A)
  DM(t.noise, nb * e->A)
  double *sqrttab, *pbctab, *logtab;
  DM(sqrttab, e->sims + 2) DM(pbctab, (size_t)(e->sims + 2) * (e->sims + 2)) DM(logtab, e->sims + 2)
#undef DM
  {
    std::vector<double> lt, st;
    mz_host_tables(*cfg, lt, st);
    // pb_c for every (parent visits, child visits) pair, in the reference's operation order
    // (pb_c = log(..) + init; pb_c *= sqrt(Np) / (Nc + 1)); IEEE double on the host, no contraction
    const int T = e->sims + 2;
    std::vector<double> pt((size_t)T * T);
    for (int np = 0; np < T; ++np)
      for (int nc = 0; nc < T; ++nc) {
        volatile double q = st[np] / (double)(nc + 1);
        volatile double v = lt[np] * q;
        pt[(size_t)np * T + nc] = v;
      }
    if (hipMemcpy(pbctab, pt.data(), pt.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(logtab, lt.data(), lt.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sqrttab, st.data(), st.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
      mz_destroy(e);
      return fail("mz_create: table upload failed");
    }
  }
  t.sqrttab = sqrttab; t.pbctab = pbctab; t.logtab = logtab;
  t.B = e->B; t.A = e->A; t.sims = e->sims; t.NN = e->NN; t.PL = e->PL;
  t.two_players = cfg->two_players; t.has_min = cfg->has_min_bound; t.has_max = cfg->has_max_bound;
  t.min_bound = cfg->min_bound; t.max_bound = cfg->max_bound; t.discount = cfg->discount;
  t.init_value_score = cfg->init_value_score;
  if (build_packing(e)) { mz_destroy(e); return -1; }
  if (hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) {
    mz_destroy(e);
    return fail("mz_create: stream creation failed");
  }
  memset(&e->sp, 0, sizeof e->sp);
  memset(&e->ev, 0, sizeof e->ev);
  *out = e;
  return 0;
}

int mz_destroy(mz_engine *e) {
  if (!e) return 0;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  e->ring.forget(0);
  for (void *ev : e->ring.pool) hipEventDestroy((hipEvent_t)ev);
  drop_graphs(e, true);
  if (e->cap_stream) hipStreamDestroy(e->cap_stream);
  for (void *p : e->allocs) hipFree(p);
  for (int w = 0; w < 2; ++w) {
    if (e->wstage[w]) hipHostFree(e->wstage[w]);
    if (e->wstage_ev[w]) hipEventDestroy(e->wstage_ev[w]);
  }
  delete e;
  return 0;
}

int mz_affine_relu(float *y, const float *scale, const float *shift, const float *residual, size_t n, int channels,
                   int hw, void *stream) {
  if (!y || !scale || !shift) return fail("mz_affine_relu: null argument");
  if (channels < 1 || hw < 4 || (hw & 3) || n % ((size_t)channels * hw)) return fail("mz_affine_relu: n %zu is not [N][%d][%d] with hw %% 4 == 0", n, channels, hw);
  if (((uintptr_t)y | (uintptr_t)residual) & 15) return fail("mz_affine_relu: tensors must be 16-byte aligned");
  const size_t n4 = n / 4;
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (residual)
    hipLaunchKernelGGL(k_affine_relu<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4 *)y, scale, shift,
                       (const float4 *)residual, n4, channels, hw / 4);
  else
    hipLaunchKernelGGL(k_affine_relu<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4 *)y, scale, shift,
                       (const float4 *)nullptr, n4, channels, hw / 4);
  HIPCHECK(hipGetLastError());
  return 0;
}

// ---- the elementwise ends of the learner step (mz_learner.hip.h); engine-free: device pointers and sizes only
int mz_learner_targets(const float *t_val, const float *t_rew, const float *value0, int bs, int k1, int sv, int vmin, int sr,
                       int rmin, int no_target_transform, float *sup_val, float *sup_rew, float *new_errors, void *stream) {
  if (!t_val || !t_rew || !value0 || !sup_val || !sup_rew || !new_errors) return fail("mz_learner_targets: null argument");
  if (bs < 1 || k1 < 1 || sv < 1 || sr < 1 || sv > 4096 || sr > 4096) return fail("mz_learner_targets: bad sizes");
  // (bs * k1 threads for the supports, then -- from the next 32-lane boundary on -- 32 lanes per sample for the priority refresh)
  hipLaunchKernelGGL(k_learner_targets, dim3((((bs * k1 + 31) & ~31) + 32 * bs + 127) / 128), dim3(128), 0, (hipStream_t)stream, t_val, t_rew, value0, bs,
                     k1, sv, vmin, sr, rmin, no_target_transform, sup_val, sup_rew, new_errors);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_soft_ce_forward(const float *logits, const float *target, int positions, int bs, int bins, int64_t target_pos_stride,
                       int64_t target_row_stride, float *loss, void *stream) {
  if (!logits || !target || !loss) return fail("mz_soft_ce_forward: null argument");
  if (positions < 1 || positions > 8) return fail("mz_soft_ce_forward: 1..8 positions (num_unroll_steps + 1), got %d", positions);
  hipLaunchKernelGGL(k_soft_ce_fwd, dim3((8 * bs + 127) / 128), dim3(128), 0, (hipStream_t)stream, logits, target, positions, bs, bins,
                     target_pos_stride, target_row_stride, loss);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_soft_ce_backward(const float *logits, const float *target, const float *grad_loss, int positions, int bs, int bins,
                        int64_t target_pos_stride, int64_t target_row_stride, float *grad_logits, void *stream) {
  if (!logits || !target || !grad_loss || !grad_logits) return fail("mz_soft_ce_backward: null argument");
  hipLaunchKernelGGL(k_soft_ce_bwd, dim3((8 * positions * bs + 127) / 128), dim3(128), 0, (hipStream_t)stream, logits, target, grad_loss,
                     positions, bs, bins, target_pos_stride, target_row_stride, grad_logits);
  HIPCHECK(hipGetLastError());
  return 0;
}

size_t mz_num_weights(const mz_engine *e) { return e ? e->n_flat : 0; }
int mz_nodes_per_tree(const mz_engine *e) { return e ? e->NN : -1; }
int mz_padded_envs(const mz_engine *e) { return e ? e->Bp : -1; }

int mz_set_weights(mz_engine *e, const float *flat, size_t n, int on_device, void *stream) {
  if (!e || !flat) return fail("mz_set_weights: null argument");
  MZ_ENTER(e);
  if (n != e->n_flat) return fail("mz_set_weights: expected %zu floats, got %zu", e->n_flat, n);
  hipStream_t s = (hipStream_t)stream;
  const float *src = flat;
  if (!on_device) {
    HIPCHECK(hipMemcpyAsync(e->flat_dev, flat, n * sizeof(float), hipMemcpyHostToDevice, s));
    src = e->flat_dev;
  }
  if (e->split_f16) {
    // the high part of a split weight is its float16 rounding: beyond the float16 range it would be inf and poison every
    // search silently.  Checked here, loudly (one small reduction + a 4-byte read back; split_f16 is opt-in).
    if (!e->absmax_dev && dmalloc(e, &e->absmax_dev, (size_t)1)) return -1;
    HIPCHECK(hipMemsetAsync(e->absmax_dev, 0, 4, s));
    hipLaunchKernelGGL(k_absmax, dim3(64), dim3(256), 0, s, src, n, e->absmax_dev);
    unsigned bits = 0;
    HIPCHECK(hipMemcpyAsync(&bits, e->absmax_dev, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    float mx;
    memcpy(&mx, &bits, 4);
    if (!(mx <= 65504.f))
      return fail("mz_set_weights: split_f16 needs every weight finite and |w| <= 65504 (the float16 range of the high part); "
                  "max |w| = %g.  Use the exact-float32 kernel (split_f16 = 0) for these weights", (double)mx);
  }
  // the device decides whether a scale exists; a 16-byte read back tells the host -- if not, the engine runs the stand-alone kernels
  // until the next weight set
  if (enqueue_pack(e, src, -1, s)) return -1;
  HIPCHECK(hipMemcpyAsync(e->relu_scale_host, e->relu_scale_dev, 4 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));     // (also: a host buffer may be freed by the caller)
  const bool scaled = e->relu_scale_host[3] != 0.f;
  if (scaled != e->stream_scaled) drop_graphs(e, true);      // captured graphs hold the launches of the other kernel set
  e->stream_scaled = scaled;
  e->scale_host_valid = true;
  e->weights_set = true;
  return 0;
}

// The host's side of k_relu_bound / k_relu_scale: the same bound in double from a HOST copy of the weights, with tighter
// limits (a factor 2 on the activation bound, 4 on the consuming layers' largest weight), so that "1" here implies the
// device's own test passes whatever the float32 rounding of its sums.
int mz_weights_scale_ok(const float *flat, size_t n, int obs_dim, int action_space, int value_outputs, int reward_outputs) {
  if (!flat) return fail("mz_weights_scale_ok: null argument");
  if (obs_dim < 1 || action_space < 1 || value_outputs < 1 || reward_outputs < 1) return fail("mz_weights_scale_ok: bad shape");
  const FlatLayout L = flat_layout(obs_dim, action_space, value_outputs, reward_outputs);
  if (n != L.total) return fail("mz_weights_scale_ok: expected %zu floats, got %zu", L.total, n);
  const int A = action_space;
  double hb[MZ_H];
  for (int i = 0; i < MZ_H; ++i) hb[i] = 7.01 * fabs((double)flat[L.ln_w + i]) + fabs((double)flat[L.ln_b + i]);
  const size_t w1[4] = {L.rew_w1, L.tr_w1, L.val_w1, L.pol_w1}, b1[4] = {L.rew_b1, L.tr_b1, L.val_b1, L.pol_b1};
  double bound = 0.0;
  bool nan = false;
  for (int h = 0; h < 4; ++h) {
    const int K = h < 2 ? MZ_H + A : MZ_H;
    for (int r = 0; r < MZ_F; ++r) {
      const float *row = flat + w1[h] + (size_t)r * K;
      double s = 0.0, oh = 0.0;
      for (int i = 0; i < MZ_H; ++i) s += fabs((double)row[i]) * hb[i];
      for (int a = MZ_H; a < K; ++a) { const double v = fabs((double)row[a]); if (v != v) nan = true; if (v > oh) oh = v; }
      s += oh + fabs((double)flat[b1[h] + r]);
      if (s != s) nan = true;
      if (s > bound) bound = s;
    }
  }
  const size_t w2[4] = {L.rew_w2, L.tr_w2, L.val_w2, L.pol_w2};
  const int J[4] = {reward_outputs, MZ_H, value_outputs, A};
  double w2max = 0.0;
  for (int h = 0; h < 4; ++h)
    for (size_t i = 0; i < (size_t)J[h] * MZ_F; ++i) {
      const double v = fabs((double)flat[w2[h] + i]);
      if (v != v) nan = true;
      if (v > w2max) w2max = v;
    }
  bound *= 1.02;
  int k = 0;
  if (bound > 1.0) (void)frexp(bound, &k);
  return (!nan && bound < 0x1p39 && w2max < ldexp(1.0, 97 - k)) ? 1 : 0;
}

// mz_set_weights without the host waiting for anything queued on `stream`: the repack runs in stream order (the moves
// queued before it keep the old weights, everything queued after it sees the new ones), which kernel set the new weights
// run on is the caller's `scale_ok` (mz_weights_scale_ok on a host copy of the SAME weights).
int mz_set_weights_async(mz_engine *e, const float *flat, size_t n, int on_device, int scale_ok, void *stream) {
  if (!e || !flat) return fail("mz_set_weights_async: null argument");
  MZ_ENTER(e);
  if (n != e->n_flat) return fail("mz_set_weights_async: expected %zu floats, got %zu", e->n_flat, n);
  if (e->split_f16) return mz_set_weights(e, flat, n, on_device, stream);      // (its float16 range check reads back: synchronous)
  hipStream_t s = (hipStream_t)stream;
  const float *src = flat;
  if (!on_device) {
    const int w = e->wstage_next;
    e->wstage_next ^= 1;
    if (!e->wstage[w]) {
      HIPCHECK(hipHostMalloc((void **)&e->wstage[w], n * sizeof(float), hipHostMallocDefault));
      HIPCHECK(hipEventCreateWithFlags(&e->wstage_ev[w], hipEventDisableTiming));
    } else {
      HIPCHECK(hipEventSynchronize(e->wstage_ev[w]));      // the copy out of this slot, two pulls ago (long complete)
    }
    memcpy(e->wstage[w], flat, n * sizeof(float));
    HIPCHECK(hipMemcpyAsync(e->flat_dev, e->wstage[w], n * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(e->wstage_ev[w], s));
    src = e->flat_dev;
  }
  if (enqueue_pack(e, src, scale_ok ? 1 : 0, s)) return -1;
  const bool scaled = scale_ok != 0;
  if (scaled != e->stream_scaled) {      // (rare: captured graphs hold the launches of the other kernel set)
    HIPCHECK(hipStreamSynchronize(s));
    drop_graphs(e, true);
  }
  e->stream_scaled = scaled;
  e->scale_host_valid = false;
  e->weights_set = true;
  return 0;
}

int mz_weight_scale(mz_engine *e, float *out, void *stream) {
  if (!e || !out) return fail("mz_weight_scale: null argument");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_weight_scale: weights not set (call mz_set_weights)");
  if (!e->scale_host_valid) {
    HIPCHECK(hipMemcpyAsync(e->relu_scale_host, e->relu_scale_dev, 4 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    e->scale_host_valid = true;
  }
  memcpy(out, e->relu_scale_host, sizeof(e->relu_scale_host));
  return 0;
}

// ---- test hooks of the packing (include/mz_engine_debug.h)
int mz_pack_host(int obs_dim, int action_space, int value_bins, int reward_bins, int split_f16, long long *out, int which, int32_t *table,
                 size_t cap) {
  if (!out || obs_dim < 1 || action_space < 1 || value_bins < 1 || reward_bins < 1 || which < 0 || which > 2 ||
      (split_f16 && action_space > MZ_H2_MAXA))
    return fail("mz_pack_host: bad argument");
  const SearchShape *row = shape_for(g_fused_shapes, action_space);
  if (!row) return fail("mz_pack_host: bad argument");
  PackPlan p;
  std::string err;
  if (pack_plan(PackShape{obs_dim, action_space, value_bins, reward_bins, row->ks1, row->jtp, row->g, split_f16 != 0}, p, err))
    return fail("%s", err.c_str());
  pack_plan_record(p, out);
  if (!table) return 0;
  const std::vector<int32_t> &t = which == 0 ? p.idx : (which == 1 ? p.idx2 : p.idx_h2);
  if (cap < t.size()) return fail("mz_pack_host: table %d has %zu entries, room for %zu", which, t.size(), cap);
  memcpy(table, t.data(), t.size() * sizeof(int32_t));
  return 0;
}

int mz_pack_indices(mz_engine *e, int which, int32_t *out, size_t cap) {
  if (!e || !out || which < 0 || which > 2) return fail("mz_pack_indices: bad argument");
  MZ_ENTER(e);
  const int32_t *t = which == 0 ? e->pack_idx : (which == 1 ? e->pack_idx2 : e->pack_idx_h2);
  const size_t n = which == 2 ? e->n_packed_h2 : e->n_packed;
  if (cap < n) return fail("mz_pack_indices: table %d has %zu entries, room for %zu", which, n, cap);
  if (n) HIPCHECK(hipMemcpy(out, t, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

#include "mz_comm.inc"

int mz_initial_inference(mz_engine *e, const float *obs, void *stream) {
  if (!e || !obs) return fail("mz_initial_inference: null argument");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_initial_inference: weights not set (call mz_set_weights)");
  hipStream_t s = (hipStream_t)stream;
  if (launch_root(e, obs, false, s)) return -1;
  if (e->root_hidden_external && e->search_graph) { hipGraphExecDestroy(e->search_graph); e->search_graph = nullptr; }
  e->root_hidden_external = false;
  e->root_ready = false;
  return 0;
}

int mz_root_load(mz_engine *e, const float *hidden, const float *value, const float *logits, void *stream) {
  if (!e || !value || !logits) return fail("mz_root_load: null argument");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  HIPCHECK(hipMemcpyAsync(e->tv.root_value, value, (size_t)e->B * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipMemcpyAsync(e->tv.root_logits, logits, (size_t)e->B * e->A * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (hidden) {
    const int n = e->B * MZ_HS;
    hipLaunchKernelGGL(k_scatter_hidden, dim3((n + 255) / 256), dim3(256), 0, s, e->tv, hidden, 1);
    HIPCHECK(hipGetLastError());
    // a hidden state from elsewhere need not be a LayerNorm output: mz_search then runs the stand-alone kernels, whose
    // weights are not scaled for the clamp ReLU (k_relu_scale)
    if (!e->root_hidden_external && e->search_graph) { hipGraphExecDestroy(e->search_graph); e->search_graph = nullptr; }
    e->root_hidden_external = true;
  }
  e->root_ready = false;
  return 0;
}

__global__ void k_copy_root_hidden(TreeView t, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B * MZ_H) return;
  const int b = i / MZ_H, k = i % MZ_H;
  out[i] = t.hpool[(size_t)b * (t.sims + 1) * MZ_HS + k];
}

int mz_root_outputs(mz_engine *e, float *value, float *logits, float *hidden, void *stream) {
  if (!e) return fail("mz_root_outputs: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (value) HIPCHECK(hipMemcpyAsync(value, e->tv.root_value, (size_t)e->B * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (logits)
    HIPCHECK(hipMemcpyAsync(logits, e->tv.root_logits, (size_t)e->B * e->A * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (hidden) {
    const int n = e->B * MZ_H;
    hipLaunchKernelGGL(k_copy_root_hidden, dim3((n + 255) / 256), dim3(256), 0, s, e->tv, hidden);
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

int mz_root_prepare(mz_engine *e, const int8_t *to_play, const uint8_t *legal, const double *noise,
                    int use_device_rng, uint64_t move_counter, void *stream) {
  if (!e) return fail("mz_root_prepare: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  const double *nz = noise;
  if (!noise && use_device_rng) {
    const int threads = 128;
    hipLaunchKernelGGL(k_dirichlet, dim3((e->B + threads - 1) / threads), dim3(threads), 0, s, e->tv, legal,
                       e->cfg.root_dirichlet_alpha, e->cfg.seed, move_counter, (const unsigned long long *)nullptr,
                       e->cfg.env_id_offset);
    HIPCHECK(hipGetLastError());
    nz = e->tv.noise;
  } else if (noise) {
    HIPCHECK(hipMemcpyAsync(e->tv.noise, noise, (size_t)e->B * e->A * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  TREE_LAUNCH(k_tree_root, s, e->tv, to_play, legal, nz, e->cfg.root_exploration_fraction, 1);
  HIPCHECK(hipGetLastError());
  step_restart(e, nz != nullptr);
  return 0;
}

int mz_search(mz_engine *e, int num_simulations, void *stream) {
  if (!e) return fail("mz_search: null engine");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_search: weights not set (call mz_set_weights)");
  if (!e->root_ready) return fail("mz_search: call mz_root_prepare first");
  if (num_simulations < 1 || e->sims_done + num_simulations > e->sims)
    return fail("mz_search: %d + %d simulations exceed the pool sized for num_simulations = %d", e->sims_done,
                num_simulations, e->sims);
  hipStream_t s = (hipStream_t)stream;
  const bool graphable = e->use_graph && e->selection_valid && e->sims_done == 0;
  if (graphable) {
    if (!e->search_graph || e->search_graph_sims != num_simulations) {
      if (e->search_graph) { hipGraphExecDestroy(e->search_graph); e->search_graph = nullptr; }
      hipGraph_t g = nullptr;
      HIPCHECK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
      int rc = launch_search(e, {num_simulations}, true, e->cap_stream);
      hipError_t ce = hipStreamEndCapture(e->cap_stream, &g);
      if (rc || ce != hipSuccess) return fail("mz_search: graph capture failed");
      HIPCHECK(hipGraphInstantiate(&e->search_graph, g, nullptr, nullptr, 0));
      hipGraphDestroy(g);
      e->search_graph_sims = num_simulations;
    }
    HIPCHECK(hipGraphLaunch(e->search_graph, s));
  } else {
    if (launch_search(e, {num_simulations, e->sims_done}, e->selection_valid, s)) return -1;
  }
  e->sims_done += num_simulations;
  e->selection_valid = false;
  return 0;
}

// which search kernel mz_search / mz_selfplay_steps will launch for this engine right now -- out4 [host]: kind (0 the
// stand-alone kernels, 1 k_search_fused, 2 k_search_h2), LDS placement of the trees (0 global pool, 1 whole trees, 2
// compact; -1 for kind 0), fc1 k-steps of the instantiation, lanes per child group.  (Tests assert the instantiation
// they mean to exercise.)
int mz_search_kernel_info(const mz_engine *e, int *out4) {
  if (!e || !out4) return fail("mz_search_kernel_info: null argument");
  const SearchPlan p = search_plan(e);
  out4[0] = p.kind; out4[1] = p.kind ? p.lt : -1; out4[2] = e->shape->ks1; out4[3] = e->G;
  return 0;
}

int mz_root_set_priors(mz_engine *e, const int8_t *to_play, const uint8_t *legal, const double *priors,
                       void *stream) {
  if (!e || !priors) return fail("mz_root_set_priors: null argument");
  MZ_ENTER(e);
  if (launch_root_priors(e, to_play, legal, priors, (hipStream_t)stream)) return -1;
  e->sims_done = 0;
  e->selection_valid = true;
  e->root_ready = true;
  return 0;
}

int mz_last_paths(mz_engine *e, int32_t *paths, int32_t *lengths, void *stream) {
  if (!e) return fail("mz_last_paths: null engine");
  MZ_ENTER(e);
  if (!e->selection_valid) return fail("mz_last_paths: no pending descent (call mz_select first)");
  hipStream_t s = (hipStream_t)stream;
  if (paths) HIPCHECK(hipMemcpyAsync(paths, e->tv.path, (size_t)e->B * e->PL * 4, hipMemcpyDeviceToDevice, s));
  if (lengths) HIPCHECK(hipMemcpyAsync(lengths, e->tv.plen, (size_t)e->B * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

int mz_search_profiled(mz_engine *e, int num_simulations, float *ms_out, void *stream) {
  if (!e || !ms_out) return fail("mz_search_profiled: null argument");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_search_profiled: weights not set (call mz_set_weights)");
  if (!e->root_ready || !e->selection_valid || e->sims_done != 0)
    return fail("mz_search_profiled: call right after mz_root_prepare");
  if (num_simulations < 1 || num_simulations > e->sims) return fail("mz_search_profiled: bad num_simulations");
  hipStream_t s = (hipStream_t)stream;
  std::vector<hipEvent_t> ev(2 * num_simulations + 1);
  for (auto &x : ev) HIPCHECK(hipEventCreate(&x));
  HIPCHECK(hipEventRecord(ev[0], s));
  for (int i = 0; i < num_simulations; ++i) {
    NET_LAUNCH(k_net_recurrent_tree, e->Bp / MZ_ROWS, s, e->nv, e->tv, i + 1);
    HIPCHECK(hipEventRecord(ev[2 * i + 1], s));
    const int more = (i + 1 < num_simulations) ? 1 : 0;
    TREE_LAUNCH(k_tree_step, s, e->tv, more);
    HIPCHECK(hipEventRecord(ev[2 * i + 2], s));
  }
  HIPCHECK(hipStreamSynchronize(s));
  ms_out[0] = ms_out[1] = 0.f;
  for (int i = 0; i < num_simulations; ++i) {
    float a = 0.f, b = 0.f;
    HIPCHECK(hipEventElapsedTime(&a, ev[2 * i], ev[2 * i + 1]));
    HIPCHECK(hipEventElapsedTime(&b, ev[2 * i + 1], ev[2 * i + 2]));
    ms_out[0] += a; ms_out[1] += b;
  }
  for (auto &x : ev) hipEventDestroy(x);
  e->sims_done = num_simulations;
  e->selection_valid = false;
  return 0;
}

int mz_search_timed(mz_engine *e, int num_simulations, float *ms_out, void *stream) {
  if (!e || !ms_out) return fail("mz_search_timed: null argument");
  MZ_ENTER(e);
  if (!fused_usable(e) || e->root_hidden_external) return fail("mz_search_timed: fused kernel not in use");
  if (!e->weights_set) return fail("mz_search_timed: weights not set (call mz_set_weights)");
  if (!e->root_ready || !e->selection_valid || e->sims_done != 0)
    return fail("mz_search_timed: call right after mz_root_prepare");
  if (num_simulations < 1 || num_simulations > e->sims) return fail("mz_search_timed: bad num_simulations");
  hipStream_t s = (hipStream_t)stream;
  SearchOpts o = {num_simulations};
  HIPCHECK(hipEventCreate(&o.ev_start));
  HIPCHECK(hipEventCreate(&o.ev_stop));
  const int rc = launch_fused(e, search_plan(e), o, s);
  hipError_t se = hipStreamSynchronize(s);
  float ms = 0.f;
  hipError_t te = (rc == 0 && se == hipSuccess) ? hipEventElapsedTime(&ms, o.ev_start, o.ev_stop) : hipErrorUnknown;
  hipEventDestroy(o.ev_start); hipEventDestroy(o.ev_stop);
  if (rc) return -1;
  if (se != hipSuccess || te != hipSuccess) return fail("mz_search_timed: %s", hipGetErrorString(se != hipSuccess ? se : te));
  *ms_out = ms;
  e->sims_done = num_simulations;
  e->selection_valid = false;
  return 0;
}

int mz_search_phase_profile(mz_engine *e, int num_simulations, unsigned long long *cycles_out, void *stream) {
  if (!e || !cycles_out) return fail("mz_search_phase_profile: null argument");
  MZ_ENTER(e);
  if (!fused_usable(e) || e->root_hidden_external) return fail("mz_search_phase_profile: fused kernel not in use");
  if (!e->root_ready || !e->selection_valid || e->sims_done != 0)
    return fail("mz_search_phase_profile: call right after mz_root_prepare");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)(e->Bp / MZ_ROWS) * 4 * MZ_NPHASE;
  unsigned long long *buf = nullptr;
  HIPCHECK(hipMalloc((void **)&buf, n * 8));
  HIPCHECK(hipMemsetAsync(buf, 0, n * 8, s));
  SearchOpts o = {num_simulations};
  o.prof = buf;
  int rc = launch_fused(e, search_plan(e), o, s);
  if (rc) { hipFree(buf); return -1; }
  HIPCHECK(hipStreamSynchronize(s));
  std::vector<unsigned long long> h(n);
  HIPCHECK(hipMemcpy(h.data(), buf, n * 8, hipMemcpyDeviceToHost));
  hipFree(buf);
  // spread of the workgroups' totals (wave 0): the launch lasts as long as its slowest workgroup
  {
    double mn = 1e300, mx = 0, sum = 0;
    for (int g = 0; g < e->Bp / MZ_ROWS; ++g) {
      double tot = 0;
      for (int p2 = 0; p2 < MZ_NPHASE; ++p2) tot += (double)h[((size_t)g * 4) * MZ_NPHASE + p2];
      mn = tot < mn ? tot : mn; mx = tot > mx ? tot : mx; sum += tot;
    }
    e->prof_spread[0] = sum / (e->Bp / MZ_ROWS); e->prof_spread[1] = mn; e->prof_spread[2] = mx;
  }
  // average over workgroups, per wave and phase: cycles_out[4][MZ_NPHASE]
  for (int w = 0; w < 4; ++w)
    for (int p = 0; p < MZ_NPHASE; ++p) {
      unsigned long long sum = 0;
      for (int g = 0; g < e->Bp / MZ_ROWS; ++g) sum += h[((size_t)g * 4 + w) * MZ_NPHASE + p];
      cycles_out[w * MZ_NPHASE + p] = sum / (unsigned long long)(e->Bp / MZ_ROWS);
    }
  e->sims_done = num_simulations;
  e->selection_valid = false;
  return 0;
}

int mz_search_phase_spread(const mz_engine *e, double *out3) {
  if (!e || !out3) return fail("mz_search_phase_spread: null argument");
  out3[0] = e->prof_spread[0]; out3[1] = e->prof_spread[1]; out3[2] = e->prof_spread[2];
  return 0;
}

int mz_select(mz_engine *e, int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth, void *stream) {
  if (!e) return fail("mz_select: null engine");
  MZ_ENTER(e);
  hipStream_t s = (hipStream_t)stream;
  if (step_pending(e, "mz_select", e->root_ready, "mz_root_prepare", [&] { TREE_LAUNCH(k_tree_select, s, e->tv); })) return -1;
  return export_selection(e, leaf_node, parent_slot, action, depth, s);
}

int mz_tree_pair_timed(mz_engine *e, const float *value, const float *reward, const float *logits, float *ms_out, void *stream) {
  if (!e || !value || !reward || !logits || !ms_out) return fail("mz_tree_pair_timed: null argument");
  MZ_ENTER(e);
  if (!e->root_ready) return fail("mz_tree_pair_timed: call mz_root_prepare first");
  if (e->sims_done >= e->sims) return fail("mz_tree_pair_timed: all %d simulations already done", e->sims);
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (auto &x : ev) HIPCHECK(hipEventCreate(&x));
  const bool pending = e->selection_valid;      // (the root's own first descent: mz_root_prepare leaves it selected)
  if (!pending) TREE_LAUNCH_EV(k_tree_select, s, ev[0], ev[1], e->tv);
  TREE_LAUNCH_EV(k_tree_expand_backup, s, ev[2], ev[3], e->tv, value, reward, logits);
  hipError_t le = hipGetLastError(), se = hipStreamSynchronize(s);
  int rc = 0;
  if (le != hipSuccess || se != hipSuccess) rc = fail("mz_tree_pair_timed: %s", hipGetErrorString(le != hipSuccess ? le : se));
  else if ((!pending && hipEventElapsedTime(&ms_out[0], ev[0], ev[1]) != hipSuccess) || hipEventElapsedTime(&ms_out[1], ev[2], ev[3]) != hipSuccess)
    rc = fail("mz_tree_pair_timed: event timing failed");
  if (pending) ms_out[0] = -1.f;
  for (auto &x : ev) hipEventDestroy(x);
  if (rc) return rc;
  e->sims_done += 1;
  e->selection_valid = false;
  return 0;
}

int mz_gather_hidden(mz_engine *e, float *hidden_out, void *stream) {
  if (!e || !hidden_out) return fail("mz_gather_hidden: null argument");
  MZ_ENTER(e);
  if (!e->selection_valid) return fail("mz_gather_hidden: call mz_select first");
  const int n = e->B * MZ_H;
  hipLaunchKernelGGL(k_gather_hidden, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->tv, hidden_out);
  HIPCHECK(hipGetLastError());
  return 0;
}

// one simulation's tree step on the caller's outputs: more = also the next descent, with mz_select's outputs
static int plain_step(mz_engine *e, const char *fn, const float *value, const float *reward, const float *logits, const float *hidden,
                      bool more, int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth, hipStream_t s) {
  return step_advance(e, fn, true, "mz_select", more, [&](bool m) {
    if (hidden) {
      const int n = e->B * MZ_HS;
      hipLaunchKernelGGL(k_scatter_hidden, dim3((n + 255) / 256), dim3(256), 0, s, e->tv, hidden, 0);
    }
    if (m) TREE_LAUNCH(k_tree_step_ext, s, e->tv, value, reward, logits, leaf_node, parent_slot, action, depth);
    else TREE_LAUNCH(k_tree_expand_backup, s, e->tv, value, reward, logits);
  });
}

int mz_expand_backup(mz_engine *e, const float *value, const float *reward, const float *logits,
                     const float *hidden, void *stream) {
  if (!e || !value || !reward || !logits) return fail("mz_expand_backup: null argument");
  MZ_ENTER(e);
  return plain_step(e, "mz_expand_backup", value, reward, logits, hidden, false, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int mz_expand_backup_select(mz_engine *e, const float *value, const float *reward, const float *logits, const float *hidden,
                            int32_t *leaf_node, int32_t *parent_slot, int32_t *action, int32_t *depth, void *stream) {
  if (!e || !value || !reward || !logits) return fail("mz_expand_backup_select: null argument");
  MZ_ENTER(e);
  return plain_step(e, "mz_expand_backup_select", value, reward, logits, hidden, step_more(e), leaf_node, parent_slot, action, depth,
                    (hipStream_t)stream);
}

int mz_recurrent_inference(mz_engine *e, const float *hidden_in, const int32_t *action, int n, float *hidden_out,
                           float *reward, float *value, float *logits, void *stream) {
  if (!e || !hidden_in || !action || !hidden_out || !reward || !value || !logits)
    return fail("mz_recurrent_inference: null argument");
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_recurrent_inference: weights not set (call mz_set_weights)");
  if (n < 1) return fail("mz_recurrent_inference: n must be >= 1");
  NET_LAUNCH(k_net_recurrent_rows, (n + MZ_ROWS - 1) / MZ_ROWS, (hipStream_t)stream, e->nv, hidden_in, action, n,
             hidden_out, reward, value, logits);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_finalize(mz_engine *e, const double *temperature, const double *uniform, uint64_t move_counter,
                int32_t *action, double *child_visits, double *root_value, double *error, int32_t *visit_counts,
                void *stream) {
  if (!e) return fail("mz_finalize: null engine");
  MZ_ENTER(e);
  if (action && !temperature) return fail("mz_finalize: temperature is required when action is requested");
  const int threads = 128;
  hipLaunchKernelGGL(k_tree_finalize, dim3((e->B + threads - 1) / threads), dim3(threads), 0, (hipStream_t)stream,
                     e->tv, temperature, uniform, e->cfg.seed, move_counter, (const unsigned long long *)nullptr,
                     e->cfg.env_id_offset, action, child_visits, root_value, error, visit_counts);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_eval_walk(mz_engine *e, int max_actions, const double *temperature, const double *uniform, uint64_t move,
                 int32_t *actions, float *pred_rewards, int32_t *n_actions, int32_t *path_lengths, void *stream) {
  if (!e || !temperature || !actions || !pred_rewards || !n_actions) return fail("mz_eval_walk: null argument");
  MZ_ENTER(e);
  if (!e->root_ready) return fail("mz_eval_walk: no tree (call mz_root_prepare and mz_search first)");
  if (max_actions < 1) return fail("mz_eval_walk: max_actions must be >= 1");
  const size_t lds = (size_t)(e->sims + 1) * sizeof(int32_t);
  if (lds > 48 * 1024) return fail("mz_eval_walk: num_simulations = %d exceeds the walk's LDS map", e->sims);
  hipLaunchKernelGGL(k_eval_walk, dim3(e->B), dim3(64), lds, (hipStream_t)stream, e->tv, e->sims_done + 1, e->tm.root_set ? 1 : 0, max_actions,
                     temperature, uniform, e->cfg.seed, move, e->cfg.env_id_offset, actions, pred_rewards, n_actions,
                     path_lengths);
  HIPCHECK(hipGetLastError());
  return 0;
}

int mz_eval_lookahead(mz_engine *e, int mode, int32_t *action, float *pred_reward, double *child_visits,
                      float *row_reward, float *row_value, void *stream) {
  if (!e || !action || !pred_reward) return fail("mz_eval_lookahead: null argument");
  if (mode != 1 && mode != 2) return fail("mz_eval_lookahead: mode must be 1 (only_prior) or 2 (only_value), got %d", mode);
  MZ_ENTER(e);
  if (!e->weights_set) return fail("mz_eval_lookahead: weights not set (call mz_set_weights)");
  if (!e->root_ready) return fail("mz_eval_lookahead: no root (call mz_initial_inference and mz_root_prepare first)");
  const size_t rows_max = (size_t)e->B * e->A;
  // scratch of the rows, allocated on the first call (which therefore synchronises: hipMalloc + hipMemset; header)
  if (!e->eval_rows && dmalloc(e, &e->eval_rows, rows_max * (MZ_H + e->A + 2))) return -1;
  float *hout = e->eval_rows, *logits = hout + rows_max * MZ_H, *rew = logits + rows_max * e->A, *val = rew + rows_max;
  hipStream_t s = (hipStream_t)stream;
  const int threads = 128, tblocks = (e->B + threads - 1) / threads;
  if (mode == 2) {      // --only_value: every (tree, action) row, then the choice
    const int n = e->B * e->A;
    float *rr = row_reward ? row_reward : rew, *rv = row_value ? row_value : val;
    NET_LAUNCH(k_eval_rows, (n + MZ_ROWS - 1) / MZ_ROWS, s, e->nv, e->tv, e->A, (const int32_t *)nullptr, n, hout, rr, rv, logits);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_eval_choose_value, dim3(tblocks), dim3(threads), 0, s, e->tv, (const float *)rr, (const float *)rv,
                       (float)e->cfg.discount, action, pred_reward, child_visits);
    HIPCHECK(hipGetLastError());
  } else {              // --only_prior: the choice, then one row per tree for its reward
    hipLaunchKernelGGL(k_eval_choose_prior, dim3(tblocks), dim3(threads), 0, s, e->tv, action, child_visits);
    HIPCHECK(hipGetLastError());
    NET_LAUNCH(k_eval_rows, (e->B + MZ_ROWS - 1) / MZ_ROWS, s, e->nv, e->tv, 1, (const int32_t *)action, e->B, hout,
               pred_reward, row_value ? row_value : val, logits);
    HIPCHECK(hipGetLastError());
    if (row_reward)
      HIPCHECK(hipMemcpyAsync(row_reward, pred_reward, (size_t)e->B * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

int mz_export_tree(mz_engine *e, int32_t *N, double *W, double *P, float *R, int32_t *E, int8_t *TP,
                   uint32_t *legal_mask, double *minmax, double *noise, float *hidden_pool) {
  if (!e) return fail("mz_export_tree: null engine");
  MZ_ENTER(e);
  HIPCHECK(hipDeviceSynchronize());
  const TreeView &t = e->tv;
  if (N || W || P || R || E || TP) {      // the record pool -> the caller's per-field arrays [B][NN]
    std::vector<MzNode> pool((size_t)e->B * e->NS);
    HIPCHECK(hipMemcpy(pool.data(), e->nodes, pool.size() * sizeof(MzNode), hipMemcpyDeviceToHost));
    for (int b = 0; b < e->B; ++b)
      for (int k = 0; k < e->NN; ++k) {
        const MzNode &n = pool[(size_t)b * e->NS + MZ_NODE_OFF + k];
        const size_t i = (size_t)b * e->NN + k;
        if (N) N[i] = n.N;
        if (W) W[i] = n.W;
        if (P) P[i] = n.P;
        if (R) R[i] = n.R;
        if (E) E[i] = n.E;
        if (TP) TP[i] = n.TP;
      }
  }
  if (legal_mask) HIPCHECK(hipMemcpy(legal_mask, t.legal, (size_t)e->B * 4, hipMemcpyDeviceToHost));
  if (minmax) {
    std::vector<double> mn(e->B), mx(e->B);
    HIPCHECK(hipMemcpy(mn.data(), t.mn, (size_t)e->B * 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(mx.data(), t.mx, (size_t)e->B * 8, hipMemcpyDeviceToHost));
    for (int b = 0; b < e->B; ++b) { minmax[2 * b] = mn[b]; minmax[2 * b + 1] = mx[b]; }
  }
  if (noise) HIPCHECK(hipMemcpy(noise, t.noise, (size_t)e->B * e->A * 8, hipMemcpyDeviceToHost));
  if (hidden_pool) {
    std::vector<float> tmp((size_t)e->B * (e->sims + 1) * MZ_HS);
    HIPCHECK(hipMemcpy(tmp.data(), t.hpool, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < (size_t)e->B * (e->sims + 1); ++r)
      memcpy(hidden_pool + r * MZ_H, tmp.data() + r * MZ_HS, MZ_H * sizeof(float));
  }
  return 0;
}

// whether engine e can play the game `kind` (mz_game_shape_ok); if not, the failure is fn's: "<fn>: <Name> needs ..."
static int game_shape(const mz_engine *e, const char *fn, int kind) {
  char why[96];
  return mz_game_shape_ok(kind, e->O, e->A, e->cfg.two_players != 0, why, sizeof why) ? 0 : fail("%s: %s", fn, why);
}

#include "mz_playout_abi.inc"
#include "mz_solve_abi.inc"
#include "mz_unroll_abi.inc"
#include "mz_truemodel_abi.inc"
#include "mz_gumbel_abi.inc"
#include "mz_selfplay_abi.inc"      // (after the two searches a game move chooses between: launch_move_game)
#include "mz_eval_abi.inc"
#include "mz_match_abi.inc"
#include "mz_reanalyse_abi.inc"
#include "mz_fcl_abi.inc"

}  // extern "C"
