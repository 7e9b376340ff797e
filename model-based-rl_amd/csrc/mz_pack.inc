// mz_pack.inc -- the gather tables of the weight streams: which element of the flat weight vector every lane of every MFMA of
// k_search_fused, k_search_h2, k_root and the stand-alone network kernels receives.  pack_plan is a pure function of the shape: standard
// library only, no HIP header (mz_engine.hip uploads what it returns; tests/pack_host.cpp and mz_pack_host run it without a device).
// The streams' lengths come from mz_stream_sizes.h, the file the kernels' schedules take theirs from.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "mz_stream_sizes.h"

// offsets of the 22 tensors inside the flat weight vector (flat_layout below)
struct FlatLayout {
  size_t rep_w1, rep_b1, rep_w2, rep_b2, val_w1, val_b1, val_w2, val_b2, pol_w1, pol_b1, pol_w2, pol_b2, rew_w1,
      rew_b1, rew_w2, rew_b2, tr_w1, tr_b1, tr_w2, tr_b2, ln_w, ln_b, total;
};

static FlatLayout flat_layout(int O, int A, int Sv, int Sr) {
  FlatLayout L;
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += n; return o; };
  const int K = MZ_H + A;
  L.rep_w1 = take((size_t)MZ_F * O); L.rep_b1 = take(MZ_F); L.rep_w2 = take((size_t)MZ_H * MZ_F); L.rep_b2 = take(MZ_H);
  L.val_w1 = take((size_t)MZ_F * MZ_H); L.val_b1 = take(MZ_F); L.val_w2 = take((size_t)Sv * MZ_F); L.val_b2 = take(Sv);
  L.pol_w1 = take((size_t)MZ_F * MZ_H); L.pol_b1 = take(MZ_F); L.pol_w2 = take((size_t)A * MZ_F); L.pol_b2 = take(A);
  L.rew_w1 = take((size_t)MZ_F * K); L.rew_b1 = take(MZ_F); L.rew_w2 = take((size_t)Sr * MZ_F); L.rew_b2 = take(Sr);
  L.tr_w1 = take((size_t)MZ_F * K); L.tr_b1 = take(MZ_F); L.tr_w2 = take((size_t)MZ_H * MZ_F); L.tr_b2 = take(MZ_H);
  L.ln_w = take(MZ_H); L.ln_b = take(MZ_H);
  L.total = off;
  return L;
}

// what the tables are built for: the network's sizes, the engine's row (ks1, jtp, g) of mz_kernels.inc, and whether the split-f16
// stream is wanted
struct PackShape { int O, A, Sv, Sr, ks1, jtp, g; bool split_f16; };

// every segment of the packed vector by name (offsets in floats, each a multiple of 4), the streams' lengths, and the tables
struct PackPlan {
  FlatLayout L;
  // the stand-alone network kernels (NetView): representation out; dynamics fc1 / out; prediction fc1 / out; LayerNorm
  size_t w0o, b0o, w1, b1, w2, b2, w3, b3, w4, b4, lnw, lnb;
  // the fused kernel's fc1 packs (bias inside the matrix), its stream [4 waves][wstride], the small-MFMA pieces, the root's stream
  size_t w1f, w3f, ws, h4, p4, is;
  size_t n_packed, wstride;           // floats in all; floats per wave of the fused stream (its action table included)
  size_t n_packed_h2;                 // float16 of the split-f16 stream, 0 without it
  int ks0, ks1, ks3;                  // k-steps of the stand-alone fc1 layers
  int nsteps, nst0, nroot, ngroups;   // FusedSched::NSTEPS; the root's run-time first stage, and that + RootSched::NS; H2Sched::NGROUPS
  // per packed float its source element (-1: 0.0; bits 29-30: the scale class), a second one to add (-1: none); per packed float16 its
  // source (bit 30: the low part)
  std::vector<int32_t> idx, idx2, idx_h2;
};

// ---- fc1 pack: weights [4 waves][4 tile groups][ks][64][4]; tile t = 4 tg + i of wave w = head t/8, features 128w + 16(t%8) + 0..15,
// input column k = 4 s + (lane >> 4).  What column k of a row maps to:
//   FC1_PLAIN     W[n][k] below K (the bias is a segment of its own, fill_fc1_bias)
//   FC1_BIASCOL   as PLAIN, and column K carries the bias (a constant-1 input): the fused kernel's prediction fc1
//   FC1_FOLDBIAS  no bias column -- the input's one-hot part holds exactly one 1, so the bias rides in the one-hot columns: their
//                 packed weight is W[n][50 + a] + b[n] (idx2 = the bias element to add, k_pack_weights).  K = 50 + A columns instead of
//                 51 + A: one k-step of four fewer for A = 6, 10, 14, ...  Only the first Kuse columns are packed: Kuse = 50 < K for the
//                 rows with an action table (mz_fused_atab), whose one-hot columns + bias go into the table (fill_action_table)
enum Fc1Cols { FC1_PLAIN, FC1_BIASCOL, FC1_FOLDBIAS };
static void fill_fc1(PackPlan &p, size_t wpos, const size_t *woff, const size_t *boff, int K, int ks, Fc1Cols cols, int Kuse) {
  for (int w = 0; w < 4; ++w)
    for (int tg = 0; tg < 4; ++tg)
      for (int s = 0; s < ks; ++s)
        for (int lane = 0; lane < 64; ++lane)
          for (int i = 0; i < 4; ++i) {
            const int t = 4 * tg + i, head = t / 8, tt = t % 8;
            const int nf = 128 * w + 16 * tt + (lane & 15), k = 4 * s + (lane >> 4);
            const size_t o = wpos + ((((size_t)(w * 4 + tg) * ks + s) * 64 + lane) * 4 + i);
            int32_t v = -1;
            if (k < Kuse) v = (int32_t)(woff[head] + (size_t)nf * K + k);
            else if (cols == FC1_BIASCOL && k == K) v = (int32_t)(boff[head] + nf);
            p.idx[o] = v;
            if (cols == FC1_FOLDBIAS) p.idx2[o] = (k >= MZ_H && k < Kuse) ? (int32_t)(boff[head] + nf) : -1;      // (else it stays -1)
          }
}

// the bias segment beside an FC1_PLAIN pack: [4 waves][16 tiles][64][4], lane row g of tile t holds features 128w + 16(t%8) + 4g + r
static void fill_fc1_bias(PackPlan &p, size_t bpos, const size_t *boff) {
  for (int w = 0; w < 4; ++w)
    for (int t = 0; t < 16; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r) {
          const int nf = 128 * w + 16 * (t % 8) + 4 * (lane >> 4) + r;
          p.idx[bpos + (((size_t)(w * 16 + t) * 64 + lane) * 4 + r)] = (int32_t)(boff[t / 8] + nf);
        }
}

// the action table of one wave (mz_fused.hip.h): T[a][tile 0..15][g 0..3][r 0..3] = W[nf][50 + a] + b[nf] -- what lane row g
// holds of accumulator tile `tile` (head tile / 8, feature nf = 128 w + 16 (tile % 8) + 4 g + r) once the one-hot columns
// and the bias are in.  Scale class 1: it is part of the fc1 layer.  Actions >= A stay zero.
static void fill_action_table(PackPlan &p, size_t pos, int w, const size_t *woff, const size_t *boff, int K, int A) {
  for (int a = 0; a < A && a < MZ_ATAB_AMAX; ++a)
    for (int t = 0; t < 16; ++t)
      for (int g = 0; g < 4; ++g)
        for (int r = 0; r < 4; ++r) {
          const int head = t / 8, nf = 128 * w + 16 * (t % 8) + 4 * g + r;
          const size_t o = pos + (size_t)a * 256 + t * 16 + g * 4 + r;
          p.idx[o] = (int32_t)(woff[head] + (size_t)nf * K + MZ_H + a) | (1 << 29);
          p.idx2[o] = (int32_t)(boff[head] + nf);
        }
}

// fc2 pack: [JT][4 waves][8 tiles][64][4]: A operand row j = 16jt + (lane&15), k = 128w + 16t + 4(lane>>4) + r
static void fill_fc2(PackPlan &p, size_t wpos, int JT, size_t woff, int J) {
  for (int jt = 0; jt < JT; ++jt)
    for (int w = 0; w < 4; ++w)
      for (int t = 0; t < 8; ++t)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + (lane & 15), nf = 128 * w + 16 * t + 4 * (lane >> 4) + r;
            p.idx[wpos + ((((size_t)(jt * 4 + w) * 8 + t) * 64 + lane) * 4 + r)] = j < J ? (int32_t)(woff + (size_t)j * MZ_F + nf) : -1;
          }
}

// small-MFMA pack, [4 waves][8 tiles][64][4]: lane l carries output row row0 + (l & 3) (< J) for the features 128w + 16t + 4(l >> 4) + r
static void fill_fc2_rows4(PackPlan &p, size_t wpos, size_t woff, int row0, int J) {
  for (int w = 0; w < 4; ++w)
    for (int t = 0; t < 8; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r) {
          const int j = row0 + (lane & 3), nf = 128 * w + 16 * t + 4 * (lane >> 4) + r;
          p.idx[wpos + (((size_t)(w * 8 + t) * 64 + lane) * 4 + r)] = j < J ? (int32_t)(woff + (size_t)j * MZ_F + nf) : -1;
        }
}

static void fill_vec(PackPlan &p, size_t pos, int padded, size_t off, int n) {
  for (int i = 0; i < padded; ++i) p.idx[pos + i] = i < n ? (int32_t)(off + i) : -1;
}

// A wave's stream in consumption order: pieces of 256 floats ([64 lanes][4]) copied from the packs above.  cls: the scale class of the
// piece (bits 29-30 of its gather indices, k_pack_weights): 0 = unscaled, 1 = an fc1 layer of the search (times 2^-k), 2 = a layer
// that consumes its activations (times 2^k) -- k_relu_scale, mz_fused.hip.h
struct PieceWriter {
  PackPlan &p;
  size_t base, piece;
  bool addends;      // the stream takes pieces that carry idx2 (the fused stream's dynamics fc1; none of the root's does)
  void put(size_t src, int cls) {
    const size_t d0 = base + piece * 256;
    for (int i = 0; i < 256; ++i) p.idx[d0 + i] = p.idx[src + i] < 0 ? -1 : (p.idx[src + i] | (cls << 29));
    if (addends)
      for (int i = 0; i < 256; ++i) p.idx2[d0 + i] = p.idx2[src + i];
    ++piece;
  }
  // the ks steps of wave w of an fc1 pack; tile t of wave w of output tile jt of an fc2 pack
  void fc1(size_t pack, int w, int ks) {
    for (int st = 0; st < ks; ++st)
      for (int tg = 0; tg < 4; ++tg) put(pack + ((size_t)(w * 4 + tg) * ks + st) * 256, 1);
  }
  void fc2(size_t pack, int jt, int w, int t, int cls) { put(pack + ((size_t)(jt * 4 + w) * 8 + t) * 256, cls); }
};

// ---- split-f16 weight stream (mz_fused_h2.hip.h): per wave [NGROUPS][8 pieces][64 lanes][8 halfs]; a group = the A operands of four
// 16 x 32 blocks ("units"): pieces 0..3 their high parts, 4..7 their low parts.  Lane l of a piece holds row l & 15, k = 8 (l >> 4) + j
// of the block.  A unit of wave w is
//   H2_FC1  a block of an fc1 layer pair (layer 0 reward | transition, K1 = 50 + A; 1 value | policy, K1 = 50): tile a of the wave (head
//           a / 8, feature 128 w + 16 (a % 8) + row), K chunk b; column K1 = bias
//   H2_FC2  a block of an output layer (0 reward, 1 transition, 2 value, 3 policy): output rows 16 a + row (< J), K pair b of the wave's
//           eight tiles of the head: k = 8 g + j  <->  feature 128 w + 16 (2 b + (j >= 4)) + 4 g + (j & 3)   (the D fragments of tiles
//           2b, 2b+1)
enum H2Kind { H2_FC1, H2_FC2 };
struct H2Unit { H2Kind kind; int layer, a, b; };
struct H2Group { H2Unit u[4]; };
#define H2_TG(L, TG, C) {{{H2_FC1, L, 4 * (TG), C}, {H2_FC1, L, 4 * (TG) + 1, C}, {H2_FC1, L, 4 * (TG) + 2, C}, {H2_FC1, L, 4 * (TG) + 3, C}}}
#define H2_FC1_STAGE(L) H2_TG(L, 0, 0), H2_TG(L, 0, 1), H2_TG(L, 1, 0), H2_TG(L, 1, 1), H2_TG(L, 2, 0), H2_TG(L, 2, 1), H2_TG(L, 3, 0), H2_TG(L, 3, 1)
#define H2_REW(OT, P) {H2_FC2, 0, OT, P}
#define H2_TR(OT, P) {H2_FC2, 1, OT, P}
#define H2_VAL(OT, P) {H2_FC2, 2, OT, P}
#define H2_POL(P) {H2_FC2, 3, 0, P}
// the groups in consumption order, stage by stage (H2Sched)
static constexpr H2Group H2_STAGE_D1[] = {H2_FC1_STAGE(0)};
static constexpr H2Group H2_STAGE_D2[] = {
    {{H2_REW(0, 0), H2_REW(1, 0), H2_TR(0, 0), H2_TR(1, 0)}}, {{H2_REW(0, 1), H2_REW(1, 1), H2_TR(0, 1), H2_TR(1, 1)}},
    {{H2_TR(2, 0), H2_TR(3, 0), H2_TR(2, 1), H2_TR(3, 1)}},
    {{H2_REW(0, 2), H2_REW(1, 2), H2_TR(0, 2), H2_TR(1, 2)}}, {{H2_REW(0, 3), H2_REW(1, 3), H2_TR(0, 3), H2_TR(1, 3)}},
    {{H2_TR(2, 2), H2_TR(3, 2), H2_TR(2, 3), H2_TR(3, 3)}}};
static constexpr H2Group H2_STAGE_P1[] = {H2_FC1_STAGE(1)};
static constexpr H2Group H2_STAGE_P2[] = {{{H2_VAL(0, 0), H2_VAL(1, 0), H2_VAL(0, 1), H2_VAL(1, 1)}},
                                          {{H2_VAL(0, 2), H2_VAL(1, 2), H2_VAL(0, 3), H2_VAL(1, 3)}},
                                          {{H2_POL(0), H2_POL(1), H2_POL(2), H2_POL(3)}}};
#define H2_LEN(T) (int)(sizeof(T) / sizeof *(T))
static_assert(H2_LEN(H2_STAGE_D1) == H2Sched::D1 && H2_LEN(H2_STAGE_D2) == H2Sched::D2 && H2_LEN(H2_STAGE_P1) == H2Sched::P1 &&
              H2_LEN(H2_STAGE_P2) == H2Sched::P2, "the split-f16 stream holds the groups the kernel's stages consume");
static const struct { const H2Group *g; int n; } H2_STAGES[4] = {{H2_STAGE_D1, H2Sched::D1}, {H2_STAGE_D2, H2Sched::D2},
                                                                 {H2_STAGE_P1, H2Sched::P1}, {H2_STAGE_P2, H2Sched::P2}};
#undef H2_TG
#undef H2_FC1_STAGE
#undef H2_REW
#undef H2_TR
#undef H2_VAL
#undef H2_POL
#undef H2_LEN

// source index of (row 0..15, k 0..31) of one unit of wave w, or -1
static int32_t h2_source(const H2Unit &u, const PackShape &s, const FlatLayout &L, int w, int row, int kl) {
  if (u.kind == H2_FC1) {
    const size_t woff[2][2] = {{L.rew_w1, L.tr_w1}, {L.val_w1, L.pol_w1}}, boff[2][2] = {{L.rew_b1, L.tr_b1}, {L.val_b1, L.pol_b1}};
    const int K1 = u.layer == 0 ? MZ_H + s.A : MZ_H;
    const int head = u.a / 8, nf = 128 * w + 16 * (u.a % 8) + row, k = 32 * u.b + kl;
    if (k < K1) return (int32_t)(woff[u.layer][head] + (size_t)nf * K1 + k);
    if (k == K1) return (int32_t)(boff[u.layer][head] + nf);
    return -1;
  }
  const size_t woff[4] = {L.rew_w2, L.tr_w2, L.val_w2, L.pol_w2};
  const int J[4] = {s.Sr, MZ_H, s.Sv, s.A};
  const int r = 16 * u.a + row, g = kl / 8, j = kl % 8;
  if (r >= J[u.layer]) return -1;
  const int feat = 128 * w + 16 * (2 * u.b + (j >= 4 ? 1 : 0)) + 4 * g + (j & 3);
  return (int32_t)(woff[u.layer] + (size_t)r * MZ_F + feat);
}

static void pack_plan_h2(const PackShape &s, PackPlan &p) {
  const FlatLayout &L = p.L;
  p.ngroups = H2Sched::NGROUPS;
  const size_t per_wave = (size_t)H2Sched::NGROUPS * 8 * 512;
  p.n_packed_h2 = 4 * per_wave;
  p.idx_h2.assign(p.n_packed_h2, -1);
  for (int w = 0; w < 4; ++w) {
    size_t group = 0;
    for (const auto &stage : H2_STAGES)
      for (int gi = 0; gi < stage.n; ++gi, ++group)
        for (int part = 0; part < 2; ++part)
          for (int u = 0; u < 4; ++u) {
            const size_t base = (size_t)w * per_wave + (group * 8 + (size_t)part * 4 + u) * 512;
            for (int lane = 0; lane < 64; ++lane)
              for (int j = 0; j < 8; ++j) {
                const int32_t sidx = h2_source(stage.g[gi].u[u], s, L, w, lane & 15, 8 * (lane >> 4) + j);
                p.idx_h2[base + (size_t)lane * 8 + j] = sidx < 0 ? -1 : (sidx | (part ? 0x40000000 : 0));
              }
          }
  }
}

// The plan of a shape; 0, or -1 with err set.
static int pack_plan(const PackShape &s, PackPlan &p, std::string &err) {
  char msg[160];
  const int O = s.O, A = s.A, Sv = s.Sv, Sr = s.Sr, jtp = s.jtp;
  const FlatLayout L = flat_layout(O, A, Sv, Sr);
  p.L = L;
  if (L.total >= ((size_t)1 << 29)) {
    snprintf(msg, sizeof msg, "internal: %zu weights do not fit the gather index", L.total);
    err = msg;
    return -1;
  }
  p.ks0 = (O + 3) / 4; p.ks1 = (MZ_H + A + 3) / 4; p.ks3 = (MZ_H + 3) / 4;
  size_t pos = 0;
  auto seg = [&](size_t n) { size_t q = pos; pos += (n + 3) & ~(size_t)3; return q; };
  p.w0o = seg(4 * 4 * 8 * 256); p.b0o = seg(64);
  p.w1 = seg((size_t)4 * 4 * p.ks1 * 256); p.b1 = seg(4 * 16 * 256); p.w2 = seg(6 * 4 * 8 * 256); p.b2 = seg(96);
  p.w3 = seg((size_t)4 * 4 * p.ks3 * 256); p.b3 = seg(4 * 16 * 256);
  p.w4 = seg((size_t)(2 + jtp) * 4 * 8 * 256); p.b4 = seg(32 + 16 * jtp);
  p.lnw = seg(64); p.lnb = seg(64);
  // fused kernel: fc1 weights with the bias inside the packed matrix -- prediction: one more input column (constant-1 input);
  // dynamics: added to the one-hot columns (FC1_FOLDBIAS); the k-step count is that of the kernel instantiation chosen for this action
  // count (zero-padded above 50+A)
  // (rows with an action table: K = 50, 13 k-steps; the one-hot columns + bias are the table behind each wave's stream)
  const bool atab = mz_fused_atab(s.ks1, jtp, s.g);
  const int ks1f = mz_fused_fc1(s.ks1, atab), ks3f = mz_pred_fc1(), nj2 = 2 + jtp;
  p.w1f = seg((size_t)4 * 4 * ks1f * 256); p.w3f = seg((size_t)4 * 4 * ks3f * 256);
  p.nsteps = mz_fused_nsteps(s.ks1, jtp, atab);
  p.wstride = (size_t)p.nsteps * 4 * 256 + (atab ? MZ_ATAB_WAVE_FLOATS : 0);
  p.ws = seg(4 * p.wstride);
  // A operands of the small MFMA (mz_fused.hip.h): rows 48..51 of the next hidden state; the policy head when A <= 4
  p.h4 = seg((size_t)4 * 8 * 256); p.p4 = seg((size_t)4 * 8 * 256);
  const bool p4 = A <= 4;
  // root kernel stream: [nst0 first-stage steps][8 representation-out][13 prediction fc1][2*nj2 prediction out]
  p.nst0 = mz_root_nst0(O);
  p.nroot = p.nst0 + mz_root_ns(jtp);
  p.is = seg((size_t)4 * p.nroot * 4 * 256);
  p.n_packed = pos;
  p.idx.assign(pos, -1);
  p.idx2.assign(pos, -1);
  const size_t dyn_w[2] = {L.rew_w1, L.tr_w1}, dyn_b[2] = {L.rew_b1, L.tr_b1};
  const size_t pred_w[2] = {L.val_w1, L.pol_w1}, pred_b[2] = {L.val_b1, L.pol_b1};
  fill_fc2(p, p.w0o, 4, L.rep_w2, MZ_H);
  fill_vec(p, p.b0o, 64, L.rep_b2, MZ_H);
  fill_fc1(p, p.w1, dyn_w, dyn_b, MZ_H + A, p.ks1, FC1_PLAIN, MZ_H + A);
  fill_fc1_bias(p, p.b1, dyn_b);
  fill_fc2(p, p.w2, 2, L.rew_w2, Sr);
  fill_fc2(p, p.w2 + (size_t)2 * 4 * 8 * 256, 4, L.tr_w2, MZ_H);
  fill_vec(p, p.b2, 32, L.rew_b2, Sr);
  fill_vec(p, p.b2 + 32, 64, L.tr_b2, MZ_H);
  fill_fc1(p, p.w3, pred_w, pred_b, MZ_H, p.ks3, FC1_PLAIN, MZ_H);
  fill_fc1_bias(p, p.b3, pred_b);
  fill_fc2(p, p.w4, 2, L.val_w2, Sv);
  fill_fc2(p, p.w4 + (size_t)2 * 4 * 8 * 256, jtp, L.pol_w2, A);
  fill_vec(p, p.b4, 32, L.val_b2, Sv);
  fill_vec(p, p.b4 + 32, 16 * jtp, L.pol_b2, A);
  fill_vec(p, p.lnw, 64, L.ln_w, MZ_H);
  fill_vec(p, p.lnb, 64, L.ln_b, MZ_H);
  fill_fc1(p, p.w1f, dyn_w, dyn_b, MZ_H + A, ks1f, FC1_FOLDBIAS, atab ? MZ_H : MZ_H + A);
  fill_fc1(p, p.w3f, pred_w, pred_b, MZ_H, ks3f, FC1_BIASCOL, MZ_H);
  fill_fc2_rows4(p, p.h4, L.tr_w2, 48, MZ_H);
  fill_fc2_rows4(p, p.p4, L.pol_w2, 0, A);

  // the fused kernel's weight stream: per wave [nsteps][4 pieces][64 lanes][4], consumption order
  const int real_steps = mz_fused_real(s.ks1, jtp, atab);
  for (int w = 0; w < 4; ++w) {
    PieceWriter out{p, p.ws + (size_t)w * p.wstride, 0, true};
    out.fc1(p.w1f, w, ks1f);
    for (int t = 0; t < 8; ++t)
      for (int jt = 0; jt < 6; ++jt)
        if (jt == 5) out.put(p.h4 + (size_t)(w * 8 + t) * 256, 2);
        else out.fc2(p.w2, jt, w, t, 2);
    out.fc1(p.w3f, w, ks3f);
    for (int t = 0; t < 8; ++t)
      for (int jt = 0; jt < nj2; ++jt)
        if (p4 && jt == 2) out.put(p.p4 + (size_t)(w * 8 + t) * 256, 2);
        else out.fc2(p.w4, jt, w, t, 2);
    if ((int)out.piece != real_steps * 4) {
      snprintf(msg, sizeof msg, "internal: weight stream has %zu pieces, expected %d", out.piece, real_steps * 4);
      err = msg;
      return -1;
    }
    // the remaining (nsteps - real_steps) * 4 pieces are padding (index -1 -> 0.0), loaded but never used
    if (atab) fill_action_table(p, out.base + (size_t)p.nsteps * 4 * 256, w, dyn_w, dyn_b, MZ_H + A, A);
  }

  // the root kernel's stream (mz_root.hip.h).  First stage, wave w, step st, piece q: k-step 2*st + (q>>1),
  // tiles 4*(q&1)..+3 of the wave's 8 (features 128w + 16*tile + (lane&15)), k = 4*kstep + (lane>>4); column O
  // carries the bias.
  for (int w = 0; w < 4; ++w) {
    PieceWriter out{p, p.is + (size_t)w * p.nroot * 4 * 256, (size_t)p.nst0 * 4, false};
    for (int st = 0; st < p.nst0; ++st)
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int i = 0; i < 4; ++i) {
            const int tile = 4 * (q & 1) + i, nf = 128 * w + 16 * tile + (lane & 15);
            const int k = 4 * (2 * st + (q >> 1)) + (lane >> 4);
            int32_t v = -1;
            if (k < O) v = (int32_t)(L.rep_w1 + (size_t)nf * O + k);
            else if (k == O) v = (int32_t)(L.rep_b1 + nf);
            p.idx[out.base + ((size_t)(st * 4 + q) * 64 + lane) * 4 + i] = v;
          }
    // (the root's prediction stage shares the search's scaled layers: its v_max ReLU is scale-blind; the representation
    // layers take raw observations, for which no bound exists: unscaled)
    for (int t = 0; t < 8; ++t)
      for (int jt = 0; jt < 4; ++jt) out.fc2(p.w0o, jt, w, t, 0);
    out.fc1(p.w3f, w, ks3f);
    for (int t = 0; t < 8; ++t)
      for (int jt = 0; jt < nj2; ++jt) out.fc2(p.w4, jt, w, t, 2);
    if ((int)out.piece != p.nroot * 4) {
      snprintf(msg, sizeof msg, "internal: root stream has %zu pieces, expected %d", out.piece, p.nroot * 4);
      err = msg;
      return -1;
    }
  }

  p.n_packed_h2 = 0;
  p.ngroups = 0;
  p.idx_h2.clear();
  if (s.split_f16) pack_plan_h2(s, p);
  return 0;
}

// the plan's numbers in the order mz_pack_host reports them (include/mz_engine_debug.h: MZ_PACK_FIELDS)
static void pack_plan_record(const PackPlan &p, long long *out) {
  const size_t f[] = {p.L.total, p.n_packed, p.w0o, p.b0o, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, p.w4, p.b4, p.lnw, p.lnb, p.w1f, p.w3f,
                      p.ws, p.h4, p.p4, p.is, p.wstride, p.n_packed_h2};
  const int g[] = {p.ks0, p.ks1, p.ks3, p.nsteps, p.nst0, p.nroot, p.ngroups};
  int n = 0;
  for (size_t v : f) out[n++] = (long long)v;
  for (int v : g) out[n++] = v;
}
