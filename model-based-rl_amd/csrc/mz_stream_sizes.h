// mz_stream_sizes.h -- the geometry of the per-wave weight streams, stated once: what the kernels' schedules (FusedSched, RootSched,
// H2Sched: mz_fused.hip.h, mz_root.hip.h, mz_fused_h2.hip.h) and the host's packing (mz_pack.inc) agree on.  Macros and constexpr
// functions, no device code: a host-only program can include this file.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define MZ_SIZES_FN __host__ __device__ constexpr
#else
#define MZ_SIZES_FN constexpr
#endif

#define MZ_H 50          // FCNetwork hidden_dim (reference networks.py:135)
#define MZ_F 512         // FC head width

// ---- k_search_fused (mz_fused.hip.h): steps of 16 MFMAs = 4 pieces of [64 lanes][4 floats] per wave
#ifndef MZ_NB
#define MZ_NB 4      // register ring depth in steps (prefetch distance NB-1 steps = ~1600 cycles; A/B on one box:
#endif               // 4 buffers + 13 resident steps 406 us, 5 + 12: 410, 3 + 14: 407)
// steps of the stream held in registers (AGPRs) across all simulations: less L2 traffic and no load issue in those
// steps (a streamed step runs at ~37 cycles/MFMA, a resident one at 32).  As many as the register file takes
// without scratch: the wide-action instantiations (two tree passes, two policy tiles) have fewer to spare.
#ifndef MZ_RS_MAIN
#define MZ_RS_MAIN 13
#endif
MZ_SIZES_FN int mz_fused_rs(int ks1, int jtp) { return jtp > 1 ? 9 : (ks1 > 16 ? 11 : (ks1 > 14 ? 12 : MZ_RS_MAIN)); }

// Action table (the rows of mz_kernels.inc for which mz_fused_atab holds: the A <= 4 row).  For one tree the one-hot
// columns of the dynamics fc1 contribute nothing but W[n][50 + a] + b[n], a vector chosen by the tree's action: no
// multiplication is needed for it.  The host packs that vector for every action as the accumulator tiles themselves
// (T[a][tile 0..15][lane row g][r], per wave: what lane (g, .) of tile t holds), each lane reads its column's vector
// straight into acc[0..15] before the first k-step, and that step accumulates instead of starting from zero.  The
// dynamics fc1 is then K = 50: 13 k-steps instead of 14, all of them resident.  The term is the first addend of the
// sum instead of the last: the same products in another float32 order.
// -DMZ_ACTION_COLUMNS (development switch, A/B builds): the earlier form, K = 50 + A columns.
MZ_SIZES_FN bool mz_fused_atab(int ks1, int jtp, int g) {
#ifdef MZ_ACTION_COLUMNS
  return false;
#else
  return ks1 == 14 && jtp == 1 && g == 4;
#endif
}
#define MZ_ATAB_AMAX 4                         // actions the packed table has room for (the row's largest action count)
#define MZ_ATAB_WAVE_FLOATS (MZ_ATAB_AMAX * 256)   // one wave's slice behind its weight stream: [a][16 tiles][4 g][4 r]
// LDS copy (trees in the pool or whole trees in LDS): [a][wave][256 floats], the action stride padded by 64 bytes so that
// the four actions x four lane rows of one read cover 256 distinct bytes (lanes with the same action and lane row read
// the same address: a broadcast).  Beside compact trees (lt = 2) the table stays in global memory.
#define MZ_ATAB_LDS_STRIDE (4096 + 64)
MZ_SIZES_FN size_t mz_fused_atab_lds(bool atab, int A, int lt) {
  return atab && lt != 2 ? (size_t)A * MZ_ATAB_LDS_STRIDE : 0;
}

// the per-simulation schedule, in steps (FusedSched)
// dynamics fc1: K = 50 + A (the bias rides in the one-hot columns), 4 per step; with the action table K = 50 (ks1 stays the row's label)
MZ_SIZES_FN int mz_fused_fc1(int ks1, bool atab) { return atab ? (MZ_H + 3) / 4 : ks1; }
#define MZ_FUSED_FC2 12                                                      // reward (2 tiles) + next hidden (4 tiles): 48 pieces
MZ_SIZES_FN int mz_pred_fc1() { return (MZ_H + 1 + 3) / 4; }                 // prediction fc1: K = 51 -> 13 steps
MZ_SIZES_FN int mz_pred_fc2(int jtp) { return 2 * (2 + jtp); }               // value (2 tiles) + policy (jtp tiles)
MZ_SIZES_FN int mz_fused_real(int ks1, int jtp, bool atab) { return mz_fused_fc1(ks1, atab) + MZ_FUSED_FC2 + mz_pred_fc1() + mz_pred_fc2(jtp); }
// streamed steps, padded to the ring depth (the first mz_fused_rs steps stay resident in registers for the whole launch)
MZ_SIZES_FN int mz_fused_nring(int ks1, int jtp, bool atab) {
  return (mz_fused_real(ks1, jtp, atab) - mz_fused_rs(ks1, jtp) + MZ_NB - 1) / MZ_NB * MZ_NB;
}
// schedule length incl. padding steps (prefetch only)
MZ_SIZES_FN int mz_fused_nsteps(int ks1, int jtp, bool atab) { return mz_fused_rs(ks1, jtp) + mz_fused_nring(ks1, jtp, atab); }

// ---- k_root (mz_root.hip.h): nst0 run-time first-stage steps, then the unrolled schedule (RootSched)
#define MZ_ROOT_R2 8                                                         // representation out: 4 tiles x this wave's 8 hidden tiles
MZ_SIZES_FN int mz_root_ns(int jtp) { return MZ_ROOT_R2 + mz_pred_fc1() + mz_pred_fc2(jtp); }
// steps of the run-time first stage: two k-steps of K0 = obs_dim + 1 (bias column) per step
MZ_SIZES_FN int mz_root_nst0(int O) { return ((O + 1 + 3) / 4 + 1) / 2; }

// ---- k_search_h2 (mz_fused_h2.hip.h): groups of 8 pieces of [64 lanes][8 float16] per wave
#ifndef MZ_H2_NBG
#define MZ_H2_NBG 3       // ring depth (groups)
#endif
#ifndef MZ_H2_RSG
#define MZ_H2_RSG 4       // resident groups
#endif
// (A/B on one box, us per launch of the headline workload: RSG / NBG = 4 / 3: 269, 1 / 4: 283, 5 / 2: 276 -- both the
// bytes streamed and the prefetch distance matter.  Resident groups in arch VGPRs (5 / 4 with one of them there) were
// tried: under the register pressure that creates the compiler moves operands around with VALU copies right in front of
// the asm MFMAs, whose wait states it cannot know -- wrong results on a full grid; dropped.)
#define MZ_H2_MAXA 13
struct H2Sched {
  static constexpr int D1 = 8, D2 = 6, P1 = 8, P2 = 3;                      // groups per stage
  static constexpr int E_D1 = D1, E_D2 = E_D1 + D2, E_P1 = E_D2 + P1, E_P2 = E_P1 + P2;
  static constexpr int REAL = E_P2;                                          // 25 groups = 200 KiB per wave and simulation
  static constexpr int RSG = MZ_H2_RSG, NBG = MZ_H2_NBG;
  static constexpr int NRING = (REAL - RSG + NBG - 1) / NBG * NBG;
  static constexpr int NGROUPS = RSG + NRING;
};
static_assert(H2Sched::NRING == H2Sched::REAL - H2Sched::RSG, "no padding groups: (REAL - RSG) must be a multiple of NBG");
