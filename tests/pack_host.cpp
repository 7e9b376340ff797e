// pack_host.cpp -- pack_plan (csrc/mz_pack.inc), the pure function that builds the weight streams' gather tables, compiled into a
// stand-alone program.  tests/test_pack_cpu.py builds it with the host compiler under AddressSanitizer + UBSan and runs it.  No GPU is
// touched.
//   (no argument)  the whole case grid of tests/golden/pack_sha256.json: every plan is built under the sanitizers -- that run is what
//                  this program is for -- and its fields are held to each other, every index to its range and every segment to its
//                  place.  (That the lengths are the schedules' own is test_pack_cpu.py's check, against formulas restated there: here
//                  it would compare mz_stream_sizes.h with itself.)  Output: "ok <cases>"; a disagreement prints "MISMATCH ..." and
//                  exits 1.
//   --dump         cases "O A Sv Sr split" from stdin -> per case the record, idx, idx2 and idx_h2 on stdout, binary (the format of
//                  scripts/make_pack_goldens.py's program for the parent commit)
//   --time N       seconds per pack_plan (A = 4, O = 8, no split-f16 stream), mean of N
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "mz_pack.inc"
#include "mz_kernels.inc"
#include "mz_engine_debug.h"      // MZ_PACK_FIELDS

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

struct Row { int amax, ks1, jtp, g; };
#define MZ_ROW_F(AMAX, KS1, JTP, G) {AMAX, KS1, JTP, G},
static const Row ROWS[] = {MZ_FUSED_ROWS(MZ_ROW_F)};

static PackShape shape_of(int O, int A, int Sv, int Sr, int split) {
  for (const Row &r : ROWS)
    if (A <= r.amax) return PackShape{O, A, Sv, Sr, r.ks1, r.jtp, r.g, split != 0};
  CHECK(false, "no row for %d actions", A);
  return PackShape{};
}

static void check_plan(const PackShape &s, const PackPlan &p) {
  const bool atab = mz_fused_atab(s.ks1, s.jtp, s.g);
  CHECK(p.wstride == (size_t)p.nsteps * 1024 + (atab ? MZ_ATAB_WAVE_FLOATS : 0), "A %d: wave stride", s.A);
  CHECK(p.idx.size() == p.n_packed && p.idx2.size() == p.n_packed && p.idx_h2.size() == p.n_packed_h2, "A %d: table sizes", s.A);
  CHECK(p.n_packed_h2 == (size_t)4 * p.ngroups * 8 * 512 && (p.ngroups != 0) == s.split_f16, "A %d: split-f16 size", s.A);
  // the segments tile the packed vector in their order, 16-byte aligned, the root's stream last
  const size_t seg[] = {p.w0o, p.b0o, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, p.w4, p.b4, p.lnw, p.lnb, p.w1f, p.w3f, p.ws, p.h4, p.p4, p.is, p.n_packed};
  CHECK(seg[0] == 0, "first segment");
  for (size_t i = 1; i < sizeof seg / sizeof *seg; ++i) CHECK(seg[i] > seg[i - 1] && seg[i] % 4 == 0, "A %d: segment %zu", s.A, i);
  CHECK(p.is + (size_t)4 * p.nroot * 1024 == p.n_packed && p.ws + 4 * p.wstride == p.h4, "A %d: stream extents", s.A);
  for (size_t i = 0; i < p.n_packed; ++i) {
    CHECK(p.idx[i] >= -1 && (p.idx[i] < 0 || ((size_t)(p.idx[i] & 0x1fffffff) < p.L.total && (p.idx[i] >> 29) < 3)), "A %d: idx[%zu]", s.A, i);
    CHECK(p.idx2[i] >= -1 && (p.idx2[i] < 0 || ((size_t)p.idx2[i] < p.L.total && p.idx[i] >= 0)), "A %d: idx2[%zu]", s.A, i);
  }
  for (size_t i = 0; i < p.n_packed_h2; ++i)
    CHECK(p.idx_h2[i] >= -1 && (p.idx_h2[i] < 0 || (size_t)(p.idx_h2[i] & 0x3fffffff) < p.L.total), "A %d: idx_h2[%zu]", s.A, i);
}

int main(int argc, char **argv) {
  PackPlan p;
  std::string err;
  if (argc == 3 && !strcmp(argv[1], "--time")) {
    const int n = atoi(argv[2]);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) CHECK(pack_plan(shape_of(8, 4, 31, 31, 0), p, err) == 0, "%s", err.c_str());
    printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--dump")) {
    int O, A, Sv, Sr, split;
    while (scanf("%d %d %d %d %d", &O, &A, &Sv, &Sr, &split) == 5) {
      CHECK(pack_plan(shape_of(O, A, Sv, Sr, split), p, err) == 0, "%s", err.c_str());
      long long rec[MZ_PACK_FIELDS];
      pack_plan_record(p, rec);
      fwrite(rec, sizeof rec, 1, stdout);
      fwrite(p.idx.data(), 4, p.idx.size(), stdout);
      fwrite(p.idx2.data(), 4, p.idx2.size(), stdout);
      fwrite(p.idx_h2.data(), 4, p.idx_h2.size(), stdout);
    }
    return 0;
  }
  static const int ACTIONS[] = {1, 2, 4, 5, 6, 8, 9, 10, 13, 14, 16, 17, 21, 22, 32}, OBS[] = {1, 4, 27, 128, 257};
  static const int SUPPORTS[][2] = {{31, 31}, {1, 1}, {32, 32}, {21, 5}};
  long cases = 0;
  for (int A : ACTIONS)
    for (int O : OBS)
      for (const auto &S : SUPPORTS) {
        const PackShape s = shape_of(O, A, S[0], S[1], A <= MZ_H2_MAXA);
        CHECK(pack_plan(s, p, err) == 0, "%s", err.c_str());
        check_plan(s, p);
        ++cases;
      }
  // more weights than a gather index can name: refused, in words, before anything is built
  CHECK(pack_plan(shape_of(1 << 20, 4, 31, 31, 0), p, err) == -1 && err.find("do not fit the gather index") != std::string::npos, "the index check");
  printf("ok %ld\n", cases);
  return 0;
}
