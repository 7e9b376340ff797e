// fcl_plan_host.cpp -- fcl_plan (csrc/mz_fcl_plan.inc), the pure function that decides a learner step's shape, compiled into a
// stand-alone program and run over a grid wider than any test creates handles for: every batch that is a multiple of 16 up to 1024
// and the large ones, three network shapes, four CU counts, every knob set.  tests/test_fcl_plan_cpu.py builds it with the host pass
// of hipcc and -fsanitize=address,undefined and runs it.  No GPU is touched.
//
// Every plan is held to what the step's code relies on: the chain workgroups cover the batch; one row slab means one group; the
// backward chain rides in the forward launch only where the forward is one launch; the heads' jobs are among the jobs; the tapes
// lie apart in order and inside their allocation; the staging sections lie apart and inside a slot; no launch of an accepted shape
// asks for more LDS than a workgroup can have.  Output: "ok <plans>"; a disagreement prints "MISMATCH ..." and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "mz_common.h"
#include "mz_fcl_sizes.h"
#include "mz_fcl_plan.inc"

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static long check_plan(int batch, int K, int O, int A, int Sv, int Sr, int cus, const FclKnobs &kn) {
  const FclPlan p = fcl_plan(batch, K, O, A, Sv, Sr, cus, kn);
#define WHERE "batch %d K %d O %d A %d cus %d knobs %d %d %d %d %d: "
#define ARGS batch, K, O, A, cus, kn.groups, kn.slabs, kn.fuse_fwd, kn.fuse_fb, kn.fb_jobs
  CHECK(p.G == 1 || p.G == 2 || p.G == 4, WHERE "G %d", ARGS, p.G);
  CHECK(p.nwg * 4 * p.G == batch && p.nln * 4 == batch, WHERE "nwg %d G %d", ARGS, p.nwg, p.G);
  CHECK(p.S >= 1 && p.S <= batch / 16 && (p.S != 1 || p.G == 1), WHERE "S %d G %d", ARGS, p.S, p.G);
  CHECK(!fcl_fuse_fb(p) || fcl_fuse_fwd(p), WHERE "fuse_fb without fuse_fwd", ARGS);
  CHECK((p.fwd == FCL_FWD_FB) == (p.bwd == FCL_BWD_FB) && (p.bwd == FCL_BWD_SLABS) == (p.S > 1), WHERE "forms %d %d S %d", ARGS, p.fwd, p.bwd, p.S);
  CHECK(!fcl_fuse_fwd(p) || (p.S == 1 && p.G == 1 && cus >= p.nwg && p.lds_bytes <= (size_t)FCL_LDS_HEADS * 4), WHERE "the fused forward", ARGS);
  CHECK(!fcl_fuse_fb(p) || (batch <= 256 && cus >= 2 * p.nwg && p.tapes_fit), WHERE "the fused backward", ARGS);
  CHECK(p.KP >= p.KD && (p.KP == 56 || p.KP == 64) && p.xq >= O && p.XR >= O, WHERE "KP %d xq %d XR %d", ARGS, p.KP, p.xq, p.XR);
  CHECK(p.njobs_heads > 0 && p.njobs_heads < p.njobs, WHERE "jobs %d %d", ARGS, p.njobs_heads, p.njobs);
  CHECK(p.lds_bwd_dw >= p.lds_bytes && p.lds_dwa > 0, WHERE "LDS", ARGS);
  if (fcl_plan_fits(p))
    CHECK(p.lds_bytes <= FCL_LDS_MAX && p.lds_bwd_dw <= FCL_LDS_MAX && p.lds_dwa <= FCL_LDS_MAX, WHERE "LDS %zu %zu %d", ARGS, p.lds_bytes, p.lds_bwd_dw, p.lds_dwa);
  size_t end = 0;
  for (int i = 0; i < FCL_NTAPES; ++i) {
    CHECK(p.tape[i].name && p.tape[i].floats > 0 && p.tape[i].off >= end && p.tape[i].off % 16 == 0, WHERE "tape %d", ARGS, i);
    end = p.tape[i].off + p.tape[i].floats;
  }
  CHECK(end <= p.tape_floats && p.tapes_fit == (p.tape_floats * 4 <= 0x7fffffffull), WHERE "the tapes' allocation", ARGS);
  for (int i = 0; i < 6; ++i) CHECK(p.soff[i] % 16 == 0 && (i == 0 ? p.soff[0] == 0 : p.soff[i] > p.soff[i - 1]), WHERE "staging section %d", ARGS, i);
  CHECK(p.soff_lr >= p.soff[5] + (size_t)batch * 8 && p.stage_bytes >= p.soff_lr + 4, WHERE "the staging slot", ARGS);
  CHECK(p.nflags >= 2 * (batch / 16) * (K + 1), WHERE "nflags %d", ARGS, p.nflags);
  return 1;
}

int main() {
  const int shapes[3][2] = {{8, 4}, {42, 7}, {128, 6}};
  const int cu_counts[4] = {64, 128, 256, 304};
  const FclKnobs knob_sets[9] = {{}, {-1, -1, -1, 0, -1}, {-1, -1, 0, -1, -1}, {-1, -1, 1, -1, -1}, {-1, -1, -1, -1, 0},
                                 {2, 2, -1, -1, -1}, {4, 4, -1, -1, -1}, {-1, 3, -1, -1, -1}, {-1, 2, -1, -1, -1}};
  long plans = 0;
  for (const auto &sh : shapes)
    for (int cus : cu_counts)
      for (const FclKnobs &kn : knob_sets) {
        for (int batch = 16; batch <= 1024; batch += 16) plans += check_plan(batch, 5, sh[0], sh[1], 31, 31, cus, kn);
        for (int batch : {2048, 4096, 8192, 16384}) plans += check_plan(batch, 5, sh[0], sh[1], 31, 31, cus, kn);
      }
  // the limits mz_fcl_create takes: one and seven unroll steps, one bin, 1024 observation features, 14 actions; tapes past 2 GB
  for (int batch : {16, 256, 4096}) {
    plans += check_plan(batch, 1, 8, 4, 1, 1, 256, {});
    plans += check_plan(batch, 7, 1024, 14, 64, 64, 256, {});
    plans += check_plan(batch, 7, 1024, 14, 64, 64, 256, {4, 4, -1, -1, -1});
  }
  plans += check_plan(65536, 7, 1024, 1, 31, 31, 256, {});
  printf("ok %ld\n", plans);
  return 0;
}
