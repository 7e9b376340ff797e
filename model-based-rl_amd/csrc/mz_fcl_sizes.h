// mz_fcl_sizes.h -- the sizes the learner step's kernels (mz_fcl.hip.h) and its host-side plan (mz_fcl_plan.inc) agree on: workgroup
// shape and dynamic LDS per launch.  Plain macros, no device code: a host-only program can include this file.
#pragma once

#define FCL_NW 8                    // waves per workgroup of the chain and heads kernels
#define FCL_THREADS (FCL_NW * 64)
#define FCL_MAXP 8                  // unroll positions K + 1

// LDS of the heads kernel (floats): X [1024] | A1 [8192] | red [8192] | Y [1024] | S [1024] | PV [576] (PV: the small
// parameter vectors, read once per launch): two workgroups per CU
#define FCL_LDS_HEADS (1024 + 8192 + 8192 + 1024 + 1024 + 576)

// LDS of the chain kernels (floats), G groups of 4 samples, activations SAMPLE-major: X [4 G][xq + 4] | A1 [4 G][516] | red [G][2048] | misc [16] | PV [1408] | S [4 G][64]
#define FCL_LDS4_FLOATS(xq, G) (4 * (G) * ((xq) + 4) + 4 * (G) * 516 + (G) * 2048 + 16 + 1408 + 256 * (G))
#define FCL_LDA 516

// a weight-gradient job's tile, NA x 16 rows of dW by NI x 16 columns, on NW waves (fcl_dw_job)
#define FCL_DW_Q(NA, NI) ((NA) * (4 * (NI) + 1))                                   // floats per lane a wave leaves in LDS
#define FCL_DW_LDS(NW, NA, NI) (((NW) * FCL_DW_Q(NA, NI) * 64 + 4) * 4)            // bytes: the waves' partial tiles + the two bias corrections
