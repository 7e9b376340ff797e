// mz_inst.hip -- one translation unit per search-kernel shape: compiled with -DMZ_INST_F=KS1,JTP,G (k_search_fused) or
// -DMZ_INST_H=G (k_search_h2), it defines every variant of that shape (mz_kernels.inc); mz_engine.hip launches them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mz_engine.h"
#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS
#include "mz_common.h"
#include "mz_net.hip.h"
#include "mz_rng.h"
#include "mz_tree.hip.h"
#include "mz_selfplay.hip.h"
#include "mz_fused.hip.h"
#include "mz_root.hip.h"
#include "mz_fused_h2.hip.h"
#include "mz_kernels.inc"

#define MZ_KF(S, ...) template __global__ void k_search_fused<MZ_UNPACK S, __VA_ARGS__> MZ_KARGS;
#define MZ_KH(S, ...) template __global__ void k_search_h2<MZ_UNPACK S, __VA_ARGS__> MZ_KARGS;
#if defined(MZ_INST_F)
MZ_VARIANTS_FUSED(MZ_KF, (MZ_INST_F))
#ifdef MZ_INST_GAME      // (the unit of MZ_GAME_SHAPE) whole moves of the device TicTacToe environment
MZ_GAME_VARIANT(MZ_KF)
#endif
#ifdef MZ_INST_CART      // (the unit of MZ_CART_SHAPE) whole moves of the device CartPole environment
MZ_CART_VARIANT(MZ_KF)
#endif
#ifdef MZ_INST_C4        // (the unit of MZ_C4_SHAPE) whole moves of the device Connect Four environment
MZ_C4_VARIANTS(MZ_KF)
#endif
#elif defined(MZ_INST_H)
MZ_VARIANTS_H2(MZ_KH, (MZ_INST_H))
#else
#error "compile with -DMZ_INST_F=KS1,JTP,G or -DMZ_INST_H=G"
#endif
