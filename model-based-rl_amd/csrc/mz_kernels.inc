// mz_kernels.inc -- the shapes and variants of the two search kernels (mz_fused.hip.h, mz_fused_h2.hip.h), listed once.
// From these lists come the explicit instantiations (mz_inst.hip: ONE shape per translation unit -- _abi.build() reads
// the rows below and compiles those units in parallel, the 128 instantiations take six minutes in one unit), the
// `extern template` declarations and the host table of kernel addresses of mz_engine.hip (which launches them and does
// not compile them), and the engine's action count -> shape mapping (mz_create).
#define MZ_KARGS \
  (NetView, TreeView, const f32x4 *, int, int, unsigned long long *, SelfplayState, int, uint64_t, MzRootArgs)

// ---- shapes, one row each; an engine runs the first row whose largest action count is >= its own.
// k_search_fused: X(largest action count, fc1 k-steps KS1, policy tiles JTP, lanes per child group G)
// (dynamics fc1: K = 50 + A columns in k-steps of 4 -- the bias rides in the one-hot columns, fill_fc1_foldbias)
// (the A <= 4 row: its one-hot columns + bias come out of an action table instead, mz_fused_atab in mz_fused.hip.h -- the
// kernel then runs 13 k-steps; KS1 = 14 stays the row's label, the schedule derives its own step count from it)
// k_search_h2:    X(largest action count, lanes per child group G)
// _DEV: the two bench shapes, all that -DMZ_DEV_ONLY compiles (kernel development: a quarter of the build time)
#define MZ_FUSED_ROWS_DEV(X) X(4, 14, 1, 4) X(6, 14, 1, 8)
#define MZ_FUSED_ROWS_MORE(X) X(8, 15, 1, 8) X(10, 15, 1, 16) X(13, 16, 1, 16) X(16, 18, 1, 16) X(21, 18, 2, 32) X(32, 21, 2, 32)
#define MZ_H2_ROWS_DEV(X) X(4, 4) X(8, 8)
#define MZ_H2_ROWS_MORE(X) X(13, 16)
// whole moves of the device TicTacToe environment (two players, 9 actions): one more kernel of this shape's row
#define MZ_GAME_SHAPE 15, 1, 16
// whole moves of the device CartPole environment (single player, 2 actions): one more kernel of the A <= 4 row
#define MZ_CART_SHAPE 14, 1, 4
// whole moves of the device Connect Four environment (two players, 7 actions): two more kernels of the A <= 8 row
#define MZ_C4_SHAPE 15, 1, 8

// ---- variants of a shape S, V(S, tree placement LT, phase stamps PROF, single player SP, whole moves HEAD)
// trees in LDS (LT 1 whole, 2 compact): both kernels; HEAD needs LDS trees, no stamps, a single player
#define MZ_VARIANTS_H2(V, S)                                                                                        \
  V(S, 1, false, false, false) V(S, 1, false, true, false) V(S, 1, true, false, false) V(S, 1, true, true, false) \
  V(S, 2, false, false, false) V(S, 2, false, true, false) V(S, 2, true, false, false) V(S, 2, true, true, false) \
  V(S, 1, false, true, true) V(S, 2, false, true, true)
// ... and trees in the global pool (LT 0): the exact-f32 kernel only
#define MZ_VARIANTS_FUSED(V, S)                                                                                     \
  V(S, 0, false, false, false) V(S, 0, false, true, false) V(S, 0, true, false, false) V(S, 0, true, true, false) \
  MZ_VARIANTS_H2(V, S)
// the game kernels: (S, LT, PROF, SP, HEAD, GAME); which environment a game kernel plays follows from SP and the shape
// (mz_game_kind, mz_fused.hip.h).  TicTacToe:
#define MZ_GAME_VARIANT(V) V((MZ_GAME_SHAPE), 2, false, false, true, true)
// the single-player game kernel (CartPole): whole trees in LDS, the placement of 2 actions at every simulation count the
// fused kernels take (16 trees of 1 + 63 * 2 nodes and the 8,320-byte action table fit beside the static LDS: 108,208 of
// 110,080 bytes at 62 simulations)
#define MZ_CART_VARIANT(V) V((MZ_CART_SHAPE), 1, false, true, true, true)
// Connect Four, trees of NN = 1 + (sims + 1) * 7 nodes beside 53,760 bytes of static LDS (mz_fused_dyn_lds): whole trees in
// LDS (LT 1) up to 24 simulations (106,304 bytes of dynamic LDS; 25: 110,512 > 110,080), the compact placement (LT 2) from 25
// to 48 (107,616 bytes; 49: 110,200) -- the default 30 among them; both boundaries confirmed through mz_search_kernel_info /
// mz_selfplay_moves_per_launch.  Other simulation counts play launch-per-step
#define MZ_C4_VARIANTS(V) V((MZ_C4_SHAPE), 1, false, false, true, true) V((MZ_C4_SHAPE), 2, false, false, true, true)

#define MZ_UNPACK(...) __VA_ARGS__      // MZ_UNPACK S: a shape tuple (KS1, JTP, G) / (G) as leading template arguments

// ---- every compiled kernel: define MZ_KF(S, LT, PROF, SP, HEAD) for k_search_fused, MZ_KG(S, LT, PROF, SP, HEAD,
// GAME) for its game kernel and MZ_KH(S, LT, PROF, SP, HEAD) for k_search_h2, then expand MZ_ALL_KERNELS
#define MZ_FUSED_ROWS(X) MZ_FUSED_ROWS_DEV(X) MZ_FUSED_ROWS_MORE(X)
#define MZ_H2_ROWS(X) MZ_H2_ROWS_DEV(X) MZ_H2_ROWS_MORE(X)
#define MZ_KF_ROW(AMAX, KS1, JTP, G) MZ_VARIANTS_FUSED(MZ_KF, (KS1, JTP, G))
#define MZ_KH_ROW(AMAX, G) MZ_VARIANTS_H2(MZ_KH, (G))
#ifdef MZ_DEV_ONLY
#define MZ_ALL_KERNELS MZ_FUSED_ROWS_DEV(MZ_KF_ROW) MZ_H2_ROWS_DEV(MZ_KH_ROW)
#else
#define MZ_ALL_KERNELS MZ_FUSED_ROWS(MZ_KF_ROW) MZ_GAME_VARIANT(MZ_KG) MZ_CART_VARIANT(MZ_KG) MZ_C4_VARIANTS(MZ_KG) MZ_H2_ROWS(MZ_KH_ROW)
#endif
