// mz_selfplay.hip.h -- the device-resident part of Actor.play_game (reference actors.py:126-176) for B
// synthetic fixed-length environments: observation generation, Dirichlet noise, env step and the
// experience record (what Game.apply / store_search_statistics append to History, game.py:79-115).
#pragma once
#include "mz_common.h"
#include "mz_rng.h"
#include "mz_tree.hip.h"
#include "mz_games.h"
#include "mz_record.h"

struct SelfplayState {
  int episode_len;
  int rec_floats, ring_moves;
  int32_t *t;            // [B] env._elapsed_steps
  int32_t *episode;      // [B] episodes finished
  float *obs;            // [Bp][O] current observation (History.observations[-1])
  double *temp;          // [B] visit-softmax temperature of the env's CURRENT game (actors.py:128-129: evaluated once per game)
  double *temp_next;     // [1] temperature the next game of every env starts with (mz_selfplay_set_temperature)
  const float *obs_min, *obs_rng;   // [O] --norm_obs: network input = (obs - min) / range (actors.py:55-58,134-137); null = raw
  int obs_u8;            // synthetic observations are uint8-valued (the -ram- envs: 128 bytes of console RAM), else ~N(0,1);
                         // 2: ... and the experience record carries them as BYTES, four per float slot (obs_slots = ceil(O / 4))
  int obs_slots;         // float slots the observation takes in a record: O, or ceil(O / 4) when packed
  int export_trees;      // write the searched trees back to the global pool at the end of every move (tests / tree export)
  double *noise_log;     // [ring_moves][B][A] or null: every move's Dirichlet draw, kept per move (mz_selfplay_noise_log: the
                         // parity tests replay the moves of a whole-moves launch on the CPU with the device's own draws)
  int32_t *action;       // [B]
  double *child_visits;  // [B][A]
  double *root_value, *error;   // [B]
  unsigned long long *movecnt;   // [B] moves completed by env b (all equal; per-env so that every thread reads and
                                 // advances only its own counter): keys the RNG and the ring slot
  // ---- a real game as the environment (mz_selfplay_set_env): TicTacToe, custom_environments/tic_tac_toe.py:5-76
  int env_kind;          // 0 = synthetic fixed-length episodes (above), 1 = TicTacToe (two players, 9 cells, 9 actions),
                         // 2 = CartPole (single player, 4 observations, 2 actions, episode_len = the time limit),
                         // 3 = Connect Four (two players, 42 cells, 7 actions)
  int8_t *board;         // [B][9] env.board: 0 empty, +1 / -1 the two players' marks (Connect Four: [B][42], cell 7 * row + col)
  int8_t *turn;          // [B] env.turn == game.to_play: +1 or -1, the player about to move
  uint8_t *legal;        // [B][A] legal_actions() of the current position as a mask (actors.py:141)
  int8_t *to_play;       // [B] game.to_play of the current move (root.expand's to_play, actors.py:142)
  double *cart;          // [Bp][4] CartPole: (x, x_dot, theta, theta_dot) of the current position, float64
  const double *draw_uniform;   // [B] or null: the uniform select_action consumes, given by the host (parity runs,
                                // mz_selfplay_set_draws); null = the device RNG keyed (seed, env, move)
  int draws_noise;       // != 0: the Dirichlet draw of the coming moves is the one the host put into TreeView::noise
  float *ring;           // [ring_moves][B][rec_floats]
  float *host_ring;      // pinned staging for drains (optional)
  unsigned long long moves_host, drained;
  int env_offset;
  bool ready;
};

// Gamma(alpha) by Marsaglia-Tsang (alpha < 1: boost with U^(1/alpha)); counter-based draws.  float32 on the hardware's
// own log2 / exp2 / cos / sqrt: this is a noise source, not a parity quantity (parity runs pass numpy's draw in), and
// the float64 libm version of the same sampler cost 5.5 us of every move (a quarter of the root kernel).
// Definition (restated in float64 by tests/dirichlet_py.py, which tests/test_gpu_dirichlet.py holds every caller to): alpha
// rounded to float32; alpha' = alpha + 1 where alpha < 1; d = alpha' - 1/3, c = 1 / sqrt(9 d).  Iteration ctr = 0, 1, .. (at
// most 64; ctr advances on every iteration, the v <= 0 ones included) draws the block of counter
// (env, (uint32)move, a | ctr << 8, MZ_RNG_DIRICHLET << 24 | (move >> 32 & 0xFFFFFF)): u1 = 1 - (x >> 8) / 2^24,
// u2 = (y >> 8) / 2^24, u = 1 - (z >> 8) / 2^24, normal = sqrt(-2 ln u1) cos(2 pi u2), v = (1 + c normal)^3, accepted when
// 1 + c normal > 0 and ln u < normal^2 / 2 + d - d v + d ln v: g = d v.  alpha < 1: g *= U^(1/alpha), U = 1 - (x >> 8) / 2^24
// of the block at ctr = 0xFFFFFF.
__device__ inline float mz_u01f(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }      // [0, 1)
__device__ inline double mz_gamma(double alpha, uint64_t seed, uint32_t env, uint64_t move, uint32_t a) {
  const float al = (float)alpha;
  const float aa = al < 1.0f ? al + 1.0f : al;
  const float d = aa - 1.0f / 3.0f, c = 1.0f / __builtin_amdgcn_sqrtf(9.0f * d);
  const float LN2 = 0.69314718f;
  const uint32_t c1 = (uint32_t)move, c3 = (MZ_RNG_DIRICHLET << 24) | ((uint32_t)(move >> 32) & 0xFFFFFFu);
  float g = d;
  int k = 0;
  uint32_t ctr = 0;
  for (int it = 0; it < 64; ++it) {
    const mz_u4 r0 = mz_philox(seed, env, c1, a | (ctr++ << 8), c3);
    const float u1 = 1.0f - mz_u01f(r0.x), u2 = mz_u01f(r0.y);                       // u1 in (0,1]
    const float x = __builtin_amdgcn_sqrtf(-2.0f * LN2 * __builtin_amdgcn_logf(u1)) * __builtin_amdgcn_cosf(u2);   // cos(2 pi u2)
    float v = 1.0f + c * x;
    if (v <= 0.0f) continue;
    v = v * v * v;
    const float u = 1.0f - mz_u01f(r0.z);
    if (LN2 * __builtin_amdgcn_logf(u) < 0.5f * x * x + d - d * v + d * LN2 * __builtin_amdgcn_logf(v)) { g = d * v; break; }
  }
  if (al < 1.0f) {
    const mz_u4 r = mz_philox(seed, env, c1, a | (0xFFFFFFu << 8), c3);
    // U^(1/alpha) = 2^e, e = log2(U) / alpha <= 0.  The power leaves float32 long before the draw stops mattering: at
    // alpha = 0.03 e < -126 in 7 % of the draws, and a row whose legal actions ALL flushed to 0 came out uniform (the
    // sum == 0 guard of the callers) where Dirichlet(0.03) is nearly one-hot: 0.8 % of the rows with two legal actions.
    // So only the fractional part of e goes through exp2 (e - k in (-1, 0]); the integer part k scales the double, which
    // holds it to 2^-1022.  (One exit and the truncating conversion: the form that keeps the headline kernel's scratch,
    // tests/test_abi.py; floorf and a second return cost it 24 bytes a lane more.)
    const float e = fmaxf(__builtin_amdgcn_logf(1.0f - mz_u01f(r.x)) / al, -2048.0f);
    k = (int)e;
    g *= __builtin_amdgcn_exp2f(e - (float)k);
  }
  return ldexp((double)g, k);
}

// noise[b] ~ Dirichlet(alpha * 1_legal)  (the draw of np.random.dirichlet in mcts.py:59, from the
// device RNG instead of numpy's global stream; parity runs pass numpy's draw in instead)
static __global__ void k_dirichlet(TreeView t, const uint8_t *legal, double alpha, uint64_t seed, uint64_t move_val,
                            const unsigned long long *move_ptr, int env_offset) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const uint64_t move = move_ptr ? (uint64_t)*move_ptr : move_val;
  const int A = t.A;
  double g[MZ_MAX_ACTIONS_K];
  double sum = 0.0;
  int nlegal = 0;
  for (int a = 0; a < A; ++a) {
    const bool ok = legal ? legal[(size_t)b * A + a] != 0 : true;
    g[a] = ok ? mz_gamma(alpha, seed, (uint32_t)(env_offset + b), move, (uint32_t)a) : 0.0;
    sum += g[a];
    nlegal += ok;
  }
  for (int a = 0; a < A; ++a) {
    const bool ok = legal ? legal[(size_t)b * A + a] != 0 : true;
    t.noise[(size_t)b * A + a] = ok ? (sum > 0.0 ? g[a] / sum : 1.0 / nlegal) : 0.0;
  }
}

// The experience record of one move: include/mz_record.h states its layout, mz_record.h here has the accessors.

// float slot k of a record's observation: obs[k], or -- packed byte observations (obs_u8 == 2) -- the bytes obs[4k .. 4k + 3]
// (History keeps the raw uint8 observation, game.py:93-96; the values are exact small integers in float32)
__device__ __forceinline__ float mz_rec_obs_slot(const SelfplayState &sp, const float *obs, int O, int k) {
  if (sp.obs_u8 != 2) return obs[k];
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j)
    if (4 * k + j < O) w |= ((uint32_t)obs[4 * k + j] & 0xFFu) << (8 * j);
  return __builtin_bit_cast(float, w);
}

// Where environment b stands after a move from step t of episode ep: at the next step of its game, or -- the move ended the
// game -- at step 0 of its next game, whose temperature is evaluated now (actors.py:128-129: once per game).  A game that goes
// on keeps its episode and temperature: those two are meaningful, and stored, only with new_game.
// The launch-per-step kernels call this.  The ends of a move that are compiled into the whole-moves search kernels --
// mz_board_apply and the two in mz_finalize_record (mz_fused.hip.h), which also mirror the result into LDS -- spell the same
// rule out: going through this function changed those kernels' code, and they are held to it byte for byte.
struct MzNextMove { int t, episode; double temp; bool new_game; };
__device__ __forceinline__ MzNextMove mz_next_move(const SelfplayState &sp, int done, int t, int ep) {
  if (done) return {0, ep + 1, *sp.temp_next, true};
  return {t + 1, ep, 0.0, false};
}
__device__ __forceinline__ void mz_store_next_move(const SelfplayState &sp, int b, const MzNextMove &nx) {
  if (nx.new_game) { sp.t[b] = nx.t; sp.episode[b] = nx.episode; sp.temp[b] = nx.temp; }
  else sp.t[b] = nx.t;
}

// Game.apply (game.py:79-104) on the synthetic env + the experience record of this move.
static __global__ void k_env_step_record(TreeView tv, SelfplayState sp, int B, int O, int A, uint64_t seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long move = sp.movecnt[b];
  sp.movecnt[b] = move + 1ull;
  // Config.select_action + store_search_statistics + root error for this tree (same code as mz_finalize)
  mz_finalize_tree(tv, b, sp.temp, nullptr, seed, move, sp.env_offset, sp.action, sp.child_visits, sp.root_value,
                   sp.error, nullptr);
  float *rec = mz_rec_slot(sp.ring, move, sp.ring_moves, B, b, sp.rec_floats);
  const int t = sp.t[b], ep = sp.episode[b];
  const int OS = sp.obs_slots;
  for (int k = 0; k < OS; ++k) rec[k] = mz_rec_obs_slot(sp, sp.obs + (size_t)b * O, O, k);
  for (int a = 0; a < A; ++a) rec[OS + a] = (float)sp.child_visits[(size_t)b * A + a];
  const float reward = mz_synth_reward(seed, (uint32_t)(sp.env_offset + b), (uint32_t)ep, (uint32_t)t);
  const int done = (t + 1 >= sp.episode_len) ? 1 : 0;
  mz_rec_put_tail(rec, OS, A, sp.root_value[b], sp.error[b], reward, sp.action[b], done, t, sp.env_offset + b, ep);
  mz_store_next_move(sp, b, mz_next_move(sp, done, t, ep));
}

// ---- a real game as the environment (mz_selfplay_set_env; the games themselves: mz_games.h).  TicTacToe keeps its board
// at stride 9 here, Connect Four at stride 42: the stride is the kind's cells.
// What Actor.play_game reads before a move (actors.py:134-142): the observation, the legal actions and game.to_play.
static __global__ void k_game_observe(SelfplayState sp, int B, int O, int A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int kind = sp.env_kind;
  const bool cart = kind == 2;
  sp.to_play[b] = (int8_t)mz_game_observe(kind, cart ? nullptr : sp.board + (size_t)b * mz_game_info(kind).cells,
                                          cart ? 1 : (int)sp.turn[b], cart ? sp.cart + (size_t)b * 4 : nullptr, true, O, A,
                                          sp.obs + (size_t)b * O, sp.legal + (size_t)b * A);
}

// Game.apply (game.py:79-104) on env.step of the board game KIND (1 TicTacToe, tic_tac_toe.py:30-51; 3 Connect Four) for
// environment b, by ONE lane, and the tail of its experience record (root value, error, reward, action, flags with the
// mover, step, env id, episode).  On done run_selfplay starts a new Game: env.reset (tic_tac_toe.py:20-25) clears the
// board, the turn is +1, the step 0, the episode advances and the next game's temperature is evaluated now.
template <int KIND>
__device__ __forceinline__ void mz_board_apply(const SelfplayState &sp, int b, int action, double root_value, double error,
                                               float *rec, int A) {
  constexpr int O = mz_game_info(KIND).cells;
  const int turn = sp.turn[b], t = sp.t[b], ep = sp.episode[b];
  int8_t *bd = sp.board + (size_t)b * O;
  bool won;
  const int done = mz_game_step(KIND, bd, turn, action, t, &won) ? 1 : 0;
  mz_rec_put_tail(rec, O, A, root_value, error, won ? 1.f : 0.f, action,
                  (done ? MZ_REC_FLAG_DONE : 0) | (turn < 0 ? MZ_REC_FLAG_P2 : 0), t, sp.env_offset + b, ep);
  if (done) {      // (mz_next_move, spelled out: this runs inside the whole-moves search kernels, whose code is held as it is)
    for (int k = 0; k < O; ++k) bd[k] = 0;
    sp.turn[b] = 1; sp.t[b] = 0; sp.episode[b] = ep + 1; sp.temp[b] = *sp.temp_next;
  } else {
    sp.turn[b] = (int8_t)(-turn); sp.t[b] = t + 1;
  }
}

// End of a move of the launch-per-step form: Config.select_action + store_search_statistics + root error
// (mz_finalize_tree), the record (pre-step observation), then Game.apply on the board game: the mover's mark goes on the
// board; a winning move has reward 1 for the mover; the turn flips.  The record carries the mover in its flags word
// (to_play), as History.to_play does.  Only TicTacToe takes the host's uniform (mz_selfplay_set_draws).
template <int KIND>
static __global__ void k_board_step_record(TreeView tv, SelfplayState sp, int B, int A, uint64_t seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long move = sp.movecnt[b];
  sp.movecnt[b] = move + 1ull;
  mz_finalize_tree(tv, b, sp.temp, KIND == 1 ? sp.draw_uniform : nullptr, seed, move, sp.env_offset, sp.action, sp.child_visits,
                   sp.root_value, sp.error, nullptr);
  constexpr int O = mz_game_info(KIND).cells;
  float *rec = mz_rec_slot(sp.ring, move, sp.ring_moves, B, b, sp.rec_floats);
  for (int k = 0; k < O; ++k) rec[k] = sp.obs[(size_t)b * O + k];
  for (int a = 0; a < A; ++a) rec[O + a] = (float)sp.child_visits[(size_t)b * A + a];
  mz_board_apply<KIND>(sp, b, sp.action[b], sp.root_value[b], sp.error[b], rec, A);
}


// ---- CartPole
// Game.apply on CartPole's env.step for environment b, by ONE lane, and the tail of its experience record.  st: the
// environment's four doubles (global memory, or the LDS words of a whole-moves launch), stepped or reset in place;
// tt / ep: its step counter and episode before the move.  Returns done; the caller stores the counters.
__device__ __forceinline__ int mz_cartpole_apply(const SelfplayState &sp, int b, int action, double root_value, double error,
                                                 float *rec, int A, double *st, int tt, int ep, uint64_t seed) {
  const int O = 4;
  const bool out = mz_cartpole_step(st, action);
  const int done = (out || tt + 1 >= sp.episode_len) ? 1 : 0;      // termination, or gym's TimeLimit
  mz_rec_put_tail(rec, O, A, root_value, error, 1.f, action, done, tt, sp.env_offset + b, ep);
  if (done) mz_cartpole_reset_state(seed, (uint32_t)(sp.env_offset + b), (uint32_t)(ep + 1), st);
  return done;
}

// End of a move of the launch-per-step form: finalize the tree, write the record (pre-step observation), step the environment
static __global__ void k_cartpole_step_record(TreeView tv, SelfplayState sp, int B, int A, uint64_t seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long move = sp.movecnt[b];
  sp.movecnt[b] = move + 1ull;
  mz_finalize_tree(tv, b, sp.temp, sp.draw_uniform, seed, move, sp.env_offset, sp.action, sp.child_visits, sp.root_value,
                   sp.error, nullptr);
  const int O = 4;
  float *rec = mz_rec_slot(sp.ring, move, sp.ring_moves, B, b, sp.rec_floats);
  for (int k = 0; k < O; ++k) rec[k] = sp.obs[(size_t)b * O + k];
  for (int a = 0; a < A; ++a) rec[O + a] = (float)sp.child_visits[(size_t)b * A + a];
  const int tt = sp.t[b], ep = sp.episode[b];
  double st[4];
  for (int k = 0; k < 4; ++k) st[k] = sp.cart[(size_t)b * 4 + k];
  const int done = mz_cartpole_apply(sp, b, sp.action[b], sp.root_value[b], sp.error[b], rec, A, st, tt, ep, seed);
  for (int k = 0; k < 4; ++k) sp.cart[(size_t)b * 4 + k] = st[k];
  mz_store_next_move(sp, b, mz_next_move(sp, done, tt, ep));
}
