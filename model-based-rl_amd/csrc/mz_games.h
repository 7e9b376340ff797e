// mz_games.h -- the device games and nothing else: TicTacToe (kind 1), CartPole (kind 2) and Connect Four (kind 3), the
// numbering of mz_selfplay_set_env.  The rules, the facts of each kind (mz_game_info) and the small things every user of a
// game needs next to the rules: the shape check, the legal mask, the i-th legal action, the engine's inputs of a position
// and the running maximum of the search-depth lists.  Every function takes the kind and the game's own data, never who is
// calling; all of them are __host__ __device__, so host programs (tests/*_host.cpp) and the debug header's host hooks run
// the very same code.  The one other statement of the rules is the bitboard form of mz_solve.hip.h.
#pragma once
#include <stdio.h>
#include "mz_common.h"
#include "mz_rng.h"

// ---- the facts of a kind.  cells: the int8 cells of its board (0: no board); longest: the plies of its longest game
// (CartPole: 0, its time limit is the caller's).  A kind that is no game has a null name.
struct MzGameInfo {
  const char *name;
  int obs_dim, actions, cells, two_players, longest;
};
#define MZ_GAME_MAX_ACTIONS 9      // the largest action count of a board game
__host__ __device__ constexpr MzGameInfo mz_game_info(int kind) {
  switch (kind) {
    case 1: return {"TicTacToe", 9, 9, 9, 1, 9};
    case 2: return {"CartPole", 4, 2, 0, 0, 0};
    case 3: return {"Connect Four", 42, 7, 42, 1, 42};
  }
  return {nullptr, 0, 0, 0, 0, 0};
}

// Whether an engine of obs_dim O, action_space A and two_players / a single player can play kind; if not, why [n] says
// what the kind needs (the caller prefixes its own name).
__host__ __device__ inline bool mz_game_shape_ok(int kind, int O, int A, bool two_players, char *why, size_t n) {
  const MzGameInfo g = mz_game_info(kind);
  if (g.name && O == g.obs_dim && A == g.actions && two_players == (g.two_players != 0)) return true;
  if (g.name) snprintf(why, n, "%s needs obs_dim %d, action_space %d and %s", g.name, g.obs_dim, g.actions,
                       g.two_players ? "two_players" : "a single player");
  else snprintf(why, n, "kind %d is no game (1 TicTacToe, 2 CartPole, 3 Connect Four)", kind);
  return false;
}


// ---- TicTacToe (custom_environments/tic_tac_toe.py:5-76; the reference's only two-player environment)
// env.step(action) (tic_tac_toe.py:30-51) for the mover `turn` on bd[9], t = the elapsed steps before this move: the mark
// goes on the cell; *won = a line through it sums to 3 * turn; returns done = won or the ninth move (tic_tac_toe.py:37).
// The one statement of the rules every device form calls.
__host__ __device__ inline bool mz_ttt_step(int8_t *bd, int turn, int action, int t, bool *won) {
  bd[action] = (int8_t)turn;
  const int r0 = 3 * (action / 3), c0 = action % 3;
  bool w = (bd[r0] + bd[r0 + 1] + bd[r0 + 2] == 3 * turn) || (bd[c0] + bd[c0 + 3] + bd[c0 + 6] == 3 * turn);
  if (action % 4 == 0) w = w || (bd[0] + bd[4] + bd[8] == 3 * turn);
  if (action == 2 || action == 4 || action == 6) w = w || (bd[2] + bd[4] + bd[6] == 3 * turn);
  *won = w;
  return w || t == 8;
}


// ---- CartPole on the device (envs.CartPole is the definition; gym's CartPole-v1 / -v0 with its TimeLimit folded in).
// sin / cos of the pole angle: fixed Taylor polynomials in z = theta * theta, Horner from the highest term down with plain
// float64 multiplies and adds -- with -ffp-contract=off the host class, the host build of this function and the device run the
// same IEEE operations, so trajectories agree bit for bit (libm's sin / cos differ between the sides in the last place,
// and the pole grows a last-place difference by ~e^0.09 per step).
__host__ __device__ inline double mz_cartpole_sin(double t) {
  const double z = t * t;
  double r = -1.0 / 1307674368000.0;
  r = r * z + 1.0 / 6227020800.0;
  r = r * z + -1.0 / 39916800.0;
  r = r * z + 1.0 / 362880.0;
  r = r * z + -1.0 / 5040.0;
  r = r * z + 1.0 / 120.0;
  r = r * z + -1.0 / 6.0;
  r = r * z + 1.0;
  return t * r;
}
__host__ __device__ inline double mz_cartpole_cos(double t) {
  const double z = t * t;
  double r = 1.0 / 20922789888000.0;
  r = r * z + -1.0 / 87178291200.0;
  r = r * z + 1.0 / 479001600.0;
  r = r * z + -1.0 / 3628800.0;
  r = r * z + 1.0 / 40320.0;
  r = r * z + -1.0 / 720.0;
  r = r * z + 1.0 / 24.0;
  r = r * z + -1.0 / 2.0;
  r = r * z + 1.0;
  return r;
}
// env.step(action) on st = (x, x_dot, theta, theta_dot), in place, in the operation order of envs.CartPole.step; returns
// whether the new state lies outside the thresholds (the time limit is the caller's: it owns the step counter).  The one
// function every device form -- and the host side of the debug header -- calls.
__host__ __device__ inline bool mz_cartpole_step(double *st, int action) {
  const double g = 9.8, M = 1.1, m_pole = 0.1, l = 0.5, pml = 0.05, F = 10.0, tau = 0.02;
  double x = st[0], x_dot = st[1], theta = st[2], theta_dot = st[3];
  const double f = action == 1 ? F : -F;
  const double c = mz_cartpole_cos(theta), s = mz_cartpole_sin(theta);
  const double temp = (f + pml * theta_dot * theta_dot * s) / M;
  const double tha = (g * s - c * temp) / (l * (4.0 / 3.0 - m_pole * c * c / M));
  const double xa = temp - pml * tha * c / M;
  x = x + tau * x_dot;
  x_dot = x_dot + tau * xa;
  theta = theta + tau * theta_dot;
  theta_dot = theta_dot + tau * tha;
  st[0] = x; st[1] = x_dot; st[2] = theta; st[3] = theta_dot;
  const double th = 12 * 2 * 3.141592653589793 / 360;
  return x < -2.4 || x > 2.4 || theta < -th || theta > th;
}
// env.reset() of episode `episode` of environment `env`: every component uniform in [-0.05, 0.05), from the counter RNG
// -- integer-derived, identical on host and device, so the host can name the start of every episode.
__host__ __device__ inline void mz_cartpole_reset_state(uint64_t seed, uint32_t env, uint32_t episode, double *out) {
  for (uint32_t j = 0; j < 2; ++j) {
    const mz_u4 r = mz_philox(seed, env, episode, 0u, (MZ_RNG_ENV << 24) | j);
    out[2 * j] = (mz_u01(r.x, r.y) - 0.5) * 0.1;
    out[2 * j + 1] = (mz_u01(r.z, r.w) - 0.5) * 0.1;
  }
}


// ---- Connect Four on the device (envs.ConnectFour is the definition: 6 rows of 7 columns, cell 7 * row + col, row 0 at the
// bottom; TicTacToe's conventions otherwise).  The rules are integer operations on the 42 int8 cells, so host and device
// agree by construction; the two functions below are all the device forms know of the game.
// env.step(col) for the mover `turn` on bd[42], the column not full (the search only offers legal columns): the stone lands
// on the lowest empty cell; *won = a line of at least four of the mover's stones passes through it (vertical, horizontal,
// the two diagonals); returns done = won or no empty cell left (a full board = a full top row).
__host__ __device__ inline bool mz_c4_step(int8_t *bd, int turn, int col, bool *won) {
  int row = 0;
  while (row < 5 && bd[7 * row + col] != 0) ++row;
  bd[7 * row + col] = (int8_t)turn;
  const int dr[4] = {1, 0, 1, 1}, dc[4] = {0, 1, 1, -1};
  bool w = false;
  for (int d = 0; d < 4; ++d) {
    int n = 0;
    for (int sg = -1; sg <= 1; sg += 2) {
      int r = row + sg * dr[d], c = col + sg * dc[d];
      while (r >= 0 && r < 6 && c >= 0 && c < 7 && bd[7 * r + c] == turn) { ++n; r += sg * dr[d]; c += sg * dc[d]; }
    }
    w = w || n >= 3;
  }
  *won = w;
  bool full = true;
  for (int c = 0; c < 7; ++c) full = full && bd[35 + c] != 0;
  return w || full;
}
// What Actor.play_game reads before a move: legal_actions() as a mask (the columns whose top cell is empty) and
// game.to_play = env.turn; obs (optional) [42] = turn * board as float32, cell k of it is mz_c4_obs_cell
__host__ __device__ inline float mz_c4_obs_cell(const int8_t *bd, int turn, int k) { return (float)(turn * (int)bd[k]); }
__host__ __device__ inline uint32_t mz_c4_view(const int8_t *bd, int turn, float *obs, int *to_play) {
  uint32_t mask = 0;
  for (int c = 0; c < 7; ++c) mask |= (bd[35 + c] == 0 ? 1u : 0u) << c;
  if (obs) for (int k = 0; k < 42; ++k) obs[k] = mz_c4_obs_cell(bd, turn, k);
  *to_play = turn;
  return mask;
}


// ---- the two board games by kind.  bd: the game's own cells, TicTacToe's 9 or Connect Four's 42, wherever the caller
// keeps them.
// legal_actions() of a position as a mask: TicTacToe's empty cells (tic_tac_toe.py:27-28), Connect Four's open columns
__host__ __device__ inline uint32_t mz_game_legal(int kind, const int8_t *bd) {
  if (kind == 3) { int tp; return mz_c4_view(bd, 1, nullptr, &tp); }
  uint32_t m = 0;
  for (int k = 0; k < 9; ++k) m |= (bd[k] == 0 ? 1u : 0u) << k;
  return m;
}
// env.step(action) for the mover `turn`, t plies played before it: *won, and returns done
__host__ __device__ inline bool mz_game_step(int kind, int8_t *bd, int turn, int action, int t, bool *won) {
  return kind == 3 ? mz_c4_step(bd, turn, action, won) : mz_ttt_step(bd, turn, action, t, won);
}
// the i-th legal action in ascending order (0 where the mask has no such bit: never asked for)
__host__ __device__ inline int mz_nth_legal(uint32_t mask, int i) {
  for (int a = 0; a < MZ_GAME_MAX_ACTIONS; ++a)
    if (((mask >> a) & 1u) && i-- == 0) return a;
  return 0;
}
// ... with the index clamped into the position's n > 0 legal actions first: what a random mover's floor(u * n), or an
// index given by a caller, becomes
__host__ __device__ inline int mz_pick_legal(uint32_t mask, int idx) {
  const int n = __builtin_popcount(mask);
  return mz_nth_legal(mask, idx < 0 ? 0 : (idx > n - 1 ? n - 1 : idx));
}

// ---- from a game's state to the engine's inputs, what Actor.play_game reads before a move (actors.py:134-142):
// obs[O] = turn * board as float32 (tic_tac_toe.py:24,50 + actors.py:134) or CartPole's state st[4] as float32,
// legal[A] = the legal actions as bytes (CartPole: every action); returns game.to_play (CartPole: +1).  A finished game
// (!live) gets the zero observation, all actions legal and +1.  bd / st: null for the kinds that have none.
__host__ __device__ inline int mz_game_observe(int kind, const int8_t *bd, int turn, const double *st, bool live, int O, int A,
                                               float *obs, uint8_t *legal) {
  uint32_t mask = 0xFFFFFFFFu;
  int to_play = 1;
  if (!live) {
    for (int k = 0; k < O; ++k) obs[k] = 0.f;
  } else if (kind == 2) {
    for (int k = 0; k < 4; ++k) obs[k] = (float)st[k];
  } else if (kind == 3) {
    mask = mz_c4_view(bd, turn, obs, &to_play);
  } else {
    for (int k = 0; k < 9; ++k) obs[k] = (float)(turn * (int)bd[k]);
    mask = mz_game_legal(kind, bd);
    to_play = turn;
  }
  for (int a = 0; a < A; ++a) legal[a] = (uint8_t)((mask >> a) & 1u);
  return to_play;
}

// ---- max() over the per-move lists of search depths is the lexicographic maximum list (evaluate.py:102): pl[sims]
// replaces dm[sims] if it is the first list or lexicographically greater.  Returns whether it did, and then *mean is
// the new maximum's mean, which is what is reported.
__host__ __device__ inline bool mz_depth_list_max(int32_t *dm, const int32_t *pl, int sims, bool first, double *mean) {
  bool greater = first;
  for (int s = 0; s < sims && !greater; ++s) {
    if (pl[s] == dm[s]) continue;
    greater = pl[s] > dm[s];
    break;
  }
  if (greater) {
    long sum = 0;
    for (int s = 0; s < sims; ++s) { dm[s] = pl[s]; sum += pl[s]; }
    *mean = (double)sum / (double)sims;
  }
  return greater;
}
