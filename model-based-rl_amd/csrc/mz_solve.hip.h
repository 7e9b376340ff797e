// mz_solve.hip.h -- the exact game solver that grades evaluation moves (DESIGN s7f): for a position of TicTacToe (kind 1)
// or Connect Four (kind 3) and each action a, the game-theoretic outcome for the mover after playing a (gfx950; included
// by mz_engine.hip).  A plain negamax with the window [-1, +1], a fixed move order and no transposition table, so a value
// depends on nothing but the position; integer arithmetic only.
//
// THIS FILE HOLDS A SECOND FORM OF THE RULES: bitboards (Connect Four: 7 columns of 7 bits, 6 cells and an always-empty
// sentinel bit, bit 7 * col + row; TicTacToe: 9 bits), beside mz_ttt_step / mz_c4_step of mz_selfplay.hip.h, which
// mz_playout.hip.h deliberately did without.  It is acceptable here only because the tests pin it against the first form:
// tests/test_solve_cpu.py holds the values on every reachable TicTacToe position and on Connect Four endgames to a minimax
// written on the first form's Python restatement (tests/playout_py.py).  The int8[42] board is converted once per position
// (sv_pack).
//
// The unit of work is the subtree under one (position, action), searched sequentially by one lane with its own node
// budget; units share nothing (no cutoff passes between them).  The bodies are __host__ __device__ and mz_solve_host
// (include/mz_engine_debug.h) runs the same units in the same order with the same budget: values, the unsolved pattern and
// the node counts are equal by construction.  Only the distribution of the units differs: the host loops over them, the
// lanes of a wave pull them from the wave's share of the list (a counter in LDS).
#pragma once
#include "mz_common.h"

#define MZ_SV_ILLEGAL (-2)
#define MZ_SV_UNSOLVED (-3)
#define MZ_SV_MAX_NODES (1 << 30)
#define MZ_SV_STACK_STRIDE 44      // bytes between two lanes' stacks: 11 words, an odd count (MZ_PO_BOARD_STRIDE's reason); one byte a level, 42 levels at the most
#define MZ_SV_MAX_UNITS_PER_LANE 16

// ---- the rules on bitboards.  cur: the stones of the side to move; mask: all stones.  A move is the bit of the cell it fills.
template <int KIND> struct SvRules;

template <> struct SvRules<3> {
  static constexpr int CELLS = 42, MOVES = 7;
  static constexpr uint64_t BOTTOM = 0x0000040810204081ull;      // bit 7 * col of the seven columns
  static constexpr uint64_t BOARD = BOTTOM * 0x3Full;            // the 42 cells (no sentinel bit)
  // the i-th column of the fixed order 3, 2, 4, 1, 5, 0, 6
  __host__ __device__ static inline int order(int i) { return (i & 1) ? 3 - ((i + 1) >> 1) : 3 + (i >> 1); }
  // the cell a stone dropped into column `col` fills; 0 where the column is full (the sum lands on the sentinel bit)
  __host__ __device__ static inline uint64_t action_bit(uint64_t mask, int col) {
    return (mask + (1ull << (7 * col))) & (0x3Full << (7 * col));
  }
  __host__ __device__ static inline uint64_t move_bit(uint64_t mask, int i) { return action_bit(mask, order(i)); }
  // the stone on top of the i-th column of the order (the move to take back)
  __host__ __device__ static inline uint64_t top_bit(uint64_t mask, int i) {
    const int s = 7 * order(i);
    return ((((mask >> s) & 0x7Full) + 1ull) >> 1) << s;
  }
  // four in a line among the stones p: vertical (shift 1), horizontal (7), the two diagonals (6, 8); the sentinel bits
  // keep a line from running over a column's end
  __host__ __device__ static inline bool has_line(uint64_t p) {
    uint64_t m = p & (p >> 1);
    bool w = (m & (m >> 2)) != 0;
    m = p & (p >> 7); w = w || (m & (m >> 14)) != 0;
    m = p & (p >> 6); w = w || (m & (m >> 12)) != 0;
    m = p & (p >> 8); w = w || (m & (m >> 16)) != 0;
    return w;
  }
  // the empty cells that would complete a line of four of p
  __host__ __device__ static inline uint64_t win_dir(uint64_t p, int s) {      // along one direction: the cell beside three, or between two and one
    uint64_t t = (p << s) & (p << (2 * s));
    uint64_t r = (t & (p << (3 * s))) | (t & (p >> s));
    t = (p >> s) & (p >> (2 * s));
    return r | (t & (p << s)) | (t & (p >> (3 * s)));
  }
  __host__ __device__ static inline uint64_t win_cells(uint64_t p, uint64_t mask) {
    const uint64_t r = ((p << 1) & (p << 2) & (p << 3)) | win_dir(p, 7) | win_dir(p, 6) | win_dir(p, 8);
    return r & (BOARD ^ mask);
  }
  // the side to move completes a line with one stone
  __host__ __device__ static inline bool can_win(uint64_t cur, uint64_t mask) {
    return (win_cells(cur, mask) & (mask + BOTTOM) & BOARD) != 0;
  }
  // bit of board cell k = 7 * row + col
  __host__ __device__ static inline uint64_t cell_bit(int k) { return 1ull << (7 * (k % 7) + k / 7); }
};

template <> struct SvRules<1> {
  static constexpr int CELLS = 9, MOVES = 9;
  __host__ __device__ static inline uint64_t action_bit(uint64_t mask, int a) { return (1ull << a) & ~mask & 0x1FFull; }
  __host__ __device__ static inline uint64_t move_bit(uint64_t mask, int i) { return action_bit(mask, i); }      // cells ascending
  __host__ __device__ static inline uint64_t top_bit(uint64_t, int i) { return 1ull << i; }
  __host__ __device__ static inline bool has_line(uint64_t p) {
    const uint32_t q = (uint32_t)p;
    return (q & 0007u) == 0007u || (q & 0070u) == 0070u || (q & 0700u) == 0700u || (q & 0111u) == 0111u ||
           (q & 0222u) == 0222u || (q & 0444u) == 0444u || (q & 0421u) == 0421u || (q & 0124u) == 0124u;
  }
  // two of the mover's marks on a line whose third cell is empty
  __host__ __device__ static inline bool line_open(uint32_t cur, uint32_t mask, uint32_t line) {
    return __builtin_popcount(cur & line) == 2 && (line & ~mask) != 0;
  }
  __host__ __device__ static inline bool can_win(uint64_t cur, uint64_t mask) {
    const uint32_t c = (uint32_t)cur, m = (uint32_t)mask;
    return line_open(c, m, 0007u) || line_open(c, m, 0070u) || line_open(c, m, 0700u) || line_open(c, m, 0111u) ||
           line_open(c, m, 0222u) || line_open(c, m, 0444u) || line_open(c, m, 0421u) || line_open(c, m, 0124u);
  }
  __host__ __device__ static inline uint64_t cell_bit(int k) { return 1ull << k; }
};

// the int8[42] board as bitboards, once per position: *cur the stones of `turn`, *mask all stones
template <int KIND>
__host__ __device__ inline void sv_pack(const int8_t *bd, int turn, uint64_t *cur, uint64_t *mask) {
  uint64_t c = 0, m = 0;
  for (int k = 0; k < SvRules<KIND>::CELLS; ++k) {
    const uint64_t b = SvRules<KIND>::cell_bit(k);
    if (bd[k] != 0) m |= b;
    if (bd[k] == turn) c |= b;
  }
  *cur = c; *mask = m;
}
// a side already has a line (such a position is refused: the game was over before it)
template <int KIND>
__host__ __device__ inline bool sv_finished(uint64_t cur, uint64_t mask) {
  return SvRules<KIND>::has_line(cur) || SvRules<KIND>::has_line(cur ^ mask);
}

// ---- one unit: action `action` by the mover of (cur, mask, `stones` on the board), then negamax for the opponent.
// Returns +1 / 0 / -1 for the mover, MZ_SV_ILLEGAL, or MZ_SV_UNSOLVED when the unit would need more than `budget` nodes;
// *nodes_out: the nodes spent (every stone placed is one node; `budget` where unsolved, 0 where illegal).
//
// At a node the mover who can win at once does (value +1, no move made); otherwise the moves are made in the fixed order
// with the window (alpha, beta) and the search leaves the node once alpha >= beta.  The search is iterative: a level's move
// index, alpha and beta are one byte of `stack` (mi | (alpha + 1) << 4 | (beta + 1) << 6), the position is made and unmade
// in the two registers.  Every turn of the loop places a stone (at most `budget` times) or leaves a level, so it ends.
template <int KIND>
__host__ __device__ inline int sv_unit(uint64_t cur, uint64_t mask, int stones, int action, uint32_t budget, uint8_t *stack,
                                       uint32_t *nodes_out) {
  typedef SvRules<KIND> R;
  uint64_t b = R::action_bit(mask, action);
  if (!b) { *nodes_out = 0; return MZ_SV_ILLEGAL; }
  uint32_t nodes = 1;
  if (R::has_line(cur | b)) { *nodes_out = nodes; return 1; }
  cur ^= mask; mask |= b; ++stones;
  if (stones >= R::CELLS) { *nodes_out = nodes; return 0; }
  if (R::can_win(cur, mask)) { *nodes_out = nodes; return -1; }
  int d = 0, mi = 0, alpha = -1, beta = 1, ret = 0;
  bool have_ret = false;
  for (;;) {
    int v;
    if (have_ret) {      // a level below returned `ret`: back to level d - 1, its move taken back
      if (d == 0) break;
      --d;
      const int s = stack[d];
      mi = s & 15; alpha = ((s >> 4) & 3) - 1; beta = ((s >> 6) & 3) - 1;
      b = R::top_bit(mask, mi);
      mask ^= b; cur ^= mask; --stones;
      v = -ret;
      have_ret = false;
    } else {
      b = 0;
      while (mi < R::MOVES && !(b = R::move_bit(mask, mi))) ++mi;
      if (!b) { ret = alpha; have_ret = true; continue; }      // every move tried
      if (nodes >= budget) { *nodes_out = budget; return MZ_SV_UNSOLVED; }
      ++nodes;
      cur ^= mask; mask |= b; ++stones;      // (the mover could not win at once: this stone completes no line)
      if (stones < R::CELLS && !R::can_win(cur, mask) && d < MZ_SV_STACK_STRIDE - 1) {      // (d < 41 always; a guard)
        stack[d] = (uint8_t)(mi | ((alpha + 1) << 4) | ((beta + 1) << 6));
        ++d;
        const int a = -beta;
        beta = -alpha; alpha = a; mi = 0;
        continue;
      }
      v = stones >= R::CELLS ? 0 : -1;      // the board is full: a draw; or the opponent wins at once
      mask ^= b; cur ^= mask; --stones;
    }
    if (v > alpha) alpha = v;
    ++mi;
    if (alpha >= beta) { ret = alpha; have_ret = true; }
  }
  *nodes_out = nodes;
  return -ret;
}

// The solver's own device memory (mz_solve), allocated on first use; separate from EvalState and PlayoutState.
struct SolveState {
  int8_t *boards;        // [B][42]
  int8_t *turn;          // [B]
  int32_t *step;         // [B]
  uint64_t *bits;        // [B][2] cur, mask
  int8_t *values;        // [B][A]
  uint32_t *nodes;       // [B][A]
};

// one thread a position: the conversion to bitboards
template <int KIND>
static __global__ __launch_bounds__(256) void k_solve_pack(const int8_t *boards, const int8_t *turn, int n, uint64_t *bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t cur, mask;
  sv_pack<KIND>(boards + (size_t)i * 42, (int)turn[i], &cur, &mask);
  bits[2 * (size_t)i] = cur; bits[2 * (size_t)i + 1] = mask;
}

// One wave a block.  Unit u = position u / A, action u % A.  The wave owns the units [blockIdx.x * per_wave, + per_wave)
// below n_units; each lane starts on one and pulls the next from the counter in LDS when it is done, so a lane that drew a
// deep subtree does not hold up the others' share.  At most per_wave turns of the loop per lane.
template <int KIND>
static __global__ __launch_bounds__(64) void k_solve(int A, const uint64_t *bits, const int32_t *step, int n_units,
                                                     int per_wave, uint32_t budget, int8_t *values, uint32_t *nodes) {
  __shared__ __align__(4) uint8_t sv_stack[64 * MZ_SV_STACK_STRIDE];
  __shared__ int sv_next;
  const int lane = threadIdx.x;
  const int base = blockIdx.x * per_wave;
  const int end = base + per_wave < n_units ? base + per_wave : n_units;
  if (lane == 0) sv_next = base + 64;
  __syncthreads();
  uint8_t *stack = sv_stack + lane * MZ_SV_STACK_STRIDE;
  int u = base + lane;
  for (int k = 0; k < per_wave && u < end; ++k) {
    const int pos = u / A, a = u - pos * A;
    uint32_t spent;
    const int v = sv_unit<KIND>(bits[2 * (size_t)pos], bits[2 * (size_t)pos + 1], step[pos], a, budget, stack, &spent);
    values[u] = (int8_t)v;
    nodes[u] = spent;
    u = atomicAdd(&sv_next, 1);
  }
}
