// mz_solve.hip.h -- the exact game solver that grades evaluation moves (DESIGN s7f): for a position of TicTacToe (kind 1)
// or Connect Four (kind 3) and each action a, the game-theoretic outcome for the mover after playing a (gfx950; included
// by mz_engine.hip).  A plain negamax with the window [-1, +1], a fixed move order and no transposition table, so a value
// depends on nothing but the position; integer arithmetic only.  A second search of the same units stands beside it at the
// end of the file (sv_unit_tt, k_solve_tt: non-losing moves, ordered, a table private to the unit).
//
// THIS FILE HOLDS A SECOND FORM OF THE RULES: bitboards (Connect Four: 7 columns of 7 bits, 6 cells and an always-empty
// sentinel bit, bit 7 * col + row; TicTacToe: 9 bits), beside mz_ttt_step / mz_c4_step of mz_games.h, which
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
  // ---- the table search (sv_unit_tt below)
  typedef uint32_t level_t;      // a level of its stack: 7 x 3 bits of move order, 3 of index, 3 x 2 of windows
  static constexpr int OBITS = 3, SLOTS = 7, LEVELS = 41;      // LEVELS: words a lane, an odd count; a node has 1 .. 41 stones
  __host__ __device__ static inline uint64_t key(uint64_t cur, uint64_t mask) { return cur + mask; }      // 49 bits, one per position
  // the moves that do not lose at once, as cells (0: none).  The opponent's playable winning cells must be filled: two of them
  // cannot be; and no stone goes under a winning cell of the opponent
  __host__ __device__ static inline uint64_t nonlosing(uint64_t cur, uint64_t mask) {
    const uint64_t opp = win_cells(cur ^ mask, mask), play = (mask + BOTTOM) & BOARD, t = opp & play;
    if (t & (t - 1)) return 0;
    return (t ? t : play) & ~(opp >> 1);
  }
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
  // the empty cells that would complete a line of p
  __host__ __device__ static inline uint32_t line_cell(uint32_t p, uint32_t mask, uint32_t line) {
    return __builtin_popcount(p & line) == 2 ? line & ~mask : 0u;
  }
  __host__ __device__ static inline uint64_t win_cells(uint64_t p, uint64_t mask) {
    const uint32_t c = (uint32_t)p, m = (uint32_t)mask;
    return line_cell(c, m, 0007u) | line_cell(c, m, 0070u) | line_cell(c, m, 0700u) | line_cell(c, m, 0111u) |
           line_cell(c, m, 0222u) | line_cell(c, m, 0444u) | line_cell(c, m, 0421u) | line_cell(c, m, 0124u);
  }
  // ---- the table search (sv_unit_tt below)
  typedef uint64_t level_t;      // a level of its stack: 8 x 4 bits of move order, 4 of index, 3 x 2 of windows
  static constexpr int OBITS = 4, SLOTS = 8, LEVELS = 9;      // LEVELS: 8-byte words a lane, an odd count; a node has 1 .. 8 marks
  __host__ __device__ static inline uint64_t key(uint64_t cur, uint64_t mask) { return cur | (mask << 9); }
  // the moves that do not lose at once, as cells (0: none): the opponent's winning cell must be filled, two cannot be
  __host__ __device__ static inline uint64_t nonlosing(uint64_t cur, uint64_t mask) {
    const uint64_t t = win_cells(cur ^ mask, mask);
    if (t & (t - 1)) return 0;
    return t ? t : ~mask & 0x1FFull;
  }
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

// ================================================================ the table search (DESIGN s7f, "The table search")
// A second exact search of the same units with the same top, outputs and budget rule.  Below the top a node differs from
// sv_unit's in three ways: only the moves that do not lose at once are tried (SvRules::nonlosing), in descending order of
// the winning cells the mover has after the move (ties in the fixed order), and a transposition table private to the unit
// holds the bounds the unit has proved.  A unit sees only entries it wrote itself, so values, the unsolved pattern and the
// node counts stay a function of the position and the budget alone.
//
// The table: direct-mapped, always-replace, 2^MZ_SVT_BITS entries of 8 bytes a lane.  An entry is the full position key (bits
// 0 .. 48), the lower and the upper bound known for the side to move (+ 1, bits 49 .. 50 and 51 .. 52) and the generation of the
// unit that wrote it (bits 53 .. 63): positions that share an index never exchange values, and an entry of another generation
// counts as empty, so no unit clears the table.  A lane's generation counter lives in device memory across launches, is
// bumped per unit (svt_next_gen) and runs 1 .. MZ_SVT_GEN_WRAP - 1; the table is zeroed at allocation (generation 0 is never
// a unit's) and the lane clears it when the counter wraps.
#define MZ_SVT_BITS 12      // part of the definition: the node counts depend on it (host and device share it)
#define MZ_SVT_GEN_WRAP (1 << 11)
#define MZ_SVT_KEY_MASK ((1ull << 49) - 1)
#define MZ_SVT_MAX_WAVES 1024

__host__ __device__ inline uint32_t svt_index(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - MZ_SVT_BITS)); }

// the generation of the next unit of the lane that owns `tab`
__host__ __device__ inline uint32_t svt_next_gen(uint64_t *tab, uint32_t gen) {
  if (++gen < MZ_SVT_GEN_WRAP) return gen;
  for (int i = 0; i < (1 << MZ_SVT_BITS); ++i) tab[i] = 0;
  return 1;
}

// leaving a node searched with the window (alpha0, beta), alpha the best value found: the bound that proves is merged into
// the node's entry, if it still is the node's, and stored
__host__ __device__ inline void svt_store(uint64_t *tab, uint32_t gen, uint64_t key, int alpha0, int alpha, int beta) {
  uint64_t *slot = tab + svt_index(key);
  const uint64_t en = *slot;
  int lo = -1, hi = 1;
  if ((en & MZ_SVT_KEY_MASK) == key && (uint32_t)(en >> 53) == gen) { lo = (int)((en >> 49) & 3) - 1; hi = (int)((en >> 51) & 3) - 1; }
  if (alpha <= alpha0) { if (alpha < hi) hi = alpha; }      // no move raised alpha: an upper bound
  else if (alpha >= beta) { if (alpha > lo) lo = alpha; }   // a cutoff: a lower bound
  else lo = hi = alpha;
  *slot = key | ((uint64_t)(lo + 1) << 49) | ((uint64_t)(hi + 1) << 51) | ((uint64_t)gen << 53);
}

// the moves `moves` (cells) of the mover of (cur, mask) as indices of the fixed order, OBITS each from bit 0, sorted by the
// winning cells the mover has after the move, descending, ties in the fixed order; every field behind the last move, and
// every bit above the SLOTS fields, is one (the end mark).  An insertion sort in two registers: `sc` holds the sorted
// scores + 1, six bits each, 0 where no move is yet.
template <int KIND>
__host__ __device__ inline typename SvRules<KIND>::level_t sv_order(uint64_t cur, uint64_t mask, uint64_t moves) {
  typedef SvRules<KIND> R;
  typedef typename R::level_t level_t;
  level_t ord = ~(level_t)0;
  uint64_t sc = 0;
  int n = 0;
  for (int i = 0; i < R::MOVES; ++i) {
    const uint64_t b = R::move_bit(mask, i) & moves;
    if (!b || n >= R::SLOTS) continue;      // (n < SLOTS always: a guard)
    const uint64_t s = (uint64_t)__builtin_popcountll(R::win_cells(cur | b, mask | b)) + 1;
    int p = 0;
    for (int j = 0; j < R::SLOTS; ++j) p += ((sc >> (6 * j)) & 63) >= s;
    const uint64_t ls = (1ull << (6 * p)) - 1;
    sc = (sc & ls) | (s << (6 * p)) | ((sc & ~ls) << 6);
    const level_t lo = (level_t)(((level_t)1 << (R::OBITS * p)) - 1);
    ord = (ord & lo) | ((level_t)i << (R::OBITS * p)) | ((ord & ~lo) << R::OBITS);
    ++n;
  }
  return ord;
}

// ---- one unit of the table search: sv_unit's arguments and results, `stack` R::LEVELS words, `tab` the lane's table, `gen`
// this unit's generation.  The top is sv_unit's.  Below it a node is entered (ENTER) with a mover who cannot win at once and a
// board that is not full -- the top ensures it for the first node, nonlosing() for every other: after a move it admits the
// opponent has no playable winning cell.  Entering: no move left, the value is -1 and nothing is stored; the node's entry
// narrows the window and the node returns max(alpha, lower bound) once the window is empty; otherwise the moves are ordered.
// NEXT places the next stone (a full board is a draw, any other position is entered one level down) or, the moves or the
// window used up, stores the node's bound and returns alpha (fail-hard).  RET takes the move of the level above back.  A level
// is one word of `stack`: the order, the index into it, alpha, beta and alpha on entry (beta does not change inside a node).
// Every turn of the loop places a stone (at most `budget` times), leaves a level, or enters the node of the stone just placed,
// and sv_order's and svt_store's loops are bounded, so it ends whatever the table holds.  A unit cut by the budget stores nothing.
template <int KIND>
__host__ __device__ inline int sv_unit_tt(uint64_t cur, uint64_t mask, int stones, int action, uint32_t budget,
                                          typename SvRules<KIND>::level_t *stack, uint64_t *tab, uint32_t gen, uint32_t *nodes_out) {
  typedef SvRules<KIND> R;
  typedef typename R::level_t level_t;
  constexpr int OS = R::OBITS * R::SLOTS;      // the level word above the order: index (OBITS), alpha, beta, alpha on entry (+ 1, 2 bits each)
  constexpr int END = (1 << R::OBITS) - 1;
  uint64_t b = R::action_bit(mask, action);
  if (!b) { *nodes_out = 0; return MZ_SV_ILLEGAL; }
  uint32_t nodes = 1;
  if (R::has_line(cur | b)) { *nodes_out = nodes; return 1; }
  cur ^= mask; mask |= b; ++stones;
  if (stones >= R::CELLS) { *nodes_out = nodes; return 0; }
  if (R::can_win(cur, mask)) { *nodes_out = nodes; return -1; }
  enum { ENTER, NEXT, RET };
  int state = ENTER, d = 0, idx = 0, alpha = -1, beta = 1, alpha0 = -1, ret = 0;
  level_t ord = ~(level_t)0;
  for (;;) {
    int v;
    if (state == ENTER) {
      const uint64_t moves = R::nonlosing(cur, mask);
      if (!moves) { ret = -1; state = RET; continue; }
      const uint64_t key = R::key(cur, mask), en = tab[svt_index(key)];
      if ((en & MZ_SVT_KEY_MASK) == key && (uint32_t)(en >> 53) == gen) {
        const int lo = (int)((en >> 49) & 3) - 1, hi = (int)((en >> 51) & 3) - 1;
        if (lo > alpha) alpha = lo;
        if (hi < beta) beta = hi;
        if (alpha >= beta) { ret = alpha; state = RET; continue; }
      }
      ord = sv_order<KIND>(cur, mask, moves);
      idx = 0; alpha0 = alpha; state = NEXT;
      continue;
    }
    if (state == RET) {      // a level below returned `ret`: back to level d - 1, its move taken back
      if (d == 0) break;
      --d;
      const level_t w = stack[d];
      ord = w | ~(level_t)(((level_t)1 << OS) - 1);
      idx = (int)(w >> OS) & END;
      alpha = ((int)(w >> (OS + R::OBITS)) & 3) - 1; beta = ((int)(w >> (OS + R::OBITS + 2)) & 3) - 1;
      alpha0 = ((int)(w >> (OS + R::OBITS + 4)) & 3) - 1;
      b = R::top_bit(mask, (int)(ord >> (R::OBITS * idx)) & END);
      mask ^= b; cur ^= mask; --stones;
      v = -ret;
    } else {
      const int i = (int)(ord >> (R::OBITS * idx)) & END;
      if (i == END) {      // every move tried
        svt_store(tab, gen, R::key(cur, mask), alpha0, alpha, beta);
        ret = alpha; state = RET;
        continue;
      }
      if (nodes >= budget || d >= R::LEVELS) { *nodes_out = budget; return MZ_SV_UNSOLVED; }      // (d < LEVELS always: a guard)
      ++nodes;
      b = R::move_bit(mask, i);
      cur ^= mask; mask |= b; ++stones;
      if (stones < R::CELLS) {
        stack[d] = (level_t)((ord & (level_t)(((level_t)1 << OS) - 1)) | ((level_t)idx << OS) |
                             ((level_t)(alpha + 1) << (OS + R::OBITS)) | ((level_t)(beta + 1) << (OS + R::OBITS + 2)) |
                             ((level_t)(alpha0 + 1) << (OS + R::OBITS + 4)));
        ++d;
        const int a = -beta;
        beta = -alpha; alpha = a; state = ENTER;
        continue;
      }
      v = 0;      // the board is full: a draw
      mask ^= b; cur ^= mask; --stones;
    }
    if (v > alpha) alpha = v;
    ++idx; state = NEXT;
    if (alpha >= beta) {
      svt_store(tab, gen, R::key(cur, mask), alpha0, alpha, beta);
      ret = alpha; state = RET;
    }
  }
  *nodes_out = nodes;
  return -ret;
}

// The table search's own device memory (mz_solve_tt), allocated on its first use; SolveState's staging is shared.
struct SolveTableState {
  uint64_t *tables;      // [waves][64][2^MZ_SVT_BITS]: a table a lane, zeroed at allocation
  uint32_t *gens;        // [waves][64]: a generation counter a lane
  int waves;             // the most waves one chunk of num_envs positions launches: min(MZ_SVT_MAX_WAVES, ceil(B * A / 64))
};

// k_solve's launch shape (one wave a block, the wave's share of the units pulled from a counter in LDS) around sv_unit_tt;
// gridDim.x <= SolveTableState::waves (mz_solve_tt's launch sees to it).  Lane `lane` of block w owns table and counter
// 64 * w + lane.  The per-lane stacks are R::LEVELS words apart, an odd count of 4-byte (Connect Four) or 8-byte
// (TicTacToe) words, so the 32 lanes one LDS cycle serves fall on distinct banks.  The launch ends whatever the input: at
// most per_wave units a lane, and each unit ends (sv_unit_tt's comment: every turn of its loop places one of at most `budget`
// stones, leaves a level or enters the node of the stone just placed; the probe, the ordering and the clearing at a wrap are
// bounded loops).
template <int KIND>
static __global__ __launch_bounds__(64) void k_solve_tt(int A, const uint64_t *bits, const int32_t *step, int n_units,
                                                        int per_wave, uint32_t budget, uint64_t *tables, uint32_t *gens,
                                                        int8_t *values, uint32_t *nodes) {
  typedef typename SvRules<KIND>::level_t level_t;
  __shared__ level_t svt_stack[64 * SvRules<KIND>::LEVELS];
  __shared__ int sv_next;
  const int lane = threadIdx.x;
  const int base = blockIdx.x * per_wave;
  const int end = base + per_wave < n_units ? base + per_wave : n_units;
  if (lane == 0) sv_next = base + 64;
  __syncthreads();
  level_t *stack = svt_stack + lane * SvRules<KIND>::LEVELS;
  const size_t owner = (size_t)blockIdx.x * 64 + lane;
  uint64_t *tab = tables + (owner << MZ_SVT_BITS);
  uint32_t gen = gens[owner];
  int u = base + lane;
  for (int k = 0; k < per_wave && u < end; ++k) {
    const int pos = u / A, a = u - pos * A;
    uint32_t spent;
    gen = svt_next_gen(tab, gen);
    const int v = sv_unit_tt<KIND>(bits[2 * (size_t)pos], bits[2 * (size_t)pos + 1], step[pos], a, budget, stack, tab, gen, &spent);
    values[u] = (int8_t)v;
    nodes[u] = spent;
    u = atomicAdd(&sv_next, 1);
  }
  gens[owner] = gen;
}
