// playout_host.cpp -- the planner bodies of csrc/mz_playout.hip.h (po_plan and what it calls: pick, playout, per-action
// results, backup) compiled for the HOST and run on random TicTacToe and Connect Four positions at 1024 playouts per move.
// A stand-alone program (tests/test_playout_cpu.py builds it with the host pass of hipcc and -fsanitize=address,undefined,
// runs it, and compares the plans it prints with the library's mz_playout_plan_host on the same positions).  No GPU is
// touched.  The tree's memory is a heap block of exactly po_wave_bytes, so a node or a board cell outside it is an
// AddressSanitizer report.  The planner knows the rules through mz_game_step / mz_game_legal of csrc/mz_games.h only
// (there is no second form of them to compare here).
//
// Output: one line per position, "kind turn step action v[0..A) w[0..A) cell[0..42)"; position i is the game with the seed
// ENV_OFFSET + i, every plan has the engine seed SEED and the move MOVE; the last line is "ok <positions>".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mz_engine.h"
#include "mz_playout.hip.h"

static const uint64_t SEED = 11;
static const int ENV_OFFSET = 5000, MOVE = 3, PLAYOUTS = 1024, PER_KIND = 150;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// a position after `plies` random legal plies in which the game has not ended (tried again until there is one)
static void random_position(int kind, int plies, int8_t *bd, int *turn) {
  for (;;) {
    memset(bd, 0, 42);
    int t = 1, p = 0;
    bool ended = false;
    for (; p < plies && !ended; ++p) {
      const uint32_t mask = po_legal(kind, bd);
      bool won;
      ended = po_step(kind, bd, t, po_nth(mask, (int)(rnd() % (uint32_t)__builtin_popcount(mask))), p, &won);
      t = -t;
    }
    if (!ended) { *turn = t; return; }
  }
}

int main() {
  const int iters = PLAYOUTS / MZ_PO_LANES;
  std::vector<double> ln((size_t)iters + 1, 0.0);
  for (int v = 1; v <= iters; ++v) ln[v] = log(64.0 * (double)v);
  int index = 0;
  for (int kind = 1; kind <= 3; kind += 2) {
    const int A = mz_game_info(kind).actions, longest = mz_game_info(kind).longest;
    const size_t bytes = po_wave_bytes(iters + 1, A);
    for (int i = 0; i < PER_KIND; ++i, ++index) {
      unsigned char *mem = (unsigned char *)malloc(bytes);      // (fresh and uninitialised for every plan: po_plan clears what it reads)
      if (!mem) return 2;
      PoTree t;
      int8_t *lane_boards, *root;
      po_carve(mem, iters + 1, A, &t, &lane_boards, &root);
      int turn;
      const int plies = (int)(rnd() % (uint32_t)(longest - 1));
      random_position(kind, plies, root, &turn);
      int8_t start[42];
      memcpy(start, root, 42);
      int32_t action = -1, visits[9], wins[9];
      po_plan(kind, t, lane_boards, root, turn, plies, iters, ln.data(), SEED, (uint32_t)(ENV_OFFSET + index), (uint32_t)MOVE, 0,
              &action, visits, wins);
      if (memcmp(start, root, 42)) { printf("MISMATCH the root position changed: position %d\n", index); return 1; }
      if (action < 0 || action >= A || !((po_legal(kind, root) >> action) & 1u)) { printf("MISMATCH an illegal plan: position %d\n", index); return 1; }
      long total = 0;
      for (int a = 0; a < A; ++a) total += visits[a];
      if (total != PLAYOUTS) { printf("MISMATCH %ld playouts at the root, not %d: position %d\n", total, PLAYOUTS, index); return 1; }
      printf("%d %d %d %d", kind, turn, plies, action);
      for (int a = 0; a < A; ++a) printf(" %d", visits[a]);
      for (int a = 0; a < A; ++a) printf(" %d", wins[a]);
      for (int k = 0; k < 42; ++k) printf(" %d", (int)root[k]);
      printf("\n");
      free(mem);
    }
  }
  printf("ok %d\n", index);
  return 0;
}
