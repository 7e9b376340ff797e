// reanalyse_tm_host.cpp -- mz_reanalyse_position (csrc/mz_reanalyse.hip.h), the decode of a stored observation into the root of a
// true-rules tree (DESIGN s7n), as a stand-alone program: tests/test_reanalyse_true_model_cpu.py builds it with the host pass of
// hipcc and -fsanitize=address,undefined, and runs it.  No GPU is touched.
//
// The positions come from the file named on the command line, one per line:
//   kind mover step  board[0] .. board[cells-1]  obs[0] .. obs[O-1]         (kind 1: cells = O = 9; kind 3: cells = O = 42)
// with the host environment's own board and ply count.  The observation buffer holds exactly O floats and the board buffer
// exactly the game's cells: a read or a write past either is a heap error.  Checked per position: every cell and the step equal
// the environment's, and mz_game_legal of the decoded board equals mz_reanalyse_legal_mask of the observation.
//
// Output: the last line is "ok <positions> positions".  Any disagreement prints "MISMATCH ..." and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mz_engine.h"
#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS      // (as mz_engine.hip sets it before the kernel headers)
#include "mz_reanalyse.hip.h"

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: reanalyse_tm_host positions.txt\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { printf("MISMATCH cannot open %s\n", argv[1]); return 1; }
  long count = 0;
  int kind, mover, step;
  while (fscanf(f, "%d %d %d", &kind, &mover, &step) == 3) {
    if ((kind != 1 && kind != 3) || (mover != 1 && mover != -1)) { fclose(f); printf("MISMATCH bad line %ld\n", count); return 1; }
    const int cells = mz_game_info(kind).cells, O = mz_game_info(kind).obs_dim, A = mz_game_info(kind).actions;
    std::vector<int8_t> want((size_t)cells), got((size_t)cells, (int8_t)77);
    std::vector<float> obs((size_t)O);
    for (int k = 0; k < cells; ++k) { int v; if (fscanf(f, "%d", &v) != 1) { fclose(f); printf("MISMATCH bad line %ld\n", count); return 1; } want[(size_t)k] = (int8_t)v; }
    for (int k = 0; k < O; ++k) { int v; if (fscanf(f, "%d", &v) != 1) { fclose(f); printf("MISMATCH bad line %ld\n", count); return 1; } obs[(size_t)k] = (float)v; }
    int32_t got_step = -1;
    mz_reanalyse_position(kind, obs.data(), mover, got.data(), &got_step);
    if (memcmp(got.data(), want.data(), (size_t)cells) != 0) { fclose(f); printf("MISMATCH board: kind %d position %ld\n", kind, count); return 1; }
    if (got_step != step) { fclose(f); printf("MISMATCH step: kind %d position %ld: %d, the environment says %d\n", kind, count, (int)got_step, step); return 1; }
    const uint32_t by_board = mz_game_legal(kind, got.data()), by_obs = mz_reanalyse_legal_mask(kind, obs.data(), A);
    if (by_board != by_obs) { fclose(f); printf("MISMATCH legal: kind %d position %ld: %u from the board, %u from the observation\n", kind, count, by_board, by_obs); return 1; }
    ++count;
  }
  fclose(f);
  printf("ok %ld positions\n", count);
  return 0;
}
