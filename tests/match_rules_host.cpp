// match_rules_host.cpp -- the per-game bodies of csrc/mz_match.hip.h (mz_match_open_game, mz_match_observe_game,
// mz_match_apply_game) compiled for the HOST and played against a rule check of this file's own: random TicTacToe and
// Connect Four games, every ply through the opening body (an index into the legal list) or the apply body (an action),
// and after every ply a window scan of the whole board for a line of three / four says who -- if anyone -- has won.
// Before the games, mz_depth_list_max (csrc/mz_games.h) is called on a handful of lists that differ.
// A stand-alone program (tests/test_match_cpu.py builds it with the host pass of hipcc and -fsanitize=address,undefined,
// runs it, and replays the digest's action lists on the envs.py classes).  No GPU is touched.
//
// Output: one line per game, "kind max_steps path result length a0 a1 ...", path 0 = opening body, 1 = apply body; the
// last line is "ok <games>".  Any disagreement prints "MISMATCH ..." and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mz_engine.h"
#include "mz_match.hip.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// +1 / -1: that player has a line of `need` anywhere on the board (scanned window by window); 0: nobody
static int scan_winner(const int8_t *bd, int rows, int cols, int need) {
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c)
      for (int d = 0; d < 4; ++d) {
        const int er = r + (need - 1) * dr[d], ec = c + (need - 1) * dc[d];
        if (er < 0 || er >= rows || ec < 0 || ec >= cols) continue;
        int sum = 0;
        for (int k = 0; k < need; ++k) sum += bd[cols * (r + k * dr[d]) + c + k * dc[d]];
        if (sum == need) return 1;
        if (sum == -need) return -1;
      }
  return 0;
}

struct Host {
  MatchState ms;
  std::vector<int8_t> board, turn, result, to_play, log_mover, log_net;
  std::vector<int32_t> step, live, n_searched, depth_max, actions, n_actions, path_lengths, log_action, log_depths, open_idx;
  std::vector<uint8_t> terminal, legal;
  std::vector<double> acc, noise, walk_u, temp, child_visits, root_value, log_reward, log_root_value, log_child_visits;
  std::vector<float> obs, pred_rewards, log_pred_reward, log_pred_value;
  Host(int kind, int max_steps, int B, int A, int O, int S) {
    memset(&ms, 0, sizeof ms);
    const int longest = mz_game_info(kind).longest;
    ms.kind = kind; ms.max_steps = max_steps; ms.cap = max_steps < longest ? max_steps : longest; ms.S = S;
    const size_t L = (size_t)B * ms.cap;
    board.assign((size_t)B * 42, 0); turn.assign(B, 1); result.assign(B, 0); to_play.assign(B, 0);
    step.assign(B, 0); live.assign(1, B); terminal.assign(B, 0); legal.assign((size_t)B * A, 0);
    acc.assign((size_t)8 * B, 0.0); n_searched.assign((size_t)2 * B, 0); depth_max.assign((size_t)2 * B * S, 0);
    obs.assign((size_t)B * O, 0.f); noise.assign((size_t)B * A, 0.0); walk_u.assign(B, 0.0); temp.assign((size_t)2 * B, 0.0);
    actions.assign(B, 0); pred_rewards.assign(B, 0.f); n_actions.assign(B, 1); path_lengths.assign((size_t)B * S, 1);
    child_visits.assign((size_t)B * A, 0.0); root_value.assign(B, 0.0); open_idx.assign(B, 0);
    log_action.assign(L, 0); log_mover.assign(L, 0); log_net.assign(L, 0); log_reward.assign(L, 0.0);
    log_pred_reward.assign(L, 0.f); log_pred_value.assign(L, 0.f); log_root_value.assign(L, 0.0);
    log_child_visits.assign(L * A, 0.0); log_depths.assign(L * S, 0);
    ms.board = board.data(); ms.turn = turn.data(); ms.step = step.data(); ms.terminal = terminal.data();
    ms.live = live.data(); ms.result = result.data(); ms.acc = acc.data(); ms.n_searched = n_searched.data();
    ms.depth_max = depth_max.data(); ms.obs = obs.data(); ms.legal = legal.data(); ms.to_play = to_play.data();
    ms.noise = noise.data(); ms.walk_u = walk_u.data(); ms.temp = temp.data(); ms.actions = actions.data();
    ms.pred_rewards = pred_rewards.data(); ms.n_actions = n_actions.data(); ms.path_lengths = path_lengths.data();
    ms.child_visits = child_visits.data(); ms.root_value = root_value.data();
    ms.log_action = log_action.data(); ms.log_mover = log_mover.data(); ms.log_net = log_net.data();
    ms.log_reward = log_reward.data(); ms.log_pred_reward = log_pred_reward.data(); ms.log_pred_value = log_pred_value.data();
    ms.log_root_value = log_root_value.data(); ms.log_child_visits = log_child_visits.data(); ms.log_depths = log_depths.data();
    ms.d_open = open_idx.data(); ms.d_open_n = 1;      // [B][1]: the index of the one opening ply a call applies
  }
};

static int fail(const char *what, int kind, int b, int ply) {
  printf("MISMATCH %s: kind %d game %d ply %d\n", what, kind, b, ply);
  return 1;
}

// B random games of one kind, all of them advanced ply by ply; game b goes through the opening body when b is even and
// through the apply body when it is odd
static int play(int kind, int max_steps, int B, long *games) {
  const int A = mz_game_info(kind).actions, O = mz_game_info(kind).obs_dim, S = 3;
  const int rows = kind == 1 ? 3 : 6, cols = kind == 1 ? 3 : 7, need = kind == 1 ? 3 : 4, cells = rows * cols;
  Host h(kind, max_steps, B, A, O, S);
  MatchState &ms = h.ms;
  std::vector<int> applied((size_t)B, 0);
  for (int ply = 0; ply < ms.cap + 2; ++ply) {      // (two plies past the longest game: a finished game is left alone)
    for (int b = 0; b < B; ++b) {
      const bool was_terminal = ms.terminal[b] != 0;
      const int step0 = ms.step[b], mover = ms.turn[b];
      int8_t before[42];
      memcpy(before, ms.board + (size_t)b * 42, 42);
      mz_match_observe_game(ms, b, O, A, ply);
      // the observation and the legal mask against the board
      int nlegal = 0, legal_list[9];
      for (int a = 0; a < A; ++a) {
        const bool open_cell = kind == 1 ? before[a] == 0 : before[35 + a] == 0;
        if (ms.legal[(size_t)b * A + a] != (was_terminal ? 1 : (open_cell ? 1 : 0))) return fail("legal mask", kind, b, ply);
        if (!was_terminal && open_cell) legal_list[nlegal++] = a;
      }
      for (int k = 0; k < O; ++k)
        if (ms.obs[(size_t)b * O + k] != (was_terminal ? 0.f : (float)(mover * before[k]))) return fail("observation", kind, b, ply);
      if (ms.to_play[b] != (was_terminal ? 1 : mover)) return fail("to_play", kind, b, ply);
      if (!was_terminal && nlegal == 0) return fail("a live game without a legal action", kind, b, ply);
      const int pick = was_terminal ? 0 : (int)(rnd() % (uint32_t)nlegal);
      const int action = was_terminal ? (int)(rnd() % (uint32_t)A) : legal_list[pick];
      bool ended;
      if (b % 2 == 0) {
        ms.opening = 1;
        h.open_idx[b] = pick;
        ended = mz_match_open_game(ms, b, A, 0, (uint32_t)b);
      } else {
        ms.actions[b] = action;
        for (int s = 0; s < S; ++s) h.path_lengths[(size_t)b * S + s] = 1 + (int)(rnd() % 3u);
        ended = mz_match_apply_game(ms, b, B, A, ply & 1, (int)(rnd() % 3u), S, 0.25f);
      }
      if (was_terminal) {      // left alone
        if (ended || ms.step[b] != step0 || memcmp(before, ms.board + (size_t)b * 42, 42)) return fail("a finished game moved", kind, b, ply);
        continue;
      }
      // exactly one stone of the mover was placed, where the rules put it
      int changed = 0, at = -1;
      for (int k = 0; k < 42; ++k)
        if (before[k] != ms.board[(size_t)b * 42 + k]) { ++changed; at = k; }
      if (changed != 1 || at >= cells || before[at] != 0 || ms.board[(size_t)b * 42 + at] != mover) return fail("one stone per ply", kind, b, ply);
      if (kind == 1 ? at != action : (at % 7 != action || (at >= 7 && before[at - 7] == 0))) return fail("the stone's cell", kind, b, ply);
      if (ms.step[b] != step0 + 1 || ms.turn[b] != -mover) return fail("step / turn", kind, b, ply);
      if (h.log_action[(size_t)b * ms.cap + step0] != action) return fail("logged action", kind, b, ply);
      ++applied[b];
      // the end of the game against the window scan
      const int winner = scan_winner(ms.board + (size_t)b * 42, rows, cols, need);
      bool full = true;
      for (int k = 0; k < cells; ++k) full = full && ms.board[(size_t)b * 42 + k] != 0;
      const bool want_end = winner != 0 || full || step0 + 1 >= max_steps;
      if (ended != want_end || (ms.terminal[b] != 0) != want_end) return fail("end of the game", kind, b, ply);
      if (want_end && ms.result[b] != winner) return fail("result", kind, b, ply);
      if (winner != 0 && winner != mover) return fail("a win by the player who did not move", kind, b, ply);
      const int8_t lm = h.log_mover[(size_t)b * ms.cap + step0];
      if (lm != ((winner != 0 || full) ? 2 * mover : mover)) return fail("logged mover / done", kind, b, ply);
      if (h.log_reward[(size_t)b * ms.cap + step0] != (winner != 0 ? 1.0 : 0.0)) return fail("logged reward", kind, b, ply);
    }
  }
  for (int b = 0; b < B; ++b) {
    if (!ms.terminal[b] || ms.step[b] != applied[b]) return fail("a game did not end", kind, b, -1);
    printf("%d %d %d %d %d", kind, max_steps, b % 2, (int)ms.result[b], (int)ms.step[b]);
    for (int p = 0; p < ms.step[b]; ++p) printf(" %d", h.log_action[(size_t)b * ms.cap + p]);
    printf("\n");
    ++*games;
  }
  return 0;
}

// mz_depth_list_max (csrc/mz_games.h) on lists that differ: the games above hand it nothing but lists it takes or ties
static int depth_lists() {
  struct Case { int32_t pl[4]; bool first, taken; const char *what; };
  const Case cases[] = {
      {{2, 1, 3, 1}, true, true, "the first list is always taken"},
      {{2, 1, 3, 1}, false, false, "an equal list"},
      {{2, 1, 2, 9}, false, false, "a list smaller at the first index that differs, greater later"},
      {{1, 9, 9, 9}, false, false, "a list smaller at index 0"},
      {{2, 2, 0, 0}, false, true, "a list greater at an early index, smaller later"},
      {{2, 2, 0, 1}, false, true, "a list greater at the last index"},
      {{0, 0, 0, 0}, true, true, "a smaller list that is the first"},
  };
  int32_t dm[4] = {7, 7, 7, 7};      // (never compared: the first case is the first list)
  double mean = -1.0;
  for (const Case &c : cases) {
    int32_t before[4];
    memcpy(before, dm, sizeof dm);
    const double mean_before = mean;
    const bool taken = mz_depth_list_max(dm, c.pl, 4, c.first, &mean);
    const int32_t *want = c.taken ? c.pl : before;
    const double want_mean = c.taken ? (double)(c.pl[0] + c.pl[1] + c.pl[2] + c.pl[3]) / 4.0 : mean_before;
    if (taken != c.taken || memcmp(dm, want, sizeof dm) || mean != want_mean) {
      printf("MISMATCH depth lists: %s\n", c.what);
      return 1;
    }
  }
  return 0;
}

int main() {
  if (depth_lists()) return 1;
  long games = 0;
  // whole games, and games cut at max_steps (5 plies of TicTacToe, 11 of Connect Four)
  if (play(1, 100, 1500, &games) || play(3, 100, 1500, &games) || play(1, 5, 300, &games) || play(3, 11, 300, &games)) return 1;
  printf("ok %ld\n", games);
  return 0;
}
