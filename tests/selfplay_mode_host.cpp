// selfplay_mode_host.cpp -- the self-play loop's search mode (csrc/mz_selfplay_mode.inc): the table of modes, the sentence of a
// refusal and the decision whether a switch may happen, compiled into a stand-alone program.  tests/test_selfplay_mode_cpu.py builds
// it with the host compiler under AddressSanitizer + UBSan and runs it.  No GPU is touched.
//
// Every combination of current mode, requested mode, on / off, parameter, environment, Gumbel search set or not, true-rules game,
// host draws, mz_sim_io and ring state goes through mz_sp_switch_ok and through a second statement of the rules below, a flat list of
// ifs with the sentences spelled out, which shares no code with the first.  Output: "ok <cases>"; a disagreement prints
// "MISMATCH ..." and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "mz_selfplay_mode.inc"

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static long cases = 0;

// the rules once more: "" = the switch happens, else the whole sentence.  g: the call is mz_selfplay_set_gumbel (else _true_model)
static std::string expected(int cur, bool g, bool on, int par, int env, bool gz, int tm, bool draws, bool io, unsigned long long waiting) {
  if (g && on && cur == 2) return "mz_selfplay_set_gumbel: the self-play moves are searched on the true rules (mz_selfplay_set_true_model 0 first)";
  if (g && on && par != 0 && par != 1) return "mz_selfplay_set_gumbel: value_kind " + std::to_string(par) + " (0 the root's mean value, 1 its v_mix)";
  if (g && on && !gz) return "mz_selfplay_set_gumbel: no Gumbel search is set on this engine (call mz_set_gumbel first)";
  if (g && on && env == 0) return "mz_selfplay_set_gumbel: the Gumbel self-play runs on the device games; set one first (mz_selfplay_set_env 1, 2 or 3)";
  if (g && on && draws) return "mz_selfplay_set_gumbel: host-given draws are set (mz_selfplay_set_draws); this mode draws its noise on the device";
  if (g && on && io) return "mz_selfplay_set_gumbel: mz_sim_io instruments the fused search kernels, which this mode does not run (mz_sim_io 0 first)";
  if (g && waiting) return "mz_selfplay_set_gumbel: " + std::to_string(waiting) + " moves wait in the device ring; drain them first";
  if (g) return "";
  if (on && cur == 1) return "mz_selfplay_set_true_model: the self-play moves are searched with the Gumbel search (mz_selfplay_set_gumbel 0 first)";
  if (on && (env == 0 || env == 2)) return "mz_selfplay_set_true_model: the true-rules self-play runs on the device board games; set one first (mz_selfplay_set_env 1 or 3)";
  if (on && env == 1 && tm != 1) return "mz_selfplay_set_true_model: the true-rules search of the environment's game is not set on this engine (call mz_set_true_model 1 first)";
  if (on && env == 3 && tm != 3) return "mz_selfplay_set_true_model: the true-rules search of the environment's game is not set on this engine (call mz_set_true_model 3 first)";
  if (on && draws) return "mz_selfplay_set_true_model: host-given draws are set (mz_selfplay_set_draws); this mode draws its noise on the device";
  if (on && io) return "mz_selfplay_set_true_model: mz_sim_io instruments the fused search kernels, which this mode does not run (mz_sim_io 0 first)";
  if (waiting) return "mz_selfplay_set_true_model: " + std::to_string(waiting) + " moves wait in the device ring; drain them first";
  return "";
}

// ... and the mode after a switch that happens
static int expected_next(int cur, bool g, bool on) {
  if (g && on) return 1;
  if (!g && on) return 2;
  if (g && cur == 1) return 0;
  if (!g && cur == 2) return 0;
  return cur;
}

static void switches() {
  static const int TM_KINDS[3] = {0, 1, 3};
  static const int PARS[4] = {0, 1, 2, -1};
  static const unsigned long long WAITING[3] = {0, 1, 37};
  for (int cur = 0; cur < 3; ++cur)
  for (int g = 0; g < 2; ++g)
  for (int on = 0; on < 2; ++on)
  for (int par : PARS)
  for (int env = 0; env < 4; ++env)
  for (int gz = 0; gz < 2; ++gz)
  for (int tm : TM_KINDS)
  for (int draws = 0; draws < 2; ++draws)
  for (int io = 0; io < 2; ++io)
  for (unsigned long long waiting : WAITING) {
    const MzSpFacts f = {(MzSpMode)cur, env, gz != 0, tm, draws != 0, io != 0, waiting};
    const char *fn = g ? "mz_selfplay_set_gumbel" : "mz_selfplay_set_true_model";
    char why[256];
    memset(why, '#', sizeof why);
    MzSpMode next = (MzSpMode)cur;
    const bool ok = mz_sp_switch_ok(f, fn, g ? MZ_SP_GUMBEL : MZ_SP_TRUE_RULES, on != 0, par, &next, why, sizeof why);
    const std::string want = expected(cur, g != 0, on != 0, par, env, gz != 0, tm, draws != 0, io != 0, waiting);
#define WHERE "cur %d %s on %d par %d env %d gz %d tm %d draws %d io %d waiting %llu", cur, fn, on, par, env, gz, tm, draws, io, waiting
    CHECK(ok == want.empty(), WHERE);
    if (ok) {
      CHECK((int)next == expected_next(cur, g != 0, on != 0), WHERE);
      if (!on && cur != (g ? 1 : 2)) CHECK((int)next == cur, WHERE);      // off of a mode that is not on: the current mode stays
    } else {
      CHECK(memchr(why, 0, sizeof why) != nullptr, WHERE);
      CHECK(want == why, "%s | %s", want.c_str(), why);
      CHECK(strncmp(why, fn, strlen(fn)) == 0 && why[strlen(fn)] == ':', "%s", why);
      CHECK(strchr(why, '\n') == nullptr && (int)next == cur, "%s", why);      // (one line; a refusal leaves *next alone)
      // refused because the other mode is on: the sentence names the call that switches that one off
      if (on && cur != 0 && cur != (g ? 1 : 2)) CHECK(strstr(why, MZ_SP_MODES[cur].undo) != nullptr, "%s", why);
    }
#undef WHERE
    ++cases;
  }
}

// the entry points that refuse while a mode is on, with the sentences they give
static void refusals() {
  static const struct { const char *fn, *why, *moves, *gumbel, *true_rules; } ENTRY[] = {
      {"mz_selfplay_set_env", "set for the current game", nullptr,
       "mz_selfplay_set_env: the self-play moves are searched with the Gumbel search, set for the current game (mz_selfplay_set_gumbel 0 first)",
       "mz_selfplay_set_env: the self-play moves are searched on the true rules, set for the current game (mz_selfplay_set_true_model 0 first)"},
      {"mz_selfplay_set_draws", "a mode that draws its noise on the device", nullptr,
       "mz_selfplay_set_draws: the self-play moves are searched with the Gumbel search, a mode that draws its noise on the device (mz_selfplay_set_gumbel 0 first)",
       "mz_selfplay_set_draws: the self-play moves are searched on the true rules, a mode that draws its noise on the device (mz_selfplay_set_true_model 0 first)"},
      {"mz_sim_io", "which the fused kernels do not run", nullptr,
       "mz_sim_io: the self-play moves are searched with the Gumbel search, which the fused kernels do not run (mz_selfplay_set_gumbel 0 first)",
       "mz_sim_io: the self-play moves are searched on the true rules, which the fused kernels do not run (mz_selfplay_set_true_model 0 first)"},
      {"mz_selfplay_steps_timed", "a search without a clocked dispatch", "the moves",
       "mz_selfplay_steps_timed: the moves are searched with the Gumbel search, a search without a clocked dispatch (mz_selfplay_set_gumbel 0 first)",
       "mz_selfplay_steps_timed: the moves are searched on the true rules, a search without a clocked dispatch (mz_selfplay_set_true_model 0 first)"},
  };
  for (const auto &en : ENTRY)
    for (int mode = 1; mode < 3; ++mode) {
      char buf[256], bare[256];
      if (en.moves) mz_sp_refusal(buf, sizeof buf, en.fn, (MzSpMode)mode, en.why, en.moves);
      else mz_sp_refusal(buf, sizeof buf, en.fn, (MzSpMode)mode, en.why);
      CHECK(strcmp(buf, mode == 1 ? en.gumbel : en.true_rules) == 0, "%s", buf);
      CHECK(strncmp(buf, en.fn, strlen(en.fn)) == 0 && strstr(buf, MZ_SP_MODES[mode].undo) != nullptr, "%s", buf);
      // without the name (a caller that puts it in front itself): the same sentence behind "<fn>: "
      if (en.moves) mz_sp_refusal(bare, sizeof bare, nullptr, (MzSpMode)mode, en.why, en.moves);
      else mz_sp_refusal(bare, sizeof bare, nullptr, (MzSpMode)mode, en.why);
      CHECK(strcmp(buf + strlen(en.fn) + 2, bare) == 0, "%s | %s", buf, bare);
      char tiny[24];      // a short buffer truncates, it is never overrun (the sanitizer watches)
      mz_sp_refusal(tiny, sizeof tiny, en.fn, (MzSpMode)mode, en.why);
      CHECK(strlen(tiny) == sizeof tiny - 1 && strncmp(tiny, buf, sizeof tiny - 1) == 0, "%s", tiny);
      ++cases;
    }
  CHECK(sizeof MZ_SP_MODES / sizeof MZ_SP_MODES[0] == 3 && !MZ_SP_MODES[MZ_SP_PUCT].how, "one row per mode");
}

int main() {
  switches();
  refusals();
  printf("ok %ld\n", cases);
  return 0;
}
