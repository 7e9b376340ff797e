// mz_selfplay_mode.inc -- how the self-play loop searches a move (DESIGN s7l): the one mode of an engine, how a refusal names it, and
// whether a switch of it may happen.  Pure host code over the C library, no HIP header (mz_selfplay_abi.inc gathers the facts and
// makes the HIP calls), so that tests/selfplay_mode_host.cpp can hold every rule to a flat restatement without a GPU.
#pragma once
#include <stddef.h>
#include <stdio.h>

// PUCT on the learned model (the default, and the only mode of the fused kernels and of whole moves per launch), the Gumbel search
// (mz_selfplay_set_gumbel; DESIGN s7i), PUCT on the game's true rules (mz_selfplay_set_true_model; s7k)
enum MzSpMode { MZ_SP_PUCT = 0, MZ_SP_GUMBEL = 1, MZ_SP_TRUE_RULES = 2 };

// per mode: how a sentence names it, and the call that switches it off.  A new mode is one more row.
static const struct { const char *how, *undo; } MZ_SP_MODES[] = {
    {nullptr, nullptr}, {"with the Gumbel search", "mz_selfplay_set_gumbel 0"}, {"on the true rules", "mz_selfplay_set_true_model 0"}};

// "[<fn>: ]<moves> are searched <how>[, <why>] (<undo> first)": what an entry point refuses while `mode` (not PUCT) is on; fn null:
// without the prefix, for a caller that puts its name in front itself
inline const char *mz_sp_refusal(char *buf, size_t n, const char *fn, MzSpMode mode, const char *why, const char *moves = "the self-play moves") {
  snprintf(buf, n, "%s%s%s are searched %s%s%s (%s first)", fn ? fn : "", fn ? ": " : "", moves, MZ_SP_MODES[mode].how, why ? ", " : "",
           why ? why : "", MZ_SP_MODES[mode].undo);
  return buf;
}

// what a switch reads: the current mode; the loop's environment (mz_selfplay_set_env); whether a Gumbel search is set (mz_set_gumbel);
// the game of the true-rules search (mz_set_true_model: 0 none); host-given draws set; mz_sim_io on; moves waiting in the device ring
struct MzSpFacts { MzSpMode mode; int env_kind; bool gumbel_set; int tm_kind; bool draws_set, sim_io; unsigned long long undrained; };

// May fn -- mz_selfplay_set_gumbel (which = MZ_SP_GUMBEL, par = value_kind) or mz_selfplay_set_true_model (MZ_SP_TRUE_RULES; any par) -- switch its mode on / off?
// true: *next is the mode afterwards (off of a mode that is not on leaves the current one); false: why holds the sentence of the first rule not met, fn in front.
inline bool mz_sp_switch_ok(const MzSpFacts &f, const char *fn, MzSpMode which, bool on, int par, MzSpMode *next, char *why, size_t n) {
  if (on && f.mode != MZ_SP_PUCT && f.mode != which) { mz_sp_refusal(why, n, fn, f.mode, nullptr); return false; }
  char own[192] = "";
#define NO(...) snprintf(own, sizeof own, __VA_ARGS__)
  if (on && which == MZ_SP_GUMBEL) {
    if (par != 0 && par != 1) NO("value_kind %d (0 the root's mean value, 1 its v_mix)", par);
    else if (!f.gumbel_set) NO("no Gumbel search is set on this engine (call mz_set_gumbel first)");
    else if (!f.env_kind) NO("the Gumbel self-play runs on the device games; set one first (mz_selfplay_set_env 1, 2 or 3)");
  } else if (on) {
    if (f.env_kind != 1 && f.env_kind != 3) NO("the true-rules self-play runs on the device board games; set one first (mz_selfplay_set_env 1 or 3)");
    else if (f.tm_kind != f.env_kind)
      NO("the true-rules search of the environment's game is not set on this engine (call mz_set_true_model %d first)", f.env_kind);
  }
  if (on && !own[0] && f.draws_set) NO("host-given draws are set (mz_selfplay_set_draws); this mode draws its noise on the device");
  else if (on && !own[0] && f.sim_io) NO("mz_sim_io instruments the fused search kernels, which this mode does not run (mz_sim_io 0 first)");
  if (!own[0] && f.undrained) NO("%llu moves wait in the device ring; drain them first", f.undrained);
#undef NO
  if (own[0]) { snprintf(why, n, "%s: %s", fn, own); return false; }
  *next = on ? which : (f.mode == which ? MZ_SP_PUCT : f.mode);
  return true;
}
