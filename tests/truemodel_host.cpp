// truemodel_host.cpp -- mz_tm_search_host (csrc/mz_truemodel_host.inc), the host twin of the true-rules search, compiled
// into a stand-alone program and run on random TicTacToe and Connect Four positions with a leaf evaluation of this file's
// own (a hash of the observation: values in (-1, 1), logits on a grid so that ties occur).  tests/test_truemodel_cpu.py
// builds it with the host pass of hipcc and -fsanitize=address,undefined and runs it.  No GPU is touched.
//
// After every search the trees are checked against what the definition promises whatever the network says: the root's
// visit count and its children's sum are the simulations run; a taken slot's child mask is the legal mask of its stored
// position, or empty exactly when the position is finished; no child of a finished slot was created; every visited
// child's reward is 0 or 1.  Output: "ok <trees>"; any disagreement prints "MISMATCH ..." and exits 1.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mz_engine.h"
#include "mz_engine_debug.h"
#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS      // (as mz_engine.hip sets it for mz_tree.hip.h)
#include "mz_truemodel.hip.h"

static int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  return -1;
}

extern "C" {
#include "mz_truemodel_host.inc"
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Ctx { int O, A; long calls; };

static void eval_hash(void *ctx, const float *obs, int n, float *value, float *logits) {
  Ctx *c = (Ctx *)ctx;
  c->calls += 1;
  for (int i = 0; i < n; ++i) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (int k = 0; k < c->O; ++k) h = (h ^ (uint64_t)((int)obs[(size_t)i * c->O + k] + 1)) * 0x100000001B3ull;
    value[i] = (float)((double)(2 * (int64_t)((h >> 20) & 0x3FFFFF) - 0x3FFFFF) / (double)0x400000);
    for (int a = 0; a < c->A; ++a) {
      h = h * 6364136223846793005ull + 1442695040888963407ull;
      logits[(size_t)i * c->A + a] = (float)((int)((h >> 58) & 63) - 32) / 16.f;
    }
  }
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static int run_kind(int kind, int n, int sims, bool with_noise) {
  const MzGameInfo g = mz_game_info(kind);
  const int A = g.actions, O = g.obs_dim, S = sims + 1, NN = 1 + S * A;
  std::vector<int8_t> boards((size_t)n * 42, 0), turn(n, 1);
  std::vector<int32_t> step(n, 0);
  for (int b = 0; b < n; ++b) {      // random legal plies from the empty board; a game that ends starts over
    for (;;) {
      int8_t *bd = boards.data() + (size_t)b * 42;
      memset(bd, 0, 42);
      int t = 0, mover = 1;
      const int plies = (int)(rnd() % (uint32_t)(g.longest - 1));
      bool over = false;
      for (; t < plies && !over; ++t) {
        const uint32_t mask = mz_game_legal(kind, bd);
        bool won = false;
        over = mz_game_step(kind, bd, mover, mz_pick_legal(mask, (int)(rnd() % 9u)), t, &won);
        mover = -mover;
      }
      if (over) continue;
      turn[b] = (int8_t)mover; step[b] = t;
      break;
    }
  }
  mz_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.num_envs = n; cfg.obs_dim = O; cfg.action_space = A; cfg.num_simulations = sims; cfg.two_players = 1;
  cfg.value_support_min = cfg.reward_support_min = -15; cfg.value_support_max = cfg.reward_support_max = 15;
  cfg.discount = 0.997; cfg.pb_c_base = 19652; cfg.pb_c_init = 1.25; cfg.root_dirichlet_alpha = 0.25;
  cfg.root_exploration_fraction = 0.25;
  Ctx ctx = {O, A, 0};
  std::vector<float> obs((size_t)n * O), v(n), lg((size_t)n * A);
  for (int b = 0; b < n; ++b)
    for (int k = 0; k < O; ++k) obs[(size_t)b * O + k] = (float)(turn[b] * boards[(size_t)b * 42 + k]);
  eval_hash(&ctx, obs.data(), n, v.data(), lg.data());
  std::vector<double> noise((size_t)n * A, 0.0);
  for (int b = 0; b < n; ++b) {
    const uint32_t mask = mz_game_legal(kind, boards.data() + (size_t)b * 42);
    double sum = 0.0;
    for (int a = 0; a < A; ++a) if ((mask >> a) & 1u) sum += noise[(size_t)b * A + a] = 1.0 + (double)(rnd() % 1000u);
    for (int a = 0; a < A; ++a) noise[(size_t)b * A + a] /= sum;
  }
  std::vector<int32_t> N((size_t)n * NN), E((size_t)n * NN), nexp(n), sstep((size_t)n * S), depth((size_t)n * sims);
  std::vector<double> W((size_t)n * NN), P((size_t)n * NN), mm((size_t)n * 2);
  std::vector<float> R((size_t)n * NN);
  std::vector<int8_t> TP((size_t)n * NN), sb((size_t)n * S * 42), smover((size_t)n * S);
  std::vector<uint32_t> legal(n), smask((size_t)n * S);
  std::vector<uint8_t> sfin((size_t)n * S);
  ctx.calls = 0;
  const int rc = mz_tm_search_host(&cfg, kind, n, boards.data(), turn.data(), step.data(), lg.data(), with_noise ? noise.data() : nullptr,
                                   sims, eval_hash, &ctx, N.data(), W.data(), P.data(), R.data(), E.data(), TP.data(), legal.data(),
                                   mm.data(), nexp.data(), sb.data(), smover.data(), sstep.data(), smask.data(), sfin.data(), depth.data());
  CHECK(rc == 0, "kind %d: the twin failed", kind);
  CHECK(ctx.calls == sims, "kind %d: %ld evaluations for %d simulations", kind, ctx.calls, sims);
  for (int b = 0; b < n; ++b) {
    const size_t o = (size_t)b * NN;
    CHECK(N[o] == sims, "kind %d tree %d: N[root] %d", kind, b, N[o]);
    long sum = 0;
    for (int a = 0; a < A; ++a) if ((legal[b] >> a) & 1u) sum += N[o + 1 + a];
    CHECK(sum == sims, "kind %d tree %d: the root's children were visited %ld times", kind, b, sum);
    CHECK(nexp[b] >= 2 && nexp[b] <= S, "kind %d tree %d: nexp %d", kind, b, nexp[b]);
    for (int e = 0; e < nexp[b]; ++e) {
      const size_t i = (size_t)b * S + e;
      const uint32_t want = mz_game_legal(kind, sb.data() + i * 42);
      CHECK(sfin[i] ? smask[i] == 0u : smask[i] == want && want != 0u, "kind %d tree %d slot %d: mask %x, legal %x, finished %d", kind,
            b, e, smask[i], want, sfin[i]);
      for (int a = 0; a < A; ++a) {
        const size_t c = o + 1 + (size_t)e * A + a;
        if (!((smask[i] >> a) & 1u)) CHECK(N[c] == 0 && E[c] == -1 && TP[c] == 0 && P[c] == 0.0, "kind %d tree %d: a child that does not exist was touched", kind, b);
        else CHECK(R[c] == 0.f || R[c] == 1.f, "kind %d tree %d: reward %g", kind, b, (double)R[c]);
      }
    }
  }
  return n;
}

int main() {
  int trees = 0;
  for (int kind = 1; kind <= 3; kind += 2)
    for (int noise = 0; noise < 2; ++noise) trees += run_kind(kind, kind == 1 ? 200 : 100, 30, noise != 0);
  printf("ok %d\n", trees);
  return 0;
}
