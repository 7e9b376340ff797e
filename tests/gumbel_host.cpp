// gumbel_host.cpp -- mz_gz_search_host (csrc/mz_gumbel_host.inc), the host twin of the Gumbel search, compiled into a
// stand-alone program and run on random roots with a leaf evaluation of this file's own (a hash of (tree, parent slot,
// action): values and rewards in sixteenths, logits in eighths, so that ties occur).  tests/test_gumbel_cpu.py builds it
// with the host pass of hipcc and -fsanitize=address,undefined and runs it.  No GPU is touched.
//
// After every search the trees are checked against what the definition promises whatever the network says: the root's
// visit count and its legal children's sum are the simulations run; no illegal root child was visited; simulation s went
// to a root child that had seq(m, n)[s] visits; the chosen action is legal and among the most visited; pi' is 0 on illegal
// actions and sums to 1; every path ends at the node the expansion took.  Output: "ok <trees>"; any disagreement prints
// "MISMATCH ..." and exits 1.
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
#include "mz_gumbel.hip.h"

static int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  return -1;
}

extern "C" {
#include "mz_gumbel_host.inc"
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Ctx { int A; uint64_t salt; long calls; };

static void eval_hash(void *ctx, int sim, const int32_t *slot, const int32_t *act, int n, float *value, float *reward, float *logits) {
  Ctx *c = (Ctx *)ctx;
  (void)sim;
  c->calls += 1;
  for (int i = 0; i < n; ++i) {
    uint64_t h = (c->salt ^ (uint64_t)i) * 0x100000001B3ull;
    h = (h ^ (uint64_t)slot[i]) * 0x100000001B3ull;
    h = (h ^ (uint64_t)act[i]) * 0x100000001B3ull;
    h = h * 6364136223846793005ull + 1442695040888963407ull;
    value[i] = (float)((int)((h >> 59) & 31) - 16) / 16.f;
    h = h * 6364136223846793005ull + 1442695040888963407ull;
    reward[i] = (float)((int)((h >> 60) & 15) - 8) / 16.f;
    for (int a = 0; a < c->A; ++a) {
      h = h * 6364136223846793005ull + 1442695040888963407ull;
      logits[(size_t)i * c->A + a] = (float)((int)((h >> 59) & 31) - 16) / 8.f;
    }
  }
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static int run_shape(int A, bool two, bool bounds, int n, int sims, int considered, double scale) {
  const int S = sims + 1, NN = 1 + S * A, PL = sims + 2;
  mz_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.num_envs = n; cfg.obs_dim = 4; cfg.action_space = A; cfg.num_simulations = sims; cfg.two_players = two ? 1 : 0;
  cfg.has_min_bound = cfg.has_max_bound = bounds ? 1 : 0; cfg.min_bound = -1.0; cfg.max_bound = 1.0;
  cfg.value_support_min = cfg.reward_support_min = -15; cfg.value_support_max = cfg.reward_support_max = 15;
  cfg.discount = 0.997; cfg.pb_c_base = 19652; cfg.pb_c_init = 1.25; cfg.root_dirichlet_alpha = 0.25;
  cfg.root_exploration_fraction = 0.25;
  std::vector<int8_t> tp(n);
  std::vector<uint8_t> legal((size_t)n * A, 0);
  std::vector<float> rv(n), lg((size_t)n * A);
  std::vector<double> G((size_t)n * A);
  for (int b = 0; b < n; ++b) {
    tp[b] = (two && (rnd() & 1u)) ? -1 : 1;
    const int k = 1 + (int)(rnd() % (uint32_t)A);      // 1 .. A legal actions
    for (int placed = 0; placed < k;) {
      const int a = (int)(rnd() % (uint32_t)A);
      if (!legal[(size_t)b * A + a]) { legal[(size_t)b * A + a] = 1; ++placed; }
    }
    rv[b] = (float)((int)(rnd() % 32u) - 16) / 16.f;
    for (int a = 0; a < A; ++a) {
      lg[(size_t)b * A + a] = (float)((int)(rnd() % 32u) - 16) / 8.f;
      G[(size_t)b * A + a] = (double)((int)(rnd() % 512u) - 256) / 64.0;
    }
  }
  Ctx ctx = {A, (uint64_t)rnd(), 0};
  std::vector<int32_t> N((size_t)n * NN), E((size_t)n * NN), ss((size_t)n * sims), sa((size_t)n * sims), paths((size_t)n * sims * PL),
      plens((size_t)n * sims), action(n), seq(sims);
  std::vector<double> W((size_t)n * NN), P((size_t)n * NN), mm((size_t)n * 2), pi((size_t)n * A), vmix(n);
  std::vector<float> R((size_t)n * NN), vhat((size_t)n * S), pr(n);
  std::vector<int8_t> TP((size_t)n * NN);
  std::vector<uint32_t> mask(n);
  double gap = 0.0;
  const int rc = mz_gz_search_host(&cfg, n, tp.data(), legal.data(), rv.data(), lg.data(), scale != 0.0 ? G.data() : nullptr, considered,
                                   50.0, 1.0, scale, sims, eval_hash, &ctx, N.data(), W.data(), P.data(), R.data(), E.data(), TP.data(),
                                   mask.data(), mm.data(), vhat.data(), ss.data(), sa.data(), paths.data(), plens.data(), action.data(),
                                   pr.data(), pi.data(), vmix.data(), &gap);
  CHECK(rc == 0, "A %d: the twin failed", A);
  CHECK(ctx.calls == sims, "A %d: %ld evaluations for %d simulations", A, ctx.calls, sims);
  CHECK(gap > 0.0, "A %d: min_gap %g", A, gap);
  for (int b = 0; b < n; ++b) {
    const size_t o = (size_t)b * NN;
    CHECK(N[o] == sims, "A %d tree %d: N[root] %d", A, b, N[o]);
    long sum = 0;
    int nl = 0, maxn = 0;
    for (int a = 0; a < A; ++a) {
      if ((mask[b] >> a) & 1u) { sum += N[o + 1 + a]; ++nl; maxn = N[o + 1 + a] > maxn ? N[o + 1 + a] : maxn; }
      else CHECK(N[o + 1 + a] == 0 && pi[(size_t)b * A + a] == 0.0, "A %d tree %d: an illegal root child was touched", A, b);
      CHECK(((mask[b] >> a) & 1u) == (uint32_t)legal[(size_t)b * A + a], "A %d tree %d: the legal mask", A, b);
    }
    CHECK(sum == sims, "A %d tree %d: the root's children were visited %ld times", A, b, sum);
    CHECK(action[b] >= 0 && ((mask[b] >> action[b]) & 1u) && N[o + 1 + action[b]] == maxn, "A %d tree %d: action %d", A, b, action[b]);
    double ps = 0.0;
    for (int a = 0; a < A; ++a) ps += pi[(size_t)b * A + a];
    CHECK(fabs(ps - 1.0) < 1e-12, "A %d tree %d: pi' sums to %.17g", A, b, ps);
    mz_gz_seq(considered < nl ? considered : nl, sims, seq.data());
    std::vector<int> visits(A, 0);
    for (int s = 0; s < sims; ++s) {
      const size_t i = (size_t)b * sims + s;
      const int32_t *pa = paths.data() + i * PL;
      CHECK(plens[i] >= 2 && plens[i] <= PL && pa[0] == 0, "A %d tree %d sim %d: path length %d", A, b, s, plens[i]);
      const int ra = pa[1] - 1;
      CHECK(ra >= 0 && ra < A && ((mask[b] >> ra) & 1u), "A %d tree %d sim %d: root action %d", A, b, s, ra);
      CHECK(visits[ra] == seq[s], "A %d tree %d sim %d: root action %d had %d visits, seq says %d", A, b, s, ra, visits[ra], seq[s]);
      visits[ra] += 1;
      const int leaf = pa[plens[i] - 1];
      CHECK(leaf == 1 + ss[i] * A + sa[i] && E[o + leaf] == s + 1, "A %d tree %d sim %d: the leaf", A, b, s);
    }
  }
  return n;
}

int main() {
  int trees = 0;
  trees += run_shape(9, true, true, 100, 16, 16, 1.0);       // TicTacToe shapes
  trees += run_shape(9, true, true, 100, 30, 4, 0.0);
  trees += run_shape(7, true, true, 100, 30, 16, 1.0);       // Connect Four shapes
  trees += run_shape(7, true, true, 50, 5, 3, 1.0);          // fewer simulations than actions
  trees += run_shape(4, false, false, 100, 16, 16, 1.0);     // one player, no known bounds
  trees += run_shape(4, false, false, 50, 50, 2, 0.0);
  trees += run_shape(32, false, false, 50, 40, 16, 1.0);     // the widest node the engine takes
  trees += run_shape(1, false, true, 50, 8, 16, 1.0);        // a single action
  printf("ok %d\n", trees);
  return 0;
}
