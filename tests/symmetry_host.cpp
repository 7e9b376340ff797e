// symmetry_host.cpp -- the per-element bodies of csrc/mz_symmetry.hip.h (the draw, the tables, sym_element) compiled for the
// HOST and run over 300 random batches per kind.  A stand-alone program (tests/test_symmetry_cpu.py builds it with the host
// pass of hipcc and -fsanitize=address,undefined, runs it, and compares the digests it prints with the library's
// mz_fcl_symmetry_host on the same batches).  No GPU is touched.  Every array is a heap block of exactly its size, so a cell,
// an action or a policy entry read or written outside its batch is an AddressSanitizer report.
//
// The program also holds every image to the DEFINITION, through the forward permutations only (the kernel gathers through the
// inverse tables): obs'[p_g(c)] = obs[c], actions'[k] = a_g(actions[k]), policies'[k][a_g(a)] = policies[k][a].
//
// Batch n = 0 .. 599 (kind 1 for n < 300, then kind 3): its generator starts from SEED0 + n * STEP, so that the test can make
// any batch again by itself; batch size 1 + (7 n) % 48, K = 1 + n % 7, int32 actions for odd n, update = n, seed SEED.  Some
// actions are no actions of the game (-1, A): they stay what they are.
// Output: one line per batch, "n kind batch K i32 digest"; digest = sum of word[i] * (i + 1) over the 32-bit words of obs',
// actions', policies' and the elements, modulo 2^64.  The last line is "ok <batches>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mz_symmetry.hip.h"

static const uint64_t SEED = 6, SEED0 = 0x9E3779B97F4A7C15ull, STEP = 0xD1B54A32D192ED03ull;
static const int PER_KIND = 300;

static uint64_t g_state;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static uint64_t digest(uint64_t h, uint64_t *at, const void *p, size_t bytes) {
  const unsigned char *q = (const unsigned char *)p;
  for (size_t i = 0; i + 4 <= bytes; i += 4) {
    uint32_t w;
    memcpy(&w, q + i, 4);
    h += (uint64_t)w * ++*at;
  }
  return h;
}

// p_g(c) by the definition's words, not by a table
static int forward_cell(int kind, int g, int cell) {
  if (kind == 1) {
    int r = cell / 3, c = cell % 3;
    for (int q = 0; q < (g & 3); ++q) { const int t = r; r = c; c = 2 - t; }
    if (g >> 2) c = 2 - c;
    return 3 * r + c;
  }
  return 7 * (cell / 7) + (g ? 6 - cell % 7 : cell % 7);
}
static int forward_action(int kind, int g, int a) { return kind == 1 ? forward_cell(1, g, a) : (g ? 6 - a : a); }

int main() {
  int n = 0;
  for (int kind = 1; kind <= 3; kind += 2) {
    const int O = sym_cells(kind), A = sym_actions(kind);
    for (int i = 0; i < PER_KIND; ++i, ++n) {
      g_state = SEED0 + (uint64_t)n * STEP;
      const int bs = 1 + (7 * n) % 48, K = 1 + n % 7, i32 = n & 1, PA = (K + 1) * A;
      const size_t n_obs = (size_t)bs * O, n_act = (size_t)bs * K, n_pol = (size_t)bs * PA, aw = i32 ? 4 : 8;
      float *obs = (float *)malloc(n_obs * 4), *obs_out = (float *)malloc(n_obs * 4);
      float *pol = (float *)malloc(n_pol * 4), *pol_out = (float *)malloc(n_pol * 4);
      unsigned char *act = (unsigned char *)malloc(n_act * aw), *act_out = (unsigned char *)malloc(n_act * aw);
      int32_t *el = (int32_t *)malloc((size_t)bs * 4);
      if (!obs || !obs_out || !pol || !pol_out || !act || !act_out || !el) return 2;
      for (size_t j = 0; j < n_obs; ++j) obs[j] = (float)((int)(rnd() % 3u) - 1);
      for (size_t j = 0; j < n_act; ++j) {
        const uint32_t r = rnd();
        const int64_t a = (r >> 28) == 0 ? -1 : ((r >> 28) == 1 ? A : (int64_t)(r % (uint32_t)A));
        if (i32) { const int32_t v = (int32_t)a; memcpy(act + j * 4, &v, 4); }
        else memcpy(act + j * 8, &a, 8);
      }
      for (size_t j = 0; j < n_pol; ++j) pol[j] = (float)(rnd() >> 8) * (1.0f / 16777216.0f);
      SymBatch b = {obs, act, pol, obs_out, act_out, pol_out, el, SEED, (uint32_t)n, kind, bs, K, i32};
      const size_t total = sym_total(b);
      if (total != n_obs + n_act + n_pol) { printf("MISMATCH sym_total: batch %d\n", n); return 1; }
      for (size_t t = total; t-- > 0;) sym_element(b, t);      // (any order: an element depends on its own index only)
      for (int s = 0; s < bs; ++s) {
        const int g = el[s];
        if (g < 0 || g >= sym_elements(kind) || g != sym_draw(kind, SEED, (uint32_t)n, (uint32_t)s)) { printf("MISMATCH element: batch %d sample %d\n", n, s); return 1; }
        for (int c = 0; c < O; ++c)
          if (memcmp(&obs_out[(size_t)s * O + forward_cell(kind, g, c)], &obs[(size_t)s * O + c], 4)) { printf("MISMATCH obs: batch %d sample %d cell %d\n", n, s, c); return 1; }
        for (int k = 0; k < K; ++k) {
          int64_t a, a2;
          if (i32) { int32_t v, v2; memcpy(&v, act + ((size_t)s * K + k) * 4, 4); memcpy(&v2, act_out + ((size_t)s * K + k) * 4, 4); a = v; a2 = v2; }
          else { memcpy(&a, act + ((size_t)s * K + k) * 8, 8); memcpy(&a2, act_out + ((size_t)s * K + k) * 8, 8); }
          const int64_t want = (a < 0 || a >= A) ? a : (int64_t)forward_action(kind, g, (int)a);
          if (a2 != want) { printf("MISMATCH action: batch %d sample %d step %d\n", n, s, k); return 1; }
        }
        for (int k = 0; k <= K; ++k)
          for (int a = 0; a < A; ++a)
            if (memcmp(&pol_out[(size_t)s * PA + (size_t)k * A + forward_action(kind, g, a)], &pol[(size_t)s * PA + (size_t)k * A + a], 4)) {
              printf("MISMATCH policy: batch %d sample %d position %d action %d\n", n, s, k, a);
              return 1;
            }
      }
      uint64_t at = 0, h = 0;
      h = digest(h, &at, obs_out, n_obs * 4);
      h = digest(h, &at, act_out, n_act * aw);
      h = digest(h, &at, pol_out, n_pol * 4);
      h = digest(h, &at, el, (size_t)bs * 4);
      printf("%d %d %d %d %d %llu\n", n, kind, bs, K, i32, (unsigned long long)h);
      free(obs); free(obs_out); free(pol); free(pol_out); free(act); free(act_out); free(el);
    }
  }
  printf("ok %d\n", n);
  return 0;
}
