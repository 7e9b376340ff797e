// reanalyse_host.cpp -- the host side of MuZero Reanalyse as a stand-alone program (tests/test_reanalyse_cpu.py builds it with
// the host pass of hipcc and -fsanitize=address,undefined together with csrc/mz_replay.cpp, and runs it).  No GPU is touched.
//
//  1. mzr_reanalyse_pick / _write / _release on a replay fed with records, with one and with four ingest threads (deferred
//     insertion): a ticket held while the window evicts every picked leaf, then written or released; a partial eviction; a
//     second pick with a ticket outstanding; the handle destroyed with a ticket outstanding.  What the sanitizers watch is the
//     life time of the picked slices and the bounds of the row copies.
//  2. mz_reanalyse_legal_mask (csrc/mz_reanalyse.hip.h), compiled for the host, on the positions of the file named on the
//     command line: one per line, "kind mask n obs[0] .. obs[n-1]" with the mask of the host environment's legal_actions().
//
// Output: the last line is "ok <positions> masks".  Any disagreement prints "MISMATCH ..." and exits 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mz_engine.h"
#include "mz_replay.h"
#define MZ_MAX_ACTIONS_K MZ_MAX_ACTIONS      // (as mz_engine.hip sets it before the kernel headers)
#include "mz_reanalyse.hip.h"

static const int O = 9, A = 9, K = 5, TD = 3, W = 64, MH = 8, R = MZ_REC_FLOATS(O, A, 0), B = 6;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {      // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static double unit() { return (double)(rnd() >> 8) / 16777216.0; }

static int bad(const char *what, int threads) {
  printf("MISMATCH %s (ingest threads %d): %s\n", what, threads, mzr_last_error());
  return 1;
}

struct Feed {                // B environments' running step counters
  int step[B] = {};
  int episode[B] = {};
  std::vector<float> rec;
  const float *chunk(int moves, double p_done) {
    rec.assign((size_t)moves * B * R, 0.f);
    for (int m = 0; m < moves; ++m)
      for (int b = 0; b < B; ++b) {
        float *q = rec.data() + ((size_t)m * B + b) * R;
        for (int k = 0; k < O; ++k) q[k] = (float)((int)(rnd() % 3u) - 1);
        float sum = 0.f;
        for (int a = 0; a < A; ++a) { q[O + a] = (float)unit() + 0.01f; sum += q[O + a]; }
        for (int a = 0; a < A; ++a) q[O + a] /= sum;
        const double rv = 2.0 * unit() - 1.0, err = 2.0 * unit() - 1.0;
        const float reward = (float)(rnd() % 2u);
        const bool done = unit() < p_done;
        const int32_t action = (int32_t)(rnd() % (uint32_t)A);
        mz_rec_put_tail(q, O, A, rv, err, reward, action, (done ? MZ_REC_FLAG_DONE : 0) | ((step[b] & 1) ? MZ_REC_FLAG_P2 : 0), step[b], b,
                        episode[b]);
        if (done) { step[b] = 0; ++episode[b]; } else ++step[b];
      }
    return rec.data();
  }
};

static mz_replay *make(int threads) {
  mzr_config c;
  memset(&c, 0, sizeof c);
  c.window_size = W; c.window_step = W; c.obs_dim = O; c.action_space = A; c.num_unroll_steps = K; c.td_steps = TD;
  c.max_history_length = MH; c.batch_size = 16; c.epsilon = 0.01; c.alpha = 1.0; c.beta = 1.0; c.beta_increment_per_sampling = 0.001;
  c.discount = 0.997; c.two_players = 1; c.ingest_threads = threads;
  mz_replay *r = nullptr;
  return mzr_create(&c, &r) ? nullptr : r;
}

struct Picked {
  std::vector<float> rows;
  std::vector<int32_t> slice_rows;
  int64_t n = 0, slices = 0, skipped = 0;
  uint64_t ticket = 0;
};
// the buffers are exactly as large as the call is told: one row or one slice too many written is a heap overflow
static int64_t pick(mz_replay *r, int64_t max_rows, int64_t max_slices, Picked *p) {
  p->rows.assign((size_t)max_rows * R + (max_rows ? 0 : 1), -7.f);
  p->slice_rows.assign((size_t)max_slices, -1);
  p->n = mzr_reanalyse_pick(r, max_rows, p->rows.data(), p->slice_rows.data(), max_slices, &p->slices, &p->ticket, &p->skipped);
  return p->n;
}

static std::vector<float> fresh_rows(int64_t n) {
  std::vector<float> f((size_t)n * (A + 2));
  for (int64_t i = 0; i < n; ++i) {
    for (int a = 0; a < A; ++a) f[(size_t)i * (A + 2) + a] = (float)unit();
    const double v = 4.0 * unit() - 2.0;
    memcpy(&f[(size_t)i * (A + 2) + A], &v, 8);
  }
  return f;
}

static int sample_ok(mz_replay *r) {
  const int bs = 16;
  std::vector<double> draws(bs), pri(bs);
  const double total = mzr_total_priority(r);
  for (int i = 0; i < bs; ++i) draws[i] = total * (i + 0.5) / bs;
  std::vector<float> obs((size_t)bs * O), rew((size_t)bs * (K + 1)), val((size_t)bs * (K + 1)), pol((size_t)bs * (K + 1) * A);
  std::vector<int32_t> act((size_t)bs * K);
  std::vector<int64_t> idx(bs);
  return mzr_sample_batch(r, draws.data(), bs, obs.data(), act.data(), rew.data(), val.data(), pol.data(), idx.data(), pri.data());
}

static int drive(int threads) {
  mz_replay *r = make(threads);
  if (!r) return bad("create", threads);
  Feed feed;
  Picked p, q;
  if (pick(r, 100, 100, &p) != 0 || p.ticket != 0) return bad("an empty replay", threads);
  for (int c = 0; c < 2; ++c)
    if (mzr_ingest_records(r, feed.chunk(7, 0.12), 7, B, R)) return bad("ingest", threads);
  // (a) pick everything, evict everything, write: nothing is written, nothing dangles
  if (pick(r, 4096, 256, &p) <= 0 || !p.ticket) return bad("pick", threads);
  int64_t sum = 0;
  for (int64_t i = 0; i < p.slices; ++i) sum += p.slice_rows[(size_t)i];
  if (sum != p.n) return bad("slice_rows do not add up", threads);
  if (pick(r, 4096, 256, &q) != -2) return bad("a second pick with a ticket out must return -2", threads);
  for (int c = 0; c < 3; ++c)
    if (mzr_ingest_records(r, feed.chunk(7, 0.12), 7, B, R)) return bad("ingest", threads);
  std::vector<float> f = fresh_rows(p.n);
  double stats[3] = {-1, -1, -1};
  if (mzr_reanalyse_write(r, p.ticket, f.data(), p.n, stats) != 0 || stats[0] != 0.0) return bad("write after a full eviction", threads);
  if (mzr_reanalyse_write(r, p.ticket, f.data(), p.n, stats) >= 0) return bad("a ticket was written twice", threads);
  if (sample_ok(r)) return bad("sample", threads);
  // (b) the same with release
  if (pick(r, 4096, 256, &p) <= 0) return bad("pick", threads);
  for (int c = 0; c < 3; ++c)
    if (mzr_ingest_records(r, feed.chunk(7, 0.12), 7, B, R)) return bad("ingest", threads);
  if (mzr_reanalyse_release(r, p.ticket)) return bad("release", threads);
  if (mzr_reanalyse_release(r, p.ticket) == 0) return bad("a ticket was released twice", threads);
  // (c) a partial eviction, then a write: the surviving slices take their rows, and a later pick reads them back
  if (pick(r, 4096, 256, &p) <= 0) return bad("pick", threads);
  {      // 32 of the 64 leaves overwritten: a slice has at most 16 consecutive leaves, so one lost all of them and one kept some
    const std::vector<double> half(32, 0.5);
    if (mzr_tree_add(r, half.data(), 32, nullptr)) return bad("tree_add", threads);
  }
  f = fresh_rows(p.n);
  const int64_t wrote = mzr_reanalyse_write(r, p.ticket, f.data(), p.n - 1, stats);      // a wrong row count: refused, the ticket stays
  if (wrote >= 0) return bad("a wrong row count was accepted", threads);
  const int64_t w2 = mzr_reanalyse_write(r, p.ticket, f.data(), p.n, stats);
  if (w2 <= 0 || w2 >= p.n || stats[0] != (double)w2 || !(stats[1] > 0.0) || !(stats[2] > 0.0)) return bad("write after a partial eviction", threads);
  // (d) small passes round the ring with buffers of exactly the size named; the rows read back carry the written values
  int64_t matched = 0;
  for (int it = 0; it < 40; ++it) {
    const int64_t max_rows = 16 + (int64_t)(rnd() % 20u), max_slices = 1 + (int64_t)(rnd() % 3u);
    if (pick(r, max_rows, max_slices, &q) < 0) return bad("small pick", threads);
    if (q.n > max_rows || q.slices > max_slices) return bad("a pick exceeded its limits", threads);
    for (size_t i = (size_t)q.n * R; i < q.rows.size(); ++i)
      if (q.rows[i] != -7.f) return bad("rows beyond the picked ones were written", threads);
    for (int64_t i = 0; i < q.n; ++i)
      for (int64_t j = 0; j < p.n; ++j)
        if (!memcmp(&q.rows[(size_t)i * R + O], &f[(size_t)j * (A + 2)], (A + 2) * 4)) { ++matched; break; }
    if (q.ticket && (it % 2 ? mzr_reanalyse_release(r, q.ticket) : (mzr_reanalyse_write(r, q.ticket, &q.rows[O], 0, nullptr) >= 0)))
      return bad(it % 2 ? "release" : "a write of zero rows for a ticket with rows was accepted", threads);
    if (q.ticket && !(it % 2) && mzr_reanalyse_release(r, q.ticket)) return bad("release after a refused write", threads);
  }
  if (matched < w2) return bad("the written rows did not come back", threads);
  // (e) a slice longer than max_rows is skipped and counted
  if (pick(r, 0, 4, &q) != 0 || q.skipped < 1 || q.ticket) return bad("oversized slices", threads);
  // (f) the handle goes away with a ticket outstanding
  if (pick(r, 4096, 256, &p) <= 0) return bad("pick", threads);
  if (mzr_ingest_records(r, feed.chunk(7, 0.12), 7, B, R)) return bad("ingest", threads);
  mzr_destroy(r);
  return 0;
}

static int refuse_bytes() {
  mzr_config c;
  memset(&c, 0, sizeof c);
  c.window_size = W; c.window_step = W; c.obs_dim = 128; c.action_space = 6; c.num_unroll_steps = K; c.td_steps = TD;
  c.max_history_length = MH; c.batch_size = 16; c.epsilon = 0.01; c.alpha = 1.0; c.beta = 1.0; c.discount = 0.997; c.obs_u8 = 1;
  mz_replay *r = nullptr;
  if (mzr_create(&c, &r)) return bad("create", 0);
  Picked p;
  p.rows.assign(4096, 0.f); p.slice_rows.assign(4, 0);
  const int64_t n = mzr_reanalyse_pick(r, 4, p.rows.data(), p.slice_rows.data(), 4, &p.slices, &p.ticket, nullptr);
  const bool ok = n < 0 && strstr(mzr_last_error(), "byte observations");
  mzr_destroy(r);
  return ok ? 0 : bad("byte observations were not refused", 0);
}

static int masks(const char *path, long *count) {
  FILE *f = fopen(path, "r");
  if (!f) { printf("MISMATCH cannot open %s\n", path); return 1; }
  int kind, n;
  unsigned want;
  while (fscanf(f, "%d %u %d", &kind, &want, &n) == 3) {
    if (n < 1 || n > 64) { fclose(f); printf("MISMATCH bad line\n"); return 1; }
    std::vector<float> obs((size_t)n);      // exactly the observation: a read past it is a heap overflow
    for (int k = 0; k < n; ++k) { int v; if (fscanf(f, "%d", &v) != 1) { fclose(f); printf("MISMATCH bad line\n"); return 1; } obs[(size_t)k] = (float)v; }
    const int acts = kind == 1 ? 9 : 7;
    const uint32_t got = mz_reanalyse_legal_mask(kind, obs.data(), acts);
    if (got != want) { fclose(f); printf("MISMATCH legal mask: kind %d position %ld: %u, the environment says %u\n", kind, *count, got, want); return 1; }
    ++*count;
  }
  fclose(f);
  // kinds without a rule of their own: every action, at any action count up to the mask's width
  const float none[4] = {0.f, 1.f, -1.f, 0.f};
  for (int kind = 0; kind <= 2; kind += 2)
    for (int acts = 1; acts <= 32; ++acts)
      if (mz_reanalyse_legal_mask(kind, none, acts) != (acts == 32 ? 0xFFFFFFFFu : ((1u << acts) - 1u))) { printf("MISMATCH all-legal mask\n"); return 1; }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: reanalyse_host positions.txt\n"); return 2; }
  if (drive(1) || drive(4) || refuse_bytes()) return 1;
  long count = 0;
  if (masks(argv[1], &count)) return 1;
  printf("ok %ld masks\n", count);
  return 0;
}
