// selfplay_ring_host.cpp -- RecordRing (csrc/mz_selfplay_ring.inc), the bookkeeping of the self-play loop's experience ring, compiled
// into a stand-alone program.  tests/test_selfplay_ring_cpu.py builds it with the host compiler under AddressSanitizer + UBSan and
// runs it.  No GPU is touched, no clock is read, the pseudo-random sequences come from a fixed seed.
//
// Ordering: sequences of produce(k), drain(n, stream) and forget are run through the struct and through a model that has no queue --
// per slot it keeps which outstanding drains still read it, and it knows that drains complete in issue order (the struct chains
// them: checked).  Before every produce the token to wait for must be that of the newest outstanding drain reading a slot about
// to be written -- no older one (a read would be overtaken), no newer one (the launch would stand behind a copy it does not need).
// Drain runs, the room predicate against both of its earlier formulas, the direct origin, the capacity rule and the failed-call guard
// are checked exhaustively over their small domains.  Output: "ok <cases>"; a disagreement prints "MISMATCH ..." and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "mz_selfplay_ring.inc"
#include "../include/mz_record.h"      // MZ_REC_FLOATS: the record's width

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static const int CAPS[4] = {32, 33, 53, 256};
static long cases = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {      // (xorshift64*)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

// ---- ordering
struct Model {
  int cap;
  unsigned long long produced = 0, drained = 0;
  std::vector<std::vector<int>> readers;      // per slot: the outstanding drains (by issue number) whose copy reads it
  std::vector<void *> token;                  // per drain issued
  int completed = 0;                          // drains below this number are known complete (issue order)
  void *last_stream = nullptr;
  size_t most_outstanding = 0;
  explicit Model(int c) : cap(c), readers(c) {}
  int outstanding() const { return (int)token.size() - completed; }
  bool in_use(void *t) const { return std::find(token.begin() + completed, token.end(), t) != token.end(); }
  void complete_through(int d) {
    completed = d + 1;
    for (auto &r : readers) r.erase(std::remove_if(r.begin(), r.end(), [&](int x) { return x <= d; }), r.end());
  }
};

struct Harness {
  RecordRing ring;
  Model m;
  uintptr_t made = 0;      // tokens made so far; a token is its number
  explicit Harness(int cap) : m(cap) { ring.capacity = cap; }

  void agree(const char *after) {
    CHECK(ring.produced == m.produced && ring.drained == m.drained, "%s: counters %llu %llu, model %llu %llu", after, ring.produced,
          ring.drained, m.produced, m.drained);
    CHECK((int)ring.q.size() == m.outstanding(), "%s: %zu drains queued, %d outstanding", after, ring.q.size(), m.outstanding());
    CHECK(ring.latest() == (m.outstanding() ? m.token.back() : nullptr), "%s: the latest token", after);
    for (void *t : ring.pool) CHECK(!m.in_use(t), "%s: token %zu is in the pool and still queued", after, (size_t)(uintptr_t)t);
    CHECK(ring.pool.size() + ring.q.size() == made && made <= m.most_outstanding, "%s: %zu tokens made, at most %zu drains outstanding at once",
          after, (size_t)made, m.most_outstanding);
    ++cases;
  }
  void produce(int k) {
    CHECK(ring.fits(k), "produce(%d) does not fit: cap %d undrained %llu", k, m.cap, m.produced - m.drained);
    int newest = -1;      // the newest outstanding drain that reads a slot about to be written
    for (int i = 0; i < k; ++i)
      for (int d : m.readers[(m.produced + i) % m.cap]) newest = std::max(newest, d);
    void *got = ring.order_behind_drains(k);
    CHECK(got == (newest < 0 ? nullptr : m.token[newest]), "cap %d produced %llu k %d: waits for token %zu, the model for drain %d", m.cap,
          m.produced, k, (size_t)(uintptr_t)got, newest);
    if (newest >= 0) m.complete_through(newest);
    ring.produced += (unsigned long long)k;
    m.produced += k;
    agree("produce");
  }
  void drain(int n, void *stream) {
    const RingDrain d = ring.plan_drain(n, stream);
    const int want = (int)std::min<unsigned long long>(m.produced - m.drained, (unsigned long long)n);
    CHECK(d.moves == want, "drain(%d) takes %d moves, the model %d", n, d.moves, want);
    CHECK(d.chain == (m.outstanding() && stream != m.last_stream ? m.token.back() : nullptr), "drain on %s stream: chain token %zu",
          stream != m.last_stream ? "another" : "the same", (size_t)(uintptr_t)d.chain);
    int i = 0;
    for (int r = 0; r < d.runs; ++r)
      for (int j = 0; j < d.run[r].moves; ++j, ++i)
        CHECK(d.run[r].slot + j == (int)((m.drained + i) % m.cap), "drain(%d): run %d slot %d", n, r, d.run[r].slot + j);
    CHECK(i == want && d.runs <= 2, "drain(%d): runs cover %d moves", n, i);
    if (!want) return;
    void *t = ring.take_token();
    if (t) CHECK(!m.in_use(t), "token %zu taken from the pool is still queued", (size_t)(uintptr_t)t);
    else t = (void *)(++made);
    ring.note_drain(want, t, stream);
    for (int j = 0; j < want; ++j) m.readers[(m.drained + j) % m.cap].push_back((int)m.token.size());
    m.token.push_back(t);
    m.drained += want;
    m.last_stream = stream;
    m.most_outstanding = std::max(m.most_outstanding, (size_t)m.outstanding());
    agree("drain");
  }
  void forget(unsigned long long at) {
    ring.forget(at);
    if (!m.token.empty()) m.complete_through((int)m.token.size() - 1);
    m.produced = m.drained = at;
    CHECK(ring.q.empty() && ring.latest() == nullptr, "forget leaves a drain queued");
    agree("forget");
  }
};

static void ordering(int cap) {
  static int other;
  void *streams[2] = {nullptr, &other};      // (the default stream is a null pointer)
  // scripted: chunks of every size drained at once on one, then on alternating streams; chunks that do not divide the ring
  for (int nstreams = 1; nstreams <= 2; ++nstreams)
    for (int k = 1; k <= cap; ++k) {
      Harness h(cap);
      for (int i = 0; i < 7; ++i) {
        h.produce(k);
        h.drain(k, streams[i % nstreams]);
      }
      h.forget(0);
      h.produce(k);
    }
  // scripted: several small drains outstanding when a large produce comes
  for (int nstreams = 1; nstreams <= 2; ++nstreams) {
    Harness h(cap);
    for (int round = 0; round < 6; ++round) {
      h.produce(cap - (int)(h.ring.undrained()));
      for (int i = 0; h.ring.undrained(); ++i) h.drain(1 + (i + round) % 5, streams[i % nstreams]);
      h.produce(3 + round);
    }
  }
  // pseudo-random, the counters starting where their low words wrap
  const unsigned long long bases[4] = {0, (1ull << 30) - 7, (1ull << 32) - 9, (1ull << 40) + 3};
  for (int seq = 0; seq < 48; ++seq) {
    Harness h(cap);
    const int nstreams = 1 + seq % 2;
    h.forget(bases[seq % 4]);
    for (int op = 0; op < 300; ++op) {
      const uint32_t what = rnd(100);
      const int room = cap - (int)h.ring.undrained();
      if (what < 45 && room > 0) h.produce(rnd(4) == 0 ? room : 1 + (int)rnd((uint32_t)(room < 20 ? room : 20)));
      else if (what < 97) h.drain(1 + (int)rnd((uint32_t)(rnd(3) ? 20 : cap + 3)), streams[rnd((uint32_t)nstreams)]);
      else h.forget(h.ring.undrained() ? 0 : bases[rnd(4)]);      // (mz_selfplay_reset at any time, mz_selfplay_set_moves on an empty ring)
    }
  }
}

// ---- drain runs: every (drained % capacity, n)
static void drain_runs(int cap) {
  for (int at = 0; at < cap; ++at)
    for (int n = 0; n <= cap; ++n)
      for (int extra = 0; extra <= 1; ++extra) {      // asked for exactly n of more, or for more than the n there are
        RecordRing r;
        r.capacity = cap;
        r.drained = 5ull * cap + at;
        r.produced = r.drained + (extra ? n : cap);
        const RingDrain d = r.plan_drain(extra ? n + 1 + at : n, nullptr);
        CHECK(d.moves == n && d.runs <= 2 && (d.runs > 0) == (n > 0) && d.chain == nullptr, "cap %d at %d n %d: %d moves in %d runs", cap, at, n, d.moves, d.runs);
        int covered = 0;
        for (int i = 0; i < d.runs; ++i) {
          CHECK(d.run[i].moves > 0 && d.run[i].slot >= 0 && d.run[i].slot + d.run[i].moves <= cap, "cap %d at %d n %d: run %d leaves the ring", cap, at, n, i);
          CHECK(d.run[i].slot == (at + covered) % cap && d.run[i].slot == r.slot(r.drained + covered), "cap %d at %d n %d: run %d starts at slot %d", cap, at, n, i, d.run[i].slot);
          covered += d.run[i].moves;
        }
        CHECK(covered == n, "cap %d at %d n %d: runs cover %d", cap, at, n, covered);
        ++cases;
      }
}

// ---- room: the one predicate against the two formulas it replaces
static void room(int cap) {
  for (unsigned long long base : {0ull, (1ull << 32) - 3, (1ull << 40) + 1})
    for (int undrained = 0; undrained <= cap; ++undrained)
      for (int moves = 0; moves <= cap + 40; ++moves) {
        RecordRing r;
        r.capacity = cap;
        r.drained = base;
        r.produced = base + undrained;
        const unsigned long long moves_host = r.produced, drained = r.drained;
        const int ring_moves = cap;
        const bool refused_steps = moves_host + moves - drained > (unsigned long long)ring_moves;                       // mz_selfplay_steps
        const bool refused_timed = (unsigned long long)moves > (unsigned long long)ring_moves - (moves_host - drained);   // _steps_timed, _phase_profile
        CHECK(r.fits(moves) == !refused_steps && r.fits(moves) == !refused_timed, "cap %d undrained %d moves %d: fits %d, the formulas refuse %d %d", cap,
              undrained, moves, (int)r.fits(moves), (int)refused_steps, (int)refused_timed);
        ++cases;
      }
}

// ---- direct origin
static void direct_origin() {
  const unsigned long long R0 = 1ull << 30, R1 = R0 - 4096;
  std::vector<unsigned long long> first;
  for (unsigned long long m = 0; m <= 40; ++m) first.push_back(m);
  auto window = [&](unsigned long long c) { for (unsigned long long m = c - 4136; m <= c + 40; ++m) first.push_back(m); };
  for (unsigned long long c : {R0, 1ull << 31, 1ull << 32, 1ull << 40}) window(c);
  // (multiples up to the largest count above, 2^40; both moduli would wrap only just below a multiple of 2^30 (2^18 - 1) ~ 2^48)
  for (unsigned long long j : {1ull, 2ull, 3ull, 5ull, 1023ull, 1024ull}) window(j * R1);
  const unsigned long long dst = 1ull << 46;      // the buffer's address, as an integer
  for (size_t bytes : {(size_t)16 * 22 * 4, (size_t)4096 * 22 * 4, (size_t)130 * 47 * 4 + 4})      // (the last: no multiple of 16 bytes)
    for (unsigned long long f : first)
      for (int k = 1; k <= MZ_GRAPH_MOVES; ++k) {
        const DirectOrigin o = RecordRing::direct_origin(f, k, bytes);
        const unsigned long long R = (unsigned long long)o.R;
        CHECK((R == R0 || R == R1) && f % R + (unsigned long long)k <= R, "first_move %llu k %d: R %llu wraps", f, k, R);
        const unsigned long long origin = dst - o.back_bytes;
        for (int i = 0; i < k; ++i)
          CHECK(origin + (f + i) % R * bytes == dst + (unsigned long long)i * bytes, "first_move %llu k %d bytes %zu: move %d misses its slot", f, k, bytes, i);
        ++cases;
      }
}

static void capacity() {
  CHECK(RecordRing::capacity_for((size_t)2100 * MZ_REC_FLOATS(4000, 3, 0) * 4) == 32, "capacity of B 2100, O 4000, A 3");
  CHECK(RecordRing::capacity_for((size_t)16 * MZ_REC_FLOATS(8, 4, 0) * 4) == 256, "capacity of B 16, O 8, A 4");
  CHECK(RecordRing::capacity_for((size_t)4096 * MZ_REC_FLOATS(8, 4, 0) * 4) == 256, "capacity of B 4096, O 8, A 4");
  CHECK(RecordRing::capacity_for((size_t)4096 * MZ_REC_FLOATS(128, 6, 0) * 4) == 56, "capacity of B 4096, O 128, A 6");      // (128 MiB / 2 359 296 bytes)
  CHECK(RecordRing::capacity_for((size_t)1 << 40) == 2 * MZ_GRAPH_MOVES, "the least capacity");
  cases += 5;
}

static void guard() {
  for (int attempted = 0; attempted <= 2; ++attempted)
    for (int ok = 0; ok <= 1; ++ok) {
      bool ready = true;
      {
        ProduceGuard g{ready};
        g.attempted += attempted;
        g.ok = ok != 0;
      }
      CHECK(ready == (ok || attempted == 0), "guard: %d launches attempted, ok %d, ready %d", attempted, ok, (int)ready);
      ++cases;
    }
}

int main() {
  for (int cap : CAPS) {
    ordering(cap);
    drain_runs(cap);
    room(cap);
  }
  direct_origin();
  capacity();
  guard();
  printf("ok %ld\n", cases);
  return 0;
}
