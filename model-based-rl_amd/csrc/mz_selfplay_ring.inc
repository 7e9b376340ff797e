// mz_selfplay_ring.inc -- the bookkeeping of the self-play loop's experience ring: how many moves it holds, which slot a move's
// records take, what a drain copies, and which drain's copy the compute stream has to wait for before it writes again.
// Pure host code over the standard library, no HIP header: an event is an opaque token and a stream an opaque pointer here
// (mz_selfplay_abi.inc makes the HIP calls), so that tests/selfplay_ring_host.cpp can hold every rule to a brute-force model
// without a GPU.
#pragma once
#include <stddef.h>
#include <deque>
#include <utility>
#include <vector>

#define MZ_GRAPH_MOVES 16    // most self-play moves of one launch: a hipGraph of them (3 kernel nodes per move), or whole moves in one kernel

// what one drain copies: `moves` moves as `runs` contiguous runs of slots, in move order
struct RingDrain {
  int moves, runs;
  struct { int slot, moves; } run[2];      // (a drain never exceeds the capacity: it wraps at most once)
  void *chain;                             // token the drain's stream waits for first, or null
};

// mz_selfplay_steps_into's ring of R slots whose origin lies `back_bytes` before the caller's buffer
struct DirectOrigin { int R; unsigned long long back_bytes; };

struct RecordRing {
  int capacity = 0;                                     // moves the ring holds
  unsigned long long produced = 0, drained = 0;         // moves played / moves handed to a drain (or stored directly), as the devices' counters count
  // every drain whose copy may still be reading the ring: (first move it does not cover, its token), oldest first.  Drains
  // complete in this order: one issued on another stream than the one before it is chained behind it.
  std::deque<std::pair<unsigned long long, void *>> q;
  unsigned long long q_start = 0;                       // first move q.front() covers
  std::vector<void *> pool;                             // tokens no drain in q uses
  void *latest_stream = nullptr;                        // stream of q.back()

  // 128 MiB of records, at least two launches' worth of moves -- so that a drain on a copy stream and the next chunk's moves
  // use different slots (where they cannot, order_behind_drains) -- and at most 256
  static int capacity_for(size_t bytes_per_move) {
    const size_t moves = ((size_t)128 << 20) / bytes_per_move;
    return (int)(moves < 2 * MZ_GRAPH_MOVES ? 2 * MZ_GRAPH_MOVES : (moves > 256 ? 256 : moves));
  }
  int slot(unsigned long long move) const { return (int)(move % (unsigned long long)capacity); }
  unsigned long long undrained() const { return produced - drained; }
  // do `moves` (>= 0) more moves fit beside the undrained ones?
  bool fits(int moves) const { return (unsigned long long)moves <= (unsigned long long)capacity - undrained(); }
  void *latest() const { return q.empty() ? nullptr : q.back().second; }

  // The slots the coming `moves` moves write may still be the source of a drain's copy on another stream: the token the compute
  // stream must wait for first, or null -- that of the OLDEST queued drain that reaches the moves below produced + moves - capacity,
  // whose slots are lost (it covers every earlier drain).  Waiting for the latest drain instead exposed a whole chunk's copy every
  // time the ring wrapped: with 16-move chunks of 2.4 MB records (Pong-ram shapes, a 53-move ring) every third launch stood
  // behind the copy of the chunk just before it -- 272 us per launch, 2.2 % of the loop.  The drains waited for leave the
  // queue; their tokens are free again (re-recorded only by a later drain, i.e. after the caller has enqueued this wait).
  void *order_behind_drains(int moves) {
    const unsigned long long end = produced + (unsigned long long)moves;
    void *wait_for = nullptr;
    while (!q.empty() && q_start + (unsigned long long)capacity < end) {
      wait_for = q.front().second;
      q_start = q.front().first;
      pool.push_back(wait_for);
      q.pop_front();
    }
    return wait_for;
  }

  // a drain of up to max_moves moves issued on `stream`; the drain that follows another stream's is chained behind it, so that
  // the newest token covers every copy issued so far
  RingDrain plan_drain(int max_moves, void *stream) const {
    RingDrain d = {};
    d.chain = latest_stream != stream ? latest() : nullptr;
    d.moves = (int)(undrained() < (unsigned long long)max_moves ? undrained() : (unsigned long long)max_moves);
    if (d.moves > 0) {
      const int first = slot(drained), head = d.moves < capacity - first ? d.moves : capacity - first;
      d.run[d.runs++] = {first, head};
      if (head < d.moves) d.run[d.runs++] = {0, d.moves - head};
    }
    return d;
  }
  // a free token for the drain's copies, or null: the caller makes a new one
  void *take_token() {
    if (pool.empty()) return nullptr;
    void *t = pool.back();
    pool.pop_back();
    return t;
  }
  // The planned drain of moves > 0 moves is enqueued on `stream` with `token` recorded behind its copies.  `drained` advances
  // at that point, not when the copy has run: the slots are reusable only once order_behind_drains has handed out the token.
  void note_drain(int moves, void *token, void *stream) {
    if (q.empty()) q_start = drained;
    drained += (unsigned long long)moves;
    q.emplace_back(drained, token);
    latest_stream = stream;
  }

  // The ring is empty and no copy reads it any more (the caller has waited for latest(), or for the device): both counters
  // continue at `at`, every queued token is free.
  void forget(unsigned long long at) {
    for (auto &d : q) pool.push_back(d.second);
    q.clear();
    produced = drained = at;
  }

  // mz_selfplay_steps_into without touching the kernels: they keep computing slot = move % ring_moves, and the host hands them a
  // "ring" of ~2^30 slots whose origin lies (first_move % R) slots BEFORE the caller's buffer, so that the k <= MZ_GRAPH_MOVES
  // moves from first_move on land in its slots 0 .. k-1.  R is 2^30, or 2^30 - 4096 where the k moves would wrap 2^30 (both
  // would wrap only in the 16 moves below a multiple of 2^30 (2^18 - 1), a count no run reaches).
  static DirectOrigin direct_origin(unsigned long long first_move, int k, size_t bytes_per_move) {
    unsigned long long R = 1ull << 30;
    if (first_move % R + (unsigned long long)k > R) R -= 4096;
    return {(int)R, first_move % R * (unsigned long long)bytes_per_move};
  }
};

// A producing call that fails AFTER a launch of it was attempted leaves the device's move counters ahead of `produced`: the
// next call's direct origin would disagree with the kernels' slot and a direct launch would write records outside the caller's
// pinned buffer.  Such a state is not resumed: the self-play state is marked not ready -- every later call fails with "call
// mz_selfplay_reset first".  `attempted` is advanced where a launch is issued (one that returns an error counts), `ok` set at the end.
struct ProduceGuard {
  bool &ready;
  int attempted = 0;
  bool ok = false;
  ~ProduceGuard() { if (!ok && attempted > 0) ready = false; }
};
