// record_host.cpp -- the experience record's accessors (csrc/mz_record.h over include/mz_record.h) in a stand-alone host program,
// built with AddressSanitizer + UBSan by tests/test_record_cpu.py.  For every shape (O, packed, A) it writes rows into a small
// ring through mz_rec_slot / mz_rec_put_tail, reads them back through the getters, and prints what went in and the row's 32-bit
// words as they lie in memory; the Python test decodes the words with the offsets written out there.  The ring is allocated to
// the byte, so a store past a record is the sanitizer's.
//
// output: one line per row,  "row O packed A | flags action step env_id episode reward rv err | obs.. | visits.. | words.."  (hex; obs
// as float words, or as bytes when packed), then "ok <rows>".
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mz_record.h"

#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t fbits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t dbits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static double dfrom(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }

int main() {
  const int Os[] = {1, 3, 4, 5, 9, 128}, As[] = {2, 7, 18};
  // 0.0, -0.0, a denormal, 1e300, a NaN with a payload
  const uint64_t vals[] = {dbits(0.0), dbits(-0.0), 5ull, dbits(1e300), 0x7ff8dead0000beefull};
  const int ring_moves = 4, B = 3;
  long rows = 0;
  for (int O : Os)
    for (int packed = 0; packed <= 1; ++packed)
      for (int A : As) {
        const int OS = MZ_REC_OBS_SLOTS(O, packed), R = MZ_REC_FLOATS(O, A, packed);
        std::vector<float> ring((size_t)ring_moves * B * R, 0.f);
        int r = 0;
        for (int flags = 0; flags < 4; ++flags)
          for (int v = 0; v < 5; ++v, ++r) {
            const unsigned long long move = (1ull << 33) + 5ull * r + 1;      // (past 2^32: the slot is move % ring_moves in 64 bits)
            const int b = r % B;
            float *rec = mz_rec_slot(ring.data(), move, ring_moves, B, b, R);
            CHECK(rec == ring.data() + ((size_t)(move % 4) * 3 + b) * R, "slot of move %llu, b %d", move, b);
            for (int k = 0; k < R; ++k) rec[k] = -7.f;      // (every word of the row is written below)
            const double rv = dfrom(vals[v]), err = dfrom(vals[(v + flags + 1) % 5]);
            const float reward = (r & 1) ? -0.0f : 0.25f * r - 1.f;
            const int32_t action = r % 3 == 0 ? INT32_MAX : r % A, step = r % 4 == 1 ? 0 : 1000 * r;
            const int32_t env_id = r % 2 ? 2147483647 : r, episode = r % 5 == 2 ? INT32_MAX : r;
            printf("row %d %d %d | %x %x %x %x %x %08x %016llx %016llx |", O, packed, A, flags, action, step, env_id, episode, fbits(reward),
                   (unsigned long long)dbits(rv), (unsigned long long)dbits(err));
            for (int k = 0; k < O; ++k) {
              if (packed) { const uint8_t by = (uint8_t)(37 * k + 11 * r + 200); ((uint8_t *)rec)[k] = by; printf(" %02x", by); }
              else { rec[k] = 0.5f * k - 3.f + r; printf(" %08x", fbits(rec[k])); }
            }
            if (packed) for (int k = O; k < 4 * OS; ++k) ((uint8_t *)rec)[k] = 0;
            printf(" |");
            for (int a = 0; a < A; ++a) { rec[OS + a] = (float)(a + 1) / (float)(A + r + 1); printf(" %08x", fbits(rec[OS + a])); }
            mz_rec_put_tail(rec, OS, A, rv, err, reward, action, flags, step, env_id, episode);
            const float *tail = mz_rec_tail((const float *)rec, OS, A);
            CHECK(tail == rec + OS + A && tail + MZ_REC_EXTRA == rec + R, "tail");
            CHECK(dbits(mz_rec_root_value(tail)) == dbits(rv) && dbits(mz_rec_error(tail)) == dbits(err), "float64 round trip, row %d", r);
            CHECK(fbits(mz_rec_reward(tail)) == fbits(reward) && mz_rec_action(tail) == action && mz_rec_flags(tail) == flags &&
                  mz_rec_step(tail) == step && mz_rec_env_id(tail) == env_id && mz_rec_episode(tail) == episode, "getters, row %d", r);
            CHECK(!(mz_rec_flags(tail) & MZ_REC_FLAG_DONE) == !(flags & 1) && !(mz_rec_flags(tail) & MZ_REC_FLAG_P2) == !(flags & 2), "flag bits");
            printf(" |");
            for (int k = 0; k < R; ++k) { uint32_t w; memcpy(&w, rec + k, 4); printf(" %08x", w); }
            printf("\n");
            ++rows;
          }
      }
  printf("ok %ld\n", rows);
  return 0;
}
