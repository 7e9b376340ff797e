// mz_record.h -- accessors of the experience record (include/mz_record.h states the layout; nothing else spells its
// offsets).  Plain C++ for the host replay (g++, mz_replay.cpp) and the host tests, __host__ __device__ under hipcc for the
// kernels that write and read records.  Everything is forced inline: the whole-moves search kernels end a move with these
// stores inside a register budget that has no room for a call (tests/test_abi.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mz_record.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MZ_REC_FN __host__ __device__ __forceinline__
#else
#define MZ_REC_FN static inline __attribute__((always_inline))
#endif

// a record's slots as integer words.  The slots are declared float and the words alias them: the host compilers are told so;
// device code keeps the plain types its writers always used (may_alias changes the search kernels' code)
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t mz_rec_u32;
typedef int32_t mz_rec_i32;
#else
typedef uint32_t __attribute__((may_alias)) mz_rec_u32;
typedef int32_t __attribute__((may_alias)) mz_rec_i32;
#endif

// record (move, b) of a ring of ring_moves moves of B records: ring [ring_moves][B][rec_floats], a move's slot is move % ring_moves
MZ_REC_FN float *mz_rec_slot(float *ring, unsigned long long move, int ring_moves, int B, int b, int rec_floats) {
  return ring + ((size_t)(move % (unsigned long long)ring_moves) * B + b) * rec_floats;
}
// the tail of a record whose observation takes OS slots (MZ_REC_OBS_SLOTS)
MZ_REC_FN float *mz_rec_tail(float *rec, int OS, int A) { return rec + OS + A; }
MZ_REC_FN const float *mz_rec_tail(const float *rec, int OS, int A) { return rec + OS + A; }

// a float64 in two slots (4-byte aligned), as two 32-bit words, low word first
MZ_REC_FN void mz_rec_put_double(float *dst, double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  ((mz_rec_u32 *)dst)[0] = (uint32_t)u; ((mz_rec_u32 *)dst)[1] = (uint32_t)(u >> 32);
}
MZ_REC_FN double mz_rec_get_double(const float *src) {
  const mz_rec_u32 *w = (const mz_rec_u32 *)src;
  return __builtin_bit_cast(double, (unsigned long long)w[0] | (unsigned long long)w[1] << 32);
}
MZ_REC_FN void mz_rec_put_int(float *tail, int slot, int32_t v) { ((mz_rec_i32 *)tail)[slot] = v; }
MZ_REC_FN int32_t mz_rec_get_int(const float *tail, int slot) { return ((const mz_rec_i32 *)tail)[slot]; }

// The tail of the record rec, whose observation takes OS slots.  A macro, not a function: every argument is evaluated where
// it is stored, in slot order.  The whole-moves search kernels end a move with exactly these stores -- the synthetic
// environment draws its reward between them -- and a function, which evaluates all its arguments first, moves that work
// ahead of the stores and changes the schedule of kernels that are held to their code byte for byte.  (For the same
// reason the reward's slot is indexed from the record and the others from the tail, as the device writers always had it.)
#define mz_rec_put_tail(rec, OS, A, root_value, error, reward, action, flags, step, env_id, episode) do { \
    float *const mz_tail_ = mz_rec_tail((rec), (OS), (A));                                                  \
    mz_rec_put_double(mz_tail_ + MZ_REC_ROOT_VALUE, (root_value));                                          \
    mz_rec_put_double(mz_tail_ + MZ_REC_ERROR, (error));                                                    \
    (rec)[(OS) + (A) + MZ_REC_REWARD] = (reward);                                                           \
    mz_rec_put_int(mz_tail_, MZ_REC_ACTION, (action)); mz_rec_put_int(mz_tail_, MZ_REC_FLAGS, (flags));     \
    mz_rec_put_int(mz_tail_, MZ_REC_STEP, (step)); mz_rec_put_int(mz_tail_, MZ_REC_ENV_ID, (env_id));       \
    mz_rec_put_int(mz_tail_, MZ_REC_EPISODE, (episode));                                                    \
  } while (0)
MZ_REC_FN double mz_rec_root_value(const float *tail) { return mz_rec_get_double(tail + MZ_REC_ROOT_VALUE); }
MZ_REC_FN double mz_rec_error(const float *tail) { return mz_rec_get_double(tail + MZ_REC_ERROR); }
MZ_REC_FN float mz_rec_reward(const float *tail) { return tail[MZ_REC_REWARD]; }
MZ_REC_FN int32_t mz_rec_action(const float *tail) { return mz_rec_get_int(tail, MZ_REC_ACTION); }
MZ_REC_FN int32_t mz_rec_flags(const float *tail) { return mz_rec_get_int(tail, MZ_REC_FLAGS); }
MZ_REC_FN int32_t mz_rec_step(const float *tail) { return mz_rec_get_int(tail, MZ_REC_STEP); }
MZ_REC_FN int32_t mz_rec_env_id(const float *tail) { return mz_rec_get_int(tail, MZ_REC_ENV_ID); }
MZ_REC_FN int32_t mz_rec_episode(const float *tail) { return mz_rec_get_int(tail, MZ_REC_EPISODE); }
