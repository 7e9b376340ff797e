/*
 * mz_record.h -- the experience record of one self-play move: the ONE statement of its layout.
 *
 * A record is what Game.apply / store_search_statistics append to History for one move (game.py:79-115), as float32
 * slots.  The device self-play loop writes it (mz_selfplay_drain, mz_engine.h), the host replay keeps a history slice
 * as its records (mz_replay.h), Reanalyse reads and refreshes them, and model-based-rl_amd/record.py is the Python side.
 * Every one of them takes the numbers from here (C and C++: csrc/mz_record.h has the accessors; Python: record.py, held
 * to this file by tests/test_record_cpu.py).
 *
 *   obs           [MZ_REC_OBS_SLOTS(O, packed)]  the observation BEFORE the move, raw, as History keeps it (game.py:93-96):
 *                                  O float32, or -- packed byte observations -- O bytes, four per slot, low byte first
 *   child_visits  [A]              float32: the visit shares of the root's children (the Gumbel search: pi')
 *   tail          [MZ_REC_EXTRA]   from slot MZ_REC_OBS_SLOTS(O, packed) + A on, by the offsets below:
 *     root_value  float64 in two slots, low word first (the reference keeps root value and error as Python floats,
 *     error       float64 likewise      actors.py:147-148, game.py:112: priorities and value targets are its doubles)
 *     reward      float32
 *     action, flags, step, env_id, episode   int32 bit patterns; step is the game's step BEFORE the move;
 *                 flags: MZ_REC_FLAG_DONE the move ended the game, MZ_REC_FLAG_P2 the mover was player -1
 *                 (History.to_play, game.py:100-101; always clear for the single-player environments)
 */
#ifndef MZ_RECORD_H
#define MZ_RECORD_H

#define MZ_REC_ROOT_VALUE 0
#define MZ_REC_ERROR 2
#define MZ_REC_REWARD 4
#define MZ_REC_ACTION 5
#define MZ_REC_FLAGS 6
#define MZ_REC_STEP 7
#define MZ_REC_ENV_ID 8
#define MZ_REC_EPISODE 9
#define MZ_REC_EXTRA 10      /* slots of the tail */

#define MZ_REC_FLAG_DONE 1
#define MZ_REC_FLAG_P2 2

#define MZ_REC_OBS_SLOTS(O, packed) ((packed) ? ((O) + 3) / 4 : (O))
#define MZ_REC_FLOATS(O, A, packed) (MZ_REC_OBS_SLOTS(O, packed) + (A) + MZ_REC_EXTRA)      /* float32 slots of a record */

#endif /* MZ_RECORD_H */
