/* Rank groups of the stand-in collective library (tests/rccl_shim): who belongs to a communicator, the host barrier
 * between its ranks, and the abort flag.  Plain C with pthreads and no HIP in it, so that a CPU program can drive it
 * (tests/c/shim_group_sanitize.c).
 *
 * All ranks are threads of one process.  A rank joins the group named by the 128-byte id and is held until all
 * `nranks` have joined.  Every barrier carries a tag (the communicator's sequence number and the phase inside the
 * collective); ranks that meet with different tags have lost step with each other and the group aborts.  Every wait is
 * timed: when the cap runs out the group aborts, and an aborted group makes every pending and later call return at
 * once with an error.  Leaving never waits; a group whose member has left fails the barriers of those who stay.
 */
#ifndef NB_TEST_SHIM_GROUP_H
#define NB_TEST_SHIM_GROUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHIM_MAX_RANKS 16
#define SHIM_ID_BYTES 128
#define SHIM_SLOT_WORDS 4

enum { SHIM_OK = 0, SHIM_ABORTED = 1, SHIM_TIMEOUT = 2, SHIM_MISMATCH = 3, SHIM_INVALID = 4, SHIM_NOMEM = 5, SHIM_DEPARTED = 6 };

typedef struct shim_group shim_group;

/* Blocks until `nranks` ranks have joined the group of `id` (or the cap runs out / the group aborts). */
int shim_group_join(const unsigned char id[SHIM_ID_BYTES], int nranks, int rank, shim_group** out);
/* All ranks meet here with the same tag.  SHIM_OK, or why this rank may not go on. */
int shim_group_barrier(shim_group* g, int rank, uint64_t tag);
void shim_group_abort(shim_group* g);
int shim_group_aborted(shim_group* g);
/* Never waits.  The last rank to leave frees the group (after on_free, if one was set). */
void shim_group_leave(shim_group* g, int rank);
/* SHIM_SLOT_WORDS pointers per rank: written by their owner before a barrier, read by the others after it. */
void** shim_group_slot(shim_group* g, int rank);
/* Called once, by whichever rank leaves last, before the group's memory goes. */
void shim_group_on_free(shim_group* g, void (*fn)(shim_group*));
/* The cap of every timed wait, 30 s unless changed. */
void shim_set_cap_ms(long ms);
/* Aborts every live group: what a test driver calls when one of its rank threads has died. */
void shim_abort_all(void);
/* Number of groups alive (leak check of the CPU test). */
int shim_live_groups(void);

#ifdef __cplusplus
}
#endif
#endif
