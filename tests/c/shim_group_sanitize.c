/* The rank groups of the stand-in collective library (tests/rccl_shim/shim_group.c) under a sanitizer, on the CPU:
 * 2, 3 and 4 threads through a thousand matched barriers with a late joiner, then every way a group can break --
 * an abort, a rank that stops coming, ranks out of step, a rank that leaves, a join that never fills -- each of which
 * must send every other rank home with an error inside the cap and leave nobody waiting.
 * Built by tests/test_rccl_shim_cpu.py with -fsanitize=thread (or address,undefined). */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../rccl_shim/shim_group.h"

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

enum { ROUNDS = 500 };          /* two barriers each */
enum { PLAIN, ABORTS, STOPS, WRONG_TAG, LEAVES };

typedef struct {
    unsigned char id[SHIM_ID_BYTES];
    int nranks, rank, mode, late_ms;
    int join_rc, rounds_done, last_rc;
    double waited_ms;           /* in the call that failed */
} rank_arg;

static double now_ms(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec / 1e6;
}

static void nap_ms(int ms)
{
    struct timespec t = {ms / 1000, (ms % 1000) * 1000000L};
    nanosleep(&t, NULL);
}

/* One rank: publish the round number, barrier, read everybody's, barrier -- the shape of a collective of the library. */
static void* rank_main(void* p)
{
    rank_arg* a = (rank_arg*)p;
    shim_group* g = NULL;
    uint64_t seq = 0;
    const int breaks_at = 10;
    if (a->late_ms) nap_ms(a->late_ms);
    a->join_rc = shim_group_join(a->id, a->nranks, a->rank, &g);
    if (a->join_rc != SHIM_OK) return NULL;
    for (int k = 1; k <= ROUNDS; ++k) {
        const int me_breaks = a->rank == 0 && k == breaks_at;
        double t0;
        ++seq;
        if (me_breaks && a->mode == ABORTS) { shim_group_abort(g); break; }
        if (me_breaks && a->mode == STOPS) { nap_ms(600); break; }              /* longer than the cap of that case */
        if (me_breaks && a->mode == LEAVES) break;
        shim_group_slot(g, a->rank)[0] = (void*)(uintptr_t)k;
        t0 = now_ms();
        a->last_rc = shim_group_barrier(g, a->rank, ((seq + (me_breaks && a->mode == WRONG_TAG)) << 2) | 0u);
        a->waited_ms = now_ms() - t0;
        if (a->last_rc != SHIM_OK) break;
        for (int q = 0; q < a->nranks; ++q)
            CHECK((uintptr_t)shim_group_slot(g, q)[0] == (uintptr_t)k, "rank %d sees round %lu of rank %d in round %d", a->rank,
                  (unsigned long)(uintptr_t)shim_group_slot(g, q)[0], q, k);
        t0 = now_ms();
        a->last_rc = shim_group_barrier(g, a->rank, (seq << 2) | 1u);
        a->waited_ms = now_ms() - t0;
        if (a->last_rc != SHIM_OK) break;
        a->rounds_done = k;
    }
    shim_group_leave(g, a->rank);
    return NULL;
}

static void run_case(int nranks, int mode, long cap_ms, const char* what)
{
    static unsigned serial = 0;
    pthread_t th[SHIM_MAX_RANKS];
    rank_arg arg[SHIM_MAX_RANKS];
    const double t0 = now_ms();
    shim_set_cap_ms(cap_ms);
    ++serial;
    for (int r = 0; r < nranks; ++r) {
        memset(&arg[r], 0, sizeof arg[r]);
        memcpy(arg[r].id, &serial, sizeof serial);
        arg[r].nranks = nranks; arg[r].rank = r; arg[r].mode = mode;
        arg[r].late_ms = r == nranks - 1 ? 50 : 0;                                /* the late joiner */
        CHECK(pthread_create(&th[r], NULL, rank_main, &arg[r]) == 0, "pthread_create");
    }
    for (int r = 0; r < nranks; ++r) pthread_join(th[r], NULL);                  /* returns at all: nobody is left waiting */
    for (int r = 0; r < nranks; ++r) {
        CHECK(arg[r].join_rc == SHIM_OK, "%s: rank %d join %d", what, r, arg[r].join_rc);
        if (mode == PLAIN) {
            CHECK(arg[r].rounds_done == ROUNDS && arg[r].last_rc == SHIM_OK, "%s: rank %d did %d rounds, rc %d", what, r, arg[r].rounds_done, arg[r].last_rc);
        } else if (r != 0) {
            CHECK(arg[r].last_rc != SHIM_OK, "%s: rank %d was not told", what, r);
            CHECK(arg[r].rounds_done == 9, "%s: rank %d did %d rounds", what, r, arg[r].rounds_done);
            CHECK(arg[r].waited_ms < cap_ms + 250.0, "%s: rank %d waited %.0f ms (cap %ld)", what, r, arg[r].waited_ms, cap_ms);
            if (mode != STOPS) CHECK(arg[r].waited_ms < 250.0, "%s: rank %d sat out %.0f ms", what, r, arg[r].waited_ms);
        }
    }
    CHECK(shim_live_groups() == 0, "%s: %d groups leaked", what, shim_live_groups());
    printf("ok %-28s %d ranks  %.0f ms\n", what, nranks, now_ms() - t0);
}

/* a group that never fills: the one rank that came goes home with an error when the cap runs out */
static void lonely_join(void)
{
    unsigned char id[SHIM_ID_BYTES];
    shim_group* g = NULL;
    double t0;
    memset(id, 0xab, sizeof id);
    shim_set_cap_ms(200);
    t0 = now_ms();
    CHECK(shim_group_join(id, 2, 1, &g) == SHIM_TIMEOUT && g == NULL, "a lonely join must time out");
    CHECK(now_ms() - t0 < 450.0, "a lonely join took %.0f ms", now_ms() - t0);
    CHECK(shim_live_groups() == 0, "the lonely group leaked");
    CHECK(shim_group_join(id, 0, 0, &g) == SHIM_INVALID && shim_group_join(id, 2, 2, &g) == SHIM_INVALID, "bad arguments");
    CHECK(shim_group_join(id, 1, 0, &g) == SHIM_OK && g, "a group of one");
    CHECK(shim_group_barrier(g, 0, 4) == SHIM_OK && !shim_group_aborted(g), "a barrier of one");
    shim_abort_all();
    CHECK(shim_group_aborted(g) && shim_group_barrier(g, 0, 8) == SHIM_ABORTED, "abort_all reaches a complete group");
    shim_group_leave(g, 0);
    CHECK(shim_live_groups() == 0, "the group of one leaked");
    printf("ok joins that cannot fill, a group of one\n");
}

int main(void)
{
    for (int n = 2; n <= 4; ++n) run_case(n, PLAIN, 30000, "matched barriers");
    for (int n = 2; n <= 4; ++n) {
        run_case(n, ABORTS, 30000, "a rank aborts");
        run_case(n, WRONG_TAG, 30000, "a rank out of step");
        run_case(n, LEAVES, 30000, "a rank leaves");
        run_case(n, STOPS, 300, "a rank stops coming");
    }
    lonely_join();
    printf("ok shim groups under the sanitizer\n");
    return 0;
}
