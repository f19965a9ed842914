/* See shim_group.h.  Lock order: the registry's mutex, then a group's. */
#define _POSIX_C_SOURCE 200809L
#include "shim_group.h"

#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

struct shim_group {
    unsigned char id[SHIM_ID_BYTES];
    int nranks;
    int joined, left;
    int open;                       /* still takes joiners */
    int present[SHIM_MAX_RANKS];
    int aborted;
    uint64_t gen;                   /* barriers passed */
    int arrived;
    uint64_t tag;                   /* of the barrier being filled: the first arrival's */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    void* slot[SHIM_MAX_RANKS][SHIM_SLOT_WORDS];
    void (*on_free)(shim_group*);
    shim_group* next;
};

static pthread_mutex_t g_reg = PTHREAD_MUTEX_INITIALIZER;
static shim_group* g_all = NULL;
static long g_cap_ms = 30000;       /* guarded by g_reg */

void shim_set_cap_ms(long ms)
{
    pthread_mutex_lock(&g_reg);
    g_cap_ms = ms > 0 ? ms : 1;
    pthread_mutex_unlock(&g_reg);
}

static struct timespec deadline_from_now(void)
{
    struct timespec t;
    long ms;
    pthread_mutex_lock(&g_reg);
    ms = g_cap_ms;
    pthread_mutex_unlock(&g_reg);
    clock_gettime(CLOCK_MONOTONIC, &t);
    t.tv_sec += ms / 1000;
    t.tv_nsec += (ms % 1000) * 1000000L;
    if (t.tv_nsec >= 1000000000L) { t.tv_sec += 1; t.tv_nsec -= 1000000000L; }
    return t;
}

static shim_group* group_new(const unsigned char* id, int nranks)
{
    shim_group* g = (shim_group*)calloc(1, sizeof *g);
    pthread_condattr_t ca;
    if (!g) return NULL;
    memcpy(g->id, id, SHIM_ID_BYTES);
    g->nranks = nranks;
    g->open = 1;
    pthread_mutex_init(&g->mu, NULL);
    pthread_condattr_init(&ca);
    pthread_condattr_setclock(&ca, CLOCK_MONOTONIC);
    pthread_cond_init(&g->cv, &ca);
    pthread_condattr_destroy(&ca);
    return g;
}

static void group_free(shim_group* g)
{
    shim_group** p;
    pthread_mutex_lock(&g_reg);
    for (p = &g_all; *p; p = &(*p)->next)
        if (*p == g) { *p = g->next; break; }
    pthread_mutex_unlock(&g_reg);
    if (g->on_free) g->on_free(g);
    pthread_cond_destroy(&g->cv);
    pthread_mutex_destroy(&g->mu);
    free(g);
}

int shim_group_join(const unsigned char id[SHIM_ID_BYTES], int nranks, int rank, shim_group** out)
{
    shim_group* g;
    struct timespec until;
    int rc = SHIM_OK;
    if (out) *out = NULL;
    if (!id || !out || nranks < 1 || nranks > SHIM_MAX_RANKS || rank < 0 || rank >= nranks) return SHIM_INVALID;
    until = deadline_from_now();
    pthread_mutex_lock(&g_reg);
    for (g = g_all; g; g = g->next) {
        int fits;
        pthread_mutex_lock(&g->mu);
        fits = g->open && g->nranks == nranks && !g->present[rank] && memcmp(g->id, id, SHIM_ID_BYTES) == 0;
        if (fits) break;            /* keeps g->mu */
        pthread_mutex_unlock(&g->mu);
    }
    if (!g) {
        g = group_new(id, nranks);
        if (!g) { pthread_mutex_unlock(&g_reg); return SHIM_NOMEM; }
        g->next = g_all;
        g_all = g;
        pthread_mutex_lock(&g->mu);
    }
    g->present[rank] = 1;
    if (++g->joined == nranks) { g->open = 0; pthread_cond_broadcast(&g->cv); }
    pthread_mutex_unlock(&g_reg);
    while (g->open && !g->aborted) {
        if (pthread_cond_timedwait(&g->cv, &g->mu, &until) == ETIMEDOUT && g->open && !g->aborted) {
            g->aborted = 1;
            rc = SHIM_TIMEOUT;
            pthread_cond_broadcast(&g->cv);
        }
    }
    if (rc == SHIM_OK && g->aborted) rc = SHIM_ABORTED;
    if (rc != SHIM_OK) g->open = 0;         /* nobody else may join what has failed */
    pthread_mutex_unlock(&g->mu);
    if (rc != SHIM_OK) { shim_group_leave(g, rank); return rc; }
    *out = g;
    return SHIM_OK;
}

int shim_group_barrier(shim_group* g, int rank, uint64_t tag)
{
    struct timespec until;
    uint64_t mine;
    int rc = SHIM_OK;
    if (!g || rank < 0 || rank >= g->nranks) return SHIM_INVALID;
    until = deadline_from_now();
    pthread_mutex_lock(&g->mu);
    if (g->aborted) { pthread_mutex_unlock(&g->mu); return SHIM_ABORTED; }
    if (g->left) { g->aborted = 1; pthread_cond_broadcast(&g->cv); pthread_mutex_unlock(&g->mu); return SHIM_DEPARTED; }
    if (g->arrived == 0) g->tag = tag;
    else if (g->tag != tag) { g->aborted = 1; pthread_cond_broadcast(&g->cv); pthread_mutex_unlock(&g->mu); return SHIM_MISMATCH; }
    if (++g->arrived == g->nranks) {
        g->arrived = 0;
        ++g->gen;
        pthread_cond_broadcast(&g->cv);
        pthread_mutex_unlock(&g->mu);
        return SHIM_OK;
    }
    mine = g->gen;
    while (g->gen == mine && !g->aborted) {
        if (pthread_cond_timedwait(&g->cv, &g->mu, &until) == ETIMEDOUT && g->gen == mine && !g->aborted) {
            g->aborted = 1;
            rc = SHIM_TIMEOUT;
            pthread_cond_broadcast(&g->cv);
        }
    }
    if (rc == SHIM_OK && g->gen == mine) rc = SHIM_ABORTED;     /* a barrier that did fill counts as passed */
    pthread_mutex_unlock(&g->mu);
    return rc;
}

void shim_group_abort(shim_group* g)
{
    if (!g) return;
    pthread_mutex_lock(&g->mu);
    g->aborted = 1;
    pthread_cond_broadcast(&g->cv);
    pthread_mutex_unlock(&g->mu);
}

int shim_group_aborted(shim_group* g)
{
    int a;
    if (!g) return 1;
    pthread_mutex_lock(&g->mu);
    a = g->aborted;
    pthread_mutex_unlock(&g->mu);
    return a;
}

void shim_group_leave(shim_group* g, int rank)
{
    int last;
    if (!g || rank < 0 || rank >= g->nranks) return;
    pthread_mutex_lock(&g->mu);
    ++g->left;
    if (g->arrived) { g->aborted = 1; }     /* someone waits in a barrier this rank will never reach */
    pthread_cond_broadcast(&g->cv);
    last = !g->open && g->left == g->joined;
    pthread_mutex_unlock(&g->mu);
    if (last) group_free(g);
}

void** shim_group_slot(shim_group* g, int rank)
{
    return (g && rank >= 0 && rank < g->nranks) ? g->slot[rank] : NULL;
}

void shim_group_on_free(shim_group* g, void (*fn)(shim_group*))
{
    if (!g) return;
    pthread_mutex_lock(&g->mu);
    g->on_free = fn;
    pthread_mutex_unlock(&g->mu);
}

void shim_abort_all(void)
{
    shim_group* g;
    pthread_mutex_lock(&g_reg);
    for (g = g_all; g; g = g->next) {
        pthread_mutex_lock(&g->mu);
        g->aborted = 1;
        pthread_cond_broadcast(&g->cv);
        pthread_mutex_unlock(&g->mu);
    }
    pthread_mutex_unlock(&g_reg);
}

int shim_live_groups(void)
{
    shim_group* g;
    int k = 0;
    pthread_mutex_lock(&g_reg);
    for (g = g_all; g; g = g->next) ++k;
    pthread_mutex_unlock(&g_reg);
    return k;
}
