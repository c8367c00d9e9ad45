/*
 * rfec_rx_pool.h -- the receiver session's replay threads (rfec_rx_pool.c):
 * workers beside the calling thread, woken per batch (a generation counter; a
 * short spin, then a condition variable).  Host only: no GPU runtime.
 */
#ifndef RFEC_RX_POOL_H
#define RFEC_RX_POOL_H

#include <pthread.h>
#include <stdint.h>

#include "rfec_rx_sim.h" /* RX_MAX_THREADS */

#pragma GCC visibility push(hidden)

typedef struct rx_pool rx_pool;
typedef struct {
    rx_pool* pool;
    uint32_t idx;
} rx_worker;
struct rx_pool {
    pthread_t th[RX_MAX_THREADS];
    rx_worker w[RX_MAX_THREADS];
    uint32_t nth; /* workers started */
    uint32_t base; /* the first worker's index: 1 (the caller runs fn(arg, 0)) or 0 (workers run every index) */
    pthread_mutex_t mu;
    pthread_cond_t go, fin;
    uint32_t gen, done; /* atomics */
    int stop;           /* atomic */
    double spin_us;     /* how long a worker (or the caller) spins before sleeping on the condition variable:
                           RFEC_RX_SPIN_US, default 50 us, read by pool_start (spinning threads share the
                           process's CPU quota and cores with the caller's serial work) */
    void (*fn)(void*, uint32_t);
    void* arg;
};

int pool_start(rx_pool* P, uint32_t workers, uint32_t base);
void pool_stop(rx_pool* P);
/* fn(arg, 0) here (base 1) and fn(arg, i) on the workers; returns when all are done */
void pool_run(rx_pool* P, void (*fn)(void*, uint32_t), void* arg);

#pragma GCC visibility pop

#endif
