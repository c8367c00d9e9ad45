/*
 * rfec_rx_pool.c -- the receiver session's replay threads and their CPU
 * placement.  Host only: no GPU runtime.
 */
#define _GNU_SOURCE /* sched_getcpu, CPU_SET, pthread_attr_setaffinity_np: the replay threads' placement */
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "rfec_rx_pool.h"

static void cpu_relax(void)
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

static int pool_stopping(const rx_pool* P) { return __atomic_load_n(&P->stop, __ATOMIC_ACQUIRE); }

static void* pool_main(void* p)
{
    rx_worker* W = (rx_worker*)p;
    rx_pool* P = W->pool;
    uint32_t seen = 0;
    for (;;) {
        const double t0 = now_us();
        for (uint32_t i = 0; __atomic_load_n(&P->gen, __ATOMIC_ACQUIRE) == seen && !pool_stopping(P); ++i) {
            cpu_relax();
            if ((i & 63) == 63 && now_us() - t0 > P->spin_us) {
                pthread_mutex_lock(&P->mu);
                while (__atomic_load_n(&P->gen, __ATOMIC_ACQUIRE) == seen && !pool_stopping(P))
                    pthread_cond_wait(&P->go, &P->mu);
                pthread_mutex_unlock(&P->mu);
            }
        }
        if (pool_stopping(P))
            return NULL;
        seen = __atomic_load_n(&P->gen, __ATOMIC_ACQUIRE);
        P->fn(P->arg, W->idx);
        if (__atomic_add_fetch(&P->done, 1u, __ATOMIC_ACQ_REL) == P->nth) {
            pthread_mutex_lock(&P->mu);
            pthread_cond_broadcast(&P->fin);
            pthread_mutex_unlock(&P->mu);
        }
    }
}

/* The CPUs the replay threads run on: RFEC_RX_CPUS ("a-b,c,..."), else those
 * sharing the last-level cache with the creating thread's CPU (one CCD of an
 * EPYC: the records, the shards and the device tables pass between the
 * threads through that L3; across CCDs every such line is a fabric round
 * trip, and the replay ran slower in parallel than alone), within the
 * process's affinity.  RFEC_RX_PIN=0: no placement.  0 when nothing applies. */
static int parse_cpus(const char* s, cpu_set_t* set)
{
    CPU_ZERO(set);
    int n = 0;
    while (s && *s) {
        char* e;
        long a = strtol(s, &e, 10), b = a;
        if (e == s)
            break;
        if (*e == '-')
            b = strtol(e + 1, &e, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c, ++n)
            CPU_SET((int)c, set);
        s = *e == ',' ? e + 1 : e;
        if (*s == '\n')
            break;
    }
    return n;
}

static int rx_worker_cpus(cpu_set_t* set)
{
    const char* pin = getenv("RFEC_RX_PIN");
    if (pin && pin[0] == '0')
        return 0;
    const char* cpus = getenv("RFEC_RX_CPUS");
    if (cpus)
        return parse_cpus(cpus, set) > 0;
    const int cpu = sched_getcpu();
    if (cpu < 0)
        return 0;
    char path[96], buf[512];
    snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
    FILE* f = fopen(path, "r");
    if (!f)
        return 0;
    const int ok = fgets(buf, sizeof(buf), f) != NULL;
    fclose(f);
    if (!ok || parse_cpus(buf, set) < 2)
        return 0;
    cpu_set_t mine;
    if (pthread_getaffinity_np(pthread_self(), sizeof(mine), &mine))
        return 0;
    CPU_AND(set, set, &mine);
    return CPU_COUNT(set) >= 2;
}

int pool_start(rx_pool* P, uint32_t workers, uint32_t base)
{
    memset(P, 0, sizeof(*P));
    P->base = base;
    const char* spin = getenv("RFEC_RX_SPIN_US");
    P->spin_us = spin ? atof(spin) : 50.0;
    pthread_mutex_init(&P->mu, NULL);
    pthread_cond_init(&P->go, NULL);
    pthread_cond_init(&P->fin, NULL);
    cpu_set_t cpus;
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    /* one CPU per worker, in the set's order (a CCD's physical cores come first in its list), so a shard's
       state stays in one core's L2 from batch to batch; the set as a whole if it has fewer CPUs */
    int list[CPU_SETSIZE], ncpu = 0;
    const int pinned = rx_worker_cpus(&cpus);
    for (int c = 0; pinned && c < CPU_SETSIZE; ++c)
        if (CPU_ISSET(c, &cpus))
            list[ncpu++] = c;
    for (uint32_t i = 0; i < workers; ++i) {
        if (pinned) {
            cpu_set_t one;
            CPU_ZERO(&one);
            if ((uint32_t)ncpu >= workers + P->base)
                CPU_SET(list[i + P->base], &one);
            else
                one = cpus;
            pthread_attr_setaffinity_np(&attr, sizeof(one), &one);
        }
        P->w[i] = (rx_worker){P, i + P->base};
        if (pthread_create(&P->th[i], &attr, pool_main, &P->w[i])) {
            pthread_attr_destroy(&attr);
            return -1;
        }
        P->nth = i + 1;
    }
    pthread_attr_destroy(&attr);
    return 0;
}

void pool_stop(rx_pool* P)
{
    pthread_mutex_lock(&P->mu);
    __atomic_store_n(&P->stop, 1, __ATOMIC_RELEASE);
    pthread_cond_broadcast(&P->go);
    pthread_mutex_unlock(&P->mu);
    for (uint32_t i = 0; i < P->nth; ++i)
        pthread_join(P->th[i], NULL);
    pthread_mutex_destroy(&P->mu);
    pthread_cond_destroy(&P->go);
    pthread_cond_destroy(&P->fin);
    P->nth = 0;
}

void pool_run(rx_pool* P, void (*fn)(void*, uint32_t), void* arg)
{
    P->fn = fn;
    P->arg = arg;
    __atomic_store_n(&P->done, 0u, __ATOMIC_RELEASE);
    pthread_mutex_lock(&P->mu);
    __atomic_add_fetch(&P->gen, 1u, __ATOMIC_ACQ_REL);
    pthread_cond_broadcast(&P->go);
    pthread_mutex_unlock(&P->mu);
    if (P->base)
        fn(arg, 0);
    const double t0 = now_us();
    for (uint32_t i = 0; __atomic_load_n(&P->done, __ATOMIC_ACQUIRE) < P->nth; ++i) {
        cpu_relax();
        if ((i & 63) == 63 && now_us() - t0 > P->spin_us) {
            pthread_mutex_lock(&P->mu);
            while (__atomic_load_n(&P->done, __ATOMIC_ACQUIRE) < P->nth)
                pthread_cond_wait(&P->fin, &P->mu);
            pthread_mutex_unlock(&P->mu);
        }
    }
}
