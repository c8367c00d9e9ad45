/*
 * rfec_rx_plane.c -- the receiver's host control plane over T shards: the
 * sharded replay of a batch (split, parallel or in-order replay, ownership
 * check, rollback, merge), evictions over the union of the shards, and the
 * host halves of compaction and of one call's device tables (the plan of the
 * delivering groups, the host peel of large groups, the table fill).
 */
#define _GNU_SOURCE /* posix_memalign */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rfec_rx_plane.h"

/* D->ev by packet id: an LSD radix sort of (packet id, position) keys, 4 x 8
 * bits, then one permutation (qsort's comparisons were ~20 % of the device
 * tables' host time at ~900 deliveries a batch); stable */
static int rx_sort_events(rx_dev* D)
{
    const uint32_t n = D->nev;
    uint64_t* k = (uint64_t*)malloc((size_t)n * 2 * sizeof(uint64_t));
    rx_event* tmp = (rx_event*)malloc((size_t)n * sizeof(rx_event));
    if (!k || !tmp) {
        free(k);
        free(tmp);
        return -1;
    }
    uint64_t* src = k;
    uint64_t* dst = k + n;
    for (uint32_t i = 0; i < n; ++i)
        src[i] = (uint64_t)D->ev[i].hdr.seq << 32 | i;
    for (uint32_t sh = 32; sh < 64; sh += 8) {
        uint32_t cnt[257] = {0};
        for (uint32_t i = 0; i < n; ++i)
            cnt[((src[i] >> sh) & 0xFFu) + 1]++;
        for (uint32_t b = 1; b <= 256; ++b)
            cnt[b] += cnt[b - 1];
        for (uint32_t i = 0; i < n; ++i)
            dst[cnt[(src[i] >> sh) & 0xFFu]++] = src[i];
        uint64_t* t = src;
        src = dst;
        dst = t;
    }
    for (uint32_t i = 0; i < n; ++i)
        tmp[i] = D->ev[(uint32_t)src[i]];
    memcpy(D->ev, tmp, (size_t)n * sizeof(rx_event));
    free(k);
    free(tmp);
    return 0;
}

void rx_dev_free(rx_dev* D)
{
    free(D->ev);
    free(D->dl);
    free(D->C);
    free(D->cls);
    free(D->jobs);
    free(D->jlevel);
    free(D->jmem);
    memset(D, 0, sizeof(*D));
}

/* A group recovered by line jobs (rx_line_jobs: above RFEC_MAX_K segments or a
 * huge shape -- a foreign peer's flex): the canonical
 * peel (lines in plan order -- rows, then columns -- to a fixpoint, with
 * flex_fec_recover's header checks, flex_fec_xor.c:60-99) from its arrived
 * members and registered parities, over headers on the host; each firing
 * becomes a line job the device runs (rfec_launch_line_jobs).  job_of[t]: the
 * job recovering member t, or -1.  Returns -1 when out of memory. */
static int rx_big_peel(const rx_sim* X, rx_dev* D, uint32_t gi, int32_t* job_of)
{
    const rx_inst* g = &X->G[gi];
    const rx_shape* sh = &X->S[g->shape];
    const uint32_t k = g->count, NL = sh->n_lines;
    rfec_hdr* hd = (rfec_hdr*)malloc((size_t)k * sizeof(rfec_hdr));
    int32_t* src = (int32_t*)malloc((size_t)k * sizeof(int32_t));
    uint16_t* lvl = (uint16_t*)malloc((size_t)k * sizeof(uint16_t));
    uint8_t* have = (uint8_t*)malloc(k);
    if (!hd || !src || !lvl || !have) {
        free(hd);
        free(src);
        free(lvl);
        free(have);
        return -1;
    }
    for (uint32_t i = 0; i < k; ++i) {
        job_of[i] = -1;
        lvl[i] = 0;
        src[i] = X->slot_src[g->slot0 + i];
        have[i] = src[i] >= 0; /* the peel starts from the arrived members */
        if (have[i])
            hd[i] = X->slot_hdr[g->slot0 + i];
    }
    for (int progress = 1; progress && !D->oom;) {
        progress = 0;
        for (uint32_t l = 0; l < NL && !D->oom; ++l) {
            uint32_t first, stride;
            int reg;
            const uint32_t n = rx_line(X, g, l, &first, &stride, &reg);
            if (!reg)
                continue;
            uint32_t miss = 0, present = 0, t = 0;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t i = first + q * stride;
                if (have[i]) {
                    present++;
                } else {
                    miss++;
                    t = i;
                }
            }
            if (miss != 1 || present == 0)
                continue;
            const rfec_wire_rec* f = &X->R[X->line_par[g->line0 + l]];
            const uint32_t L = f->data_size;
            if (L > X->capacity)
                continue;
            rfec_hdr h = f->hdr;
            int ok = 1;
            uint16_t level = 0;
            for (uint32_t q = 0; q < n && ok; ++q) {
                const uint32_t i = first + q * stride;
                if (i == t)
                    continue;
                const rfec_hdr* m = &hd[i];
                ok = m->size <= L;
                rx_hdr_xor(&h, m);
                level = lvl[i] > level ? lvl[i] : level;
            }
            if (!ok || h.size > L)
                continue;
            RX_GROW_F(D->oom, D->jobs, D->njobs, D->jobcap, 1, rfec_line_job);
            RX_GROW_F(D->oom, D->jlevel, D->njobs, D->jlevelcap, 1, uint16_t);
            RX_GROW_F(D->oom, D->jmem, D->njmem, D->jmemcap, present, int32_t);
            if (D->oom)
                break;
            rfec_line_job* J = &D->jobs[D->njobs];
            J->out = (int32_t)D->njobs;
            J->parity = X->line_par[g->line0 + l];
            J->member0 = D->njmem;
            J->n_members = present;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t i = first + q * stride;
                if (i != t)
                    D->jmem[D->njmem++] = src[i];
            }
            D->jlevel[D->njobs] = (uint16_t)(level + 1);
            job_of[t] = (int32_t)D->njobs;
            src[t] = -1 - (int32_t)D->njobs;
            lvl[t] = (uint16_t)(level + 1);
            hd[t] = h;
            have[t] = 1;
            D->njobs++;
            progress = 1;
        }
    }
    free(hd);
    free(src);
    free(lvl);
    free(have);
    return D->oom ? -1 : 0;
}

static int same_geometry(const rx_shape* a, const rx_shape* b)
{
    return a->count == b->count && a->row == b->row && a->col == b->col && a->xcol[0] == b->xcol[0] &&
           a->xcol[1] == b->xcol[1];
}

void rx_fill(const rx_tabs* A, uint32_t only)
{
    const rx_dev* D = A->D;
    for (uint32_t d = 0; d < D->ndl; ++d) {
        const uint32_t t = (uint32_t)(D->dl[d] >> 32);
        if (only != UINT32_MAX && t != only)
            continue;
        const rx_sim* X = A->XS[t];
        const rx_inst* g = &X->G[(uint32_t)D->dl[d]];
        const rx_shape* sh = &X->S[g->shape];
        if (rx_line_jobs(sh))
            continue;
        const rx_dclass* C = RX_CLASS(D, A->sbase, t, g);
        const uint32_t gg = C->group0 + g->gslot, r0 = C->row0 + g->gslot * sh->count;
        const uint32_t p0 = C->prow0 + g->gslot * sh->n_lines;
        A->pres[2 * gg] = g->arrived[0];
        A->pres[2 * gg + 1] = g->arrived[1];
        A->ppm[gg] = g->ppm;
        for (uint32_t i = 0; i < sh->count; ++i) {
            const int32_t src = X->slot_src[g->slot0 + i];
            A->map[r0 + i] = src;
            if (src >= 0)
                A->hh[r0 + i] = X->slot_hdr[g->slot0 + i];
            else
                memset(&A->hh[r0 + i], 0, sizeof(rfec_hdr));
        }
        for (uint32_t l = 0; l < sh->n_lines; ++l) {
            const int32_t src = X->line_par[g->line0 + l];
            A->map[A->r_par + p0 + l] = src;
            if (src >= 0) {
                A->mh[p0 + l] = X->R[src].hdr;
                A->fsz[p0 + l] = X->R[src].data_size;
            } else {
                memset(&A->mh[p0 + l], 0, sizeof(rfec_hdr));
                A->fsz[p0 + l] = 0;
            }
        }
    }
    for (uint32_t q = 0; q < D->nev; ++q) {
        const rx_event* ev = &D->ev[q];
        if (only != UINT32_MAX && ev->shard != only)
            continue;
        const rx_sim* X = A->XS[ev->shard];
        const rx_inst* g = &X->G[ev->inst];
        const rx_shape* sh = &X->S[g->shape];
        const uint32_t t = ev->hdr.seq - g->base;
        if (rx_line_jobs(sh)) { /* the job that recovers t */
            A->omap[q] = t < g->count && A->job_of[g->gslot + t] >= 0
                             ? (int32_t)(A->r_job + (uint32_t)A->job_of[g->gslot + t]) : -1;
            continue;
        }
        const rx_dclass* C = RX_CLASS(D, A->sbase, ev->shard, g);
        uint32_t e = UINT32_MAX;
        if (t < g->count && !((g->arrived[t >> 6] >> (t & 63)) & 1ull)) {
            const uint64_t lo = t >= 64 ? ~g->arrived[0] : ~g->arrived[0] & ((1ull << t) - 1);
            const uint64_t hi = t >= 64 ? ~g->arrived[1] & ((1ull << (t - 64)) - 1) : 0;
            e = (uint32_t)(__builtin_popcountll(lo) + __builtin_popcountll(hi));
        }
        A->omap[q] = e < C->E ? (int32_t)(A->r_dense + C->dense0 + g->gslot * C->E + e) : -1;
    }
}

void rx_fill_job(void* arg, uint32_t t) { rx_fill((const rx_tabs*)arg, t); }

/* The large groups' line jobs sorted by dependency level (stable; they are
 * launched level by level): member codes and job_of follow.  L->lvl_n and
 * L->maxlvl.  RFEC_OK or an error code (rfec_last_error set). */
static int rx_sort_jobs(rx_dev* D, rx_layout* L, int32_t* job_of, uint32_t nbig)
{
    for (uint32_t j = 0; j < D->njobs; ++j) {
        if (D->jlevel[j] > RX_MAX_LEVEL)
            return rfec_set_error(RFEC_EINVAL, "rx: line job chain too deep");
        L->maxlvl = D->jlevel[j] > L->maxlvl ? D->jlevel[j] : L->maxlvl;
        L->lvl_n[D->jlevel[j]]++;
    }
    uint32_t start[RX_MAX_LEVEL + 2] = {0};
    for (uint32_t v = 1; v <= L->maxlvl; ++v)
        start[v + 1] = start[v] + L->lvl_n[v];
    uint32_t* jperm = (uint32_t*)malloc((size_t)D->njobs * sizeof(uint32_t));
    rfec_line_job* sorted = (rfec_line_job*)malloc((size_t)D->njobs * sizeof(rfec_line_job));
    if (jperm && sorted) {
        for (uint32_t j = 0; j < D->njobs; ++j)
            jperm[j] = start[D->jlevel[j]]++;
        for (uint32_t j = 0; j < D->njobs; ++j) {
            sorted[jperm[j]] = D->jobs[j];
            sorted[jperm[j]].out = (int32_t)jperm[j];
        }
        memcpy(D->jobs, sorted, (size_t)D->njobs * sizeof(rfec_line_job));
        for (uint32_t m = 0; m < D->njmem; ++m)
            if (D->jmem[m] < 0)
                D->jmem[m] = -1 - (int32_t)jperm[-1 - D->jmem[m]];
        for (uint32_t i = 0; i < nbig; ++i)
            if (job_of[i] >= 0)
                job_of[i] = (int32_t)jperm[job_of[i]];
    }
    const int ok = jperm && sorted;
    free(jperm);
    free(sorted);
    return ok ? RFEC_OK : rfec_set_error(RFEC_ENOMEM, "rx: line jobs");
}

/* The host half of the device side of one call: the groups that delivered
 * something in this call (over the T shards XS), to be rebuilt on the device
 * from their arrived members and registered parities and peeled there. */
int rx_plan(rx_sim* const* XS, uint32_t T, rx_dev* D, uint32_t stride, rx_layout* L)
{
    memset(L, 0, sizeof(*L));
    D->nev = D->ndl = D->nc = D->njobs = D->njmem = 0;
    /* 1. the deliveries of every shard, ascending packet id */
    uint32_t total = 0, nshape = 0;
    for (uint32_t t = 0; t < T; ++t) {
        total += XS[t]->nout;
        nshape += XS[t]->ns;
    }
    if (total == 0) /* nothing recovered: no device work */
        return RFEC_OK;
    RX_GROW_F(D->oom, D->ev, 0, D->evcap, total, rx_event);
    RX_GROW_F(D->oom, D->cls, 0, D->clscap, nshape + 1, uint32_t);
    if (D->oom)
        return rfec_set_error(RFEC_ENOMEM, "rx: delivery list");
    uint32_t* sbase = L->sbase;
    for (uint32_t t = 0; t < T; ++t) {
        const rx_sim* X = XS[t];
        for (uint32_t q = 0; q < X->nout; ++q) {
            D->ev[D->nev] = X->out[q];
            D->ev[D->nev++].shard = t;
        }
        sbase[t + 1] = sbase[t] + X->ns;
    }
    if (D->nev > 1 && rx_sort_events(D)) /* ascending packet id (each shard's list is in its arrival order) */
        return rfec_set_error(RFEC_ENOMEM, "rx: delivery list");
    memset(D->cls, 0, (size_t)nshape * sizeof(uint32_t));
    /* 2. delivering groups, by device shape (work proportional to the deliveries, not to the open flexes) */
    for (uint32_t t = 0; t < T; ++t) {
        rx_sim* X = XS[t];
        if (++X->epoch == 0) { /* wrapped: no instance may carry a stale stamp */
            for (uint32_t gi = 0; gi < X->ng; ++gi)
                X->G[gi].gstamp = 0;
            X->epoch = 1;
        }
    }
    for (uint32_t q = 0; q < D->nev; ++q) {
        rx_sim* X = XS[D->ev[q].shard];
        rx_inst* g = &X->G[D->ev[q].inst];
        if (g->gstamp == X->epoch)
            continue;
        g->gstamp = X->epoch;
        RX_GROW_F(D->oom, D->dl, D->ndl, D->dlcap, 1, uint64_t);
        if (D->oom)
            return rfec_set_error(RFEC_ENOMEM, "rx: delivery list");
        D->dl[D->ndl++] = (uint64_t)D->ev[q].shard << 32 | D->ev[q].inst;
        uint32_t* c = &D->cls[sbase[D->ev[q].shard] + g->shape];
        if (!*c) { /* this shard's shape: an existing device shape of the same geometry, or a new one */
            const rx_shape* sh = &X->S[g->shape];
            uint32_t k = 0;
            while (k < D->nc && !same_geometry(D->C[k].sh, sh))
                ++k;
            if (k == D->nc) {
                RX_GROW_F(D->oom, D->C, D->nc, D->ccap, 1, rx_dclass);
                if (D->oom)
                    return rfec_set_error(RFEC_ENOMEM, "rx: device shapes");
                D->C[D->nc++] = (rx_dclass){sh, 0, 0, 0, 0, 0, 0};
            }
            *c = k + 1;
        }
        g->gslot = D->C[*c - 1].n_groups++;
    }
    for (uint32_t k = 0; k < D->nc; ++k) {
        rx_dclass* C = &D->C[k];
        C->row0 = L->nrows;
        C->prow0 = L->prows;
        C->group0 = L->ngs;
        if (rx_line_jobs(C->sh)) /* line jobs instead (below) */
            continue;
        L->nrows += C->n_groups * C->sh->count;
        L->prows += C->n_groups * C->sh->n_lines;
        L->ngs += C->n_groups;
    }
    /* groups above RFEC_MAX_K: the host peel's line jobs, output rows after
     * the batched peel's rows, launched level by level (jobs sorted by level) */
    uint32_t nbig = 0;
    for (uint32_t d = 0; d < D->ndl; ++d) {
        const rx_sim* X = XS[D->dl[d] >> 32];
        const rx_inst* g = &X->G[(uint32_t)D->dl[d]];
        if (rx_line_jobs(&X->S[g->shape]))
            nbig += g->count;
    }
    int32_t* job_of = nbig ? (int32_t*)malloc((size_t)nbig * sizeof(int32_t)) : NULL;
    if (nbig && !job_of)
        return rfec_set_error(RFEC_ENOMEM, "rx: large groups");
    for (uint32_t d = 0, off = 0; d < D->ndl; ++d) {
        rx_sim* X = XS[D->dl[d] >> 32];
        rx_inst* g = &X->G[(uint32_t)D->dl[d]];
        if (!rx_line_jobs(&X->S[g->shape]))
            continue;
        g->gslot = off; /* (a large group's slot: its job_of range) */
        if (rx_big_peel(X, D, (uint32_t)D->dl[d], job_of + off))
            D->oom = 1;
        off += g->count;
    }
    const int rc = D->oom ? rfec_set_error(RFEC_ENOMEM, "rx: line jobs") : D->njobs ? rx_sort_jobs(D, L, job_of, nbig)
                                                                                     : RFEC_OK;
    if (rc) {
        free(job_of);
        return rc;
    }
    L->job_of = job_of;
    /* dense output per device shape: E slots per group, the shape's largest erasure count among its
       delivering groups (the e-th erased member of a group, index order, goes to slot e) */
    for (uint32_t k = 0; k < D->nc; ++k)
        D->C[k].E = 0;
    for (uint32_t d = 0; d < D->ndl; ++d) {
        const uint32_t t = (uint32_t)(D->dl[d] >> 32);
        const rx_sim* X = XS[t];
        const rx_inst* g = &X->G[(uint32_t)D->dl[d]];
        if (rx_line_jobs(&X->S[g->shape]))
            continue;
        rx_dclass* C = RX_CLASS(D, sbase, t, g);
        const uint32_t er = g->count - (uint32_t)(__builtin_popcountll(g->arrived[0]) + __builtin_popcountll(g->arrived[1]));
        C->E = er > C->E ? er : C->E;
    }
    size_t ws_bytes = 0;
    for (uint32_t k = 0; k < D->nc; ++k) {
        rx_dclass* C = &D->C[k];
        if (rx_line_jobs(C->sh) || !C->n_groups)
            continue;
        C->E = C->E < 1 ? 1 : C->E > C->sh->count ? C->sh->count : C->E;
        C->dense0 = L->ndense;
        L->ndense += C->n_groups * C->E;
        ws_bytes += RX_ALIGN(rfec_recover_workspace_size(&C->sh->plan, C->n_groups));
    }
    /* rows on the device, one region: [nrows members][njobs line-job outputs][prows parities][ndense] */
    L->r_job = L->nrows;
    L->r_par = L->nrows + D->njobs;
    L->r_dense = L->nmap = L->r_par + L->prows;
    L->o_map = 0;
    L->o_hdr = RX_ALIGN((size_t)L->nmap * 4);
    L->o_meta = RX_ALIGN(L->o_hdr + (size_t)L->nrows * sizeof(rfec_hdr));
    L->o_fs = RX_ALIGN(L->o_meta + (size_t)L->prows * sizeof(rfec_hdr));
    L->o_pres = RX_ALIGN(L->o_fs + (size_t)L->prows * 2);
    L->o_pp = RX_ALIGN(L->o_pres + (size_t)L->ngs * 16);
    L->o_omap = RX_ALIGN(L->o_pp + (size_t)L->ngs * 8);
    L->o_jobs = RX_ALIGN(L->o_omap + (size_t)D->nev * 4);
    L->o_jmem = RX_ALIGN(L->o_jobs + (size_t)D->njobs * sizeof(rfec_line_job));
    L->o_in_end = L->o_rec = L->d_rows = RX_ALIGN(L->o_jmem + (size_t)D->njmem * 4);
    L->host_bytes = RX_ALIGN(L->o_rec + (size_t)L->ngs * 16);
    L->d_ws = RX_ALIGN(L->d_rows + ((size_t)L->r_dense + L->ndense) * stride);
    L->d_ohdr = RX_ALIGN(L->d_ws + ws_bytes);
    L->d_oidx = RX_ALIGN(L->d_ohdr + (size_t)L->ndense * sizeof(rfec_hdr));
    L->d_out = RX_ALIGN(L->d_oidx + L->ndense);
    L->dev_bytes = RX_ALIGN(L->d_out + (size_t)D->nev * stride);
    return RFEC_OK;
}

/* a shard's state on cache lines of its own: the replay threads write their
 * shard's counters on every record (two shards on one line ping-pong it) */
static rx_sim* rx_sim_alloc(void)
{
    const size_t sz = (sizeof(rx_sim) + 127) & ~(size_t)127;
    void* p = NULL;
    if (posix_memalign(&p, 128, sz))
        return NULL;
    memset(p, 0, sz);
    return (rx_sim*)p;
}

static void rx_shards_free(rx_plane* S)
{
    for (uint32_t t = 0; t < S->T; ++t)
        if (S->XS[t]) {
            rx_sim_free(S->XS[t]);
            free(S->XS[t]);
            S->XS[t] = NULL;
        }
}

static void rx_pool_off(rx_plane* S)
{
    if (S->pool_on)
        pool_stop(&S->pool);
    S->pool_on = 0;
}

static void rx_vown_free(rx_plane* S)
{
    if (S->vown_on)
        for (uint32_t t = 0; t < S->T; ++t)
            pm_free(&S->vown[t]);
    S->vown_on = 0;
}

int rx_shards_init(rx_plane* S, uint32_t T, uint32_t capacity)
{
    rx_pool_off(S);
    rx_shards_free(S);
    S->T = T;
    const char* pf = getenv("RFEC_RX_PREFETCH");
    const int v = pf ? atoi(pf) : 16;
    S->prefetch = v < 0 ? 0u : v > 64 ? 64u : (uint32_t)v;
    for (uint32_t f = 0; f < 65536; ++f)
        S->shard_of[f] = (uint8_t)(f % T);
    for (uint32_t t = 0; t < T; ++t) {
        rx_sim* X = rx_sim_alloc();
        S->XS[t] = X;
        if (!X || rx_tables_init(X))
            return -1;
        X->capacity = capacity;
    }
    if (T > 1) {
        /* RFEC_RX_CALLER=0: the calling thread replays no shard (every shard on the pinned workers, which
           share one last-level cache; the caller may run elsewhere) */
        const char* c = getenv("RFEC_RX_CALLER");
        const uint32_t base = c && c[0] == '0' ? 0u : 1u;
        if (pool_start(&S->pool, T - base, base)) {
            S->pool_on = 1;
            return -1;
        }
        S->pool_on = 1;
    }
    return 0;
}

void rx_plane_free(rx_plane* S)
{
    rx_pool_off(S);
    if (getenv("RFEC_RX_TRACE"))
        for (uint32_t t = 0; t < S->T; ++t)
            if (S->XS[t] && S->XS[t]->tw_n)
                fprintf(stderr, "rx shard %u: %u replays, start +%.1f us, run %.1f us (before the first arrival %.1f), "
                        "%.1f records (per replay)\n", t, S->XS[t]->tw_n, S->XS[t]->tw_wake / S->XS[t]->tw_n,
                        S->XS[t]->tw_run / S->XS[t]->tw_n, S->XS[t]->tw_pre / S->XS[t]->tw_n,
                        (double)S->XS[t]->tw_recs / S->XS[t]->tw_n);
    rx_shards_free(S);
    rx_vown_free(S);
    free(S->pshard);
    free(S->lst);
    free(S->smin);
}

/* The shards merged into one serial state, for good: a batch broke the
 * partition (a packet id under two fec_ids, a recovery outside its flex, or
 * parity ranges too large to claim).  Instances, shapes, slot / line tables
 * and recovered headers are concatenated; map values follow. */
static int rx_merge(rx_plane* S)
{
    const uint32_t T = S->T;
    if (T == 1)
        return RFEC_OK;
    rx_sim* M = rx_sim_alloc();
    uint32_t ng = 0, nslot = 0, nline = 0, ns = 0, nrh = 0;
    for (uint32_t t = 0; t < T; ++t) {
        const rx_sim* X = S->XS[t];
        ng += X->ng, nslot += X->nslot, nline += X->nline, ns += X->ns, nrh += X->nrh;
    }
    if (!M || rx_tables_init(M))
        goto oom;
    M->R = S->XS[0]->R;
    M->capacity = S->XS[0]->capacity;
    M->max_ts = S->max_ts;
    M->G = (rx_inst*)malloc(((size_t)ng + 1) * sizeof(rx_inst));
    M->S = (rx_shape*)malloc(((size_t)ns + 1) * sizeof(rx_shape));
    M->slot_src = (int32_t*)malloc(((size_t)nslot + 1) * sizeof(int32_t));
    M->slot_hdr = (rfec_hdr*)malloc(((size_t)nslot + 1) * sizeof(rfec_hdr));
    M->line_par = (int32_t*)malloc(((size_t)nline + 1) * sizeof(int32_t));
    M->rh = (rfec_hdr*)malloc(((size_t)nrh + 1) * sizeof(rfec_hdr));
    if (!M->G || !M->S || !M->slot_src || !M->slot_hdr || !M->line_par || !M->rh)
        goto oom;
    M->gcap = ng + 1, M->scap = ns + 1, M->slotcap = M->slothcap = nslot + 1, M->linecap = nline + 1;
    M->rhcap = nrh + 1;
    for (uint32_t t = 0; t < T; ++t) {
        const rx_sim* X = S->XS[t];
        const uint32_t og = M->ng, os = M->ns, oslot = M->nslot, oline = M->nline, orh = M->nrh;
        for (uint32_t i = 0; i < X->ng; ++i) {
            rx_inst g = X->G[i];
            g.slot0 += oslot;
            g.line0 += oline;
            if (g.shape != UINT32_MAX)
                g.shape += os;
            g.gstamp = g.jstamp = 0;
            M->G[M->ng++] = g;
        }
        for (uint32_t i = 0; i < X->ns; ++i) {
            const rx_shape* sh = &X->S[i];
            M->S[M->ns++] = *sh;
            const uint32_t key = sh->count << 16 | sh->row << 8 | sh->col;
            if (!sh->xcol[0] && !sh->xcol[1] && !hm_get(&M->shape_of, key) && hm_put(&M->shape_of, key, os + i + 1))
                goto oom;
        }
        memcpy(M->slot_src + oslot, X->slot_src, (size_t)X->nslot * sizeof(int32_t));
        memcpy(M->slot_hdr + oslot, X->slot_hdr, (size_t)X->nslot * sizeof(rfec_hdr));
        memcpy(M->line_par + oline, X->line_par, (size_t)X->nline * sizeof(int32_t));
        memcpy(M->rh + orh, X->rh, (size_t)X->nrh * sizeof(rfec_hdr));
        M->nslot += X->nslot, M->nline += X->nline, M->nrh += X->nrh;
        for (PM_EACH(&X->seen, k, v))
            if (pm_put(&M->seen, k, *v))
                goto oom;
        for (PM_EACH(&X->cache, k, v))
            if (pm_put(&M->cache, k, (*v & 0x80000000u) ? (0x80000000u | ((*v & 0x7FFFFFFFu) + orh)) : *v))
                goto oom;
        for (PM_EACH(&X->flex_of, k, v))
            if (pm_put(&M->flex_of, k, *v + og))
                goto oom;
    }
    rx_vown_free(S);
    rx_shards_free(S);
    rx_pool_off(S);
    S->XS[0] = M;
    S->T = 1;
    return RFEC_OK;
oom:
    if (M) {
        rx_sim_free(M);
        free(M);
    }
    return rfec_set_error(RFEC_ENOMEM, "rx session: merge");
}

/* Phase 0 of a sharded batch split on the host, serial over the records [a0, a0 + n): each
 * record's shard, the per-shard lists, smin, whether a parity of the batch
 * could meet the 3 s drop through a segment timestamp before it (`risky`). */
static int rx_phase0(rx_plane* S, uint32_t a0, uint32_t n, int* risky)
{
    if (S->lcap < n) {
        const uint32_t c = n + n / 4 + 64;
        uint8_t* ps = (uint8_t*)realloc(S->pshard, c);
        if (ps)
            S->pshard = ps;
        uint32_t* l = (uint32_t*)realloc(S->lst, (size_t)c * 4);
        if (l)
            S->lst = l;
        uint32_t* m = (uint32_t*)realloc(S->smin, (size_t)c * 4);
        if (m)
            S->smin = m;
        if (!ps || !l || !m)
            return rfec_set_error(RFEC_ENOMEM, "rx session: batch lists");
        S->lcap = c;
    }
    const uint32_t T = S->T;
    const rfec_wire_rec* R = S->XS[0]->R + a0;
    uint32_t cnt[RX_MAX_THREADS] = {0};
    uint32_t pm = S->max_ts;
    int rk = 0;
    for (uint32_t p = 0; p < n; ++p) {
        const rfec_wire_rec* r = &R[p];
        uint32_t t = 0xFF;
        if (r->status == RFEC_WIRE_OK && r->mid == RFEC_WIRE_SEG) {
            t = r->fec_id ? S->shard_of[r->fec_id] : r->hdr.seq % T;
            if (r->fec_id && r->hdr.seq && r->hdr.ts > pm) /* (an upper bound of what raises max_ts) */
                pm = r->hdr.ts;
        } else if (r->status == RFEC_WIRE_OK && r->mid == RFEC_WIRE_FEC) {
            t = S->shard_of[r->fec_id];
            if (r->send_ts + 3000u < pm) /* sim_fec.c:148 could drop it */
                rk = 1;
        }
        S->pshard[p] = (uint8_t)t;
        if (t != 0xFF)
            cnt[t]++;
    }
    uint32_t m = UINT32_MAX;
    for (uint32_t p = n; p-- > 0;) {
        S->smin[p] = m;
        const rfec_wire_rec* r = &R[p];
        if (r->status == RFEC_WIRE_OK && r->mid == RFEC_WIRE_FEC && r->send_ts + 3000u < m)
            m = r->send_ts + 3000u;
    }
    S->loff[0] = 0;
    for (uint32_t t = 0; t < T; ++t)
        S->loff[t + 1] = S->loff[t] + cnt[t];
    uint32_t pos[RX_MAX_THREADS];
    memcpy(pos, S->loff, T * sizeof(uint32_t));
    for (uint32_t p = 0; p < n; ++p)
        if (S->pshard[p] != 0xFF)
            S->lst[pos[S->pshard[p]]++] = a0 + p;
    *risky = rk;
    return RFEC_OK;
}

/* shard t replays its records of the batch in arrival order */
static void rx_shard_replay(rx_plane* S, rx_sim* X, const rx_par* P, uint32_t t);
static void rx_shard_job(void* arg, uint32_t t)
{
    rx_plane* S = (rx_plane*)arg;
    rx_sim* X = S->XS[t];
    const rx_par* P = &S->par;
    const double ts = now_us();
    X->tw_wake += ts - P->t0;
    X->tw_n++;
    X->tw_start = ts;
    rx_shard_replay(S, X, P, t);
    X->tw_run += now_us() - ts;
}

static void rx_shard_replay(rx_plane* S, rx_sim* X, const rx_par* P, uint32_t t)
{
    if (P->sum) {
        /* the device's split, taken apart in chunks by rx_split_job: the drop check over the chunks (a
           parity's limit against max_ts at the batch's start and the segment timestamps before it), then
           this shard's records of every chunk, in arrival order, each with its smin */
        const uint32_t T = S->T;
        uint32_t run = P->max0, suf[RX_MAX_THREADS + 1], nm = 0;
        for (uint32_t j = 0; j < T; ++j) {
            const rx_sim* C = S->XS[j];
            if (C->c_flag || C->c_minfec < run) {
                rx_conflict(X, RX_CONFLICT_RISKY);
                return;
            }
            run = C->c_maxseg > run ? C->c_maxseg : run;
        }
        suf[T] = UINT32_MAX;
        for (uint32_t j = T; j-- > 0;)
            suf[j] = S->XS[j]->c_minfec < suf[j + 1] ? S->XS[j]->c_minfec : suf[j + 1];
        RX_GROW(X->mine, 0, X->minecap, P->n, uint32_t);
        if (X->oom)
            return;
        if (!(X->mine_sm = (uint32_t*)realloc(X->mine_sm, (size_t)X->minecap * 4))) {
            X->oom = 1;
            return;
        }
        for (uint32_t j = 0; j < T; ++j) {
            const rx_sim* C = S->XS[j];
            for (uint32_t q = C->cof[t]; q < C->cof[t + 1]; ++q) {
                X->mine[nm] = P->a0 + C->cpos[q];
                X->mine_sm[nm++] = C->csm[q] < suf[j + 1] ? C->csm[q] : suf[j + 1];
            }
        }
        /* the records, prefetched a few arrivals ahead: the device wrote them (cache-cold here) and a shard's
           records are scattered over the batch, so the hardware prefetcher does not follow them (each one a
           DRAM round trip: a shard replayed 3-4 x slower per arrival than one thread over the whole batch) */
        const rfec_wire_rec* R = X->R;
        const uint32_t pf = S->prefetch;
        for (uint32_t i = 0; i < nm && i < pf; ++i)
            __builtin_prefetch(&R[X->mine[i]]);
        X->tw_pre += now_us() - X->tw_start;
        X->tw_recs += nm;
        for (uint32_t i = 0; i < nm && !X->oom; ++i) {
            if (i + pf < nm)
                __builtin_prefetch(&R[X->mine[i + pf]]);
            if ((i & 15) == 0 && __atomic_load_n(&S->par.conflict, __ATOMIC_RELAXED))
                return;
            X->smin_cur = X->mine_sm[i];
            rx_arrival(X, X->mine[i]);
        }
    } else {
        const uint32_t* L = S->lst + S->loff[t];
        const uint32_t n = S->loff[t + 1] - S->loff[t];
        X->tw_pre += now_us() - X->tw_start;
        for (uint32_t i = 0; i < n && !X->oom; ++i) {
            if ((i & 15) == 0 && __atomic_load_n(&S->par.conflict, __ATOMIC_RELAXED))
                return;
            X->smin_cur = P->smin[L[i] - P->a0];
            rx_arrival(X, L[i]);
        }
    }
    rx_bucket_claims(X, S->T);
}

/* Chunk j of the batch's split summary (positions [j n / T, (j + 1) n / T)),
 * on shard j's thread before the replay: its positions grouped by shard (a
 * counting pass, then a backward fill that keeps each shard's arrival order
 * and carries the chunk-local suffix min of the parity limits), and the
 * chunk's drop-check figures.  Every replay thread then reads only its own
 * records' positions (each thread walking the whole summary cost ~25 us a
 * batch: 4,096 records, two passes, branchy). */
static void rx_split_job(void* arg, uint32_t j)
{
    rx_plane* S = (rx_plane*)arg;
    rx_sim* X = S->XS[j];
    const rx_par* P = &S->par;
    const uint32_t T = S->T, n = P->n;
    const uint32_t p0 = (uint32_t)((uint64_t)n * j / T), p1 = (uint32_t)((uint64_t)n * (j + 1) / T);
    const rfec_rx_split* sum = P->sum;
    uint32_t cnt[RX_MAX_THREADS + 1] = {0};
    uint32_t pm = 0, mf = UINT32_MAX;
    int flag = 0;
    if (X->ccap < p1 - p0) {
        const uint32_t c = p1 - p0 + (p1 - p0) / 4 + 64;
        uint32_t* a = (uint32_t*)realloc(X->cpos, (size_t)c * 4);
        if (a)
            X->cpos = a;
        uint32_t* b = (uint32_t*)realloc(X->csm, (size_t)c * 4);
        if (b)
            X->csm = b;
        if (!a || !b) {
            X->oom = 1;
            X->c_flag = 1;
            return;
        }
        X->ccap = c;
    }
    for (uint32_t p = p0; p < p1; ++p) {
        const rfec_rx_split e = sum[p];
        if (e.kind == RX_SPLIT_SEG_TS) {
            pm = e.value > pm ? e.value : pm;
        } else if (e.kind == RX_SPLIT_FEC) {
            flag |= e.value < pm;
            mf = e.value < mf ? e.value : mf;
        }
        cnt[e.shard == 0xFF ? T : e.shard]++;
    }
    X->cof[0] = 0;
    for (uint32_t u = 0; u < T; ++u)
        X->cof[u + 1] = X->cof[u] + cnt[u];
    uint32_t end[RX_MAX_THREADS];
    memcpy(end, X->cof + 1, T * sizeof(uint32_t));
    uint32_t m = UINT32_MAX;
    for (uint32_t p = p1; p-- > p0;) {
        const rfec_rx_split e = sum[p];
        if (e.shard != 0xFF) {
            const uint32_t q = --end[e.shard];
            X->cpos[q] = p;
            X->csm[q] = m;
        }
        if (e.kind == RX_SPLIT_FEC && e.value < m)
            m = e.value;
    }
    X->c_maxseg = pm;
    X->c_minfec = mf;
    X->c_flag = flag;
}

/* the batch's packet-id claims into the owner tables: thread j takes the ids
 * of its partition from every shard's log; an id under two fec_ids is a
 * conflict */
static void rx_verify_job(void* arg, uint32_t j)
{
    rx_plane* S = (rx_plane*)arg;
    pmap* V = &S->vown[j];
    const uint32_t T = S->T;
    for (uint32_t u = 0; u < T; ++u) {
        const rx_sim* X = S->XS[u];
        for (uint32_t q = X->coff[j]; q < X->coff[j + 1]; ++q) {
            const uint32_t seq = (uint32_t)(X->cpart[q] >> 32), code = (uint32_t)X->cpart[q];
            const uint32_t v = pm_get(V, seq);
            if (!v) {
                if (pm_put(V, seq, code))
                    __atomic_fetch_or(&S->par.conflict, RX_CONFLICT_OWNER, __ATOMIC_RELAXED); /* (no memory: serial) */
            } else if (v != code) {
                __atomic_fetch_or(&S->par.conflict, RX_CONFLICT_OWNER, __ATOMIC_RELAXED);
                return;
            }
        }
    }
}

/* the batch in arrival order over the shards, one max_ts (then the claims bucketed) */
static void rx_serial_over_shards(rx_plane* S, uint32_t a0, uint32_t n)
{
    uint32_t m = S->max_ts;
    const rfec_rx_split* sum = S->par.sum;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t t = sum ? sum[p].shard : S->pshard[p];
        if (t == 0xFF)
            continue;
        rx_sim* X = S->XS[t];
        X->max_ts = m;
        rx_arrival(X, a0 + p);
        m = X->max_ts;
        if (X->oom || __atomic_load_n(&S->par.conflict, __ATOMIC_RELAXED))
            break;
    }
    for (uint32_t t = 0; t < S->T; ++t)
        rx_bucket_claims(S->XS[t], S->T);
}

static int rx_any_oom(const rx_plane* S)
{
    for (uint32_t t = 0; t < S->T; ++t)
        if (S->XS[t]->oom)
            return 1;
    return 0;
}

/* the batch over one serial state (T == 1: from the start, or just merged) */
static int rx_ingest_serial(rx_plane* S, uint32_t a0, uint32_t n)
{
    rx_sim* X = S->XS[0];
    X->P = NULL;
    X->nout = X->dropped = X->unmodelled = 0;
    X->max_ts = S->max_ts;
    rx_run(X, a0, n);
    S->max_ts = X->max_ts;
    S->n_serial++;
    return X->oom ? rfec_set_error(RFEC_ENOMEM, "rx session: host tables") : RFEC_OK;
}

int rx_ingest(rx_plane* S, const rfec_wire_rec* R, uint32_t a0, uint32_t n, const rfec_rx_split* sum)
{
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        X->R = R;
        X->nout = X->dropped = X->unmodelled = 0;
    }
    int rc, risky = 0;
    if (S->T == 1) {
        const double tr = now_us();
        rc = rx_ingest_serial(S, a0, n);
        S->t_replay += now_us() - tr;
        return rc;
    }
    if (!S->vown_on) {
        for (uint32_t t = 0; t < S->T; ++t)
            if (pm_init(&S->vown[t]))
                return rfec_set_error(RFEC_ENOMEM, "rx session: packet ids");
        S->vown_on = 1;
    }
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        if (!X->claimed && !(X->claimed = (uint32_t*)calloc(2u * (65536u / S->T + 1u), sizeof(uint32_t))))
            return rfec_set_error(RFEC_ENOMEM, "rx session: claims");
        X->nclaims = 0;
    }
    if (!sum) { /* (with the device's split the replay threads take the batch apart themselves) */
        const double ts = now_us();
        if ((rc = rx_phase0(S, a0, n, &risky)))
            return rc;
        S->t_split += now_us() - ts;
    }
    const double tr = now_us();
    rx_par* P = &S->par;
    P->T = S->T;
    P->sum = sum;
    P->n = n;
    P->max0 = S->max_ts;
    P->smin = sum ? NULL : S->smin;
    P->a0 = a0;
    P->ts_check = !risky;
    P->conflict = 0;
    P->t0 = now_us();
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        X->P = P;
        X->max_ts = S->max_ts;
        rx_journal_begin(X);
    }
    if (!risky) {
        if (sum)
            pool_run(&S->pool, rx_split_job, S);
        P->t0 = now_us();
        pool_run(&S->pool, rx_shard_job, S);
    } else {
        rx_serial_over_shards(S, a0, n);
    }
    int c = __atomic_load_n(&P->conflict, __ATOMIC_RELAXED);
    S->t_replay += now_us() - tr;
    if (!c && !rx_any_oom(S)) {
        const double tv = now_us();
        pool_run(&S->pool, rx_verify_job, S); /* every packet id under one fec_id? */
        S->t_verify += now_us() - tv;
        c = __atomic_load_n(&P->conflict, __ATOMIC_RELAXED);
        if (!c)
            ++*(risky ? &S->n_serial : &S->n_parallel);
    } else if ((c & (RX_CONFLICT_TS | RX_CONFLICT_RISKY)) && !(c & RX_CONFLICT_OWNER) && !rx_any_oom(S)) {
        /* a recovery raised max_ts past a later parity's limit, or a parity could meet the drop through a
           segment timestamp before it: again, in arrival order */
        S->n_rollback++;
        for (uint32_t t = 0; t < S->T; ++t) {
            rx_rollback(S->XS[t]);
            rx_journal_begin(S->XS[t]);
        }
        P->ts_check = 0;
        P->conflict = 0;
        rx_serial_over_shards(S, a0, n); /* (the claim logs keep the first try's claims too) */
        c = __atomic_load_n(&P->conflict, __ATOMIC_RELAXED);
        if (!c && !rx_any_oom(S)) {
            pool_run(&S->pool, rx_verify_job, S);
            c = __atomic_load_n(&P->conflict, __ATOMIC_RELAXED);
        }
        if (!c)
            S->n_serial++;
    }
    if (rx_any_oom(S))
        return rfec_set_error(RFEC_ENOMEM, "rx session: host tables");
    if (c) { /* a packet id crossed fec_ids: back to the batch's start, one serial state from here on */
        S->n_rollback++;
        for (uint32_t t = 0; t < S->T; ++t) {
            rx_rollback(S->XS[t]);
            S->XS[t]->P = NULL;
        }
        if (rx_any_oom(S) || (rc = rx_merge(S)))
            return rfec_set_error(RFEC_ENOMEM, "rx session: merge");
        return rx_ingest_serial(S, a0, n);
    }
    uint32_t m = S->max_ts;
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        rx_journal_end(X);
        X->P = NULL;
        m = X->max_ts > m ? X->max_ts : m;
    }
    S->max_ts = m;
    return RFEC_OK;
}

/* Compaction keeps only what the open state refers to: the flexes still
 * registered (with their slot / line tables), the records of cached segments
 * and of those flexes' members and parities, the headers of cached recovered
 * segments -- over every shard; records are renumbered in arrival order. */
void rx_compact_free(rx_compaction* K)
{
    for (uint32_t t = 0; t < RX_MAX_THREADS; ++t) {
        free(K->K[t].NG);
        free(K->K[t].nsrc);
        free(K->K[t].nhdr);
        free(K->K[t].npar);
        free(K->K[t].hmap_);
    }
    free(K->gmap);
    free(K->rmap);
    memset(K, 0, sizeof(*K));
}

int rx_compact_mark(const rx_plane* S, uint32_t nstore, uint32_t tail, rx_compaction* K)
{
    memset(K, 0, sizeof(*K));
    uint32_t* rmap = K->rmap = (uint32_t*)calloc((size_t)nstore + 1, sizeof(uint32_t));
    if (!rmap)
        goto oom;
    /* per shard: room for the live flexes and their tables; mark the records they refer to */
    for (uint32_t t = 0; t < S->T; ++t) {
        const rx_sim* X = S->XS[t];
        rx_kept* k = &K->K[t];
        uint32_t nslot = 0, nline = 0;
        for (PM_EACH(&X->flex_of, fk, fv)) {
            const rx_inst* g = &X->G[*fv - 1];
            if (g->shape == UINT32_MAX)
                continue;
            nslot += g->count;
            nline += X->S[g->shape].n_lines;
            for (uint32_t q = 0; q < g->count; ++q)
                if (X->slot_src[g->slot0 + q] >= 0)
                    rmap[X->slot_src[g->slot0 + q]] = 1;
            for (uint32_t q = 0; q < X->S[g->shape].n_lines; ++q)
                if (X->line_par[g->line0 + q] >= 0)
                    rmap[X->line_par[g->line0 + q]] = 1;
        }
        for (PM_EACH(&X->cache, ck, cv))
            if (!(*cv & 0x80000000u))
                rmap[*cv - 1] = 1;
        k->NG = (rx_inst*)malloc(((size_t)X->flex_of.n + 1) * sizeof(rx_inst));
        k->nsrc = (int32_t*)malloc(((size_t)nslot + 1) * sizeof(int32_t));
        k->nhdr = (rfec_hdr*)malloc(((size_t)nslot + 1) * sizeof(rfec_hdr));
        k->npar = (int32_t*)malloc(((size_t)nline + 1) * sizeof(int32_t));
        k->hmap_ = (uint32_t*)calloc((size_t)X->nrh + 1, sizeof(uint32_t));
        if (!k->NG || !k->nsrc || !k->nhdr || !k->npar || !k->hmap_)
            goto oom;
    }
    for (uint32_t r = 0; r < nstore; ++r)
        K->nr += rmap[r] != 0;
    if ((K->gmap = (uint32_t*)malloc(((size_t)K->nr + tail + 1) * sizeof(uint32_t))))
        return RFEC_OK;
oom:
    rx_compact_free(K);
    return rfec_set_error(RFEC_ENOMEM, "rx session: compaction");
}

void rx_compact_renumber(rx_plane* S, uint32_t nstore, uint32_t tail, rx_compaction* K)
{
    uint32_t* rmap = K->rmap;
    /* 1. the live flexes and their tables, packed; cached recovered segments keep their header */
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        rx_kept* k = &K->K[t];
        for (PM_EACH(&X->flex_of, fk, fv)) {
            rx_inst g = X->G[*fv - 1];
            if (g.shape != UINT32_MAX) {
                const uint32_t nlines = X->S[g.shape].n_lines;
                memcpy(k->nsrc + k->ns, X->slot_src + g.slot0, g.count * sizeof(int32_t));
                memcpy(k->nhdr + k->ns, X->slot_hdr + g.slot0, g.count * sizeof(rfec_hdr));
                memcpy(k->npar + k->nl, X->line_par + g.line0, nlines * sizeof(int32_t));
                g.slot0 = k->ns;
                g.line0 = k->nl;
                k->ns += g.count;
                k->nl += nlines;
            }
            k->NG[k->ng] = g;
            *fv = ++k->ng;
        }
        for (PM_EACH(&X->cache, ck, cv))
            if (*cv & 0x80000000u)
                k->hmap_[*cv & 0x7FFFFFFFu] = 1;
    }
    /* 2. new ids, in arrival order; the row map (the pending batch's rows follow the kept ones) */
    uint32_t nr = 0;
    for (uint32_t r = 0; r < nstore; ++r)
        if (rmap[r]) {
            K->gmap[nr] = r;
            rmap[r] = ++nr;
        }
    for (uint32_t t = 0; t < tail; ++t)
        K->gmap[nr + t] = nstore + t;
    for (uint32_t t = 0; t < S->T; ++t) {
        rx_sim* X = S->XS[t];
        rx_kept* k = &K->K[t];
        for (uint32_t h = 0; h < X->nrh; ++h)
            if (k->hmap_[h])
                k->hmap_[h] = ++k->nh;
        for (uint32_t q = 0; q < k->ns; ++q)
            if (k->nsrc[q] >= 0)
                k->nsrc[q] = (int32_t)rmap[k->nsrc[q]] - 1;
        for (uint32_t q = 0; q < k->nl; ++q)
            if (k->npar[q] >= 0)
                k->npar[q] = (int32_t)rmap[k->npar[q]] - 1;
        for (PM_EACH(&X->cache, ck, cv))
            *cv = (*cv & 0x80000000u) ? (0x80000000u | (k->hmap_[*cv & 0x7FFFFFFFu] - 1)) : rmap[*cv - 1];
        for (uint32_t h = 0; h < X->nrh; ++h)
            if (k->hmap_[h])
                X->rh[k->hmap_[h] - 1] = X->rh[h];
        X->nrh = k->nh;
        /* the group tables */
        free(X->G);
        free(X->slot_src);
        free(X->slot_hdr);
        free(X->line_par);
        X->G = k->NG;
        X->ng = X->gcap = k->ng;
        X->slot_src = k->nsrc;
        X->slot_hdr = k->nhdr;
        X->nslot = X->slotcap = X->slothcap = k->ns;
        X->line_par = k->npar;
        X->nline = X->linecap = k->nl;
        k->NG = NULL;
        k->nsrc = k->npar = NULL;
        k->nhdr = NULL;
    }
}

/* One eviction walk over the union of the shards' maps m (2 flex_of, 1
 * cache), in key order: the shards' own walks (each in key order) merged, so
 * the cost is the entries evicted, not the open state (a sort of every
 * shard's keys per eviction cost ~10-20 % of a batch's host time).  Stops at
 * the first entry that stays, as the skiplist walks do. */
static void rx_evict_walk(rx_plane* S, int m)
{
    const uint32_t T = S->T;
    uint32_t key[RX_MAX_THREADS], done[RX_MAX_THREADS];
    uint32_t* val[RX_MAX_THREADS];
    for (uint32_t t = 0; t < T; ++t) {
        key[t] = done[t] = 0;
        val[t] = pm_next(rx_map(S->XS[t], m), &key[t], &done[t]);
    }
    for (;;) {
        uint32_t b = UINT32_MAX;
        for (uint32_t t = 0; t < T; ++t)
            if (val[t] && (b == UINT32_MAX || key[t] < key[b]))
                b = t;
        if (b == UINT32_MAX)
            return;
        rx_sim* X = S->XS[b];
        const uint32_t v = *val[b];
        if (m == 2) {
            const rx_inst* g = &X->G[v - 1];
            if (!(g->fec_ts + 3000u <= S->max_ts || g->nsegs >= g->count))
                return;
            rx_remove(X, v - 1);
        } else {
            const uint32_t ts = (v & 0x80000000u) ? X->rh[v & 0x7FFFFFFFu].ts : X->R[v - 1].hdr.ts;
            if (!(ts + 6000u < S->max_ts))
                return;
            pm_del(&X->cache, key[b]);
        }
        if (key[b] == UINT32_MAX) {
            val[b] = NULL;
            continue;
        }
        ++key[b];
        val[b] = pm_next(rx_map(X, m), &key[b], &done[b]);
    }
}

/* sim_fec_evict (sim_fec.c:209-241) over the shards: flexes in fec_id order
 * while stale (fec_ts + 3000 <= max_ts) or full, removed with their members'
 * cache entries; then cached segments in packet_id order while older than 6 s
 * (timestamp + 6000 < max_ts); both walks stop at the first entry that stays
 * (rx_evict's rules over the union of the shards). */
int rx_plane_evict(rx_plane* S)
{
    for (uint32_t t = 0; t < S->T; ++t)
        S->XS[t]->max_ts = S->max_ts;
    if (S->T == 1) {
        rx_evict(S->XS[0]);
    } else {
        rx_evict_walk(S, 2);
        rx_evict_walk(S, 1);
    }
    return rx_any_oom(S) ? rfec_set_error(RFEC_ENOMEM, "rx session: evict") : RFEC_OK;
}
