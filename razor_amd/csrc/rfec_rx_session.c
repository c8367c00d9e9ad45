/*
 * rfec_rx_session.c -- receiver sessions (rfec_rx_session_*): the control
 * plane kept across calls (an rx_plane: sharded by fec_id over T shards
 * replayed by a thread pool, rfec_rx_plane.c) plus the device state: records
 * by id in a pinned host store, their payload rows by id in an HBM arena, the
 * stages of the pipelined push.
 */
#include <stdlib.h>
#include <string.h>

#include "rfec_rx_dev.h"

/* a batch of the pipelined push: its parse in flight on the session's stream */
typedef struct {
    rfec_rx_split* sum;  /* pinned, device-mapped: the batch's split summary (k_rx_split) */
    rfec_rx_split* sumd; /* sum as the device addresses it */
    uint32_t sumcap;
    uint8_t* dg; /* device copy of pageable datagram slots + lengths */
    size_t dgb;
    hipEvent_t done;
} rx_stage;

struct rfec_rx_session {
    rx_plane pl;
    rx_dev dev;
    rfec_wire_rec* store;   /* every shard's R: pinned, the parse writes the records straight in */
    rfec_wire_rec* store_d; /* store as the device addresses it */
    uint32_t nstore, storecap;
    uint8_t* arena; /* [arows][stride]: rows [0, nstore) ingested, then the pending batch's */
    uint32_t arows;
    uint8_t* spare; /* the previous arena ([sprows][stride]): the next compaction's target when large enough */
    uint32_t sprows;
    int32_t* dmap;  /* compaction's row map on the device, [dmapcap] */
    uint32_t dmapcap;
    uint32_t stride, capacity;
    /* pipelined push (rfec_rx_session_push_datagrams_async) */
    hipStream_t sa;
    rx_stage st[2];
    uint32_t pend_n; /* rows of the pending batch (arena rows [nstore, nstore + pend_n)) */
    int pend;        /* its stage, -1: none */
};

static int rx_compact(rfec_rx_session* S, uint32_t extra, hipStream_t sm);

static uint32_t rx_default_threads(void)
{
    const char* v = getenv("RFEC_RX_THREADS");
    const int t = v ? atoi(v) : 8;
    return t < 1 ? 1u : t > RX_MAX_THREADS ? (uint32_t)RX_MAX_THREADS : (uint32_t)t;
}

rfec_rx_session* rfec_rx_session_create(uint32_t stride, uint32_t capacity)
{
    if (stride == 0 || stride % 16 || capacity > stride) {
        set_err(RFEC_EINVAL, "rx session: stride must be a multiple of 16 and >= capacity", 0);
        return NULL;
    }
    rfec_rx_session* s = (rfec_rx_session*)calloc(1, sizeof(*s));
    if (!s) {
        set_err(RFEC_ENOMEM, "rx session", 0);
        return NULL;
    }
    s->stride = stride;
    s->capacity = capacity;
    s->pend = -1;
    if (rx_shards_init(&s->pl, rx_default_threads(), capacity)) {
        rfec_rx_session_destroy(s);
        set_err(RFEC_ENOMEM, "rx session: host tables / threads", 0);
        return NULL;
    }
    /* the row arena and the record store now (RFEC_RX_ARENA_ROWS), not inside the first push */
    if (rx_compact(s, 0, NULL)) {
        rfec_rx_session_destroy(s);
        return NULL;
    }
    s->pl.t_compact = 0;
    return s;
}

int rfec_rx_session_set_threads(rfec_rx_session* s, uint32_t threads)
{
    if (!s || threads < 1 || threads > RX_MAX_THREADS)
        return set_err(RFEC_EINVAL, "rx session: threads must be in [1, 64]", 0);
    if (s->nstore || s->pend >= 0 || s->pl.max_ts)
        return set_err(RFEC_EINVAL, "rx session: threads are set before the first push", 0);
    if (threads == s->pl.T)
        return RFEC_OK;
    if (rx_shards_init(&s->pl, threads, s->capacity))
        return set_err(RFEC_ENOMEM, "rx session: host tables / threads", 0);
    return RFEC_OK;
}

void rfec_rx_session_destroy(rfec_rx_session* s)
{
    if (!s)
        return;
    if (s->sa) /* a pending parse still writes into the arena */
        (void)hipStreamSynchronize(s->sa);
    for (int i = 0; i < 2; ++i) {
        if (s->st[i].sum)
            (void)hipHostFree(s->st[i].sum);
        if (s->st[i].dg)
            (void)hipFree(s->st[i].dg);
        if (s->st[i].done)
            (void)hipEventDestroy(s->st[i].done);
    }
    if (s->sa)
        (void)hipStreamDestroy(s->sa);
    rx_plane_free(&s->pl);
    rx_dev_free(&s->dev);
    if (s->store)
        (void)hipHostFree(s->store);
    if (s->arena)
        (void)hipFree(s->arena);
    if (s->spare)
        (void)hipFree(s->spare);
    if (s->dmap)
        (void)hipFree(s->dmap);
    free(s);
}

static uint32_t rx_min_rows(void)
{
    const char* v = getenv("RFEC_RX_ARENA_ROWS");
    const long r = v ? atol(v) : 1l << 18;
    return r < 4096 ? 4096u : r > (1l << 26) ? (1u << 26) : (uint32_t)r;
}

/* Compaction: keeps only the records and rows the open state refers to (the
 * plane marks and renumbers them: rx_compact_mark / rx_compact_renumber),
 * their rows gathered into a fresh arena with room for `extra` more.  The
 * rows of a pending pipelined batch (parsed, not ingested) move along behind
 * the kept ones.  No shard changes until every allocation, host and device,
 * has succeeded. */
static int rx_compact(rfec_rx_session* S, uint32_t extra, hipStream_t sm)
{
    const double t0 = now_us();
    const uint32_t tail = S->pend >= 0 ? S->pend_n : 0;
    hipError_t e;
    if (tail && (e = hipEventSynchronize(S->st[S->pend].done)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx session: pending parse", e);
    /* 1. what stays, and every host table the renumbering needs (the shards are only read) */
    rx_compaction K;
    int rc = rx_compact_mark(&S->pl, S->nstore, tail, &K), ke = 0;
    if (rc)
        goto done;
    const uint32_t nm = K.nr + tail;
    /* 2. the device side's memory.  Room for 4 x what stays (compaction's host work is proportional to the
       open state: it comes back after >= 3 x that many records), at least RFEC_RX_ARENA_ROWS rows (default
       2^18: ~320 MB of HBM at 1,216-B rows; with razor's 300 ms evictions the open state stays far below it) */
    const uint64_t want = 4ull * ((uint64_t)nm + extra);
    const uint32_t arows = (uint32_t)(want > rx_min_rows() ? (want < 0xFFFFFFFFull ? want : 0xFFFFFFFFull) : rx_min_rows());
    /* the previous arena when it is large enough (no allocation per compaction: an eviction per batch
       compacts per batch), else a fresh one */
    uint8_t* arena = NULL;
    if (S->spare && S->sprows >= arows) {
        arena = S->spare;
        S->spare = NULL;
    } else if ((e = hipMalloc((void**)&arena, (size_t)arows * S->stride)) != hipSuccess) {
        rc = set_err(RFEC_ENOMEM, "rx session: arena", e);
        goto done;
    }
    if (S->dmapcap < nm) { /* the row map's device copy */
        if (S->dmap)
            (void)hipFree(S->dmap);
        S->dmap = NULL;
        S->dmapcap = 0;
        if ((e = hipMalloc((void**)&S->dmap, ((size_t)nm + nm / 2) * sizeof(int32_t))) != hipSuccess) {
            rc = set_err(RFEC_EDEVICE, "rx session: row compaction", e);
            goto fail;
        }
        S->dmapcap = nm + nm / 2;
    }
    /* the record store: the same capacity, pinned and device-mapped (the parse writes records in) */
    rfec_wire_rec* nst = S->store;
    rfec_wire_rec* nst_d = S->store_d;
    if (S->storecap < arows) {
        void* d = NULL;
        nst = NULL;
        if ((e = hipHostMalloc((void**)&nst, (size_t)arows * sizeof(rfec_wire_rec), hipHostMallocMapped)) !=
                hipSuccess ||
            (e = hipHostGetDevicePointer(&d, nst, 0)) != hipSuccess) {
            if (nst)
                (void)hipHostFree(nst);
            rc = set_err(RFEC_ENOMEM, "rx session: record store", e);
            goto fail;
        }
        nst_d = (rfec_wire_rec*)d;
    }
    /* 3. the shards renumbered; records (host: in place, gmap[i] >= i, ascending, or into the larger store)
       and rows (device) follow the new -> old map */
    rx_compact_renumber(&S->pl, S->nstore, tail, &K);
    for (uint32_t i = 0; i < nm; ++i)
        nst[i] = S->store[K.gmap[i]];
    if (nst != S->store) {
        if (S->store)
            (void)hipHostFree(S->store);
        S->store = nst;
        S->store_d = nst_d;
        S->storecap = arows;
    }
    S->nstore = K.nr;
    for (uint32_t t = 0; t < S->pl.T; ++t)
        S->pl.XS[t]->R = S->store;
    if (nm && ((e = hipMemcpyAsync(S->dmap, K.gmap, (size_t)nm * sizeof(int32_t), hipMemcpyHostToDevice, sm)) != hipSuccess ||
               (ke = rfec_launch_gather_rows(arena, S->arena, S->dmap, nm, S->stride, sm)) != 0 ||
               (e = hipStreamSynchronize(sm)) != hipSuccess)) {
        rc = set_err(RFEC_EDEVICE, "rx session: row compaction", ke ? ke : (int)e);
        goto fail;
    }
    if (S->arena) { /* the old arena is the next compaction's target (the larger of it and the spare) */
        if (S->spare && S->sprows >= S->arows) {
            (void)hipFree(S->arena);
        } else {
            if (S->spare)
                (void)hipFree(S->spare);
            S->spare = S->arena;
            S->sprows = S->arows;
        }
    }
    S->arena = arena;
    S->arows = arows;
    goto done;
fail:
    (void)hipFree(arena);
done:
    rx_compact_free(&K);
    S->pl.t_compact += now_us() - t0;
    return rc;
}

/* room for n more arena rows and records: drop what the open state no longer
 * refers to (and grow) */
static int rx_session_room(rfec_rx_session* S, uint32_t n, hipStream_t sm)
{
    int rc;
    const uint32_t tail = S->pend >= 0 ? S->pend_n : 0; /* a pending pipelined batch's rows */
    if ((S->nstore + tail + n > S->arows || S->nstore + tail + n > S->storecap) && (rc = rx_compact(S, n, sm)))
        return rc; /* (compaction sizes both: room for 4 x what stays) */
    return RFEC_OK;
}

/* a batch of n records is split by the device into its stage's summary (sharded sessions), not on the host
 * from the records (one serial state; a huge push) */
static int rx_dev_split(const rfec_rx_session* S, uint32_t n) { return S->pl.T > 1 && n <= (1u << 20); }

/* The batch's records are at store[nstore, nstore + n) already (the parse or
 * the D2H wrote them there); payload rows on the device at `payload`, or
 * already in the arena's next n rows (payload NULL; the caller made the
 * room); st: the stage holding the batch's split summary (rx_dev_split) */
static int rx_session_push_staged(rfec_rx_session* S, uint32_t n, const uint8_t* payload, const rx_stage* st,
                                  rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                                  rfec_rx_report* rep, hipStream_t sm)
{
    hipError_t e;
    int rc;
    if (payload) {
        double tt = now_us();
        if ((e = hipMemcpyAsync(S->arena + (size_t)S->nstore * S->stride, payload, (size_t)n * S->stride,
                                hipMemcpyDeviceToDevice, sm)) != hipSuccess)
            return set_err(RFEC_EDEVICE, "rx session: rows", e);
        rep->kernel_us += now_us() - tt;
    }
    const uint32_t a0 = S->nstore;
    S->nstore += n;
    const double th = now_us();
    if ((rc = rx_ingest(&S->pl, S->store, a0, n, rx_dev_split(S, n) ? st->sum : NULL)))
        return rc;
    uint32_t dropped = 0, unmod = 0;
    for (uint32_t t = 0; t < S->pl.T; ++t) {
        dropped += S->pl.XS[t]->dropped;
        unmod += S->pl.XS[t]->unmodelled;
    }
    rep->n_fec_dropped = dropped;
    rep->host_us += now_us() - th;
    const double h0 = rep->host_us;
    rc = rx_device(S->pl.XS, S->pl.T, S->pl.pool_on ? &S->pl.pool : NULL, &S->dev, S->arena, S->stride, S->capacity, 0,
                   0, out, out_payload, max_out, n_out, rep, sm);
    S->pl.t_tables += rep->host_us - h0;
    rep->n_unmodelled = unmod + S->dev.unmodelled;
    return rc;
}

/* The pushes' argument checks (in / aux: the records and payload rows, or the
 * datagram slots of `*dstride` bytes and their lengths); rep and *n_out
 * cleared.  `sync`: not while a pipelined batch is pending. */
static int rx_push_begin(const rfec_rx_session* S, uint32_t n, const void* in, const void* aux, const uint32_t* dstride,
                         const rfec_rx_seg* out, const uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                         rfec_rx_report* rep, int sync)
{
    if (!S || !n_out || !rep || (n && (!in || !aux)) || (max_out && (!out || !out_payload)))
        return set_err(RFEC_EINVAL, "rx session: bad argument", 0);
    if (sync && S->pend >= 0)
        return set_err(RFEC_EINVAL, "rx session: a pipelined batch is pending (flush it: async push with n = 0)", 0);
    memset(rep, 0, sizeof(*rep));
    *n_out = 0;
    if (n && dstride && (*dstride < 64 || *dstride > RFEC_WIRE_MAX_DSTRIDE || *dstride % 16))
        return set_err(RFEC_EINVAL, "rx session: dstride must be a multiple of 16 in [64, 2048]", 0);
    return RFEC_OK;
}

static int rx_stage_reserve(rx_stage* st, uint32_t n, size_t dg_bytes)
{
    hipError_t e;
    if (!st->done && (e = hipEventCreateWithFlags(&st->done, hipEventDisableTiming)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx session: event", e);
    if (st->sumcap < n) {
        const uint32_t c = n + n / 4 + 64;
        void* h = NULL;
        void* d = NULL;
        if ((e = hipHostMalloc(&h, (size_t)c * sizeof(rfec_rx_split), hipHostMallocMapped)) != hipSuccess)
            return set_err(RFEC_ENOMEM, "rx session: split stage", e);
        if ((e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) {
            (void)hipHostFree(h);
            return set_err(RFEC_EDEVICE, "rx session: split stage device view", e);
        }
        if (st->sum)
            (void)hipHostFree(st->sum);
        st->sum = (rfec_rx_split*)h;
        st->sumd = (rfec_rx_split*)d;
        st->sumcap = c;
    }
    if (dg_bytes > st->dgb) {
        if (st->dg)
            (void)hipFree(st->dg);
        st->dg = NULL;
        st->dgb = 0;
        const size_t b = dg_bytes + dg_bytes / 4;
        if ((e = hipMalloc((void**)&st->dg, b)) != hipSuccess)
            return set_err(RFEC_ENOMEM, "rx session: datagram stage", e);
        st->dgb = b;
    }
    return RFEC_OK;
}

/* Starts a datagram batch on stream sm: room for it (compaction on the thread's stream tsm) and its stage;
 * datagrams in pinned memory (the UDP batch slots) are read by the parse itself, pageable ones are copied
 * into the stage first (*h2d_us: issuing that, from *t_start); the parse writes the records straight into
 * the store and the payload rows into the arena at row `row0` behind the ingested ones, the split entries
 * beside (k_parse_q; the wave parses: k_rx_split). */
static int rx_batch_start(rfec_rx_session* S, rx_stage* st, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                          const uint16_t* dlen, uint32_t row0, hipStream_t tsm, hipStream_t sm, double* t_start,
                          double* h2d_us)
{
    hipError_t e;
    int rc;
    const size_t o_dl = RX_ALIGN((size_t)n * dstride);
    if ((rc = rx_session_room(S, n, tsm)) || (rc = rx_stage_reserve(st, n, o_dl + (size_t)n * 2)))
        return rc;
    const double tt = *t_start = now_us();
    const uint8_t* dg = host_mapped(dgram);
    const uint8_t* dl = host_mapped(dlen);
    if (!dg || !dl) {
        if ((e = hipMemcpyAsync(st->dg, dgram, (size_t)n * dstride, hipMemcpyHostToDevice, sm)) != hipSuccess ||
            (e = hipMemcpyAsync(st->dg + o_dl, dlen, (size_t)n * 2, hipMemcpyHostToDevice, sm)) != hipSuccess)
            return set_err(RFEC_EDEVICE, "rx session: datagrams H2D", e);
        dg = st->dg;
        dl = st->dg + o_dl;
    }
    *h2d_us = now_us() - tt;
    row0 += S->nstore; /* (after the room was made: compaction renumbers) */
    const int ke = rfec_launch_wire_parse_split(n, dstride, dg, (const uint16_t*)dl, S->stride, S->capacity,
                                                S->store_d + row0, S->arena + (size_t)row0 * S->stride,
                                                max_dlen(dlen, n), rx_dev_split(S, n) ? st->sumd : NULL, S->pl.T, sm);
    return ke ? set_err(RFEC_EDEVICE, "rx session: parse", ke) : RFEC_OK;
}

int rfec_rx_session_push(rfec_rx_session* S, uint32_t n, const rfec_wire_rec* recs, const uint8_t* payload,
                         rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                         rfec_rx_report* rep, void* stream)
{
    const double t0 = now_us();
    int rc, ke = 0;
    if ((rc = rx_push_begin(S, n, recs, payload, NULL, out, out_payload, max_out, n_out, rep, 1)) || n == 0)
        return rc;
    hipStream_t sm = (hipStream_t)stream;
    hipError_t e;
    rx_stage* st = &S->st[0];
    if ((rc = rx_session_room(S, n, sm)) || (rc = rx_stage_reserve(st, n, 0)))
        return rc;
    double tt = now_us();
    /* the records into the store, their split beside */
    if ((e = hipMemcpyAsync(S->store + S->nstore, recs, (size_t)n * sizeof(rfec_wire_rec), hipMemcpyDeviceToHost,
                            sm)) != hipSuccess ||
        (rx_dev_split(S, n) && (ke = rfec_launch_rx_split(recs, n, S->pl.T, st->sumd, sm)) != 0) ||
        (e = hipStreamSynchronize(sm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx session: records D2H", ke ? ke : (int)e);
    rep->d2h_us += now_us() - tt;
    rc = rx_session_push_staged(S, n, payload, st, out, out_payload, max_out, n_out, rep, sm);
    rep->total_us = now_us() - t0;
    return rc;
}

int rfec_rx_session_push_datagrams(rfec_rx_session* S, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                                   const uint16_t* dlen, rfec_wire_rec* recs_out, rfec_rx_seg* out,
                                   uint8_t* out_payload, uint32_t max_out, uint32_t* n_out, rfec_rx_report* rep)
{
    const double t0 = now_us();
    int rc;
    if ((rc = rx_push_begin(S, n, dgram, dlen, &dstride, out, out_payload, max_out, n_out, rep, 1)) || n == 0)
        return rc;
    hipError_t e;
    hipStream_t tsm = NULL;
    if ((rc = rx_recv_stream(&tsm)))
        return rc;
    rx_stage* st = &S->st[0];
    double tt = 0, h2d_issue = 0;
    if ((rc = rx_batch_start(S, st, n, dstride, dgram, dlen, 0, tsm, tsm, &tt, &h2d_issue)))
        return rc;
    if ((e = hipStreamSynchronize(tsm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx session: parse", e);
    const double staged = now_us() - tt;
    if (recs_out)
        memcpy(recs_out, S->store + S->nstore, (size_t)n * sizeof(rfec_wire_rec));
    rc = rx_session_push_staged(S, n, NULL, st, out, out_payload, max_out, n_out, rep, tsm);
    rep->h2d_us += h2d_issue;
    rep->kernel_us += staged - h2d_issue; /* the H2D completes inside this interval too */
    rep->total_us = now_us() - t0;
    return rc;
}

/* The pipelined push: this call starts batch i (H2D if pageable, parse into
 * the store's records and the arena's rows after the pending batch's, its
 * split summary into its stage, on the session's own stream) and then
 * ingests batch i-1 (control plane, peel on the thread's stream) while the
 * device parses batch i. */
int rfec_rx_session_push_datagrams_async(rfec_rx_session* S, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                                         const uint16_t* dlen, rfec_wire_rec* recs_out, rfec_rx_seg* out,
                                         uint8_t* out_payload, uint32_t max_out, uint32_t* n_out, rfec_rx_report* rep)
{
    const double t0 = now_us();
    int rc;
    if ((rc = rx_push_begin(S, n, dgram, dlen, &dstride, out, out_payload, max_out, n_out, rep, 0)))
        return rc;
    hipError_t e;
    hipStream_t tsm = NULL;
    if ((rc = rx_recv_stream(&tsm)))
        return rc;
    if (!S->sa && (e = hipStreamCreateWithFlags(&S->sa, hipStreamNonBlocking)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx session: stream", e);
    const int prev = S->pend;
    const uint32_t p = prev >= 0 ? S->pend_n : 0;
    int cur = -1;
    if (n) {
        /* 1. start batch i behind the pending one's rows */
        cur = prev == 0 ? 1 : 0;
        rx_stage* st = &S->st[cur];
        double tt = 0, h2d = 0;
        rc = rx_batch_start(S, st, n, dstride, dgram, dlen, p, tsm, S->sa, &tt, &h2d);
        rep->h2d_us += h2d;
        if (rc)
            return rc;
        if ((e = hipEventRecord(st->done, S->sa)) != hipSuccess)
            return set_err(RFEC_EDEVICE, "rx session: parse", e);
    }
    /* 2. ingest batch i-1 while the device parses batch i */
    if (prev >= 0) {
        rx_stage* ps = &S->st[prev];
        double tt = now_us();
        if ((e = hipEventSynchronize(ps->done)) != hipSuccess)
            return set_err(RFEC_EDEVICE, "rx session: parse", e);
        rep->kernel_us += now_us() - tt;
        if (recs_out)
            memcpy(recs_out, S->store + S->nstore, (size_t)p * sizeof(rfec_wire_rec));
        S->pend = -1; /* its records and rows are the store's and the arena's next p now */
        rc = rx_session_push_staged(S, p, NULL, ps, out, out_payload, max_out, n_out, rep, tsm);
        if (rc) {
            S->pend = cur; /* batch i stays pending behind whatever was ingested */
            S->pend_n = n;
            return rc;
        }
    }
    S->pend = cur;
    S->pend_n = n;
    rep->total_us = now_us() - t0;
    return RFEC_OK;
}

/* sim_fec_evict over the shards (rx_plane_evict).  The records and rows the
 * evicted state held are dropped by the next compaction: here once the
 * session holds more than half its arena (an eviction per batch compacted per
 * batch, ~50 us of host time and a device gather each), else when a push
 * needs the room. */
int rfec_rx_session_evict(rfec_rx_session* S, void* stream)
{
    int rc;
    if (!S)
        return set_err(RFEC_EINVAL, "rx session: NULL", 0);
    if ((rc = rx_plane_evict(&S->pl)))
        return rc;
    const uint32_t tail = S->pend >= 0 ? S->pend_n : 0;
    if (2ull * (S->nstore + tail) < S->arows)
        return RFEC_OK;
    return rx_compact(S, 0, (hipStream_t)stream);
}

int rfec_rx_session_get_info(const rfec_rx_session* S, rfec_rx_session_info* info)
{
    if (!S || !info)
        return set_err(RFEC_EINVAL, "rx session: NULL", 0);
    const rx_plane* P = &S->pl;
    memset(info, 0, sizeof(*info));
    info->max_ts = P->max_ts;
    for (uint32_t t = 0; t < P->T; ++t) {
        info->open_flexes += P->XS[t]->flex_of.n;
        info->cached_segments += P->XS[t]->cache.n;
    }
    info->records_held = S->nstore;
    info->rows_held = S->arows;
    info->pending = S->pend >= 0 ? S->pend_n : 0;
    info->threads = P->T;
    info->batches_parallel = P->n_parallel;
    info->batches_serial = P->n_serial;
    info->batches_rolled_back = P->n_rollback;
    info->split_us = P->t_split;
    info->replay_us = P->t_replay;
    info->verify_us = P->t_verify;
    info->tables_us = P->t_tables;
    info->compact_us = P->t_compact;
    return RFEC_OK;
}
