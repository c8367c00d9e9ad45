/*
 * rfec_rx_dev.c -- the device side of receiver ingestion: the run half of one
 * call's device work (rx_device: staging, peel, copy out; the plan half is
 * rfec_rx_plane.c), rfec_rx_recover and rfec_host_recv_datagrams.
 */
#include <stdlib.h>
#include <string.h>

#include "rfec_rx_dev.h"

typedef struct {
    uint8_t* h;  /* pinned, device-mapped */
    uint8_t* hd; /* h as the device addresses it */
    size_t hb;
    uint8_t* d;
    size_t db;
} rx_ctx;
static __thread rx_ctx t_rx;

/* The device address of host memory the device can read directly (pinned:
 * rfec_pinned_alloc, hipHostMalloc, registered), else NULL (pageable: the
 * caller copies).  A failed query leaves no pending HIP error behind. */
const uint8_t* host_mapped(const void* p)
{
    hipPointerAttribute_t a;
    void* d = NULL;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost ||
        hipHostGetDevicePointer(&d, (void*)p, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        return NULL;
    }
    return (const uint8_t*)d;
}

/* Grows the per-thread pinned / device areas.  The first `keep` bytes of the
 * pinned area survive a grow (copied into the new block before the old one is
 * freed: the allocator may hand back the same address, so callers cannot tell
 * a grow from the pointer). */
static int rx_reserve(size_t host_bytes, size_t dev_bytes, size_t keep)
{
    hipError_t e;
    if (t_rx.hb < host_bytes) {
        uint8_t* nh = NULL;
        host_bytes += host_bytes / 4;
        void* nd = NULL;
        if ((e = hipHostMalloc((void**)&nh, host_bytes, hipHostMallocMapped)) != hipSuccess)
            return set_err(RFEC_ENOMEM, "rx staging (host)", e);
        if ((e = hipHostGetDevicePointer(&nd, nh, 0)) != hipSuccess) {
            (void)hipHostFree(nh);
            return set_err(RFEC_EDEVICE, "rx staging (host): device view", e);
        }
        if (t_rx.h) {
            if (keep)
                memcpy(nh, t_rx.h, keep < t_rx.hb ? keep : t_rx.hb);
            (void)hipHostFree(t_rx.h);
        }
        t_rx.h = nh;
        t_rx.hd = (uint8_t*)nd;
        t_rx.hb = host_bytes;
    }
    if (t_rx.db < dev_bytes) {
        if (t_rx.d)
            (void)hipFree(t_rx.d);
        t_rx.d = NULL;
        t_rx.db = 0;
        dev_bytes += dev_bytes / 4;
        if ((e = hipMalloc((void**)&t_rx.d, dev_bytes)) != hipSuccess)
            return set_err(RFEC_ENOMEM, "rx workspace (device)", e);
        t_rx.db = dev_bytes;
    }
    return RFEC_OK;
}

/* The device side of one call: the groups that delivered something in this
 * call (over the T shards XS; rx_plan), rebuilt from their arrived members and
 * registered parities (rows of `rows`, DEVICE, indexed by record), peeled by
 * rfec_recover_batch, and the delivered rows copied out.  The pinned tables
 * go after the first `hoff` bytes of t_rx.h, which survive a grow (the
 * shards' R may live there: `r_stage`). */
static int rx_device_run(rx_sim* const* XS, uint32_t T, rx_pool* pool, rx_dev* D, const rx_layout* L,
                         const uint8_t* rows, uint32_t stride, uint32_t capacity, size_t hoff, int r_stage,
                         rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out, rfec_rx_report* rep,
                         hipStream_t sm, double th)
{
    hipError_t e = hipSuccess;
    int rc, ke = 0;
    if ((rc = rx_reserve(hoff + L->host_bytes, L->dev_bytes, hoff)))
        return rc;
    if (r_stage) /* the records live at the start of the pinned block, which may have moved */
        for (uint32_t t = 0; t < T; ++t)
            XS[t]->R = (const rfec_wire_rec*)t_rx.h;
    uint8_t* H = t_rx.h + hoff;
    uint8_t* Hd = t_rx.hd + hoff; /* H as the device addresses it */
    int32_t* map = (int32_t*)(H + L->o_map);
    int32_t* omap = (int32_t*)(H + L->o_omap);
    for (uint32_t j = 0; j < D->njobs; ++j)
        map[L->r_job + j] = -1;
    if (D->njobs) {
        memcpy(H + L->o_jobs, D->jobs, (size_t)D->njobs * sizeof(rfec_line_job));
        memcpy(H + L->o_jmem, D->jmem, (size_t)D->njmem * 4);
    }
    rx_tabs A = {XS, D, L->sbase, L->job_of, map, (rfec_hdr*)(H + L->o_hdr), (rfec_hdr*)(H + L->o_meta),
                 (uint16_t*)(H + L->o_fs), (uint64_t*)(H + L->o_pres), (uint64_t*)(H + L->o_pp), omap,
                 L->r_job, L->r_par, L->r_dense};
    if (pool && T > 1)
        pool_run(pool, rx_fill_job, &A); /* each shard's groups by the thread that replayed them */
    else
        rx_fill(&A, UINT32_MAX);
    uint32_t nok = 0;
    rep->host_us += now_us() - th;
    rep->n_groups = L->ngs;
    for (uint32_t k = 0; k < D->nc; ++k)
        rep->n_shapes += D->C[k].n_groups != 0;
    /* the device: rows and tables staged in one launch, one dense peel per device shape writing its
       recovered masks into pinned memory, the delivered rows gathered out; one synchronisation */
    uint8_t* Dv = t_rx.d;
    uint8_t* rows_d = Dv + L->d_rows;
    double tt = now_us();
    ke = rfec_launch_rx_stage(rows_d, rows, (const int32_t*)(Hd + L->o_map), L->nmap, stride, Dv, Hd, L->o_in_end, sm);
    for (uint32_t v = 1, lo = 0; v <= L->maxlvl && !ke; lo += L->lvl_n[v], ++v) /* the large groups' line jobs */
        ke = rfec_launch_line_jobs((const rfec_line_job*)(Dv + L->o_jobs) + lo, L->lvl_n[v], (const int32_t*)(Dv + L->o_jmem),
                                   rows, rows_d + (size_t)L->r_job * stride, stride, sm);
    size_t wso = 0;
    uint64_t* rec_d = (uint64_t*)(Hd + L->o_rec);
    for (uint32_t k = 0; k < D->nc && !ke; ++k) {
        const rx_dclass* C = &D->C[k];
        if (!C->n_groups || rx_line_jobs(C->sh))
            continue;
        rfec_kmask M;
        make_masks(&C->sh->plan, &M);
        const rfec_dense_out DO = {rows_d + ((size_t)L->r_dense + C->dense0) * stride,
                                   (rfec_hdr*)(Dv + L->d_ohdr) + C->dense0, Dv + L->d_oidx + C->dense0, C->E};
        ke = rfec_launch_recover_out(&M, C->n_groups, stride, capacity, rows_d + (size_t)C->row0 * stride,
                                     (const rfec_hdr*)(Dv + L->o_hdr) + C->row0, (const uint64_t*)(Dv + L->o_pres) + 2 * C->group0,
                                     rows_d + ((size_t)L->r_par + C->prow0) * stride, (const rfec_hdr*)(Dv + L->o_meta) + C->prow0,
                                     (const uint16_t*)(Dv + L->o_fs) + C->prow0, (const uint64_t*)(Dv + L->o_pp) + C->group0,
                                     rec_d + 2 * C->group0, Dv + L->d_ws + wso, sm, g_tuning, &DO);
        wso += RX_ALIGN(rfec_recover_workspace_size(&C->sh->plan, C->n_groups));
    }
    /* delivered rows: straight into the caller's output when it is pinned and
       large enough (no second round trip; rows the peel did not cover are
       squeezed out on the host below), else into the device staging */
    uint8_t* outd = D->nev && D->nev <= max_out ? (uint8_t*)host_mapped(out_payload) : NULL;
    if (!ke && D->nev)
        ke = rfec_launch_gather_rows(outd ? outd : Dv + L->d_out, rows_d, (const int32_t*)(Dv + L->o_omap), D->nev, stride,
                                     sm);
    uint64_t* rec = (uint64_t*)(H + L->o_rec);
    if (ke || (e = hipStreamSynchronize(sm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx: recover", ke ? ke : (int)e);
    rep->kernel_us += now_us() - tt;
    /* the device peel covers every packet the arrival-order pass delivered (same lines, a superset of
       the members at each firing); anything else is reported, not delivered */
    for (uint32_t q = 0; q < D->nev; ++q) {
        const rx_event* ev = &D->ev[q];
        const rx_sim* X = XS[ev->shard];
        const rx_inst* g = &X->G[ev->inst];
        const int big = rx_line_jobs(&X->S[g->shape]);
        const uint32_t t = ev->hdr.seq - g->base;
        const uint32_t gg = big ? 0 : RX_CLASS(D, L->sbase, ev->shard, g)->group0 + g->gslot;
        if (omap[q] < 0 || (!big && !((rec[2 * gg + (t >> 6)] >> (t & 63)) & 1ull))) {
            D->unmodelled++;
            omap[q] = -1;
            continue;
        }
        nok++;
    }
    if (nok > max_out) {
        *n_out = nok;
        return set_err(RFEC_EINVAL, "rx: output too small", 0);
    }
    tt = now_us();
    uint32_t o = 0;
    if (outd) { /* the rows are in out_payload already (the sync above) */
        for (uint32_t q = 0; q < D->nev; ++q) {
            if (omap[q] < 0)
                continue;
            if (o != q)
                memmove(out_payload + (size_t)o * stride, out_payload + (size_t)q * stride, stride);
            D->ev[o++] = D->ev[q];
        }
    } else if (nok == D->nev) { /* the usual case: one copy */
        if (nok)
            e = hipMemcpyAsync(out_payload, Dv + L->d_out, (size_t)nok * stride, hipMemcpyDeviceToHost, sm);
        o = nok;
    }
    for (uint32_t q = 0; q < D->nev && !outd && nok != D->nev && e == hipSuccess; ++q) {
        if (omap[q] < 0)
            continue;
        e = hipMemcpyAsync(out_payload + (size_t)o * stride, Dv + L->d_out + (size_t)q * stride, stride,
                           hipMemcpyDeviceToHost, sm);
        D->ev[o++] = D->ev[q];
    }
    for (uint32_t q = 0; q < o; ++q) {
        out[q].hdr = D->ev[q].hdr;
        out[q].fec_id = (uint16_t)XS[D->ev[q].shard]->G[D->ev[q].inst].fec_id;
        out[q].reserved = 0;
    }
    if (e == hipSuccess && !outd)
        e = hipStreamSynchronize(sm);
    if (e != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx: output D2H", e);
    rep->d2h_us += now_us() - tt;
    *n_out = o;
    rep->n_recovered = o;
    return RFEC_OK;
}

int rx_device(rx_sim* const* XS, uint32_t T, rx_pool* pool, rx_dev* D, const uint8_t* rows, uint32_t stride,
              uint32_t capacity, size_t hoff, int r_stage, rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out,
              uint32_t* n_out, rfec_rx_report* rep, hipStream_t sm)
{
    const double th = now_us();
    rx_layout L;
    *n_out = 0;
    int rc = rx_plan(XS, T, D, stride, &L);
    if (!rc && D->nev)
        rc = rx_device_run(XS, T, pool, D, &L, rows, stride, capacity, hoff, r_stage, out, out_payload, max_out, n_out,
                           rep, sm, th);
    else if (!rc) /* nothing recovered: no device work */
        rep->host_us += now_us() - th;
    free(L.job_of);
    return rc;
}

int rfec_rx_recover(uint32_t n, const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride,
                    uint32_t capacity, uint32_t* max_ts, rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out,
                    uint32_t* n_out, rfec_rx_report* rep, void* stream)
{
    const double t0 = now_us();
    if (!max_ts || !n_out || !rep || (n && (!recs || !payload)) || (max_out && (!out || !out_payload)))
        return set_err(RFEC_EINVAL, "rx: bad argument", 0);
    if (stride == 0 || stride % 16 || capacity > stride)
        return set_err(RFEC_EINVAL, "rx: stride must be a multiple of 16 and >= capacity", 0);
    memset(rep, 0, sizeof(*rep));
    *n_out = 0;
    if (n == 0)
        return RFEC_OK;
    hipStream_t sm = (hipStream_t)stream;
    hipError_t e;
    int rc = RFEC_OK;
    /* 1. the records to the host (headers only: 64 B each) */
    const size_t rec_bytes = RX_ALIGN((size_t)n * sizeof(rfec_wire_rec));
    if ((rc = rx_reserve(rec_bytes, 0, 0)))
        return rc;
    double tt = now_us();
    if ((e = hipMemcpyAsync(t_rx.h, recs, (size_t)n * sizeof(rfec_wire_rec), hipMemcpyDeviceToHost, sm)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(sm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "rx: records D2H", e);
    rep->d2h_us += now_us() - tt;
    /* 2. the control plane, in arrival order */
    const double th = now_us();
    rx_sim X;
    memset(&X, 0, sizeof(X));
    X.R = (const rfec_wire_rec*)t_rx.h;
    X.capacity = capacity;
    X.max_ts = *max_ts;
    if (rx_tables_init(&X)) {
        rx_sim_free(&X);
        return set_err(RFEC_ENOMEM, "rx: host tables", 0);
    }
    rx_run(&X, 0, n);
    if (X.oom) {
        rx_sim_free(&X);
        return set_err(RFEC_ENOMEM, "rx: host tables", 0);
    }
    *max_ts = X.max_ts;
    rep->n_fec_dropped = X.dropped;
    rep->host_us += now_us() - th;
    /* 3. the device: the records stay at the start of the pinned block */
    rx_sim* XS[1] = {&X};
    rx_dev D;
    memset(&D, 0, sizeof(D));
    rc = rx_device(XS, 1, NULL, &D, payload, stride, capacity, rec_bytes, 1, out, out_payload, max_out, n_out, rep,
                   sm);
    rep->n_unmodelled = X.unmodelled + D.unmodelled;
    rx_dev_free(&D);
    rx_sim_free(&X);
    rep->total_us = now_us() - t0;
    return rc;
}

/* ------------------------------------------------------------------------ */
/* Received datagrams (host) -> recovered segments (host)                    */
/* ------------------------------------------------------------------------ */
/* rfec_pinned_alloc / rfec_pinned_free: rfec_hostmem.c (the registry of pinned blocks the device maps) */

typedef struct {
    uint8_t* d;
    size_t db;
    hipStream_t sm;
} rv_ctx;
static __thread rv_ctx t_rv;

int rx_recv_stream(hipStream_t* sm)
{
    hipError_t e;
    if (!t_rv.sm && (e = hipStreamCreateWithFlags(&t_rv.sm, hipStreamNonBlocking)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "recv: stream", e);
    *sm = t_rv.sm;
    return RFEC_OK;
}

int rfec_host_recv_datagrams(uint32_t n, uint32_t dstride, const uint8_t* dgram, const uint16_t* dlen,
                             uint32_t stride, uint32_t capacity, uint32_t* max_ts, rfec_wire_rec* recs_out,
                             rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                             rfec_rx_report* rep)
{
    const double t0 = now_us();
    if (!max_ts || !n_out || !rep || (n && (!dgram || !dlen)))
        return set_err(RFEC_EINVAL, "recv: bad argument", 0);
    memset(rep, 0, sizeof(*rep));
    *n_out = 0;
    if (n == 0)
        return RFEC_OK;
    if (dstride < 64 || dstride > RFEC_WIRE_MAX_DSTRIDE || dstride % 16 || stride == 0 || stride % 16 ||
        capacity > stride)
        return set_err(RFEC_EINVAL, "recv: dstride must be a multiple of 16 in [64, 2048], stride >= capacity", 0);
    hipError_t e;
    hipStream_t sm = NULL;
    int rc;
    if ((rc = rx_recv_stream(&sm)))
        return rc;
    const size_t o_dl = RX_ALIGN((size_t)n * dstride), o_rec = RX_ALIGN(o_dl + (size_t)n * 2);
    const size_t o_pay = RX_ALIGN(o_rec + (size_t)n * sizeof(rfec_wire_rec));
    const size_t need = RX_ALIGN(o_pay + (size_t)n * stride);
    if (t_rv.db < need) {
        if (t_rv.d)
            (void)hipFree(t_rv.d);
        t_rv.d = NULL;
        t_rv.db = 0;
        const size_t b = need + need / 4;
        if ((e = hipMalloc((void**)&t_rv.d, b)) != hipSuccess)
            return set_err(RFEC_ENOMEM, "recv: device staging", e);
        t_rv.db = b;
    }
    uint8_t* D = t_rv.d;
    double tt = now_us();
    if ((e = hipMemcpyAsync(D, dgram, (size_t)n * dstride, hipMemcpyHostToDevice, sm)) != hipSuccess ||
        (e = hipMemcpyAsync(D + o_dl, dlen, (size_t)n * 2, hipMemcpyHostToDevice, sm)) != hipSuccess ||
        (e = hipStreamSynchronize(sm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "recv: datagrams H2D", e);
    const double h2d = now_us() - tt;
    tt = now_us();
    int ke = rfec_launch_wire_parse(n, dstride, D, (const uint16_t*)(D + o_dl), stride, capacity,
                                    (rfec_wire_rec*)(D + o_rec), D + o_pay, max_dlen(dlen, n), sm);
    if (ke || (e = hipStreamSynchronize(sm)) != hipSuccess)
        return set_err(RFEC_EDEVICE, "recv: parse", ke ? ke : (int)e);
    const double parse = now_us() - tt;
    if (recs_out) {
        tt = now_us();
        if ((e = hipMemcpyAsync(recs_out, D + o_rec, (size_t)n * sizeof(rfec_wire_rec), hipMemcpyDeviceToHost,
                                sm)) != hipSuccess ||
            (e = hipStreamSynchronize(sm)) != hipSuccess)
            return set_err(RFEC_EDEVICE, "recv: records D2H", e);
        rep->d2h_us += now_us() - tt;
    }
    const double d2h_recs = rep->d2h_us;
    rc = rfec_rx_recover(n, (const rfec_wire_rec*)(D + o_rec), D + o_pay, stride, capacity, max_ts, out,
                                   out_payload, max_out, n_out, rep, sm);
    rep->h2d_us += h2d;
    rep->kernel_us += parse;
    rep->d2h_us += d2h_recs;
    rep->total_us = now_us() - t0;
    return rc;
}

