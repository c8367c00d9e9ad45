/*
 * rfec_rx_sim.c -- one shard of the receiver's control plane: the reference's
 * receiver (sim_fec.c:104-241, flex_fec_receiver.c:69-280) replayed in arrival
 * order over headers only: admission, flex lifetime, which line recovers which
 * packet and when, so max_ts and first-arrival dedupe come out as the
 * reference's.  The bytes never leave the device (rfec_rx_dev.c).
 */
#include <stdlib.h>
#include <string.h>

#include "rfec_rx_sim.h"

/* -- the journal (sharded sessions) ------------------------------------------ */
static uint32_t rx_get(rx_sim* X, int m, uint32_t k)
{
    return m == 3 ? hm_get(&X->shape_of, k) : pm_get(rx_map(X, m), k);
}

static void rx_jlog(rx_sim* X, int m, uint32_t k, uint32_t old)
{
    RX_GROW(X->jops, X->njops, X->jopcap, 1, rx_jop);
    if (X->oom)
        return;
    X->jops[X->njops++] = (rx_jop){(uint8_t)m, k, old};
}

/* put / delete on one of X's maps, journaled while a batch may roll back */
static int rx_put(rx_sim* X, int m, uint32_t k, uint32_t v)
{
    if (X->jon)
        rx_jlog(X, m, k, rx_get(X, m, k));
    return m == 3 ? hm_put(&X->shape_of, k, v) : pm_put(rx_map(X, m), k, v);
}
/* as rx_put on map m < 3 for a key the caller just found absent (no second lookup for the journal) */
static int rx_put_new(rx_sim* X, int m, uint32_t k, uint32_t v)
{
    if (X->jon)
        rx_jlog(X, m, k, 0);
    return pm_put(rx_map(X, m), k, v);
}
static void rx_del(rx_sim* X, int m, uint32_t k)
{
    if (X->jon) {
        const uint32_t o = rx_get(X, m, k);
        if (!o)
            return;
        rx_jlog(X, m, k, o);
    }
    if (m == 3)
        hm_del(&X->shape_of, k);
    else
        pm_del(rx_map(X, m), k);
}

/* Saves instance ii (and its slot / line tables) the first time this batch
 * changes it; instances the batch created are dropped whole on rollback. */
static void rx_touch(rx_sim* X, uint32_t ii)
{
    if (!X->jon || ii >= X->j_ng || X->G[ii].jstamp == X->jepoch)
        return;
    rx_inst* g = &X->G[ii];
    const int sh = g->shape != UINT32_MAX;
    const uint32_t nc = sh ? g->count : 0, nl = sh ? X->S[g->shape].n_lines : 0;
    const size_t need = 4 + sizeof(rx_inst) + (size_t)nc * (4 + sizeof(rfec_hdr)) + (size_t)nl * 4;
    if (X->njsave + need > X->jsavecap) {
        size_t c = X->jsavecap ? 2 * X->jsavecap : 1 << 16;
        while (c < X->njsave + need)
            c *= 2;
        uint8_t* p = (uint8_t*)realloc(X->jsave, c);
        if (!p) {
            X->oom = 1;
            return;
        }
        X->jsave = p;
        X->jsavecap = c;
    }
    uint8_t* w = X->jsave + X->njsave;
    memcpy(w, &ii, 4);
    memcpy(w + 4, g, sizeof(rx_inst));
    w += 4 + sizeof(rx_inst);
    memcpy(w, X->slot_src + g->slot0, (size_t)nc * 4);
    memcpy(w + (size_t)nc * 4, X->slot_hdr + g->slot0, (size_t)nc * sizeof(rfec_hdr));
    memcpy(w + (size_t)nc * (4 + sizeof(rfec_hdr)), X->line_par + g->line0, (size_t)nl * 4);
    X->njsave += need;
    g->jstamp = X->jepoch;
}

void rx_journal_begin(rx_sim* X)
{
    X->jon = 1;
    if (++X->jepoch == 0) { /* wrapped: no instance may carry a stale stamp */
        for (uint32_t i = 0; i < X->ng; ++i)
            X->G[i].jstamp = 0;
        X->jepoch = 1;
    }
    X->njops = 0;
    X->njsave = 0;
    X->j_ng = X->ng;
    X->j_nslot = X->nslot;
    X->j_nline = X->nline;
    X->j_ns = X->ns;
    X->j_nrh = X->nrh;
    X->j_max_ts = X->max_ts;
    X->j_dropped = X->dropped;
    X->j_unmod = X->unmodelled;
}

void rx_journal_end(rx_sim* X)
{
    X->jon = 0;
    X->njops = 0;
    X->njsave = 0;
}

/* Back to the state rx_journal_begin saw. */
void rx_rollback(rx_sim* X)
{
    X->jon = 0;
    for (uint32_t q = X->njops; q-- > 0;) {
        const rx_jop* o = &X->jops[q];
        if (o->old) {
            if (o->map == 3 ? hm_put(&X->shape_of, o->key, o->old) : pm_put(rx_map(X, o->map), o->key, o->old))
                X->oom = 1;
        } else if (o->map == 3) {
            hm_del(&X->shape_of, o->key);
        } else {
            pm_del(rx_map(X, o->map), o->key);
        }
    }
    for (size_t off = 0; off < X->njsave;) {
        uint32_t ii;
        memcpy(&ii, X->jsave + off, 4);
        rx_inst* g = &X->G[ii];
        memcpy(g, X->jsave + off + 4, sizeof(rx_inst));
        const int sh = g->shape != UINT32_MAX;
        const uint32_t nc = sh ? g->count : 0, nl = sh ? X->S[g->shape].n_lines : 0;
        const uint8_t* r = X->jsave + off + 4 + sizeof(rx_inst);
        memcpy(X->slot_src + g->slot0, r, (size_t)nc * 4);
        memcpy(X->slot_hdr + g->slot0, r + (size_t)nc * 4, (size_t)nc * sizeof(rfec_hdr));
        memcpy(X->line_par + g->line0, r + (size_t)nc * (4 + sizeof(rfec_hdr)), (size_t)nl * 4);
        off += 4 + sizeof(rx_inst) + (size_t)nc * (4 + sizeof(rfec_hdr)) + (size_t)nl * 4;
    }
    X->ng = X->j_ng;
    X->nslot = X->j_nslot;
    X->nline = X->j_nline;
    X->ns = X->j_ns;
    X->nrh = X->j_nrh;
    X->max_ts = X->j_max_ts;
    X->dropped = X->j_dropped;
    X->unmodelled = X->j_unmod;
    X->npend = X->nout = 0;
    X->njops = 0;
    X->njsave = 0;
}

/* -- packet-id ownership (sharded sessions) ---------------------------------- */
/* owner-table partition of a packet id: blocks of 256 ids, round robin */
static uint32_t rx_part(uint32_t seq, uint32_t T) { return (seq >> 8) % T; }

/* the claims grouped by partition (counting sort), for the T verifiers */
void rx_bucket_claims(rx_sim* X, uint32_t T)
{
    uint32_t cnt[RX_MAX_THREADS + 1] = {0};
    RX_GROW(X->cpart, 0, X->cpartcap, X->nclaims + 1, uint64_t);
    if (X->oom)
        return;
    for (uint32_t q = 0; q < X->nclaims; ++q)
        cnt[rx_part((uint32_t)(X->claims[q] >> 32), T)]++;
    X->coff[0] = 0;
    for (uint32_t j = 0; j < T; ++j)
        X->coff[j + 1] = X->coff[j] + cnt[j];
    uint32_t pos[RX_MAX_THREADS];
    memcpy(pos, X->coff, T * sizeof(uint32_t));
    for (uint32_t q = 0; q < X->nclaims; ++q)
        X->cpart[pos[rx_part((uint32_t)(X->claims[q] >> 32), T)]++] = X->claims[q];
}

static void rx_claim(rx_sim* X, uint32_t seq, uint32_t code)
{
    RX_GROW(X->claims, X->nclaims, X->claimcap, 1, uint64_t);
    if (!X->oom)
        X->claims[X->nclaims++] = (uint64_t)seq << 32 | code;
}

/* a parity's range [base_id, base_id + count) for its fec_id (logged once per range) */
static void rx_claim_range(rx_sim* X, const rfec_wire_rec* r)
{
    uint32_t* c = X->claimed + 2u * (r->fec_id / X->P->T);
    if (c[0] == r->base_id && c[1] == (uint32_t)r->count + 1u)
        return;
    for (uint32_t i = 0; i < r->count; ++i)
        rx_claim(X, r->base_id + i, (uint32_t)r->fec_id + 1u);
    c[0] = r->base_id;
    c[1] = (uint32_t)r->count + 1u;
}

static rfec_hdr rec_hdr(const rfec_wire_rec* r)
{
    rfec_hdr h = r->hdr;
    h.size = r->data_size; /* seg.data_size = the datagram's (sim_receiver.c) */
    return h;
}

/* members of the reference's line `index` of a (count, row, col) flex:
 * flex_recover_row walks i < col, flex_recover_col i < row, both stopping at
 * the first position >= count (flex_fec_receiver.c:118-126, 175-183) */
static uint32_t rx_line_members(uint32_t count, uint32_t row, uint32_t col, uint32_t index, uint32_t* first,
                                uint32_t* stride)
{
    const uint32_t x = index & 0x7Fu;
    uint32_t n = 0;
    if (index & 0x80u) {
        while (n < row && n * col + x < count)
            ++n;
        *first = x;
        *stride = col;
    } else {
        while (n < col && x * col + n < count)
            ++n;
        *first = x * col;
        *stride = 1;
    }
    return n;
}

/* line l of flex g: its members and whether its parity is registered */
uint32_t rx_line(const rx_sim* X, const rx_inst* g, uint32_t l, uint32_t* first, uint32_t* stride, int* reg)
{
    const rx_shape* sh = &X->S[g->shape];
    if (sh->huge) {
        *reg = X->line_par[g->line0 + l] >= 0;
        return rx_line_members(g->count, g->row, g->col, l, first, stride);
    }
    const rfec_line* ln = &sh->plan.line[l];
    *reg = (int)((g->ppm >> l) & 1ull);
    *first = ln->first;
    *stride = ln->stride;
    return ln->count;
}

/* member t of flex g is in it (arrived or recovered); a huge flex's slot
 * header holds the member's seq once it is in, ~(base + t) before */
static int rx_has(const rx_sim* X, const rx_inst* g, uint32_t t)
{
    if (X->S[g->shape].huge)
        return X->slot_hdr[g->slot0 + t].seq == g->base + t;
    return (int)((g->have[t >> 6] >> (t & 63)) & 1ull);
}

static void rx_pend(rx_sim* X, const rfec_hdr* h, uint32_t inst) /* sim_fec_packet_add_recover (sim_fec.c:104-119) */
{
    for (uint32_t i = 0; i < X->npend; ++i)
        if (X->pend[i].hdr.seq == h->seq)
            return;
    RX_GROW(X->pend, X->npend, X->pendcap, 1, rx_event);
    if (X->oom)
        return;
    X->pend[X->npend].hdr = *h;
    X->pend[X->npend++].inst = inst;
}

/* flex_recover_row / flex_recover_col (flex_fec_receiver.c:105-206) over headers */
static void rx_check_line(rx_sim* X, uint32_t ii, int l)
{
    const rx_inst* g = &X->G[ii];
    if (l < 0 || g->nsegs >= g->count)
        return;
    uint32_t first, stride;
    int reg;
    const uint32_t n = rx_line(X, g, (uint32_t)l, &first, &stride, &reg);
    if (!reg)
        return;
    uint32_t loss = 0, cnt = 0;
    for (uint32_t q = 0; q < n; ++q) {
        if (rx_has(X, g, first + q * stride))
            cnt++;
        else
            loss++;
    }
    if (loss != 1 || cnt == 0)
        return;
    const rfec_wire_rec* f = &X->R[X->line_par[g->line0 + l]];
    const uint32_t L = f->data_size;
    if (L > X->capacity)
        return;
    rfec_hdr h = f->hdr; /* flex_fec_xor.c:64-99 */
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t i = first + q * stride;
        if (!rx_has(X, g, i))
            continue;
        const rfec_hdr* m = &X->slot_hdr[g->slot0 + i];
        if (L < m->size)
            return;
        rx_hdr_xor(&h, m);
    }
    if (h.size > L)
        return;
    rx_pend(X, &h, ii);
}

/* flex_fec_receiver_on_segment (flex_fec_receiver.c:243-280); src = record or -1 */
static void rx_on_segment(rx_sim* X, uint32_t ii, const rfec_hdr* h, int32_t src, int check)
{
    rx_inst* g = &X->G[ii];
    if (!g->ref_ok || h->seq < g->base)
        return;
    if (g->shape == UINT32_MAX) {
        X->unmodelled++;
        return;
    }
    rx_touch(X, ii);
    const uint32_t t = h->seq - g->base;
    if (t < g->count) {
        if (rx_has(X, g, t))
            return;
        if (!X->S[g->shape].huge)
            g->have[t >> 6] |= 1ull << (t & 63);
        X->slot_hdr[g->slot0 + t] = *h;
        if (src >= 0) {
            if (!X->S[g->shape].huge)
                g->arrived[t >> 6] |= 1ull << (t & 63);
            X->slot_src[g->slot0 + t] = src;
        }
    } else if (src < 0) {
        X->unmodelled++; /* a recovered header outside its group: inconsistent parities */
    }
    g->nsegs++;
    if (check) {
        const rx_shape* sh = &X->S[g->shape];
        const uint32_t r = t / g->col, c = t % g->col;
        rx_check_line(X, ii, r < 128 ? sh->line_of[r] : -1);
        rx_check_line(X, ii, c < 128 ? sh->line_of[0x80 | c] : -1);
    }
}

void rx_remove(rx_sim* X, uint32_t ii) /* sim_fec_evict_segment + flex removal (sim_fec.c:93-102, 199-205) */
{
    const rx_inst* g = &X->G[ii];
    for (uint32_t i = 0; i < g->count; ++i)
        rx_del(X, 1, g->base + i);
    rx_del(X, 2, g->fec_id);
}

/* sim_fec_put_segment (sim_fec.c:171-207); cache values: record + 1, or 0x80000000 | index into X->rh */
static void rx_put_segment(rx_sim* X, const rfec_hdr* h, uint16_t fec_id, uint32_t cval, int32_t src)
{
    if (h->seq == 0 || pm_get(&X->cache, h->seq))
        return;
    X->max_ts = h->ts > X->max_ts ? h->ts : X->max_ts;
    if (rx_put_new(X, 1, h->seq, cval)) {
        X->oom = 1;
        return;
    }
    const uint32_t fi = pm_get(&X->flex_of, fec_id);
    if (!fi)
        return;
    rx_on_segment(X, fi - 1, h, src, 1);
    if (X->G[fi - 1].nsegs >= X->G[fi - 1].count) /* flex_fec_receiver_full */
        rx_remove(X, fi - 1);
}

/* The device plan of a flex geometry: every row with 2+ members (also rows
 * at and beyond `row` when row * col < count: the reference bounds rows by
 * count only), every column c < col with 2+ members, and the extra columns
 * c >= col of xcol.  Lines of fewer than 2 members can never recover (one
 * missing member leaves none present).  Standard geometry (row * col >=
 * count, no extra columns) is exactly rfec_plan_matrix's plan. */
static int rx_build_plan(uint32_t count, uint32_t row, uint32_t col, const uint64_t* xcol, rfec_plan* p)
{
    if (row * col >= count && !xcol[0] && !xcol[1])
        return rfec_plan_matrix((uint16_t)count, (uint8_t)row, (uint8_t)col, RFEC_LAYER_ROWS | RFEC_LAYER_COLS, p);
    memset(p, 0, sizeof(*p));
    p->k = (uint16_t)count;
    p->row = (uint8_t)row;
    p->col = (uint8_t)col;
    p->rc = 1;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t x = 0; x < 128; ++x) {
            if (pass == 1 && x >= col && !((xcol[x >> 6] >> (x & 63)) & 1ull))
                continue;
            uint32_t first, stride;
            const uint32_t n = rx_line_members(count, row, col, pass ? (0x80u | x) : x, &first, &stride);
            if (n < 2)
                continue;
            if (p->n_lines >= RFEC_MAX_LINES)
                return RFEC_EINVAL;
            rfec_line* l = &p->line[p->n_lines++];
            l->first = (uint8_t)first;
            l->stride = (uint8_t)stride;
            l->count = (uint8_t)n;
            l->index = (uint8_t)(pass ? (0x80u | x) : x);
        }
        if (pass == 0)
            p->n_row_lines = p->n_lines;
    }
    return RFEC_OK;
}

/* flexes of up to 255 segments and 64 lines have a device plan (8-bit
 * members); above RFEC_MAX_K the device recovery takes line jobs (rx_big_peel)
 * instead of the batched peel, whose masks hold 128 members.  Larger flexes
 * (a foreign peer's: the reference receiver takes any uint16_t count,
 * flex_fec_receiver.c:69-88, and up to 128 rows and 128 columns of FEC
 * indices) are huge shapes: line = FEC index, line jobs too. */
#define RX_MAX_COUNT 255u

static uint32_t rx_shape_of(rx_sim* X, uint32_t count, uint32_t row, uint32_t col, const uint64_t* xcol)
{
    if (row > 255 || col > 255)
        return UINT32_MAX;
    const int extended = xcol[0] || xcol[1];
    const uint32_t key = count << 16 | row << 8 | col;
    if (!extended) {
        const uint32_t s = hm_get(&X->shape_of, key);
        if (s)
            return s - 1;
    } else { /* rare (a peer's extra columns): a scan */
        for (uint32_t s = 0; s < X->ns; ++s)
            if (X->S[s].count == count && X->S[s].row == row && X->S[s].col == col && X->S[s].xcol[0] == xcol[0] &&
                X->S[s].xcol[1] == xcol[1])
                return s;
    }
    RX_GROW(X->S, X->ns, X->scap, 1, rx_shape);
    if (X->oom)
        return UINT32_MAX;
    rx_shape* sh = &X->S[X->ns];
    memset(sh, 0, sizeof(*sh));
    sh->count = count;
    sh->row = row;
    sh->col = col;
    sh->xcol[0] = xcol[0];
    sh->xcol[1] = xcol[1];
    sh->huge = count > RX_MAX_COUNT || rx_build_plan(count, row, col, xcol, &sh->plan) != RFEC_OK;
    if (sh->huge) { /* every FEC index is a line */
        sh->n_lines = 256;
        for (int i = 0; i < 256; ++i)
            sh->line_of[i] = (int16_t)i;
    } else {
        sh->n_lines = sh->plan.n_lines;
        for (int i = 0; i < 256; ++i)
            sh->line_of[i] = -1;
        for (uint32_t l = 0; l < sh->n_lines; ++l)
            sh->line_of[sh->plan.line[l].index] = (int16_t)l;
    }
    if (!extended && rx_put(X, 3, key, X->ns + 1)) {
        X->oom = 1;
        return UINT32_MAX;
    }
    return X->ns++;
}

/* A parity for a column c >= col of flex ii (a peer's plan, not razor's
 * sender): the flex moves to the shape with that column added, its
 * registered parities carried over by index.  Returns the column's line in
 * the new shape, or -1 (no room: the parity stays unmodelled). */
static int rx_extend(rx_sim* X, uint32_t ii, uint32_t c)
{
    rx_touch(X, ii);
    rx_inst* g = &X->G[ii];
    uint64_t xcol[2] = {X->S[g->shape].xcol[0], X->S[g->shape].xcol[1]};
    xcol[c >> 6] |= 1ull << (c & 63);
    const uint32_t ns = rx_shape_of(X, g->count, g->row, g->col, xcol);
    if (ns == UINT32_MAX)
        return -1;
    const rx_shape* nsh = &X->S[ns]; /* (X->S may have moved) */
    const rx_shape* osh = &X->S[g->shape];
    RX_GROW(X->line_par, X->nline, X->linecap, nsh->n_lines, int32_t);
    if (X->oom)
        return -1;
    uint64_t ppm = 0;
    for (uint32_t l = 0; l < nsh->n_lines; ++l) {
        const int ol = osh->line_of[nsh->huge ? l : nsh->plan.line[l].index];
        X->line_par[X->nline + l] = ol >= 0 && ((g->ppm >> ol) & 1ull) ? X->line_par[g->line0 + ol] : -1;
        if (ol >= 0 && ((g->ppm >> ol) & 1ull) && !nsh->huge)
            ppm |= 1ull << l;
    }
    if (nsh->huge) /* more than RFEC_MAX_LINES lines now: membership moves to the slot headers (rx_has) */
        for (uint32_t t = 0; t < g->count; ++t)
            if (!((g->have[t >> 6] >> (t & 63)) & 1ull))
                X->slot_hdr[g->slot0 + t].seq = ~(g->base + t);
    g->line0 = X->nline;
    X->nline += nsh->n_lines;
    g->ppm = ppm;
    g->shape = ns;
    return nsh->line_of[0x80u | c];
}

/* sim_fec_put_fec_packet (sim_fec.c:141-169) -> flex_fec_receiver_on_fec (flex_fec_receiver.c:208-241) */
static void rx_put_fec(rx_sim* X, uint32_t a)
{
    const rfec_wire_rec* f = &X->R[a];
    if (f->base_id + f->count == 0u || f->send_ts + 3000u < X->max_ts) {
        X->dropped++;
        return;
    }
    uint32_t fi = pm_get(&X->flex_of, f->fec_id);
    if (!fi) { /* flex_fec_receiver_active (flex_fec_receiver.c:69-88) */
        RX_GROW(X->G, X->ng, X->gcap, 1, rx_inst);
        if (X->oom)
            return;
        rx_inst* g = &X->G[X->ng];
        memset(g, 0, sizeof(*g));
        g->fec_id = f->fec_id;
        g->base = f->base_id;
        g->count = f->count;
        g->row = f->row;
        g->col = f->col;
        g->fec_ts = f->send_ts;
        g->ref_ok = g->col >= 2 && g->row >= 1 && g->count >= 1;
        static const uint64_t no_xcol[2] = {0, 0};
        g->shape = g->ref_ok ? rx_shape_of(X, g->count, g->row, g->col, no_xcol) : UINT32_MAX;
        if (g->shape != UINT32_MAX) {
            const rx_shape* sh = &X->S[g->shape];
            RX_GROW(X->slot_src, X->nslot, X->slotcap, g->count, int32_t);
            RX_GROW(X->slot_hdr, X->nslot, X->slothcap, g->count, rfec_hdr);
            RX_GROW(X->line_par, X->nline, X->linecap, sh->n_lines, int32_t);
            if (X->oom)
                return;
            g->slot0 = X->nslot;
            g->line0 = X->nline;
            for (uint32_t i = 0; i < g->count; ++i) {
                X->slot_src[X->nslot + i] = -1;
                X->slot_hdr[X->nslot + i].seq = ~(g->base + i); /* rx_has: not in the flex */
            }
            for (uint32_t l = 0; l < sh->n_lines; ++l)
                X->line_par[X->nline + l] = -1;
            X->nslot += g->count;
            X->nline += sh->n_lines;
        } else if (g->ref_ok) {
            X->unmodelled++;
        }
        fi = ++X->ng;
        if (rx_put(X, 2, f->fec_id, fi)) {
            X->oom = 1;
            return;
        }
        for (uint32_t i = 0; i < g->count && g->shape != UINT32_MAX; ++i) { /* sim_fec_add_segment_to_flex */
            const uint32_t c = pm_get(&X->cache, g->base + i);
            if (!c)
                continue;
            if (c & 0x80000000u) {
                rx_on_segment(X, fi - 1, &X->rh[c & 0x7FFFFFFFu], -1, 0);
            } else {
                const rfec_hdr h = rec_hdr(&X->R[c - 1]);
                rx_on_segment(X, fi - 1, &h, (int32_t)(c - 1), 0);
            }
        }
    }
    rx_inst* g = &X->G[fi - 1];
    if (!g->ref_ok || g->shape == UINT32_MAX)
        return;
    rx_touch(X, fi - 1);
    g = &X->G[fi - 1];
    int l = X->S[g->shape].line_of[f->index];
    if (X->S[g->shape].huge) { /* line = index; the parity registered once */
        uint32_t first, stride;
        if (rx_line_members(g->count, g->row, g->col, f->index, &first, &stride) < 2 ||
            X->line_par[g->line0 + l] >= 0)
            return;
        X->line_par[g->line0 + l] = (int32_t)a;
        rx_check_line(X, fi - 1, l);
        return;
    }
    if (l < 0) {
        uint32_t first, stride;
        if (rx_line_members(g->count, g->row, g->col, f->index, &first, &stride) < 2)
            return; /* a line that can never recover (flex_fec_receiver.c:133-134, 189-190) */
        /* a column c >= col (razor's sender never emits one; a peer may) */
        if ((l = rx_extend(X, fi - 1, f->index & 0x7Fu)) < 0) {
            X->unmodelled++;
            return;
        }
        g = &X->G[fi - 1];
    }
    if (X->S[g->shape].huge) { /* (the extension took it past RFEC_MAX_LINES lines) */
        if (X->line_par[g->line0 + l] >= 0)
            return;
    } else {
        if ((g->ppm >> l) & 1ull)
            return;
        g->ppm |= 1ull << l;
    }
    X->line_par[g->line0 + l] = (int32_t)a;
    rx_check_line(X, fi - 1, l);
}

/* sim_receiver_recover (sim_receiver.c:780-804): lowest packet_id first,
 * cascading; the recoveries of one record.  In a sharded batch each delivered
 * packet must lie in its flex's range (so its id stays in this shard) and,
 * in the parallel replay, raise max_ts no higher than any later parity of
 * the batch can take (smin): else the batch is replayed otherwise. */
static void rx_drain(rx_sim* X)
{
    while (X->npend && !X->oom) {
        uint32_t b = 0;
        for (uint32_t i = 1; i < X->npend; ++i)
            if (X->pend[i].hdr.seq < X->pend[b].hdr.seq)
                b = i;
        const rx_event e = X->pend[b];
        X->pend[b] = X->pend[--X->npend];
        if (pm_get(&X->seen, e.hdr.seq))
            continue;
        if (X->P) {
            const rx_inst* g = &X->G[e.inst];
            if (e.hdr.seq - g->base >= g->count) {
                rx_conflict(X, RX_CONFLICT_OWNER);
                return;
            }
            if (X->P->ts_check && e.hdr.ts > X->smin_cur) {
                rx_conflict(X, RX_CONFLICT_TS);
                return;
            }
        }
        RX_GROW(X->out, X->nout, X->outcap, 1, rx_event);
        RX_GROW(X->rh, X->nrh, X->rhcap, 1, rfec_hdr);
        if (X->oom || rx_put_new(X, 0, e.hdr.seq, 1)) {
            X->oom = 1;
            return;
        }
        X->out[X->nout++] = e;
        X->rh[X->nrh] = e.hdr;
        const uint32_t idx = X->nrh++;
        rx_put_segment(X, &e.hdr, (uint16_t)X->G[e.inst].fec_id, 0x80000000u | idx, -1);
    }
}

void rx_sim_free(rx_sim* X)
{
    pm_free(&X->seen);
    pm_free(&X->cache);
    pm_free(&X->flex_of);
    hm_free(&X->shape_of);
    free(X->G);
    free(X->S);
    free(X->slot_src);
    free(X->slot_hdr);
    free(X->line_par);
    free(X->pend);
    free(X->out);
    free(X->rh);
    free(X->jops);
    free(X->jsave);
    free(X->claims);
    free(X->mine);
    free(X->mine_sm);
    free(X->cpos);
    free(X->csm);
    free(X->cpart);
    free(X->claimed);
}

/* sim_fec_evict (sim_fec.c:209-241) past its 300 ms wall-clock gate: flexes in
 * fec_id order while stale (fec_ts + 3000 <= max_ts) or full, removed with
 * their members' cache entries; then cached segments in packet_id order while
 * older than 6 s (timestamp + 6000 < max_ts).  Both walks stop at the first
 * entry that stays, as the skiplist walks do (pmap: key order; each step
 * looks up the next key afresh, so removals are safe). */
void rx_evict(rx_sim* X)
{
    uint32_t key = 0, done = 0;
    for (uint32_t* v; (v = pm_next(&X->flex_of, &key, &done)) != NULL;) {
        const uint32_t fi = *v - 1;
        const rx_inst* g = &X->G[fi];
        if (!(g->fec_ts + 3000u <= X->max_ts || g->nsegs >= g->count))
            break;
        rx_remove(X, fi);
        if (key == UINT32_MAX)
            break;
        ++key;
    }
    key = done = 0;
    for (uint32_t* v; (v = pm_next(&X->cache, &key, &done)) != NULL;) {
        const uint32_t c = *v;
        const uint32_t ts = (c & 0x80000000u) ? X->rh[c & 0x7FFFFFFFu].ts : X->R[c - 1].hdr.ts;
        if (!(ts + 6000u < X->max_ts))
            break;
        pm_del(&X->cache, key);
        if (key == UINT32_MAX)
            break;
        ++key;
    }
}

int rx_tables_init(rx_sim* X)
{
    return pm_init(&X->seen) || pm_init(&X->cache) || pm_init(&X->flex_of) || hm_init(&X->shape_of, 64);
}

/* One record of X->R in arrival order: sim_receiver_put /
 * sim_receiver_put_fec and the recovery cascade.  In a sharded batch the
 * record first claims its packet ids for its fec_id. */
void rx_arrival(rx_sim* X, uint32_t a)
{
    const rfec_wire_rec* r = &X->R[a];
    if (r->status != RFEC_WIRE_OK)
        return;
    if (r->mid == RFEC_WIRE_SEG) { /* sim_receiver_put (sim_receiver.c:811-827) */
        if (X->P) /* (a segment outside FEC claims its id for fec_id 0) */
            rx_claim(X, r->hdr.seq, (uint32_t)r->fec_id + 1u);
        if (pm_get(&X->seen, r->hdr.seq))
            return;
        if (rx_put_new(X, 0, r->hdr.seq, 1)) {
            X->oom = 1;
            return;
        }
        if (r->fec_id == 0)
            return;
        const rfec_hdr h = rec_hdr(r);
        rx_put_segment(X, &h, r->fec_id, a + 1, (int32_t)a);
    } else if (r->mid == RFEC_WIRE_FEC) {
        if (X->P)
            rx_claim_range(X, r);
        rx_put_fec(X, a);
    }
    rx_drain(X);
}

/* The control plane over records [a0, a0 + n) of X->R. */
void rx_run(rx_sim* X, uint32_t a0, uint32_t n)
{
    for (uint32_t a = a0; a < a0 + n && !X->oom; ++a)
        rx_arrival(X, a);
}
