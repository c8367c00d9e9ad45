/*
 * rfec_rx_sim.h -- one shard of the receiver's arrival-order control plane
 * (rfec_rx_sim.c): the reference's sim_fec.c:104-241 / flex_fec_receiver.c:
 * 69-280 over headers, with the journal that rolls a batch back and the
 * packet-id claims of a sharded session.  Host only: no GPU runtime.
 */
#ifndef RFEC_RX_SIM_H
#define RFEC_RX_SIM_H

#include <stdint.h>

#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_rx_map.h"

#pragma GCC visibility push(hidden)

typedef struct {
    uint32_t count, row, col, n_groups, n_lines, row0, prow0, group0;
    uint32_t huge;        /* count > RX_MAX_COUNT or more than RFEC_MAX_LINES lines: no plan; line l = FEC
                             index l (members by rx_line_members), n_lines 256, peeled by the host into
                             line jobs (rx_big_peel) */
    uint64_t xcol[2];     /* columns c >= col a peer's parities named (bit c) */
    int16_t line_of[256]; /* FEC index -> plan line, -1: none */
    rfec_plan plan;
} rx_shape;

/* one flex receiver (flex_fec_receiver_t) from its creation to its removal */
typedef struct {
    uint32_t fec_id, base, count, row, col;
    uint32_t shape;        /* UINT32_MAX: geometry the reference ignores (col < 2, row 0, count 0) */
    uint32_t gslot, slot0, line0;
    uint32_t nsegs;        /* flex->segs.n */
    uint64_t have[4];      /* members in the flex (arrived or recovered); huge shapes: rx_has */
    uint64_t arrived[4];   /* members that arrived: the device peel starts from these (huge: slot_src) */
    uint64_t ppm;          /* registered parities, by plan line (huge: line_par >= 0) */
    uint32_t fec_ts;       /* flex->fec_ts = send_ts of the parity that created it (sim_fec.c:157) */
    int ref_ok;            /* col >= 2 && row >= 1 && count >= 1 (flex_fec_receiver.c:214, 250) */
    uint32_t gstamp;       /* == rx_sim.epoch: gslot is this device call's group slot */
    uint32_t jstamp;       /* == rx_sim.jepoch: saved in this batch's journal (rx_touch) */
} rx_inst;

typedef struct {
    rfec_hdr hdr;
    uint32_t inst;
    uint32_t shard; /* rx_device's merged list: the shard holding inst */
} rx_event; /* a recovered segment: pending, then delivered */

/* ------------------------------------------------------------------------ */
/* Sharded sessions (rfec_rx_session_*): the control plane partitioned by     */
/* fec_id over T shards, each a full rx_sim replayed by its own thread in     */
/* arrival order.  Groups are independent in the reference (the receiver     */
/* keys a flex by fec_id, sim_fec.c:141-207), and every other piece of       */
/* state is keyed by packet id: first-arrival dedupe, the segment cache a    */
/* new flex replays (sim_fec.c:121-138), the recovered-id map (:104-119).    */
/* Those stay inside one shard as long as every packet id belongs to one     */
/* fec_id -- its segments carry it, the parity ranges [base_id, base_id +    */
/* count) claim it, and recovery stays inside its flex's range -- which is  */
/* checked after each batch (each shard logs its claims; T threads insert    */
/* them into the owner tables, partitioned by packet-id block, so no two     */
/* threads write one table; recovery ranges as they happen).  The one global */
/* quantity is max_ts, which gates the 3 s parity drop (sim_fec.c:148): a    */
/* batch runs in parallel only when no parity can be dropped by it (its      */
/* send_ts + 3000 >= every earlier segment timestamp of the batch, checked   */
/* before the replay, and >= every segment recovered before it, checked as   */
/* recoveries happen).  A batch that breaks either rule is rolled back       */
/* (journal below) and replayed in arrival order: over the shards with one   */
/* max_ts, or, when a packet id crossed fec_ids, after merging the shards    */
/* into one (the session then stays serial).                                */
/* ------------------------------------------------------------------------ */
#define RX_MAX_THREADS 64 /* shards (= replay threads) of a session */
#define RX_CONFLICT_OWNER 1
#define RX_CONFLICT_TS 2
#define RX_CONFLICT_RISKY 4 /* a parity of the batch could meet the 3 s drop (found by the replay threads) */

typedef struct { /* one batch's parallel replay, shared by the shards */
    uint32_t T;           /* shards */
    const uint32_t* smin; /* [n]: min over the batch's later parities of send_ts + 3000 (by batch position);
                             NULL: each shard computes its own from `sum` */
    const rfec_rx_split* sum; /* the batch's split summary (k_rx_split), or NULL (host lists) */
    uint32_t n, max0;     /* the batch's records; max_ts at its start */
    uint32_t a0;          /* the batch's first record */
    int ts_check;         /* recoveries checked against smin (the parallel replay) */
    int conflict;         /* RX_CONFLICT_* (atomic) */
    double t0;            /* the replay's start (now_us), for the per-shard timings */
} rx_par;

typedef struct {
    uint8_t map; /* 0 seen, 1 cache, 2 flex_of, 3 shape_of */
    uint32_t key, old; /* old value, 0 = absent */
} rx_jop;

typedef struct {
    const rfec_wire_rec* R;
    uint32_t capacity, max_ts, dropped, unmodelled;
    pmap seen, cache, flex_of; /* packet id -> 1; packet id -> record + 1 | 0x80000000 + rh index; fec_id -> instance + 1 */
    hmap shape_of;
    rx_inst* G;
    uint32_t ng, gcap;
    rx_shape* S;
    uint32_t ns, scap;
    int32_t* slot_src; /* record of an arrived member, -1 otherwise */
    rfec_hdr* slot_hdr;
    uint32_t nslot, slotcap, slothcap; /* one count, two capacities (each array grows on its own) */
    int32_t* line_par; /* record of the registered parity, -1 otherwise */
    uint32_t nline, linecap;
    rx_event* pend;
    uint32_t npend, pendcap;
    rx_event* out;         /* delivered by this call */
    uint32_t nout, outcap;
    rfec_hdr* rh;          /* headers of delivered (recovered) segments the cache refers to */
    uint32_t nrh, rhcap;
    uint32_t epoch;        /* device call counter (rx_inst.gstamp) */
    int oom;
    /* sharded sessions: the batch's shared context, and the journal that rolls
       this shard back to the batch's start (map operations, the instances the
       batch touched -- saved on first touch with their slot / line tables --,
       and the tables' lengths) */
    rx_par* P;
    uint32_t smin_cur;  /* smin of the record being replayed (parallel replay) */
    uint32_t* mine;     /* this shard's records of the batch (the device's split), and their smin */
    uint32_t* mine_sm;
    uint32_t minecap;
    /* the batch split of chunk t of the summary (rx_split_job, on this shard's thread): the chunk's
       positions grouped by shard in arrival order (cof: per-shard offsets), each with the chunk-local
       min over later parities of send_ts + 3000; the chunk's largest segment timestamp, smallest parity
       limit, and whether a parity meets a segment timestamp before it inside the chunk */
    uint32_t *cpos, *csm;
    uint32_t ccap;
    uint32_t cof[RX_MAX_THREADS + 1];
    uint32_t c_maxseg, c_minfec;
    int c_flag;
    uint64_t* claims;   /* this batch's packet-id claims: seq << 32 | fec_id + 1 */
    uint32_t nclaims, claimcap;
    uint64_t* cpart;    /* the claims by owner-table partition (rx_bucket_claims), offsets in coff */
    uint32_t cpartcap;
    uint32_t coff[RX_MAX_THREADS + 1];
    uint32_t* claimed;  /* [65536 / T + 1][2]: the range last claimed per fec_id / T (base, count + 1) */
    int jon;
    uint32_t jepoch, j_ng, j_nslot, j_nline, j_ns, j_nrh, j_max_ts, j_dropped, j_unmod;
    rx_jop* jops;
    uint32_t njops, jopcap;
    uint8_t* jsave;
    size_t njsave, jsavecap;
    double tw_wake, tw_run, tw_pre; /* parallel replays: this shard's start after the replay's, its run and the
                                       part of it before the first arrival (us, summed) */
    double tw_start;
    uint32_t tw_n, tw_recs;
} rx_sim;

#define RX_GROW_F(flag, ptr, n, cap, need, T)                                          \
    do {                                                                                \
        if ((n) + (need) > (cap)) {                                                     \
            uint32_t c_ = (cap) ? 2 * (cap) : 1024;                                     \
            while (c_ < (n) + (need))                                                   \
                c_ *= 2;                                                                \
            T* p_ = (T*)realloc((ptr), (size_t)c_ * sizeof(T));                         \
            if (!p_) {                                                                  \
                (flag) = 1;                                                             \
                break;                                                                  \
            }                                                                           \
            (ptr) = p_;                                                                 \
            (cap) = c_;                                                                 \
        }                                                                               \
    } while (0)
#define RX_GROW(ptr, n, cap, need, T) RX_GROW_F(X->oom, ptr, n, cap, need, T)

static inline pmap* rx_map(rx_sim* X, int m) /* 0 seen, 1 cache, 2 flex_of (3: shape_of, a hash map) */
{
    return m == 0 ? &X->seen : m == 1 ? &X->cache : &X->flex_of;
}
/* one member's header into a line's XOR (flex_fec_xor.c:64-99) */
static inline void rx_hdr_xor(rfec_hdr* h, const rfec_hdr* m)
{
    h->seq ^= m->seq, h->fid ^= m->fid, h->ts ^= m->ts, h->index ^= m->index, h->total ^= m->total;
    h->ftype ^= m->ftype, h->payload_type ^= m->payload_type, h->size ^= m->size;
}
static inline void rx_conflict(rx_sim* X, int what) { __atomic_fetch_or(&X->P->conflict, what, __ATOMIC_RELAXED); }

int rx_tables_init(rx_sim* X);
void rx_sim_free(rx_sim* X);
/* the journal (sharded sessions): begin before a batch that may roll back */
void rx_journal_begin(rx_sim* X);
void rx_journal_end(rx_sim* X);
void rx_rollback(rx_sim* X);
void rx_bucket_claims(rx_sim* X, uint32_t T);
uint32_t rx_line(const rx_sim* X, const rx_inst* g, uint32_t l, uint32_t* first, uint32_t* stride, int* reg);
void rx_arrival(rx_sim* X, uint32_t a);
void rx_run(rx_sim* X, uint32_t a0, uint32_t n);
void rx_remove(rx_sim* X, uint32_t ii);
void rx_evict(rx_sim* X);

#pragma GCC visibility pop

#endif
