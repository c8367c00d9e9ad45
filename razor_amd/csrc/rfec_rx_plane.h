/*
 * rfec_rx_plane.h -- the receiver's host control plane over T shards (rfec_rx_plane.c): the sharded replay of
 * a batch with its rollback and merge, the evictions over the union of the shards, the host halves of compaction
 * and of one call's device tables.  Host only: no GPU runtime (the device halves: rfec_rx_dev.c, rfec_rx_session.c).
 */
#ifndef RFEC_RX_PLANE_H
#define RFEC_RX_PLANE_H

#include "rfec_rx_pool.h"
#include "rfec_rx_sim.h"

#pragma GCC visibility push(hidden)

/* The device side of one ingestion call over T shards (one for rfec_rx_recover
 * and a merged session): the shards' deliveries merged in packet-id order, the
 * delivering groups laid out by device shape (the same geometry on several
 * shards is one launch), the line jobs of the large groups. */
typedef struct {
    const rx_shape* sh; /* any shard's shape of this geometry (plans are a function of it) */
    uint32_t n_groups, row0, prow0, group0;
    uint32_t E, dense0; /* dense output slots per group, the shape's first dense row */
} rx_dclass;

typedef struct {
    rx_event* ev;          /* this call's deliveries, all shards, ascending packet id */
    uint32_t nev, evcap;
    uint64_t* dl;          /* delivering groups: shard << 32 | instance */
    uint32_t ndl, dlcap;
    rx_dclass* C;          /* device shapes */
    uint32_t nc, ccap;
    uint32_t* cls;         /* per (shard, shape): its device shape */
    uint32_t clscap;
    rfec_line_job* jobs;   /* groups above RFEC_MAX_K: this call's line jobs (rx_big_peel) */
    uint32_t njobs, jobcap;
    uint16_t* jlevel;      /* a job's dependency level (1 = arrived members only) */
    uint32_t jlevelcap;
    int32_t* jmem;         /* member codes: record >= 0, job j as -1 - j */
    uint32_t njmem, jmemcap;
    uint32_t unmodelled;
    int oom;
} rx_dev;

/* a line fires at most once, so a chain is at most as deep as a group has lines (256 FEC indices) */
#define RX_MAX_LEVEL 256u

/* A group whose device recovery runs as the host peel's line jobs: above
 * RFEC_MAX_K segments (the batched peel's masks hold 128 members), or a huge
 * shape of any count (no device plan: more than RFEC_MAX_LINES lines, e.g. a
 * peer's 128-segment flex of 64 rows x 2 columns, or one rx_extend took past
 * 64 lines; its parity rows sit at a 256-line stride). */
static inline int rx_line_jobs(const rx_shape* sh) { return sh->count > RFEC_MAX_K || sh->huge; }

/* The device tables of one call (rx_device), for the delivering groups and
 * the deliveries of shard t (UINT32_MAX: all): member and parity row maps,
 * header records, masks, sizes, and each delivery's output row -- the
 * recovering group's dense slot (its rank among the group's erased members)
 * or the line job that recovers it.  Sharded sessions fill them on the
 * replay threads, each over the state its own thread wrote. */
typedef struct {
    rx_sim* const* XS;
    const rx_dev* D;
    const uint32_t* sbase; /* per shard: its first entry in D->cls */
    const int32_t* job_of;
    int32_t* map;
    rfec_hdr *hh, *mh;
    uint16_t* fsz;
    uint64_t *pres, *ppm;
    int32_t* omap;
    uint32_t r_job, r_par, r_dense;
} rx_tabs;

/* One call's device tables as rx_plan lays them out: rows on the device in one region, [nrows members][njobs
 * line-job outputs][prows parities][ndense]; o_*: offsets into the pinned tables (staged to the device at the
 * same offsets up to o_in_end), d_*: into the device workspace. */
typedef struct {
    uint32_t sbase[RX_MAX_THREADS + 1]; /* per shard: its first entry in D->cls */
    uint32_t nrows, prows, ngs, ndense, nmap, r_job, r_par, r_dense;
    uint32_t maxlvl, lvl_n[RX_MAX_LEVEL + 1]; /* line jobs per dependency level (jobs sorted by level) */
    size_t o_map, o_hdr, o_meta, o_fs, o_pres, o_pp, o_omap, o_jobs, o_jmem, o_in_end, o_rec, host_bytes;
    size_t d_rows, d_ws, d_ohdr, d_oidx, d_out, dev_bytes;
    int32_t* job_of; /* per member of the large groups: the job recovering it, or -1 (the caller frees it) */
} rx_layout;

#define RX_ALIGN(x) (((x) + 255) & ~(size_t)255)
#define RX_CLASS(D, sbase, t, g) (&(D)->C[(D)->cls[(sbase)[t] + (g)->shape] - 1])

/* The host half of one call's device side: D and L from the shards'
 * deliveries (D->nev == 0: nothing recovered, no device work).  RFEC_OK, or
 * an error code with rfec_last_error set (L->job_of is NULL then). */
int rx_plan(rx_sim* const* XS, uint32_t T, rx_dev* D, uint32_t stride, rx_layout* L);
void rx_fill(const rx_tabs* A, uint32_t only);
void rx_fill_job(void* arg, uint32_t t); /* rx_fill(arg, t) for pool_run */
void rx_dev_free(rx_dev* D);

/* The sharded plane of a session: the shards (fec_id % T; T = 1: one serial
 * state), the replay threads, the packet-id owner tables, one batch's lists. */
typedef struct {
    rx_sim* XS[RX_MAX_THREADS];
    uint32_t T;
    uint32_t max_ts;            /* sim_receiver_fec_t.max_ts, over the shards */
    uint32_t prefetch;          /* records a shard's replay prefetches ahead (RFEC_RX_PREFETCH, default 16,
                                   0..64), read by rx_shards_init */
    rx_pool pool;
    int pool_on;
    pmap vown[RX_MAX_THREADS];  /* sharded: packet id -> fec_id + 1, partition (seq >> 8) % T */
    int vown_on;
    rx_par par;
    uint8_t* pshard;            /* per batch record: its shard (0xFF: no control-plane effect) */
    uint32_t* lst;              /* per shard, its records of the batch in arrival order */
    uint32_t* smin;
    uint32_t lcap;
    uint32_t loff[RX_MAX_THREADS + 1];
    uint8_t shard_of[65536];    /* fec_id % T (no division per record) */
    uint32_t n_parallel, n_serial, n_rollback; /* batches by replay (rfec_rx_session_info) */
    double t_split, t_replay, t_verify, t_tables, t_compact; /* host time split (rfec_rx_session_info) */
} rx_plane;

/* T empty shards of payload capacity `capacity` (and, for T > 1, the replay threads); -1: no memory */
int rx_shards_init(rx_plane* P, uint32_t T, uint32_t capacity);
void rx_plane_free(rx_plane* P); /* threads, shards, owner tables, batch lists */
/* The control plane over records [a0, a0 + n) of R (every shard's records
 * from here on); `sum`: the batch's split summary, or NULL (split here). */
int rx_ingest(rx_plane* P, const rfec_wire_rec* R, uint32_t a0, uint32_t n, const rfec_rx_split* sum);
int rx_plane_evict(rx_plane* P); /* sim_fec_evict over the union of the shards */

/* Compaction, host halves.  rx_compact_mark reads the shards only: it marks the records the open state refers
 * to (K->nr of them) and allocates every host table the renumbering needs.  After the caller has every device
 * allocation too, rx_compact_renumber (which cannot fail) renumbers the shards' records in arrival order and
 * fills K->gmap: new row -> old row, the `tail` rows of a pending batch behind the kept ones. */
typedef struct {
    rx_inst* NG;
    int32_t* nsrc;
    rfec_hdr* nhdr;
    int32_t* npar;
    uint32_t* hmap_; /* old rh -> new + 1 */
    uint32_t ng, ns, nl, nh;
} rx_kept;
typedef struct {
    rx_kept K[RX_MAX_THREADS];
    uint32_t* rmap; /* old record -> new + 1 */
    uint32_t* gmap; /* [nr + tail] */
    uint32_t nr;
} rx_compaction;
int rx_compact_mark(const rx_plane* P, uint32_t nstore, uint32_t tail, rx_compaction* K);
void rx_compact_renumber(rx_plane* P, uint32_t nstore, uint32_t tail, rx_compaction* K);
void rx_compact_free(rx_compaction* K);

#pragma GCC visibility pop

#endif
