/*
 * rfec_rx_map.h -- the receiver control plane's two containers, inlined into
 * their users (pm_get / pm_put are on the per-record path): hmap, an open
 * addressing u32 -> u32 table, and pmap, a radix table over packet ids.
 */
#ifndef RFEC_RX_MAP_H
#define RFEC_RX_MAP_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { /* open addressing u32 -> u32, value 0 = empty */
    uint32_t* k;
    uint32_t* v;
    uint32_t mask, n;
} hmap;

/* Home slot: keys in blocks of 16 (consecutive keys, consecutive slots: one
 * cache line serves several lookups, as packet ids and fec_ids arrive nearly
 * in sequence), the blocks spread by Fibonacci hashing on the table's bit
 * width.  (A multiplicative hash of each key sent every lookup of the c3
 * stream to a new line; the key's low bits alone alias a shard's keys, which
 * take every T-th group, onto a quarter of the table.) */
static inline uint32_t key_home(uint32_t mask, uint32_t k)
{
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(mask); /* log2(capacity), >= 6 */
    return ((((k >> 4) * 0x9E3779B1u) >> (36u - bits)) << 4 | (k & 15u)) & mask;
}
static inline uint32_t hm_home(const hmap* m, uint32_t k) { return key_home(m->mask, k); }

static inline int hm_init(hmap* m, uint32_t n)
{
    uint32_t cap = 64;
    while (cap < 2 * n + 64)
        cap <<= 1;
    m->k = (uint32_t*)malloc(cap * sizeof(uint32_t));
    m->v = (uint32_t*)calloc(cap, sizeof(uint32_t));
    m->mask = cap - 1;
    m->n = 0;
    return m->k && m->v ? 0 : -1;
}
static inline void hm_free(hmap* m)
{
    free(m->k);
    free(m->v);
    m->k = m->v = NULL;
}
static inline uint32_t hm_slot(const hmap* m, uint32_t k)
{
    uint32_t h = hm_home(m, k);
    while (m->v[h] && m->k[h] != k)
        h = (h + 1) & m->mask;
    return h;
}
static inline uint32_t hm_get(const hmap* m, uint32_t k) { return m->v[hm_slot(m, k)]; }
static inline int hm_put(hmap* m, uint32_t k, uint32_t v)
{
    if (2 * (m->n + 1) > m->mask + 1) {
        hmap g;
        if (hm_init(&g, 2 * (m->mask + 1)))
            return -1;
        for (uint32_t i = 0; i <= m->mask; ++i)
            if (m->v[i]) {
                const uint32_t s = hm_slot(&g, m->k[i]);
                g.k[s] = m->k[i];
                g.v[s] = m->v[i];
                g.n++;
            }
        hm_free(m);
        *m = g;
    }
    const uint32_t s = hm_slot(m, k);
    m->n += m->v[s] == 0;
    m->k[s] = k;
    m->v[s] = v;
    return 0;
}
static inline void hm_del(hmap* m, uint32_t k) /* backward-shift deletion */
{
    uint32_t h = hm_slot(m, k);
    if (!m->v[h])
        return;
    m->v[h] = 0;
    m->n--;
    for (uint32_t j = (h + 1) & m->mask; m->v[j]; j = (j + 1) & m->mask)
        if (((j - hm_home(m, m->k[j])) & m->mask) >= ((j - h) & m->mask)) {
            m->k[h] = m->k[j];
            m->v[h] = m->v[j];
            m->v[j] = 0;
            h = j;
        }
}

/* Packet-id maps (first-arrival dedupe, the segment cache, fec_id -> flex,
 * packet-id ownership): u32 key -> u32 value (0 = absent) in a radix table,
 * 14 + 10 + 8 key bits: a directory of mids, a mid of leaves, a leaf of 256
 * values, allocated on first use and freed when empty.  Ids arrive nearly in
 * sequence, so consecutive lookups hit one leaf (the last one is cached): no
 * hashing, no probing, no rehash, and the key order is the walk order (the
 * evictions' sorted walks).  (An open-addressing hash spent 35-70 % of the
 * control plane in probes that missed the cache, and its growth in page
 * faults.)  Each level keeps a bitmap of what is occupied below it, so a walk
 * (pm_next) skips empty directory slots, leaves and values by bit scans: the
 * evictions and compaction walk the open state, not the key space (the
 * directory scan from key 0 was ~30 % of the control plane with an eviction
 * per batch). */
#define PM_LEAF_BITS 8
#define PM_MID_BITS 10
#define PM_DIR_BITS (32 - PM_LEAF_BITS - PM_MID_BITS)
#define PM_LEAF (1u << PM_LEAF_BITS)
#define PM_MID (1u << PM_MID_BITS)
#define PM_DIR (1u << PM_DIR_BITS)
typedef struct {
    uint32_t n;
    uint64_t bits[PM_LEAF / 64]; /* values != 0 */
    uint32_t v[PM_LEAF];
} pm_leaf;
typedef struct {
    pm_leaf* leaf[PM_MID];
    uint64_t bits[PM_MID / 64]; /* leaves present */
    uint32_t nleaf;
} pm_mid;
typedef struct {
    pm_mid** dir; /* [PM_DIR] */
    uint64_t* dbits; /* [PM_DIR / 64]: mids present */
    uint32_t n;   /* entries */
    uint32_t last_pg;
    pm_leaf* last; /* the leaf of page last_pg (key >> PM_LEAF_BITS), or NULL */
} pmap;

static inline int pm_init(pmap* m)
{
    memset(m, 0, sizeof(*m));
    m->dir = (pm_mid**)calloc(PM_DIR, sizeof(pm_mid*));
    m->dbits = (uint64_t*)calloc(PM_DIR / 64, sizeof(uint64_t));
    return m->dir && m->dbits ? 0 : -1;
}

static inline void pm_free(pmap* m)
{
    if (m->dir)
        for (uint32_t d = 0; d < PM_DIR; ++d)
            if (m->dir[d]) {
                for (uint32_t l = 0; l < PM_MID; ++l)
                    free(m->dir[d]->leaf[l]);
                free(m->dir[d]);
            }
    free(m->dir);
    free(m->dbits);
    memset(m, 0, sizeof(*m));
}

static inline pm_leaf* pm_find(pmap* m, uint32_t k)
{
    const uint32_t pg = k >> PM_LEAF_BITS;
    if (m->last && m->last_pg == pg)
        return m->last;
    const pm_mid* d = m->dir[pg >> PM_MID_BITS];
    pm_leaf* f = d ? d->leaf[pg & (PM_MID - 1)] : NULL;
    if (f) {
        m->last = f;
        m->last_pg = pg;
    }
    return f;
}

static inline uint32_t pm_get(pmap* m, uint32_t k)
{
    const pm_leaf* f = pm_find(m, k);
    return f ? f->v[k & (PM_LEAF - 1)] : 0u;
}

static inline int pm_put(pmap* m, uint32_t k, uint32_t v) /* v != 0 */
{
    pm_leaf* f = pm_find(m, k);
    if (!f) {
        const uint32_t pg = k >> PM_LEAF_BITS, di = pg >> PM_MID_BITS, li = pg & (PM_MID - 1);
        pm_mid** d = &m->dir[di];
        if (!*d) {
            if (!(*d = (pm_mid*)calloc(1, sizeof(pm_mid))))
                return -1;
            m->dbits[di >> 6] |= 1ull << (di & 63);
        }
        if (!(f = (pm_leaf*)calloc(1, sizeof(pm_leaf))))
            return -1;
        (*d)->leaf[li] = f;
        (*d)->bits[li >> 6] |= 1ull << (li & 63);
        (*d)->nleaf++;
        m->last = f;
        m->last_pg = pg;
    }
    const uint32_t i = k & (PM_LEAF - 1);
    uint32_t* s = &f->v[i];
    if (*s == 0) {
        f->n++;
        m->n++;
        f->bits[i >> 6] |= 1ull << (i & 63);
    }
    *s = v;
    return 0;
}

static inline void pm_del(pmap* m, uint32_t k)
{
    pm_leaf* f = pm_find(m, k);
    const uint32_t i = k & (PM_LEAF - 1);
    uint32_t* s = f ? &f->v[i] : NULL;
    if (!s || !*s)
        return;
    *s = 0;
    f->bits[i >> 6] &= ~(1ull << (i & 63));
    m->n--;
    if (--f->n == 0) { /* the leaf (and an empty mid) go */
        const uint32_t pg = k >> PM_LEAF_BITS, di = pg >> PM_MID_BITS, li = pg & (PM_MID - 1);
        pm_mid** d = &m->dir[di];
        (*d)->leaf[li] = NULL;
        (*d)->bits[li >> 6] &= ~(1ull << (li & 63));
        free(f);
        if (--(*d)->nleaf == 0) {
            free(*d);
            *d = NULL;
            m->dbits[di >> 6] &= ~(1ull << (di & 63));
        }
        m->last = NULL;
    }
}

/* the first set bit of bits[0, nbits) at or after `from`, or nbits */
static inline uint32_t pm_scan(const uint64_t* bits, uint32_t nbits, uint32_t from)
{
    if (from >= nbits)
        return nbits;
    uint32_t w = from >> 6;
    uint64_t x = bits[w] & (~0ull << (from & 63));
    while (!x) {
        if (++w >= nbits / 64)
            return nbits;
        x = bits[w];
    }
    return w * 64 + (uint32_t)__builtin_ctzll(x);
}

/* In key order: the next entry at or after *key (its value's address, the key
 * in *key), NULL past the last.  Start with *key = 0; continue from key + 1. */
static inline uint32_t* pm_next(const pmap* m, uint32_t* key, uint32_t* done)
{
    uint32_t pg = *key >> PM_LEAF_BITS, i = *key & (PM_LEAF - 1);
    uint32_t di = pg >> PM_MID_BITS, li = pg & (PM_MID - 1);
    if (!m->dir) {
        *done = 1;
        return NULL;
    }
    for (;;) {
        const pm_mid* d = m->dir[di];
        if (!d) { /* the next mid */
            if ((di = pm_scan(m->dbits, PM_DIR, di + 1)) >= PM_DIR)
                break;
            li = i = 0;
            continue;
        }
        pm_leaf* f = d->leaf[li];
        if (f && (i = pm_scan(f->bits, PM_LEAF, i)) < PM_LEAF) {
            *key = (di << (PM_MID_BITS + PM_LEAF_BITS)) | (li << PM_LEAF_BITS) | i;
            return &f->v[i];
        }
        i = 0;
        if ((li = pm_scan(d->bits, PM_MID, li + 1)) < PM_MID)
            continue;
        if ((di = pm_scan(m->dbits, PM_DIR, di + 1)) >= PM_DIR)
            break;
        li = 0;
    }
    *done = 1;
    return NULL;
}
/* for (PM_EACH(m, key, val)) { ... *val ... } -- entries in key order; the body
 * may change *val (not to 0) but not insert or delete */
#define PM_EACH(m, key, val)                                                                        \
    uint32_t key = 0, *val = NULL, pm_d_ = 0;                                                       \
    !pm_d_ && (val = pm_next((m), &key, &pm_d_)) != NULL;                                           \
    key = key == UINT32_MAX ? (pm_d_ = 1, key) : key + 1

#endif
