// rfec_peel.hip -- the generic recover of the flex-FEC engine (gfx950): the LDS peel and the schedule replay,
// with their launchers; rfec_kernels.hip picks it (rfec_launch_recover[_out], rfec_launch_recover_indexed).
//
// Arithmetic restated from the reference (yuanrongxi/razor):
//   recovery        = parity ^ XOR of present members      flex_fec_xor.c:64-95
//   peeling order / conditions                             flex_fec_receiver.c:105-206
//  Where no one-launch form applies (and RFEC_TUNE_GENERIC): k_peel_lds (schedule records) + k_recover_flat
//  (replay); through a slot map over a row pool, every plan but the row layouts: k_peel_lds + k_recover_indexed.
#include "rfec_families.h"

namespace {

// ---------------------------------------------------------------------------
// Recover.
//
// Peeling = the fixpoint reached by flex_recover_row / flex_recover_col
// (flex_fec_receiver.c:105-206) as segments, parities and recovered segments
// (sim_receiver.c:780-804) arrive; canonical order: lines in plan order,
// repeated until nothing fires.  A line fires when its parity is present,
// exactly one member is missing, at least one is present (:133-140,
// :189-196) and flex_fec_recover would succeed: fec_data_size within the
// capacity, every member's data_size <= fec_data_size (flex_fec_xor.c:88-89)
// and the recovered data_size <= fec_data_size (:98-99).
//
// Two-kernel form (generic): k_peel_lds runs that peel, one lane per group,
// over the group's headers / line metadata staged in LDS by coalesced dword
// loads, and writes the recovered headers and a schedule record per group:
//   byte 0 = steps, byte 1 = 1 when no step reads a segment recovered by an
//   earlier step (single level), then (line, target) byte pairs.
// k_recover_flat: one lane per (group, 16-B chunk column) replays the record;
// single-level schedules run BATCH steps with every load in flight at once.
// ---------------------------------------------------------------------------
constexpr int kPeelDwords = 8192; // 32 KiB of LDS per peel block

// One peel block: groups [blk*gpb, ...), one lane per group, records staged in
// LDS.  Dense output (out_per_group = E > 0): only erased segments of rank < E
// are targets; their headers go to out_hdr, the out_index row is written.
template <int LDSD>
__device__ void peel_block(const PeelArgs& A, const rfec_kmask& M, uint32_t blk)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[LDSD];
    const rfec_kplan& P = M.plan;
    const uint32_t K = P.k, NL = P.n_lines;
    const uint32_t g0 = blk * A.gpb;
    const uint32_t ng = min(A.gpb, A.groups - g0);
    const uint32_t g = g0 + threadIdx.x;
    // this lane's masks first, so their latency overlaps the staging below
    uint64_t have0 = 0, have1 = 0, ppm = 0;
    if (threadIdx.x < ng) {
        have0 = A.present[2 * g];
        have1 = A.present[2 * g + 1];
        ppm = A.parity_present[g];
    }
    const uint32_t nh = ng * K * 5, nm = ng * NL * 5, nf = ng * NL;
    uint32_t* Lh = lds;                            // [ng][K][5]
    uint32_t* Lm = Lh + ((nh + 3) & ~3u);          // [ng][NL][5]
    uint16_t* Lf = reinterpret_cast<uint16_t*>(Lm + ((nm + 3) & ~3u)); // [ng][NL]
    stage_dwords(Lh, reinterpret_cast<const uint32_t*>(A.hdr + (size_t)g0 * K), nh);
    stage_dwords(Lm, reinterpret_cast<const uint32_t*>(A.meta + (size_t)g0 * NL), nm);
    const uint16_t* fsrc = A.fsize + (size_t)g0 * NL;
    if ((reinterpret_cast<uintptr_t>(fsrc) & 3) == 0) {
        stage_dwords(reinterpret_cast<uint32_t*>(Lf), reinterpret_cast<const uint32_t*>(fsrc), nf / 2);
        if ((nf & 1) && threadIdx.x == 0)
            Lf[nf - 1] = fsrc[nf - 1];
    } else {
        for (uint32_t i = threadIdx.x; i < nf; i += kBlock)
            Lf[i] = fsrc[i];
    }
    __syncthreads();
    if (threadIdx.x >= ng)
        return;
    uint32_t* h = Lh + threadIdx.x * K * 5;
    const uint32_t* m = Lm + threadIdx.x * NL * 5;
    const uint16_t* f = Lf + threadIdx.x * NL;
    uint64_t rec0 = 0, rec1 = 0;
    uint8_t* rec = A.sched + (size_t)g * A.rec_bytes;
    uint32_t n = 0, single = 1;
    const uint32_t E = A.out_per_group;
    const uint64_t er0 = ~have0, er1 = ~have1; // erased (rank order of the dense output)
    // with pairwise-disjoint lines (e.g. the row layer alone) a recovery can
    // never complete another line, so one pass reaches the fixpoint
    bool progress = true;
    for (uint32_t pass = 0; progress && !(A.disjoint && pass > 0); ++pass) {
        progress = false;
        for (uint32_t l = 0; l < NL; ++l) {
            if (!((ppm >> l) & 1ull))
                continue;
            const uint64_t m0 = M.mask[l][0], m1 = M.mask[l][1];
            const uint64_t x0 = m0 & ~have0, x1 = m1 & ~have1;
            if (__popcll(x0) + __popcll(x1) != 1)
                continue;
            if (((m0 & have0) | (m1 & have1)) == 0)
                continue;
            const uint32_t t = x0 ? (uint32_t)__ffsll((long long)x0) - 1
                                  : 64u + (uint32_t)__ffsll((long long)x1) - 1;
            const uint32_t L = f[l];
            if (L > A.capacity || (E && missing_rank(~er0, ~er1, t) >= E))
                continue;
            uint32_t r0 = m[l * 5], r1 = m[l * 5 + 1], r2 = m[l * 5 + 2], r3 = m[l * 5 + 3], r4 = m[l * 5 + 4];
            bool ok = true;
            const bool reads_recovered = ((m0 & rec0) | (m1 & rec1)) != 0;
            const rfec_line ln = P.line[l];
            for (uint32_t q = 0; q < ln.count; ++q) {
                const uint32_t i = ln.first + q * ln.stride;
                if (i == t)
                    continue;
                const uint32_t* r = h + i * 5;
                r0 ^= r[0];
                r1 ^= r[1];
                r2 ^= r[2];
                r3 ^= r[3];
                r4 ^= r[4];
                ok = ok && (r[4] >> 16) <= L;
            }
            if (!ok || (r4 >> 16) > L)
                continue;
            uint32_t* ht = h + t * 5;
            ht[0] = r0, ht[1] = r1, ht[2] = r2, ht[3] = r3, ht[4] = r4;
            uint32_t* gh = E ? reinterpret_cast<uint32_t*>(A.out_hdr + (size_t)g * E + missing_rank(~er0, ~er1, t))
                             : reinterpret_cast<uint32_t*>(A.hdr + (size_t)g * K + t);
            gh[0] = r0, gh[1] = r1, gh[2] = r2, gh[3] = r3, gh[4] = r4;
            rec[2 + 2 * n] = (uint8_t)l;
            rec[3 + 2 * n] = (uint8_t)t;
            ++n;
            if (reads_recovered)
                single = 0;
            if (t < 64) {
                have0 |= 1ull << t;
                rec0 |= 1ull << t;
            } else {
                have1 |= 1ull << (t - 64);
                rec1 |= 1ull << (t - 64);
            }
            progress = true;
        }
    }
    rec[0] = (uint8_t)n;
    rec[1] = (uint8_t)single;
    A.recovered[2 * g] = rec0;
    A.recovered[2 * g + 1] = rec1;
    if (E) { // out_index: the e-th erased segment's index where it was recovered, else 0xFF
        const uint64_t km0 = K >= 64 ? ~0ull : (1ull << K) - 1ull;
        const uint64_t km1 = K <= 64 ? 0ull : (K >= 128 ? ~0ull : (1ull << (K - 64)) - 1ull);
        uint64_t e0 = er0 & km0, e1 = er1 & km1;
        for (uint32_t e = 0; e < E; ++e) {
            uint32_t v = 0xFF;
            if (e0 | e1) {
                const uint32_t i = e0 ? (uint32_t)__ffsll((long long)e0) - 1 : 64u + (uint32_t)__ffsll((long long)e1) - 1;
                if (has_bit(rec0, rec1, i))
                    v = i;
                if (e0)
                    e0 &= e0 - 1;
                else
                    e1 &= e1 - 1;
            }
            A.out_index[(size_t)g * E + e] = (uint8_t)v;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_peel_lds(PeelArgs A, rfec_kmask M)
{
    peel_block<kPeelDwords>(A, M, blockIdx.x);
}

__device__ __forceinline__ uint32_t rec_byte(const v4u& r, uint32_t b)
{
    return (r[b >> 2] >> (8 * (b & 3))) & 0xffu;
}

// Replays one group's schedule record over one chunk column: grp / par point
// at chunk j of the group's segment / parity slots, r0 = first 16 record bytes.
// Dense output (out != nullptr, the group's first out slot at chunk j): a
// recovered segment goes to out slot rank(t) (h0 / h1: the received masks),
// and a later step reads it back from there (same lane, same address, in order).
template <int MAXC, int BATCH>
__device__ __forceinline__ void replay(v4u* grp, const v4u* __restrict__ par, const uint8_t* __restrict__ rec,
                                       const v4u r0, uint32_t C, uint32_t fast_ok, const uint32_t* lplan,
                                       v4u* out, uint64_t h0, uint64_t h1)
{
    const uint32_t n = rec_byte(r0, 0);
    uint32_t s = 0;
    if (fast_ok && rec_byte(r0, 1)) {
        // single level: BATCH steps at a time, all loads in flight together
        const uint32_t nf = n < 7 ? n : 7; // steps carried in the first 16 record bytes
        for (; s < nf; s += BATCH) {
            // (unconditional loads, see k_decode_rows; an off step re-reads
            // the first step's parity chunk)
            v4u acc[BATCH], mv[BATCH][MAXC];
            uint32_t tg[BATCH], l0 = 0;
            bool on[BATCH], use[BATCH][MAXC];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                on[b] = s + b < nf;
                const uint32_t l = on[b] ? rec_byte(r0, 2 + 2 * (s + b)) : l0;
                l0 = l;
                tg[b] = rec_byte(r0, 3 + 2 * (s + b));
                const uint32_t ln = lplan[l];
                const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
                const v4u* pl = par + (size_t)l * C;
                acc[b] = ld16(pl);
                const ptrdiff_t to_par = pl - grp;
#pragma unroll
                for (int q = 0; q < MAXC; ++q) {
                    const uint32_t i = first + q * stride;
                    use[b][q] = on[b] && (uint32_t)q < count && i != tg[b];
                    mv[b][q] = ld16(grp + (use[b][q] ? (ptrdiff_t)i * C : to_par));
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
#pragma unroll
                for (int q = 0; q < MAXC; ++q)
                    acc[b] ^= use[b][q] ? mv[b][q] : v4u{0, 0, 0, 0};
                if (on[b])
                    st16(out ? out + (size_t)missing_rank(h0, h1, tg[b]) * C : grp + (size_t)tg[b] * C, acc[b]);
            }
        }
        s = nf;
    }
    // remaining / multi-level steps, one at a time in schedule order (a step
    // reads what this lane stored before: same address, same lane, in order)
    for (; s < n; ++s) {
        const uint32_t l = s < 7 ? rec_byte(r0, 2 + 2 * s) : rec[2 + 2 * s];
        const uint32_t tt = s < 7 ? rec_byte(r0, 3 + 2 * s) : rec[3 + 2 * s];
        const uint32_t ln = lplan[l];
        const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
        v4u acc = ld16(par + (size_t)l * C);
        for (uint32_t q = 0; q < count; ++q) {
            const uint32_t i = first + q * stride;
            if (i != tt)
                acc ^= (out && !has_bit(h0, h1, i)) ? out[(size_t)missing_rank(h0, h1, i) * C] : grp[(size_t)i * C];
        }
        st16(out ? out + (size_t)missing_rank(h0, h1, tt) * C : grp + (size_t)tt * C, acc);
    }
}

template <int MAXC, int BATCH>
__global__ __launch_bounds__(kBlock) void k_recover_flat(v4u* shards, const v4u* __restrict__ parity,
                                                         const uint8_t* __restrict__ sched, uint32_t total,
                                                         uint32_t C, FastDiv divC, uint32_t rec_bytes,
                                                         uint32_t fast_ok, rfec_kplan P, DenseOut D,
                                                         const uint64_t* __restrict__ present)
{
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    stage_plan(lplan, P);
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divC);
    const uint32_t j = t - g * divC.d; // chunk column (divC.d = chunks of work per slot)
    const uint8_t* rec = sched + (size_t)g * rec_bytes;
    const v4u r0 = *reinterpret_cast<const v4u*>(rec);
    v4u* out = D.E ? D.sh + (size_t)g * D.E * C + j : nullptr;
    const uint64_t h0 = D.E ? present[2 * g] : 0ull, h1 = D.E ? present[2 * g + 1] : 0ull;
    replay<MAXC, BATCH>(shards + (size_t)g * P.k * C + j, parity + (size_t)g * P.n_lines * C + j, rec, r0, C,
                        fast_ok, lplan, out, h0, h1);
}

// The replay of rfec_recover_indexed_out: k_recover_flat's, dense output only, with member i of the group read
// from row so[i] of the pool and parity line l from row so[K + l] (so: the group's K + NL words of src_of, rows:
// chunk j of row 0).  A row index is clamped to `last` = n_rows - 1 before it is used, so a broken map reads
// other rows, never past the pool; row addresses are 64-bit.  Only the entries of slots a step reads are loaded
// (present members and received parities); a step reads an earlier step's result from the dense out slot.
template <int MAXC, int BATCH>
__device__ __forceinline__ void replay_indexed(const v4u* rows, const uint32_t* __restrict__ so, uint32_t K,
                                               uint32_t last, const uint8_t* __restrict__ rec, const v4u r0,
                                               uint32_t C, uint32_t fast_ok, const uint32_t* lplan, v4u* out,
                                               uint64_t h0, uint64_t h1)
{
    const uint32_t n = rec_byte(r0, 0);
    uint32_t s = 0;
    if (fast_ok && rec_byte(r0, 1)) {
        const uint32_t nf = n < 7 ? n : 7;
        for (; s < nf; s += BATCH) {
            // (unconditional loads: the map words of a batch first, then its rows; an unused member and an off
            // step re-read a parity chunk of the batch)
            v4u acc[BATCH], mv[BATCH][MAXC];
            const v4u* src[BATCH][MAXC + 1];
            uint32_t tg[BATCH], l0 = 0;
            bool on[BATCH], use[BATCH][MAXC];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                on[b] = s + b < nf;
                const uint32_t l = on[b] ? rec_byte(r0, 2 + 2 * (s + b)) : l0;
                l0 = l;
                tg[b] = rec_byte(r0, 3 + 2 * (s + b));
                const uint32_t ln = lplan[l];
                const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
                src[b][MAXC] = pool_row(rows, so, K + l, last, C);
#pragma unroll
                for (int q = 0; q < MAXC; ++q) {
                    const uint32_t i = first + q * stride;
                    use[b][q] = on[b] && (uint32_t)q < count && i != tg[b];
                    src[b][q] = pool_row(rows, so, use[b][q] ? i : K + l, last, C);
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                acc[b] = ld16(src[b][MAXC]);
#pragma unroll
                for (int q = 0; q < MAXC; ++q)
                    mv[b][q] = ld16(src[b][q]);
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
#pragma unroll
                for (int q = 0; q < MAXC; ++q)
                    acc[b] ^= use[b][q] ? mv[b][q] : v4u{0, 0, 0, 0};
                if (on[b])
                    st16(out + (size_t)missing_rank(h0, h1, tg[b]) * C, acc[b]);
            }
        }
        s = nf;
    }
    for (; s < n; ++s) {
        const uint32_t l = s < 7 ? rec_byte(r0, 2 + 2 * s) : rec[2 + 2 * s];
        const uint32_t tt = s < 7 ? rec_byte(r0, 3 + 2 * s) : rec[3 + 2 * s];
        const uint32_t ln = lplan[l];
        const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
        v4u acc = ld16(pool_row(rows, so, K + l, last, C));
        for (uint32_t q = 0; q < count; ++q) {
            const uint32_t i = first + q * stride;
            if (i != tt)
                acc ^= !has_bit(h0, h1, i) ? out[(size_t)missing_rank(h0, h1, i) * C] : *pool_row(rows, so, i, last, C);
        }
        st16(out + (size_t)missing_rank(h0, h1, tt) * C, acc);
    }
}

template <int MAXC, int BATCH>
__global__ __launch_bounds__(kBlock) void k_recover_indexed(const v4u* rows, uint32_t last,
                                                            const uint32_t* __restrict__ src_of,
                                                            const uint8_t* __restrict__ sched, uint32_t total,
                                                            uint32_t C, FastDiv divC, uint32_t rec_bytes,
                                                            uint32_t fast_ok, rfec_kplan P, DenseOut D,
                                                            const uint64_t* __restrict__ present)
{
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    stage_plan(lplan, P);
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divC);
    const uint32_t j = t - g * divC.d; // chunk column (divC.d = chunks of work per slot)
    const uint8_t* rec = sched + (size_t)g * rec_bytes;
    const v4u r0 = *reinterpret_cast<const v4u*>(rec);
    replay_indexed<MAXC, BATCH>(rows + j, src_of + (size_t)g * (P.k + P.n_lines), P.k, last, rec, r0, C, fast_ok,
                                lplan, D.sh + (size_t)g * D.E * C + j, present[2 * g], present[2 * g + 1]);
}

} // namespace

PeelGeom peel_args(PeelArgs* B, const rfec_kmask& M, uint32_t groups, uint32_t capacity, rfec_hdr* hdr,
                   const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                   const uint64_t* parity_present, uint64_t* recovered, void* ws, const rfec_dense_out* out)
{
    const rfec_kplan& P = M.plan;
    const bool dense = out && out->per_group;
    PeelGeom g = {1, 0, 0};
    uint64_t seen0 = 0, seen1 = 0;
    for (uint32_t l = 0; l < P.n_lines; ++l) {
        if ((seen0 & M.mask[l][0]) | (seen1 & M.mask[l][1]))
            g.disjoint = 0;
        seen0 |= M.mask[l][0];
        seen1 |= M.mask[l][1];
        g.maxc = P.line[l].count > g.maxc ? P.line[l].count : g.maxc;
    }
    // LDS per group: K + NL header records (5 dwords) + NL u16 sizes; block
    // ranges start on 8-group boundaries so the staged slices are 16-B aligned
    const uint32_t per = 5u * P.k + 6u * P.n_lines;
    // (at most 64 groups per block: the peel is one serial chain per lane, so
    // more, smaller blocks give each SIMD more chains to interleave)
    uint32_t gpb = (kPeelDwords - 8) / per;
    gpb = gpb > 64u ? 64u : gpb;
    if (gpb >= 8)
        gpb &= ~7u;
    g.gpb = gpb < 1 ? 1 : gpb;
    // (in the order of PeelArgs' fields; no header lanes, no packed records)
    *B = PeelArgs{hdr, present, meta, fsize, parity_present, recovered, reinterpret_cast<uint8_t*>(ws),
                  groups, capacity, g.gpb, rfec_sched_record_bytes(P.k, P.n_lines), g.disjoint, /* nlp_log2 */ 0,
                  dense ? out->hdr : nullptr, dense ? out->index : nullptr, dense ? out->per_group : 0u,
                  /* packed, pk_stride, pk_slot */ nullptr, 0, 0};
    return g;
}

void launch_peel(const PeelArgs& B, const rfec_kmask& M, hipStream_t st)
{
    RFEC_LAUNCH(k_peel_lds, dim3((B.groups + B.gpb - 1) / B.gpb), dim3(kBlock), 0, st, B, M);
}

void launch_replay_flat(const PeelArgs& B, const rfec_kplan& P, v4u* shards, const v4u* parity, uint32_t C,
                        uint32_t cd, uint32_t maxc, const DenseOut& D, hipStream_t st)
{
    const uint32_t total = B.groups * cd, fast = maxc <= 8 ? 1u : 0u;
    const dim3 grid(blocks_for(total));
    if (maxc <= 4)
        RFEC_LAUNCH((k_recover_flat<4, 2>), grid, dim3(kBlock), 0, st, shards, parity, B.sched, total, C,
                    make_fastdiv(cd), B.rec_bytes, fast, P, D, B.present);
    else
        RFEC_LAUNCH((k_recover_flat<8, 1>), grid, dim3(kBlock), 0, st, shards, parity, B.sched, total, C,
                    make_fastdiv(cd), B.rec_bytes, fast, P, D, B.present);
}

void launch_replay_indexed(const PeelArgs& B, const rfec_kplan& P, const v4u* pool, uint32_t last,
                           const uint32_t* src_of, uint32_t C, uint32_t cd, uint32_t maxc, const DenseOut& D,
                           hipStream_t st)
{
    const uint32_t total = B.groups * cd, fast = maxc <= 8 ? 1u : 0u;
    const dim3 grid(blocks_for(total));
    if (maxc <= 4)
        RFEC_LAUNCH((k_recover_indexed<4, 2>), grid, dim3(kBlock), 0, st, pool, last, src_of, B.sched, total, C,
                    make_fastdiv(cd), B.rec_bytes, fast, P, D, B.present);
    else
        RFEC_LAUNCH((k_recover_indexed<8, 1>), grid, dim3(kBlock), 0, st, pool, last, src_of, B.sched, total, C,
                    make_fastdiv(cd), B.rec_bytes, fast, P, D, B.present);
}
