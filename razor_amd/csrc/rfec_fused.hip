// rfec_fused.hip -- the one-launch decodes of plans with pairwise disjoint lines (gfx950), the packed erasure
// records' packer and decode, and their launchers; rfec_kernels.hip picks among them (rfec_launch_recover[_out],
// rfec_launch_recover_indexed), rfec_host.c calls the packed records' shims.
//  Header lanes (one per (group, line)) spread over the grid, then k_decode_rows (row layouts: one lane per
//  (group, row or output slot, chunk)), k_decode_out (other plans, slots of >= 64 chunks) or k_decode_disjoint (one
//  lane per (group, chunk column)); through a slot map over a row pool, row layouts: k_decode_rows_indexed.
//  (line_headers and k_decode_rows_indexed's payload lane live in rfec_row_blocks.h: rfec_cascade.hip runs them too.)
#include "rfec_row_blocks.h"

namespace {

// ---------------------------------------------------------------------------
// Recover, fused form for plans whose lines are pairwise disjoint (the row
// layer alone, strip mode).  No recovery there can complete another line, so
// which lines fire follows from the received masks alone and no schedule has
// to travel between kernels.  Header blocks spread over the grid do the
// peel's header work (size checks, recovered headers, the recovered mask);
// the payload lanes XOR each line with exactly one missing member and its
// parity received into that member's slot (or its dense output slot).  A line
// the header checks reject is still written, into an erased slot whose
// recovered bit stays clear (rfec_recover_batch documents such slots as
// unspecified).  (The header blocks' body is line_headers, rfec_row_blocks.h.)
// ---------------------------------------------------------------------------

// Header lanes of the packed decode (rfec_recover_packed_out), one per (group,
// output slot e): 2^nlp_log2 >= E consecutive lanes per group.  Slot e's
// record holds the fec_meta, fec_data_size and the other members' records of
// the row of the group's e-th erased segment, so a lane's header bytes are one
// contiguous run after the group's two masks (line_headers reads them from
// three arrays: the meta and member runs in sectors shared with the lines that
// do not fire).  The checks and the recovered record are line_headers'.
template <int COL>
__device__ void packed_headers(const PeelArgs& A, uint32_t blk, uint32_t KK, uint32_t CC)
{
    const uint32_t ep = 1u << A.nlp_log2;
    const uint32_t hl = blk * kBlock + threadIdx.x;
    const uint32_t g = hl >> A.nlp_log2, e = hl & (ep - 1);
    uint64_t rec = 0;
    if (g < A.groups && e < A.out_per_group) {
        const uint8_t* pg = A.packed + (size_t)g * A.pk_stride;
        const uint64_t h = reinterpret_cast<const uint64_t*>(pg)[0], pp = reinterpret_cast<const uint64_t*>(pg)[1];
        uint64_t m = ~h & (KK == 64 ? ~0ull : (1ull << KK) - 1ull);
        for (uint32_t u = 0; u < e; ++u) // the e-th erased segment
            m &= m - 1ull;
        uint32_t v = 0xFF;
        if (m) {
            const uint32_t tgt = (uint32_t)__ffsll((long long)m) - 1, r = tgt / CC;
            const uint32_t R = (KK + CC - 1) / CC, cnt = r + 1 < R ? CC : KK - (R - 1) * CC;
            const uint64_t rm = ((1ull << cnt) - 1ull) << (r * CC);
            if (__popcll(rm & ~h) == 1 && (rm & h) && ((pp >> r) & 1ull)) {
                const uint32_t* sr = reinterpret_cast<const uint32_t*>(pg + 16 + (size_t)e * A.pk_slot);
                uint32_t r0 = sr[0], r1 = sr[1], r2 = sr[2], r3 = sr[3], r4 = sr[4];
                const uint32_t L = sr[5] & 0xFFFFu;
                uint32_t w[COL - 1][5];
#pragma unroll
                for (int q = 0; q < COL - 1; ++q) // one round of loads, as line_headers
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        w[q][d] = (uint32_t)q + 1 < cnt ? sr[6 + 5 * q + d] : 0u;
                bool ok = L <= A.capacity;
#pragma unroll
                for (int q = 0; q < COL - 1; ++q) {
                    r0 ^= w[q][0];
                    r1 ^= w[q][1];
                    r2 ^= w[q][2];
                    r3 ^= w[q][3];
                    r4 ^= w[q][4];
                    ok = ok && (w[q][4] >> 16) <= L;
                }
                if (ok && (r4 >> 16) <= L) {
                    uint32_t* ht = reinterpret_cast<uint32_t*>(A.out_hdr + (size_t)g * A.out_per_group + e);
                    ht[0] = r0, ht[1] = r1, ht[2] = r2, ht[3] = r3, ht[4] = r4;
                    v = tgt;
                    rec = 1ull << tgt;
                }
            }
        }
        A.out_index[(size_t)g * A.out_per_group + e] = (uint8_t)v;
    }
    for (uint32_t sh = 1; sh < ep; sh <<= 1)
        rec |= __shfl_xor(rec, sh);
    if (g < A.groups && e == 0) {
        A.recovered[2 * g] = rec;
        A.recovered[2 * g + 1] = 0;
    }
}

// Flat form, slots under 64 chunks (k = 32 / 256 B): one lane per (group,
// chunk column) XORs every fired line of its group, two lines' loads in
// flight together, in place or into the dense output.
template <int MAXC>
__global__ __launch_bounds__(kBlock) void k_decode_disjoint(v4u* shards, const v4u* __restrict__ parity,
                                                            uint32_t total, uint32_t C, FastDiv divC,
                                                            uint32_t n_hdr_blocks, uint32_t hdr_every, PeelArgs A,
                                                            rfec_kmask M, DenseOut D)
{
    uint32_t hb, pb;
    if (header_block(n_hdr_blocks, hdr_every, &hb, &pb)) {
        line_headers(A, M, hb);
        return;
    }
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    const rfec_kplan& P = M.plan;
    stage_plan(lplan, P);
    const uint32_t t = pb * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divC);
    const uint32_t j = t - g * divC.d; // chunk column (divC.d = chunks of work per slot)
    const uint64_t h0 = A.present[2 * g], h1 = A.present[2 * g + 1];
    uint64_t fire = A.parity_present[g];
    v4u* grp = shards + (size_t)g * P.k * C + j;
    v4u* out = D.E ? D.sh + (size_t)g * D.E * C + j : nullptr;
    // descriptors over the wave's first group (its lanes span a few groups)
    const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    const __amdgpu_buffer_rsrc_t rs = wave_rsrc(shards + (size_t)gb * P.k * C);
    const __amdgpu_buffer_rsrc_t rp = wave_rsrc(parity + (size_t)gb * P.n_lines * C);
    const uint32_t grp0 = ((g - gb) * P.k * C + j) * 16u, par0 = ((g - gb) * P.n_lines * C + j) * 16u;
    {   // lines with their parity received and exactly one member missing
        // (uniform loop: the line masks stay scalar kernel-argument loads)
        uint64_t f = 0;
        for (uint32_t l = 0; l < P.n_lines; ++l) {
            const uint64_t x0 = M.mask[l][0] & ~h0, x1 = M.mask[l][1] & ~h1;
            if (__popcll(x0) + __popcll(x1) == 1)
                f |= 1ull << l;
        }
        fire &= f;
    }
    while (fire) {
        // two fired lines per round, every load of both in flight together
        // (predicated loads through the wave's descriptors, see wave_rsrc)
        v4u acc[2], mv[2][MAXC];
        uint32_t tg[2];
        bool on[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            on[b] = fire != 0;
            const uint32_t l = on[b] ? (uint32_t)__ffsll((long long)fire) - 1 : 0;
            fire &= fire - 1;
            const uint32_t ln = lplan[l];
            const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
            acc[b] = bld16(rp, on[b] ? par0 + l * C * 16u : kNoLoad);
            tg[b] = first;
#pragma unroll
            for (int q = 0; q < MAXC; ++q) {
                const uint32_t i = first + q * stride;
                const bool in = on[b] && (uint32_t)q < count, have = has_bit(h0, h1, i);
                tg[b] = in && !have ? i : tg[b];
                mv[b][q] = bld16(rs, in && have ? grp0 + i * C * 16u : kNoLoad);
            }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int q = 0; q < MAXC; ++q)
                acc[b] ^= mv[b][q];
            if (on[b]) {
                if (!D.E) {
                    st16(grp + (size_t)tg[b] * C, acc[b]);
                } else {
                    const uint32_t e = missing_rank(h0, h1, tg[b]);
                    if (e < D.E)
                        st16(out + (size_t)e * C, acc[b]);
                }
            }
        }
    }
}

// Fused disjoint-plan decode, output-mapped (slots of >= 64 chunks): one lane
// per (group, line, chunk column).  A lane whose line does not fire (parity
// missing, or not exactly one member missing) exits; the others load the
// parity chunk and the line's present members' chunks, all in flight, and
// store one chunk of the missing member.  A wave's loads and its store each
// cover 1 KiB of one slot.  142.7 us vs 157.8 us flat at k = 10 / 1,200 B.
// SLOTS (dense output): one lane per (group, output slot e, chunk column)
// instead: slot e's target is the group's e-th erased segment and its line
// comes from a segment -> line table (disjoint plan), so no lane sits on a
// line that does not fire (divLC divides by E C then).
template <int MAXC, bool SLOTS>
__global__ __launch_bounds__(kBlock) void k_decode_out(v4u* shards, const v4u* __restrict__ parity, uint32_t total,
                                                       uint32_t C, FastDiv divC, FastDiv divLC,
                                                       uint32_t n_hdr_blocks, uint32_t hdr_every, PeelArgs A,
                                                       rfec_kmask M, DenseOut D)
{
    uint32_t hb, pb;
    if (header_block(n_hdr_blocks, hdr_every, &hb, &pb)) {
        line_headers(A, M, hb);
        return;
    }
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    __shared__ uint64_t lmask[RFEC_MAX_LINES][2];
    __shared__ uint8_t sline[SLOTS ? RFEC_MAX_K : 1]; // segment -> its line (0xFF: none)
    const rfec_kplan& P = M.plan;
    if (threadIdx.x < P.n_lines) {
        lmask[threadIdx.x][0] = M.mask[threadIdx.x][0];
        lmask[threadIdx.x][1] = M.mask[threadIdx.x][1];
    }
    if constexpr (SLOTS) {
        if (threadIdx.x < P.k) {
            const uint32_t i = threadIdx.x;
            uint32_t li = 0xFF;
            for (uint32_t q = 0; q < P.n_lines; ++q) { // (uniform loads of the line masks)
                const uint64_t w = i < 64 ? M.mask[q][0] : M.mask[q][1];
                li = (w >> (i & 63)) & 1ull ? q : li;
            }
            sline[i] = (uint8_t)li;
        }
    }
    stage_plan(lplan, P); // ends in a barrier
    const uint32_t t = pb * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divLC);
    const uint32_t rem = t - g * divLC.d;
    const uint32_t q0 = fdiv(rem, divC); // line, or output slot (SLOTS)
    const uint32_t j = rem - q0 * divC.d;
    const uint64_t h0 = A.present[2 * g], h1 = A.present[2 * g + 1];
    uint32_t l = q0, tgt = 0;
    if constexpr (SLOTS) { // the q0-th erased segment among [0, k)
        const uint32_t k = P.k;
        uint64_t m0 = ~h0 & (k >= 64 ? ~0ull : (1ull << k) - 1ull);
        uint64_t m1 = k > 64 ? ~h1 & (k >= 128 ? ~0ull : (1ull << (k - 64)) - 1ull) : 0ull;
        const uint32_t c0 = (uint32_t)__popcll(m0);
        uint64_t m = q0 < c0 ? m0 : m1;
        for (uint32_t u = 0, ue = q0 < c0 ? q0 : q0 - c0; u < ue; ++u)
            m &= m - 1ull;
        if (!m)
            return;
        tgt = (q0 < c0 ? 0u : 64u) + (uint32_t)__ffsll((long long)m) - 1;
        l = sline[tgt];
        if (l == 0xFFu)
            return;
    }
    if (!((A.parity_present[g] >> l) & 1ull))
        return;
    const uint64_t x0 = lmask[l][0] & ~h0, x1 = lmask[l][1] & ~h1;
    if (__popcll(x0) + __popcll(x1) != 1 || ((lmask[l][0] & h0) | (lmask[l][1] & h1)) == 0)
        return;
    if constexpr (!SLOTS)
        tgt = x0 ? (uint32_t)__ffsll((long long)x0) - 1 : 64u + (uint32_t)__ffsll((long long)x1) - 1;
    v4u* grp = shards + (size_t)g * P.k * C + j;
    v4u* dst = grp + (size_t)tgt * C;
    if constexpr (SLOTS) {
        dst = D.sh + ((size_t)g * D.E + q0) * C + j;
    } else if (D.E) {
        const uint32_t e = missing_rank(h0, h1, tgt);
        if (e >= D.E)
            return;
        dst = D.sh + ((size_t)g * D.E + e) * C + j;
    }
    const uint32_t ln = lplan[l];
    const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
    const v4u* pl = parity + ((size_t)g * P.n_lines + l) * C + j;
    v4u acc = ld16(pl);
    const ptrdiff_t to_par = pl - grp;
    v4u mv[MAXC];
    bool use[MAXC];
#pragma unroll
    for (int q = 0; q < MAXC; ++q) { // (unconditional loads, see k_decode_rows)
        const uint32_t i = first + q * stride;
        use[q] = (uint32_t)q < count && i != tgt; // every other member of a firing line is present
        mv[q] = ld16(grp + (use[q] ? (ptrdiff_t)i * C : to_par));
    }
#pragma unroll
    for (int q = 0; q < MAXC; ++q)
        acc ^= use[q] ? mv[q] : v4u{0, 0, 0, 0};
    st16(dst, acc);
}

// The same for the row layouts (rows of COL consecutive segments, K <= 64):
// the line masks and members are arithmetic in the row index, so no plan is
// staged through LDS (no barrier before the first load).  SLOTS (dense
// output): one lane per (group, output slot e, chunk) instead of (group, row,
// chunk): slot e's target is the group's e-th erased segment, recovered when
// its row fires, so no lane sits on a row that does not (divRC divides by E C
// then; c3: 125-127 vs 137-141 us).  XCD-swizzled blocks in rounds of 8
// (traffic 1.077 vs 1.107 x algorithmic at k = 10 / 1,200 B).
// K = 0: k and col at run time (k_rt <= 64, col_rt <= COL), the member loads
// unrolled to COL and predicated on the row's size (the strip-mode plans).
// PK (with SLOTS): the masks and header records from the packed erasure
// records (rfec_recover_packed_out), header lanes packed_headers.
template <int K, int COL, bool SLOTS, bool PK = false>
__global__ __launch_bounds__(kBlock) void k_decode_rows(v4u* shards, const v4u* __restrict__ parity, uint32_t total,
                                                        uint32_t C, FastDiv divC, FastDiv divRC,
                                                        uint32_t n_hdr_blocks, uint32_t hdr_every, PeelArgs A,
                                                        rfec_kmask M, DenseOut D, uint32_t npay8, uint32_t k_rt,
                                                        uint32_t col_rt, FastDiv divCol)
{
    static_assert(K <= 64, "row decode keeps the present mask in one word");
    static_assert(!PK || SLOTS, "packed records are per output slot");
    const uint32_t KK = K ? (uint32_t)K : k_rt, CC = K ? (uint32_t)COL : col_rt;
    uint32_t hb, pb;
    if (header_block_xcd((n_hdr_blocks + 7u) >> 3, hdr_every, npay8, &hb, &pb)) {
        if (hb < n_hdr_blocks) {
            if constexpr (PK)
                packed_headers<COL>(A, hb, KK, CC);
            else
                line_headers(A, M, hb);
        }
        return;
    }
    const uint32_t R = (KK + CC - 1) / CC, LAST = KK - (R - 1) * CC;
    const uint32_t t = pb * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divRC);
    const uint32_t rem = t - g * divRC.d;
    const uint32_t q0 = fdiv(rem, divC); // row, or output slot (SLOTS)
    const uint32_t j = rem - q0 * divC.d;
    uint64_t h, ppm = 0;
    if constexpr (PK) { // the record's two masks: one 16-B load
        const uint64_t* pg = reinterpret_cast<const uint64_t*>(A.packed + (size_t)g * A.pk_stride);
        h = pg[0];
        ppm = pg[1];
    } else {
        h = A.present[2 * g];
    }
    uint32_t r, tgt;
    if constexpr (SLOTS) {
        uint64_t m = ~h & (KK == 64 ? ~0ull : (1ull << KK) - 1ull);
        for (uint32_t u = 0; u < q0; ++u) // the q0-th erased segment
            m &= m - 1ull;
        if (!m)
            return;
        tgt = (uint32_t)__ffsll((long long)m) - 1;
        r = K ? tgt / (uint32_t)COL : fdiv(tgt, divCol);
    } else {
        r = q0;
    }
    const uint32_t cnt = r + 1 < R ? CC : LAST;
    const uint64_t rm = ((1ull << cnt) - 1ull) << (r * CC);
    const uint64_t miss = rm & ~h;
    if (__popcll(miss) != 1 || !(((PK ? ppm : A.parity_present[g]) >> r) & 1ull))
        return;
    if constexpr (!SLOTS)
        tgt = (uint32_t)__ffsll((long long)miss) - 1;
    v4u* dst = shards + ((size_t)g * KK + tgt) * C + j;
    if constexpr (SLOTS) {
        dst = D.sh + ((size_t)g * D.E + q0) * C + j;
    } else if (D.E) {
        const uint32_t e = (uint32_t)__popcll(~h & ((1ull << tgt) - 1ull));
        if (e >= D.E)
            return;
        dst = D.sh + ((size_t)g * D.E + e) * C + j;
    }
    // members through a descriptor over the wave's first group (wave_rsrc)
    const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    const __amdgpu_buffer_rsrc_t rs = wave_rsrc(shards + (size_t)gb * KK * C);
    const uint32_t row0 = (((g - gb) * KK + r * CC) * C + j) * 16u;
    v4u acc = ld16(parity + ((size_t)g * R + r) * C + j);
    v4u mv[COL];
#pragma unroll
    for (int q = 0; q < COL; ++q)
        mv[q] = bld16(rs, (uint32_t)q < cnt && r * CC + q != tgt ? row0 + (uint32_t)q * C * 16u : kNoLoad);
#pragma unroll
    for (int q = 0; q < COL; ++q)
        acc ^= mv[q];
    st16(dst, acc);
}

// k_decode_rows<K, COL, SLOTS = true> for rfec_recover_indexed_out: the same grid, header blocks and lanes per
// (group, output slot, chunk), with the row's parity chunk read from row src_of[g (KK + R) + KK + r] of the pool
// and member i from row src_of[g (KK + R) + i].  The rows lie anywhere in the pool, so no descriptor spans a
// wave's loads: they are plain 64-bit addresses, the map words loaded first, then the parity and the COL member
// chunks unconditionally and in flight together; a member that is not wanted (past the row's end, or the
// target) re-reads the parity chunk, as in k_decode_out, and only wanted slots' map words are read.  A row index
// is clamped to `last` = n_rows - 1 before it is used.
template <int K, int COL>
__global__ __launch_bounds__(kBlock) void k_decode_rows_indexed(const v4u* rows, uint32_t last,
                                                                const uint32_t* __restrict__ src_of, uint32_t total,
                                                                uint32_t C, FastDiv divC, FastDiv divRC,
                                                                uint32_t n_hdr_blocks, uint32_t hdr_every, PeelArgs A,
                                                                rfec_kmask M, DenseOut D, uint32_t npay8,
                                                                uint32_t k_rt, uint32_t col_rt, FastDiv divCol)
{
    static_assert(K <= 64, "row decode keeps the present mask in one word");
    const uint32_t KK = K ? (uint32_t)K : k_rt, CC = K ? (uint32_t)COL : col_rt;
    uint32_t hb, pb;
    if (header_block_xcd((n_hdr_blocks + 7u) >> 3, hdr_every, npay8, &hb, &pb)) {
        if (hb < n_hdr_blocks)
            line_headers(A, M, hb);
        return;
    }
    RFEC_ROWS_INDEXED_LANE(K, COL, rows, last, src_of, total, C, divC, divRC, A, D, KK, CC, divCol, pb)
}

// The batch layout -> packed erasure records (rfec_pack_erasures): one lane
// per (group, output slot e), 2^lg >= E lanes per group.  Slot e: the fec_meta
// and fec_data_size of the row of the group's e-th erased segment and the
// row's other members' records in index order (zeros past the row's end);
// all zeros where the group has no e-th erased segment.  Lane 0 writes the
// masks and zeros the record's tail.
__global__ __launch_bounds__(kBlock) void k_pack_rows(uint8_t* __restrict__ packed, const uint32_t* __restrict__ hdr,
                                                      const uint64_t* __restrict__ present,
                                                      const uint32_t* __restrict__ meta,
                                                      const uint16_t* __restrict__ fsize,
                                                      const uint64_t* __restrict__ parity_present, uint32_t groups,
                                                      uint32_t KK, uint32_t CC, uint32_t NL, uint32_t E, uint32_t lg,
                                                      uint32_t pk_stride, uint32_t pk_slot)
{
    const uint32_t hl = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t g = hl >> lg, e = hl & ((1u << lg) - 1u);
    if (g >= groups || e >= E)
        return;
    uint8_t* pg = packed + (size_t)g * pk_stride;
    const uint64_t h = present[2 * g];
    if (e == 0) {
        reinterpret_cast<uint64_t*>(pg)[0] = h;
        reinterpret_cast<uint64_t*>(pg)[1] = parity_present[g];
        for (uint32_t o = 16 + E * pk_slot; o < pk_stride; o += 4)
            *reinterpret_cast<uint32_t*>(pg + o) = 0;
    }
    uint64_t m = ~h & (KK == 64 ? ~0ull : (1ull << KK) - 1ull);
    for (uint32_t u = 0; u < e; ++u)
        m &= m - 1ull;
    uint32_t* so = reinterpret_cast<uint32_t*>(pg + 16 + (size_t)e * pk_slot);
    const uint32_t nd = pk_slot / 4;
    if (!m) {
        for (uint32_t d = 0; d < nd; ++d)
            so[d] = 0;
        return;
    }
    const uint32_t tgt = (uint32_t)__ffsll((long long)m) - 1, r = tgt / CC;
    const uint32_t first = r * CC, cnt = KK - first < CC ? KK - first : CC;
    const uint32_t* mr = meta + ((size_t)g * NL + r) * 5;
    for (uint32_t d = 0; d < 5; ++d)
        so[d] = mr[d];
    so[5] = fsize[(size_t)g * NL + r];
    uint32_t o = 6;
    for (uint32_t i = first; i < first + cnt; ++i) {
        if (i == tgt)
            continue;
        const uint32_t* hr = hdr + ((size_t)g * KK + i) * 5;
        for (uint32_t d = 0; d < 5; ++d)
            so[o + d] = hr[d];
        o += 5;
    }
    for (; o < nd; ++o)
        so[o] = 0;
}

// header_block()'s period for npay payload blocks: n_hdr periods of
// (every + 1) blocks must fit the grid: every <= npay / n_hdr, so fewer
// payload than header blocks keeps them at the head.
inline uint32_t hdr_every(const FusedArgs& F, uint32_t npay) { return F.n_hdr ? npay / F.n_hdr : 0; }

// The row decodes' compile-time shapes <K, 4>: k = 10 and 32 in rows of 4, else k and col at run time (K = 0, rows
// of <= 4).  f(std::integral_constant<int, K>{}) is called with the K that (k, col) takes.
template <class Fn>
void for_row_shape(uint32_t k, uint32_t col, Fn&& f)
{
    if (k == 10 && col == 4)
        f(std::integral_constant<int, 10>{});
    else if (k == 32 && col == 4)
        f(std::integral_constant<int, 32>{});
    else
        f(std::integral_constant<int, 0>{});
}

// The row decodes' grid and divisors: `per` payload slots per group (rows, or dense output slots) of cd chunks,
// in rounds of 8 blocks with the header rounds spread over them.  These kernels take the header BLOCKS.
struct RowsGrid {
    uint32_t total; // payload lanes, < 2^32: checked by the caller
    Rounds8 g;
    FastDiv dC, dRC, dCol;
};

RowsGrid rows_grid(const FusedArgs& F, uint32_t groups, uint32_t per, uint32_t cd, uint32_t col)
{
    const uint32_t total = groups * per * cd;
    return RowsGrid{total, rounds_of_8(F.n_hdr, blocks_for(total)), make_fastdiv(cd), make_fastdiv(per * cd),
                    make_fastdiv(col)};
}

} // namespace

// output-mapped fused decode: one lane per (group, line or output slot, chunk column)
void launch_fused_out(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t cd, bool slots,
                      uint32_t maxc)
{
    const uint32_t per = slots ? F.D.E : M.plan.n_lines;
    const uint32_t total = B.groups * per * cd; // < 2^32: checked by the caller
    const uint32_t npay = blocks_for(total);
    const dim3 grid(F.n_hdr + npay);
    const FastDiv dC = make_fastdiv(cd), dLC = make_fastdiv(per * cd);
    const uint32_t every = hdr_every(F, npay);
    RFEC_TAG(RFEC_PATH_DEC_OUT, (maxc <= 4 ? 4u : 8u) | (slots ? RFEC_PATH_SLOTS : 0u));
#define RFEC_DO(MAXC, SLOTS)                                                                                      \
    RFEC_LAUNCH((k_decode_out<MAXC, SLOTS>), grid, dim3(kBlock), 0, F.stream, F.shards, F.parity, total, F.C, dC, \
                dLC, F.n_hdr, every, B, M, F.D)
    if (maxc <= 4) {
        if (slots)
            RFEC_DO(4, true);
        else
            RFEC_DO(4, false);
    } else {
        if (slots)
            RFEC_DO(8, true);
        else
            RFEC_DO(8, false);
    }
#undef RFEC_DO
}

// row-layout fused decode: one lane per (group, row, chunk column), or per
// (group, dense output slot, chunk column) when `slots`
void launch_fused_rows(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t cd, bool slots,
                       uint32_t col)
{
    const uint32_t k = M.plan.k;
    const RowsGrid r = rows_grid(F, B.groups, slots ? F.D.E : (k + col - 1) / col, cd, col);
    for_row_shape(k, col, [&](auto s) {
        constexpr int K = decltype(s)::value, COL = 4;
        RFEC_TAG(RFEC_PATH_DEC_ROWS, K | (slots ? RFEC_PATH_SLOTS : 0u));
        if (slots)
            RFEC_LAUNCH((k_decode_rows<K, COL, true>), dim3(r.g.grid), dim3(kBlock), 0, F.stream, F.shards, F.parity,
                        r.total, F.C, r.dC, r.dRC, r.g.hdr_blocks, r.g.every, B, M, F.D, r.g.npay8, k, col, r.dCol);
        else
            RFEC_LAUNCH((k_decode_rows<K, COL, false>), dim3(r.g.grid), dim3(kBlock), 0, F.stream, F.shards, F.parity,
                        r.total, F.C, r.dC, r.dRC, r.g.hdr_blocks, r.g.every, B, M, F.D, r.g.npay8, k, col, r.dCol);
    });
}

// the same lanes per (group, dense output slot, chunk column) with the rows read through src_of from a pool
// (rfec_recover_indexed_out): k_decode_rows_indexed
void launch_rows_indexed(const v4u* pool, uint32_t last, const uint32_t* src_of, const FusedArgs& F,
                         const PeelArgs& B, const rfec_kmask& M, uint32_t cd, uint32_t col)
{
    const uint32_t k = M.plan.k;
    const RowsGrid r = rows_grid(F, B.groups, F.D.E, cd, col);
    for_row_shape(k, col, [&](auto s) {
        constexpr int K = decltype(s)::value, COL = 4;
        RFEC_LAUNCH((k_decode_rows_indexed<K, COL>), dim3(r.g.grid), dim3(kBlock), 0, F.stream, pool, last, src_of,
                    r.total, F.C, r.dC, r.dRC, r.g.hdr_blocks, r.g.every, B, M, F.D, r.g.npay8, k, col, r.dCol);
    });
}

void launch_fused_flat(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t maxc)
{
    const uint32_t npay = blocks_for(F.total);
    const dim3 grid(F.n_hdr + npay);
    RFEC_TAG(RFEC_PATH_DEC_FLAT, maxc <= 4 ? 4u : 8u);
    if (maxc <= 4)
        RFEC_LAUNCH((k_decode_disjoint<4>), grid, dim3(kBlock), 0, F.stream, F.shards, F.parity, F.total, F.C, F.f,
                    F.n_hdr, hdr_every(F, npay), B, M, F.D);
    else
        RFEC_LAUNCH((k_decode_disjoint<8>), grid, dim3(kBlock), 0, F.stream, F.shards, F.parity, F.total, F.C, F.f,
                    F.n_hdr, hdr_every(F, npay), B, M, F.D);
}

extern "C" {

int rfec_launch_pack_rows(const rfec_kplan* P, uint32_t col, uint32_t groups, const rfec_hdr* hdr,
                          const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                          const uint64_t* parity_present, uint32_t per_group, uint8_t* packed, uint32_t pk_stride,
                          uint32_t pk_slot, void* stream)
{
    const uint32_t lg = rfec_ceil_log2(per_group);
    const uint32_t lanes = groups << lg; // < 2^32: host-checked
    RFEC_TAG(RFEC_PATH_PACK_ROWS, 0);
    RFEC_LAUNCH(k_pack_rows, dim3(blocks_for(lanes)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), packed,
                reinterpret_cast<const uint32_t*>(hdr), present, reinterpret_cast<const uint32_t*>(meta), fsize,
                parity_present, groups, P->k, col, P->n_lines, per_group, lg, pk_stride, pk_slot);
    return (int)hipGetLastError();
}

// packed dense decode of row layouts: lanes per (group, output slot, chunk column), header lanes per
// (group, output slot)
int rfec_launch_recover_packed(const rfec_kmask* M, uint32_t col, uint32_t groups, uint32_t stride,
                               uint32_t capacity, const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                               uint32_t pk_stride, uint32_t pk_slot, uint64_t* recovered,
                               const rfec_dense_out* out, void* stream)
{
    PeelArgs B = {};
    B.recovered = recovered;
    B.groups = groups;
    B.capacity = capacity;
    B.out_hdr = out->hdr;
    B.out_index = out->index;
    B.out_per_group = out->per_group;
    B.packed = packed;
    B.pk_stride = pk_stride;
    B.pk_slot = pk_slot;
    B.nlp_log2 = rfec_ceil_log2(out->per_group);
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, k = M->plan.k;
    const uint32_t n_hdr = blocks_for((uint64_t)groups << B.nlp_log2);
    const DenseOut DO = {reinterpret_cast<v4u*>(out->shards), out->per_group};
    const FusedArgs F = {const_cast<v4u*>(reinterpret_cast<const v4u*>(shards)), reinterpret_cast<const v4u*>(parity),
                         groups * cd, stride / 16, make_fastdiv(cd), n_hdr, reinterpret_cast<hipStream_t>(stream), DO};
    const RowsGrid r = rows_grid(F, groups, DO.E, cd, col);
    for_row_shape(k, col, [&](auto s) {
        constexpr int K = decltype(s)::value, COL = 4;
        RFEC_TAG(RFEC_PATH_DEC_ROWS, K | RFEC_PATH_SLOTS | RFEC_PATH_PACKED);
        RFEC_LAUNCH((k_decode_rows<K, COL, true, true>), dim3(r.g.grid), dim3(kBlock), 0, F.stream, F.shards, F.parity,
                    r.total, F.C, r.dC, r.dRC, r.g.hdr_blocks, r.g.every, B, *M, F.D, r.g.npay8, k, col, r.dCol);
    });
    return (int)hipGetLastError();
}

} // extern "C"
