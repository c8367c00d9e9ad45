// rfec_row_blocks.h -- the two block bodies of the indexed row decode (C++ only).  Not installed.
//
// k_decode_rows_indexed (rfec_fused.hip) and the row sections of k_decode_shapes_indexed (rfec_cascade.hip) run the
// same header block (line_headers, which the other fused decodes of rfec_fused.hip run too) and the same payload
// lane (RFEC_ROWS_INDEXED_LANE): one copy of each, here.  Internal linkage: every unit that includes this header
// compiles its own.
#ifndef RFEC_ROW_BLOCKS_H_
#define RFEC_ROW_BLOCKS_H_

#include "rfec_families.h"

namespace {

// Header work of the fused decode, one lane per (group, line): NLP = 2^nlp_log2
// >= n_lines consecutive lanes per group.  A line fires as in peel_block (one
// member missing, one present, its parity received, sizes within bounds); it
// reads only its own members' headers, so a group costs the fired lines'
// records instead of all K + NL staged.  Lines are pairwise disjoint, so the
// lines of a group are independent; the group's recovered mask is OR-reduced
// over its NLP lanes (all in one wave: NLP <= 64).
__device__ void line_headers(const PeelArgs& A, const rfec_kmask& M, uint32_t blk)
{
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    __shared__ uint64_t lmask[RFEC_MAX_LINES][2];
    const rfec_kplan& P = M.plan;
    if (threadIdx.x < P.n_lines) {
        lmask[threadIdx.x][0] = M.mask[threadIdx.x][0];
        lmask[threadIdx.x][1] = M.mask[threadIdx.x][1];
    }
    stage_plan(lplan, P);
    const uint32_t nlp = 1u << A.nlp_log2;
    const uint32_t hl = blk * kBlock + threadIdx.x;
    const uint32_t g = hl >> A.nlp_log2, l = hl & (nlp - 1);
    uint64_t rec0 = 0, rec1 = 0; // recovered mask (no dynamic register index: no scratch)
    if (g < A.groups && l < P.n_lines && ((A.parity_present[g] >> l) & 1ull)) {
        const uint64_t h0 = A.present[2 * g], h1 = A.present[2 * g + 1];
        const uint64_t m0 = lmask[l][0], m1 = lmask[l][1];
        const uint64_t x0 = m0 & ~h0, x1 = m1 & ~h1;
        if (__popcll(x0) + __popcll(x1) == 1 && ((m0 & h0) | (m1 & h1)) != 0) {
            // one round of loads: fec_data_size, fec_meta and the present
            // members' records together (the size check comes after them)
            const uint32_t t = x0 ? (uint32_t)__ffsll((long long)x0) - 1 : 64u + (uint32_t)__ffsll((long long)x1) - 1;
            const uint32_t L = A.fsize[(size_t)g * P.n_lines + l];
            const uint32_t* mr = reinterpret_cast<const uint32_t*>(A.meta + (size_t)g * P.n_lines + l);
            uint32_t r0 = mr[0], r1 = mr[1], r2 = mr[2], r3 = mr[3], r4 = mr[4];
            const uint32_t ln = lplan[l];
            const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
            const uint32_t* gh = reinterpret_cast<const uint32_t*>(A.hdr + (size_t)g * P.k);
            uint32_t w[8][5];
#pragma unroll
            for (int q = 0; q < 8; ++q) { // fused decodes: lines of at most 8 members
                const uint32_t i = first + q * stride;
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    w[q][d] = 0;
                if ((uint32_t)q < count && i != t) {
                    const uint32_t* r = gh + i * 5;
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        w[q][d] = r[d];
                }
            }
            bool ok = L <= A.capacity;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                r0 ^= w[q][0];
                r1 ^= w[q][1];
                r2 ^= w[q][2];
                r3 ^= w[q][3];
                r4 ^= w[q][4];
                ok = ok && (w[q][4] >> 16) <= L;
            }
            if (ok && (r4 >> 16) <= L) {
                uint32_t* ht = nullptr;
                if (!A.out_per_group) {
                    ht = reinterpret_cast<uint32_t*>(A.hdr + (size_t)g * P.k + t);
                } else {
                    const uint32_t e = missing_rank(h0, h1, t);
                    if (e < A.out_per_group)
                        ht = reinterpret_cast<uint32_t*>(A.out_hdr + (size_t)g * A.out_per_group + e);
                }
                if (ht) {
                    ht[0] = r0, ht[1] = r1, ht[2] = r2, ht[3] = r3, ht[4] = r4;
                    if (t < 64)
                        rec0 = 1ull << t;
                    else
                        rec1 = 1ull << (t - 64);
                }
            }
        }
    }
    for (uint32_t sh = 1; sh < nlp; sh <<= 1) {
        rec0 |= __shfl_xor(rec0, sh);
        rec1 |= __shfl_xor(rec1, sh);
    }
    if (g < A.groups && l == 0) {
        A.recovered[2 * g] = rec0;
        A.recovered[2 * g + 1] = rec1;
        if (A.out_per_group) {
            // out_index: the e-th erased segment's index where it was recovered, else 0xFF
            const uint32_t K = P.k;
            uint64_t m0 = ~A.present[2 * g] & (K >= 64 ? ~0ull : (1ull << K) - 1ull);
            uint64_t m1 = K <= 64 ? 0ull : ~A.present[2 * g + 1] & (K >= 128 ? ~0ull : (1ull << (K - 64)) - 1ull);
            uint8_t* oi = A.out_index + (size_t)g * A.out_per_group;
            for (uint32_t e = 0; e < A.out_per_group; ++e) {
                uint32_t v = 0xFF;
                if (m0 | m1) {
                    const uint32_t i = m0 ? (uint32_t)__ffsll((long long)m0) - 1 : 64u + (uint32_t)__ffsll((long long)m1) - 1;
                    if (has_bit(rec0, rec1, i))
                        v = i;
                    if (m0)
                        m0 &= m0 - 1;
                    else
                        m1 &= m1 - 1;
                }
                oi[e] = (uint8_t)v;
            }
        }
    }
}

// The payload lanes of block pb of the indexed row decode, the statements that end a void kernel: lane (group,
// output slot, chunk) of `total` reads the row's parity chunk from row src_of[g (KK + R) + KK + r] of the pool and
// member i from row src_of[g (KK + R) + i] (k_decode_rows_indexed says why the loads have this form).  K != 0:
// k = K in rows of COL at compile time; K == 0: KK and CC <= COL at run time, divCol = CC.  Of A (a PeelArgs) only
// present and parity_present are read; D is the DenseOut.
// A macro and not a function: as a forced-inline function, with its arguments by reference, by value or as plain
// pointers, k_decode_rows_indexed's three instances compiled to another schedule and register allocation (the
// exits inside an inlined function: DESIGN 7.13 and 7.15), and that kernel's code is not to move.
#define RFEC_ROWS_INDEXED_LANE(K, COL, rows, last, src_of, total, C, divC, divRC, A, D, KK, CC, divCol, pb) \
    const uint32_t R = (KK + CC - 1) / CC, LAST = KK - (R - 1) * CC;                                                 \
    const uint32_t t = pb * kBlock + threadIdx.x;                                                                    \
    if (t >= total)                                                                                                  \
        return;                                                                                                      \
    const uint32_t g = fdiv(t, divRC);                                                                               \
    const uint32_t rem = t - g * divRC.d;                                                                            \
    const uint32_t q0 = fdiv(rem, divC); /* output slot */                                                           \
    const uint32_t j = rem - q0 * divC.d;                                                                            \
    const uint64_t h = A.present[2 * g];                                                                             \
    uint64_t m = ~h & (KK == 64 ? ~0ull : (1ull << KK) - 1ull);                                                      \
    for (uint32_t u = 0; u < q0; ++u) /* the q0-th erased segment */                                                 \
        m &= m - 1ull;                                                                                               \
    if (!m)                                                                                                          \
        return;                                                                                                      \
    const uint32_t tgt = (uint32_t)__ffsll((long long)m) - 1;                                                        \
    const uint32_t r = K ? tgt / (uint32_t)COL : fdiv(tgt, divCol);                                                  \
    const uint32_t cnt = r + 1 < R ? CC : LAST;                                                                      \
    const uint64_t rm = ((1ull << cnt) - 1ull) << (r * CC);                                                          \
    if (__popcll(rm & ~h) != 1 || !((A.parity_present[g] >> r) & 1ull))                                              \
        return;                                                                                                      \
    const uint32_t* so = src_of + (size_t)g * (KK + R);                                                              \
    const v4u* src[COL + 1];                                                                                         \
    bool use[COL];                                                                                                   \
    src[COL] = pool_row(rows, so, KK + r, last, C) + j;                                                              \
    _Pragma("unroll") for (int q = 0; q < COL; ++q) {                                                                \
        use[q] = (uint32_t)q < cnt && r * CC + q != tgt;                                                             \
        src[q] = pool_row(rows, so, use[q] ? r * CC + q : KK + r, last, C) + j;                                      \
    }                                                                                                                \
    v4u acc = ld16(src[COL]);                                                                                        \
    v4u mv[COL];                                                                                                     \
    _Pragma("unroll") for (int q = 0; q < COL; ++q)                                                                  \
        mv[q] = ld16(src[q]);                                                                                        \
    _Pragma("unroll") for (int q = 0; q < COL; ++q)                                                                  \
        acc ^= use[q] ? mv[q] : v4u{0, 0, 0, 0};                                                                     \
    st16(D.sh + ((size_t)g * D.E + q0) * C + j, acc);

} // namespace

#endif
