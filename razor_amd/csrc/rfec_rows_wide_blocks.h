// rfec_rows_wide_blocks.h -- the two block bodies of the wide row decode (C++ only).  Not installed.
//
// k_decode_rows_wide (rfec_rows_wide.hip, which says how the decode works) and the wide row sections of
// k_decode_window_indexed (rfec_cascade.hip) run the same header block (rows_wide_header_block) and the same payload
// block (rows_wide_payload_block) over a RowsWideArgs: one copy of each, here.  Internal linkage: every unit that
// includes this header compiles its own.
#ifndef RFEC_ROWS_WIDE_BLOCKS_H_
#define RFEC_ROWS_WIDE_BLOCKS_H_

#include "rfec_families.h"
#include "rfec_u128.h"

namespace {

// Loads in flight per round: 45 VGPRs, 8 waves per SIMD.  Rounds of 8 were measured once on the large pool (72
// VGPRs, 7 waves; the positions past a short row's end are requests too) -- one row of 100: 249.5 us against 252.5,
// the ranges overlapping; one row of 10: 291.6 against 270.0.
constexpr int kRowsRound = 4;

struct RowsWideArgs {
    const v4u* rows;               // the pool, [n_rows][C]
    const uint32_t* src_of;        // [G][K + NL]
    const uint32_t* hdr_dw;        // [G][K][5]
    const uint32_t* meta_dw;       // [G][NL][5]
    const uint16_t* fsize;         // [G][NL]
    const uint64_t* present;       // [G][2]
    const uint64_t* parity_present;
    uint64_t* recovered;           // [G][2]
    v4u* out_sh;                   // [G][E][C]
    uint32_t* out_hdr_dw;          // [G][E][5]
    uint8_t* out_index;            // [G][E]
    uint32_t E, groups, total, C, capacity, last;
    uint32_t K, COL, NL;           // the shape: NL rows of COL (the last one shorter) with a line
    uint32_t lg, n_hdr;            // header lanes per group (log2), header blocks
    FastDiv divC, divQC, divCol;   // cd, E * cd, COL
    uint32_t n_hr, every, npay8;   // the grid (Rounds8)
};

// row r of the shape (r COL < K): its member mask, as WideShape::row_mask has it (COL may be 128 here)
__device__ __forceinline__ u128 row_mask(const RowsWideArgs& A, uint32_t r)
{
    return (low128(A.COL) << (r * A.COL)) & low128(A.K);
}

// The row's members other than its target, numbered 0 .. count - 2: the p-th is member p of the row before the
// target's position ut and member p + 1 from there on (wide_other), so a round of loads holds wanted members only.
__device__ __forceinline__ uint32_t row_other(uint32_t first, uint32_t ut, uint32_t p)
{
    return first + p + (p >= ut ? 1u : 0u);
}

// ---------------------------------------------------------------------------------------------------------------
// The header lanes: lane = (group, line slot).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rows_wide_header_block(const RowsWideArgs& A, uint32_t hb)
{
    const uint32_t nlp = 1u << A.lg;
    const uint32_t hl = hb * kBlock + threadIdx.x;
    const uint32_t g = hl >> A.lg, l = hl & (nlp - 1);
    const uint32_t K = A.K, NL = A.NL, E = A.E;
    uint64_t rec0 = 0, rec1 = 0; // the recovered mask (no dynamic register index: no scratch)
    if (g < A.groups && l < NL && ((A.parity_present[g] >> l) & 1ull)) {
        const u128 have = mk128(A.present[2 * g], A.present[2 * g + 1]);
        const u128 m = row_mask(A, l), x = m & ~have;
        if (pop128(x) == 1 && (m & have) != 0) {
            const uint32_t t = ffs128(x);
            const uint32_t first = l * A.COL, count = min(A.COL, K - first), ut = t - first;
            const uint32_t L = A.fsize[(size_t)g * NL + l];
            const uint32_t* mp = A.meta_dw + ((size_t)g * NL + l) * 5;
            const uint32_t* gh = A.hdr_dw + (size_t)g * K * 5;
            uint32_t rec[5];
#pragma unroll
            for (int d = 0; d < 5; ++d)
                rec[d] = mp[d];
            bool ok = L <= A.capacity;
#pragma unroll 1
            for (uint32_t u0 = 0; u0 + 1 < count; u0 += kRowsRound) {
                uint32_t mem[kRowsRound][5];
                bool use[kRowsRound];
#pragma unroll
                for (int u = 0; u < kRowsRound; ++u) {
                    use[u] = u0 + u + 1 < count;
                    // (a position past the row's end re-reads the meta record and counts as zeros: the loads
                    // stay unconditional)
                    const uint32_t* r = use[u] ? gh + row_other(first, ut, u0 + u) * 5 : mp;
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        mem[u][d] = r[d];
                }
#pragma unroll
                for (int u = 0; u < kRowsRound; ++u) {
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        rec[d] ^= use[u] ? mem[u][d] : 0u;
                    ok = ok && (!use[u] || (mem[u][4] >> 16) <= L);
                }
            }
            const uint32_t e = rank128(~have & low128(K), t);
            if (ok && (rec[4] >> 16) <= L && e < E) {
                uint32_t* oh = A.out_hdr_dw + ((size_t)g * E + e) * 5; // the recovered header record
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    oh[d] = rec[d];
                if (t < 64)
                    rec0 = 1ull << t;
                else
                    rec1 = 1ull << (t - 64);
            }
        }
    }
    for (uint32_t sh = 1; sh < nlp; sh <<= 1) { // a group's nlp <= 64 lanes lie in one wave
        rec0 |= __shfl_xor(rec0, sh);
        rec1 |= __shfl_xor(rec1, sh);
    }
    if (g < A.groups && l == 0) {
        A.recovered[2 * g] = rec0;
        A.recovered[2 * g + 1] = rec1;
        // out_index: the e-th erased segment's index where it was recovered, else 0xFF
        const u128 rm = mk128(rec0, rec1);
        u128 e = ~mk128(A.present[2 * g], A.present[2 * g + 1]) & low128(K);
        uint8_t* oi = A.out_index + (size_t)g * E;
#pragma unroll 1
        for (uint32_t q = 0; q < E; ++q) {
            uint32_t ix = 0xFFu;
            if (e) {
                const uint32_t i = ffs128(e);
                e &= e - 1;
                if ((rm >> i) & 1)
                    ix = i;
            }
            oi[q] = (uint8_t)ix;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The payload lanes.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rows_wide_payload_block(const RowsWideArgs& A, uint32_t pb)
{
    const uint32_t t = pb * kBlock + threadIdx.x; // (XCD-swizzled: a group's lanes share one L2)
    if (t >= A.total)
        return;
    const uint32_t g = fdiv(t, A.divQC);
    const uint32_t rem = t - g * A.divQC.d;
    uint32_t q = fdiv(rem, A.divC);
    const uint32_t j = rem - q * A.divC.d;
    const uint32_t K = A.K, NL = A.NL, C = A.C;
    const u128 erased = ~mk128(A.present[2 * g], A.present[2 * g + 1]) & low128(K);
    // slot q: the q-th erased segment over the two words
    uint64_t e = (uint64_t)erased;
    uint32_t base = 0;
    const uint32_t nlo = (uint32_t)__popcll(e);
    const uint32_t slot = q;
    if (q >= nlo) {
        q -= nlo;
        e = (uint64_t)(erased >> 64);
        base = 64;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < q; ++i)
        e &= e - 1;
    if (!e)
        return;
    const uint32_t tgt = base + (uint32_t)__ffsll((long long)e) - 1;
    const uint32_t r = fdiv(tgt, A.divCol);
    // the target's row: it has a line (a last row of one segment has none), misses the target alone, has its parity
    if (r >= NL || (row_mask(A, r) & erased) != bit128(tgt) || !((A.parity_present[g] >> r) & 1ull))
        return;
    const v4u* pool = A.rows + j;
    const uint32_t* __restrict__ so = A.src_of + (size_t)g * (K + NL);
    const uint32_t first = r * A.COL, count = min(A.COL, K - first), ut = tgt - first;
    v4u acc = ld16(pool_row(pool, so, K + r, A.last, C));
#pragma unroll 1
    for (uint32_t u0 = 0; u0 + 1 < count; u0 += kRowsRound) {
        const v4u* src[kRowsRound];
        bool use[kRowsRound];
#pragma unroll
        for (int u = 0; u < kRowsRound; ++u) {
            use[u] = u0 + u + 1 < count;
            src[u] = pool_row(pool, so, use[u] ? row_other(first, ut, u0 + u) : K + r, A.last, C);
        }
        v4u mv[kRowsRound];
#pragma unroll
        for (int u = 0; u < kRowsRound; ++u)
            mv[u] = ld16(src[u]);
#pragma unroll
        for (int u = 0; u < kRowsRound; ++u)
            acc ^= use[u] ? mv[u] : v4u{0, 0, 0, 0};
    }
    st16(A.out_sh + ((size_t)g * A.E + slot) * C + j, acc);
}

} // namespace

#endif
