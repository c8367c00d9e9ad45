// rfec_rows_wide.hip -- the one-launch decode of a row layout of any width through a slot map over a row pool
// (rfec_recover_indexed_rows_wide_out, rfec_recover_indexed_rows_wide.c), gfx950: every strip-mode plan of the
// sender (one parity over the frame, or `lines` parities over rows of ceil(k / lines) consecutive segments), the
// rows-only layer of a matrix, k up to 128 in rows of 2..128.
//
// The plan's shape (k, col, NL) is a run-time argument: line l is row l, members l col .. min(k, (l + 1) col) - 1,
// for l < NL; NL is ceil(k / col), or one less when the last row has one segment (that row has no line, and its
// segment is never recovered).  So the tables' pitch is k + NL map words and NL meta records per group -- not
// ceil(k / col), which RFEC_ROWS_INDEXED_LANE (rfec_row_blocks.h) may assume for the shapes it serves.  A row's
// member mask is arithmetic over 128 bits in (k, col, l): no rfec_kmask is read and nothing is staged in LDS.
//
// Rows are pairwise disjoint: no cascade, no schedule, no fixpoint.  The grid is k_decode_rows_indexed's: rounds of
// 8 header blocks spread between the payload blocks' rounds (header_block_xcd), payload lanes (group, out slot q,
// chunk j) in XCD-swizzled blocks; the payload lanes need nothing from the header lanes, and no workgroup waits on
// another.
//
// Header lane (group, line slot), 2^lg >= NL lanes per group: line_headers' rule (rfec_row_blocks.h) unchanged --
// the line fires with its parity received, exactly one member missing and one present; fec_data_size within the
// capacity, every other member's size and the recovered size within fec_data_size; the recovered record goes to the
// out slot of the target's rank when that is below per_group; the group's lanes OR their recovered bits, and lane 0
// writes recovered and out_index.  A line has up to 128 members, not up to 8: the other members' records (one
// contiguous run of count x 20 bytes, the target's among them) are loaded in rounds of kRound in flight, the target
// skipped in the numbering.
//
// Payload lane: its target is the group's q-th erased segment over both mask words, the target's row tgt / col; the
// lane exits unless that row has a line, misses exactly that member and has its parity.  Loads as wide_line<false>
// (rfec_matrix_wide.hip): the parity chunk, then rounds of kRound members -- the round's map words first, then the
// chunks unconditionally and in flight together; a position past the line's end re-reads the parity chunk and is
// XORed as zero.
#include "rfec_families.h"

namespace {

typedef unsigned __int128 u128;

// Loads in flight per round: 45 VGPRs, 8 waves per SIMD.  Rounds of 8 were measured once on the large pool (72
// VGPRs, 7 waves; the positions past a short row's end are requests too) -- one row of 100: 249.5 us against 252.5,
// the ranges overlapping; one row of 10: 291.6 against 270.0.
constexpr int kRound = 4;

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

__device__ __forceinline__ u128 mk128(uint64_t lo, uint64_t hi) { return (u128)lo | (u128)hi << 64; }
__device__ __forceinline__ uint32_t pop128(u128 x)
{
    return (uint32_t)__popcll((uint64_t)x) + (uint32_t)__popcll((uint64_t)(x >> 64));
}
__device__ __forceinline__ uint32_t ffs128(u128 x) // x != 0: the index of its lowest bit
{
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64);
    return lo ? (uint32_t)__ffsll((long long)lo) - 1 : 63u + (uint32_t)__ffsll((long long)hi);
}
__device__ __forceinline__ u128 bit128(uint32_t i) { return (u128)1 << i; } // i < 128
__device__ __forceinline__ u128 low128(uint32_t n) { return n >= 128 ? ~(u128)0 : bit128(n) - 1; }
__device__ __forceinline__ uint32_t rank128(u128 erased, uint32_t i) { return pop128(erased & (bit128(i) - 1)); }

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
            for (uint32_t u0 = 0; u0 + 1 < count; u0 += kRound) {
                uint32_t mem[kRound][5];
                bool use[kRound];
#pragma unroll
                for (int u = 0; u < kRound; ++u) {
                    use[u] = u0 + u + 1 < count;
                    // (a position past the row's end re-reads the meta record and counts as zeros: the loads
                    // stay unconditional)
                    const uint32_t* r = use[u] ? gh + row_other(first, ut, u0 + u) * 5 : mp;
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        mem[u][d] = r[d];
                }
#pragma unroll
                for (int u = 0; u < kRound; ++u) {
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
    for (uint32_t u0 = 0; u0 + 1 < count; u0 += kRound) {
        const v4u* src[kRound];
        bool use[kRound];
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            use[u] = u0 + u + 1 < count;
            src[u] = pool_row(pool, so, use[u] ? row_other(first, ut, u0 + u) : K + r, A.last, C);
        }
        v4u mv[kRound];
#pragma unroll
        for (int u = 0; u < kRound; ++u)
            mv[u] = ld16(src[u]);
#pragma unroll
        for (int u = 0; u < kRound; ++u)
            acc ^= use[u] ? mv[u] : v4u{0, 0, 0, 0};
    }
    st16(A.out_sh + ((size_t)g * A.E + slot) * C + j, acc);
}

__global__ __launch_bounds__(kBlock) void k_decode_rows_wide(RowsWideArgs A)
{
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(A.n_hr, A.every, A.npay8, &hb, &pb)) { // the header blocks: the tables only, never a row
        if (hb < A.n_hdr)
            rows_wide_header_block(A, hb);
        return;
    }
    rows_wide_payload_block(A, pb);
}

} // namespace

extern "C" {

int rfec_rows_wide_col(const rfec_kplan* P)
{
    const uint32_t k = P->k, col = P->n_lines ? P->line[0].count : 0;
    if (col < 2 || k > RFEC_MAX_K)
        return 0;
    const uint32_t nr = (k + col - 1) / col;
    if (P->n_lines != (k - (nr - 1) * col >= 2 ? nr : nr - 1)) // a last row of one segment has no line
        return 0;
    for (uint32_t l = 0; l < P->n_lines; ++l) {
        const uint32_t first = l * col, count = k - first < col ? k - first : col;
        if (P->line[l].stride != 1 || P->line[l].first != first || P->line[l].count != count)
            return 0;
    }
    return (int)col;
}

// rfec_recover_indexed_rows_wide_out (rfec_recover_indexed_rows_wide.c): one launch of k_decode_rows_wide, no
// workspace.  n_rows == 0 (no slot can be present): the header blocks alone, with zero payload lanes -- they still
// write recovered, out_hdr and out_index, and no row is dereferenced.
int rfec_launch_recover_indexed_rows_wide(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                                          const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                          const rfec_hdr* hdr, const uint64_t* present, const rfec_hdr* meta,
                                          const uint16_t* fsize, const uint64_t* parity_present, uint64_t* recovered,
                                          const rfec_dense_out* out, void* stream)
{
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0, K = P->k;
    const uint32_t col = K >= 2 && K <= RFEC_MAX_K && P->n_lines <= RFEC_MAX_LINES ? (uint32_t)rfec_rows_wide_col(P) : 0;
    const uint32_t lg = rfec_header_lanes_log2(P->n_lines);
    if (!col || !groups || !stride || stride % 16 || capacity > stride || !E || E > K ||
        (uint64_t)groups * E * cd >= (1ull << 31) || ((uint64_t)groups << lg) >= (1ull << 32))
        return (int)hipErrorInvalidValue;
    RowsWideArgs A = {};
    A.rows = reinterpret_cast<const v4u*>(rows);
    A.src_of = src_of;
    A.hdr_dw = reinterpret_cast<const uint32_t*>(hdr);
    A.meta_dw = reinterpret_cast<const uint32_t*>(meta);
    A.fsize = fsize, A.present = present, A.parity_present = parity_present, A.recovered = recovered;
    A.out_sh = reinterpret_cast<v4u*>(out->shards);
    A.out_hdr_dw = reinterpret_cast<uint32_t*>(out->hdr);
    A.out_index = out->index;
    A.E = E, A.groups = groups, A.total = n_rows ? groups * E * cd : 0u, A.C = stride / 16, A.capacity = capacity;
    A.last = n_rows ? n_rows - 1 : 0u;
    A.K = K, A.COL = col, A.NL = P->n_lines;
    A.lg = lg, A.n_hdr = blocks_for((uint64_t)groups << lg);
    A.divC = make_fastdiv(cd), A.divQC = make_fastdiv(E * cd), A.divCol = make_fastdiv(col);
    const Rounds8 g = rounds_of_8(A.n_hdr, blocks_for(A.total));
    A.n_hr = g.hdr_rounds, A.every = g.every, A.npay8 = g.npay8;
    rfec_set_indexed_path(7u | K << 8 | col << 16);
    RFEC_LAUNCH(k_decode_rows_wide, dim3(g.grid), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), A);
    return (int)hipGetLastError();
}

} // extern "C"
