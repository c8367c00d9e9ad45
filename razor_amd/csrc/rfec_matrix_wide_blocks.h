// rfec_matrix_wide_blocks.h -- the two block bodies of the wide matrix decode (C++ only).  Not installed.
//
// k_decode_matrix_wide (rfec_matrix_wide.hip, which says how the decode works) and the wide matrix sections of
// k_decode_window_indexed (rfec_cascade.hip) run the same checker block (wide_check_block) and the same payload
// block (wide_payload_block) over a WideArgs: one copy of each, here.  Every address a body forms starts from one of
// WideArgs' bases -- the records and the out slots that carry a cascade's intermediates among them -- so a section
// of a window is this decode with the four output bases moved to the section's first output row.  Internal linkage:
// every unit that includes this header compiles its own.
#ifndef RFEC_MATRIX_WIDE_BLOCKS_H_
#define RFEC_MATRIX_WIDE_BLOCKS_H_

#include "rfec_families.h"
#include "rfec_u128.h"

namespace {

constexpr uint32_t kWideSteps = 23; // a line fires at most once: min(per_group, n_lines) <= 23 steps
// Loads in flight per round (a line has up to 11 members beside its target).  Rounds of 8 were measured: 84 VGPRs,
// 5 waves per SIMD, and the positions past a short line's end are requests too -- k = 10: 217 us against 169,
// k = 17: 159 against 128, k = 40: 106 against 109.
constexpr int kWideRound = 4;

struct WideArgs {
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
    uint32_t K, COL, NR, NL;       // the shape: NR row lines, then NL - NR column lines
    uint64_t col0[2];              // column 0's member mask
    FastDiv divC, divQC, divCol;   // cd, E * cd, COL
    uint32_t n_hr, every, npay8;   // the grid (Rounds8)
};


// line l of the shape: its member mask and its record (first, stride, count)
struct WideShape {
    uint32_t K, COL, NR, NL;
    u128 kmask, col0;
    __device__ u128 row_mask(uint32_t r) const { return ((bit128(COL) - 1) << (r * COL)) & kmask; }
    __device__ u128 col_mask(uint32_t c) const { return (col0 << c) & kmask; }
    __device__ u128 mask(uint32_t l) const { return l < NR ? row_mask(l) : col_mask(l - NR); }
    __device__ void rec(uint32_t l, uint32_t* first, uint32_t* stride, uint32_t* count) const
    {
        const bool row = l < NR;
        const uint32_t c = l - NR;
        *first = row ? l * COL : c;
        *stride = row ? 1u : COL;
        *count = row ? min(COL, K - l * COL) : (K - c + COL - 1) / COL;
    }
};

// The line's members other than its target t, numbered 0 .. count - 2: the p-th is member p of the line before the
// target's position ut and member p + 1 from there on, so a round of loads holds wanted members only.
__device__ __forceinline__ uint32_t wide_other(uint32_t first, uint32_t stride, uint32_t ut, uint32_t p)
{
    return first + (p + (p >= ut ? 1u : 0u)) * stride;
}

__device__ __forceinline__ WideShape wide_shape(const WideArgs& A)
{
    return WideShape{A.K, A.COL, A.NR, A.NL, A.K >= 128 ? ~(u128)0 : bit128(A.K) - 1, mk128(A.col0[0], A.col0[1])};
}

// ---------------------------------------------------------------------------------------------------------------
// The checker: lane = group.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wide_check_block(const WideArgs& A, uint32_t hb)
{
    const uint32_t g = hb * kBlock + threadIdx.x;
    if (g >= A.groups)
        return;
    const WideShape SH = wide_shape(A);
    const uint32_t K = A.K, NL = A.NL, E = A.E;
    const u128 erased = ~mk128(A.present[2 * g], A.present[2 * g + 1]) & SH.kmask;
    u128 have = ~erased & SH.kmask, rm = 0;
    const uint64_t ppm = A.parity_present[g];
    const uint32_t* gh = A.hdr_dw + (size_t)g * K * 5;
    const uint32_t* gm = A.meta_dw + (size_t)g * NL * 5;
    uint32_t* const ob = A.out_hdr_dw + (size_t)g * E * 5;
    uint32_t banned = 0;
    bool progress = true;
#pragma unroll 1
    while (progress) {
        progress = false;
#pragma unroll 1
        for (uint32_t l = 0; l < NL; ++l) {
            const u128 m = SH.mask(l);
            const u128 x = m & ~have;
            if (!((ppm >> l) & 1ull) || ((banned >> l) & 1u) || pop128(x) != 1 || (m & have) == 0)
                continue;
            const uint32_t t = ffs128(x), tr = rank128(erased, t);
            if (tr >= E)
                continue;
            // the step (l, t): fec_data_size, the meta record, the other members' records (a member recovered
            // by an earlier step: from the out slot of its rank, written by this lane)
            uint32_t first, stride, count;
            SH.rec(l, &first, &stride, &count);
            const uint32_t* mp = gm + l * 5;
            const uint32_t L = A.fsize[(size_t)g * NL + l];
            uint32_t rec[5];
#pragma unroll
            for (int d = 0; d < 5; ++d)
                rec[d] = mp[d];
            bool ok = L <= A.capacity;
            const uint32_t ut = l < A.NR ? t - first : fdiv(t, A.divCol); // the target's position on the line
#pragma unroll 1
            for (uint32_t u0 = 0; u0 + 1 < count; u0 += kWideRound) {
                uint32_t mem[kWideRound][5];
                bool use[kWideRound];
#pragma unroll
                for (int u = 0; u < kWideRound; ++u) {
                    const uint32_t i = wide_other(first, stride, ut, u0 + u);
                    use[u] = u0 + u + 1 < count;
                    // (a position past the line's end re-reads the meta record and counts as zeros: the loads stay unconditional)
                    const uint32_t* r = !use[u] ? mp : ((erased >> i) & 1) ? ob + rank128(erased, i) * 5 : gh + i * 5;
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        mem[u][d] = r[d];
                }
#pragma unroll
                for (int u = 0; u < kWideRound; ++u) {
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        rec[d] ^= use[u] ? mem[u][d] : 0u;
                    ok = ok && (!use[u] || (mem[u][4] >> 16) <= L);
                }
            }
            if (!ok || (rec[4] >> 16) > L) { // refused: the peel goes on without this line
                banned |= 1u << l;
                continue;
            }
            uint32_t* oh = ob + tr * 5; // the recovered header record (flex_fec_xor.c:64-85)
#pragma unroll
            for (int d = 0; d < 5; ++d)
                oh[d] = rec[d];
            have |= bit128(t);
            rm |= bit128(t);
            progress = true;
        }
    }
    A.recovered[2 * g] = (uint64_t)rm;
    A.recovered[2 * g + 1] = (uint64_t)(rm >> 64);
    // out_index: the q-th erased segment's index where it was recovered
    u128 e = erased;
#pragma unroll 1
    for (uint32_t q = 0; q < E; ++q) {
        uint32_t ix = 0xFFu;
        if (e) {
            const uint32_t i = ffs128(e);
            e &= e - 1;
            if ((rm >> i) & 1)
                ix = i;
        }
        A.out_index[(size_t)g * E + q] = (uint8_t)ix;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The payload lanes.
// ---------------------------------------------------------------------------------------------------------------

// parity row of line l XOR the line's members other than t, at the lane's chunk (pool: chunk j of row 0; so: the
// group's map words; slot0: the group's out slot 0 at chunk j).  A member that was not received comes from the
// out slot of its rank (kCascade; a line that fires at once has none).  Rounds of kWideRound loads: the map words of
// the round first, then the chunks unconditionally and in flight together; the target is skipped in the numbering
// (wide_other), and a position past the line's end re-reads the parity chunk and is XORed as zero.
template <bool kCascade>
__device__ __forceinline__ v4u wide_line(const WideArgs& A, const WideShape& SH, const v4u* pool,
                                         const uint32_t* __restrict__ so, const v4u* slot0, u128 erased, uint32_t l,
                                         uint32_t t)
{
    uint32_t first, stride, count;
    SH.rec(l, &first, &stride, &count);
    const v4u* pp = pool_row(pool, so, A.K + l, A.last, A.C);
    v4u acc = ld16(pp);
    const uint32_t ut = l < A.NR ? t - first : fdiv(t, A.divCol); // the target's position on the line
#pragma unroll 1
    for (uint32_t u0 = 0; u0 + 1 < count; u0 += kWideRound) {
        const v4u* src[kWideRound];
        bool use[kWideRound];
#pragma unroll
        for (int u = 0; u < kWideRound; ++u) {
            const uint32_t i = wide_other(first, stride, ut, u0 + u);
            use[u] = u0 + u + 1 < count;
            const bool back = kCascade && use[u] && ((erased >> i) & 1); // (its map word is not read)
            src[u] = pool_row(pool, so, use[u] && !back ? i : A.K + l, A.last, A.C);
            if (back)
                src[u] = slot0 + (size_t)rank128(erased, i) * A.C;
        }
        v4u mv[kWideRound];
#pragma unroll
        for (int u = 0; u < kWideRound; ++u)
            mv[u] = ld16(src[u]);
#pragma unroll
        for (int u = 0; u < kWideRound; ++u)
            acc ^= use[u] ? mv[u] : v4u{0, 0, 0, 0};
    }
    return acc;
}

// A schedule of up to kWideSteps steps, packed: the line of step s in 5 bits of `lines`, its target in 7 bits of
// tg0 (steps 0..17) or tg1 (steps 18..22).  No array: nothing is indexed at run time.
struct WideSched {
    uint32_t n;
    u128 lines, tg0;
    uint64_t tg1;
};
__device__ __forceinline__ uint32_t ws_line(const WideSched& S, uint32_t s) { return (uint32_t)(S.lines >> (5 * s)) & 31u; }
__device__ __forceinline__ uint32_t ws_tg(const WideSched& S, uint32_t s)
{
    return s < 18 ? (uint32_t)(S.tg0 >> (7 * s)) & 127u : (uint32_t)(S.tg1 >> (7 * (s - 18))) & 127u;
}

// the canonical schedule over the masks (cascade_schedule without the header checks): lines in plan order to a
// fixpoint, a line fires with its parity received, exactly one member missing and one present; only erased
// segments of rank < E are targets
__device__ __forceinline__ WideSched wide_schedule(const WideShape& SH, u128 have, uint64_t ppm, u128 erased, uint32_t E)
{
    WideSched S = {0, 0, 0, 0};
    bool progress = true;
#pragma unroll 1
    while (progress) {
        progress = false;
#pragma unroll 1
        for (uint32_t l = 0; l < SH.NL; ++l) {
            const u128 m = SH.mask(l);
            const u128 x = m & ~have;
            if (!((ppm >> l) & 1ull) || pop128(x) != 1 || (m & have) == 0 || S.n >= kWideSteps)
                continue;
            const uint32_t t = ffs128(x);
            if (rank128(erased, t) >= E)
                continue;
            S.lines |= (u128)l << (5 * S.n);
            if (S.n < 18)
                S.tg0 |= (u128)t << (7 * S.n);
            else
                S.tg1 |= (uint64_t)t << (7 * (S.n - 18));
            ++S.n;
            have |= bit128(t);
            progress = true;
        }
    }
    return S;
}

__device__ __forceinline__ void wide_payload_block(const WideArgs& A, uint32_t pb)
{
    const uint32_t t = pb * kBlock + threadIdx.x; // (XCD-swizzled: a group's lanes share one L2)
    if (t >= A.total)
        return;
    const uint32_t g = fdiv(t, A.divQC);
    const uint32_t rem = t - g * A.divQC.d;
    uint32_t q = fdiv(rem, A.divC);
    const uint32_t j = rem - q * A.divC.d;
    const WideShape SH = wide_shape(A);
    const uint32_t K = A.K, NR = A.NR, NL = A.NL, C = A.C;
    const uint64_t h0 = A.present[2 * g], h1 = A.present[2 * g + 1];
    const uint64_t ppm = A.parity_present[g];
    const u128 have = mk128(h0, h1) & SH.kmask, erased = ~have & SH.kmask;
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
    const u128 tb = bit128(tgt);
    const uint32_t r = fdiv(tgt, A.divCol), c = tgt - r * A.COL;
    const u128 rmk = SH.row_mask(r), cmk = SH.col_mask(c);
    const bool row_fires = r < NR && ((ppm >> r) & 1ull) && (rmk & erased) == tb && (rmk & have) != 0;
    const bool col_fires = NR + c < NL && ((ppm >> (NR + c)) & 1ull) && (cmk & erased) == tb && (cmk & have) != 0;
    const v4u* pool = A.rows + j;
    const uint32_t* so = A.src_of + (size_t)g * (K + NL);
    v4u* slot0 = A.out_sh + (size_t)g * A.E * C + j;
    v4u* dst = slot0 + (size_t)slot * C;
    if (row_fires || col_fires) { // single level
        st16(dst, wide_line<false>(A, SH, pool, so, slot0, erased, row_fires ? r : NR + c, tgt));
        return;
    }
    // a cascade: the mask schedule, the steps the target's step reads (transitively), replayed in step order
    const WideSched S = wide_schedule(SH, have, ppm, erased, A.E);
    uint32_t ss = kWideSteps;
#pragma unroll 1
    for (uint32_t s = 0; s < S.n; ++s)
        if (ws_tg(S, s) == tgt)
            ss = s;
    if (ss == kWideSteps)
        return; // not recoverable
    uint32_t need = 1u << ss;
    u128 want = SH.mask(ws_line(S, ss)) & erased & ~tb; // the recovered members the closure's steps read
#pragma unroll 1
    for (int s = (int)ss - 1; s >= 0; --s) {
        const uint32_t ts = ws_tg(S, (uint32_t)s);
        if (!((want >> ts) & 1))
            continue;
        need |= 1u << s;
        want |= SH.mask(ws_line(S, (uint32_t)s)) & erased & ~bit128(ts);
    }
#pragma unroll 1
    for (uint32_t s = 0; s <= ss; ++s) {
        if (!((need >> s) & 1u))
            continue;
        const uint32_t ts = ws_tg(S, s);
        const v4u acc = wide_line<true>(A, SH, pool, so, slot0, erased, ws_line(S, s), ts);
        // (an intermediate goes to the out slot of its rank: this lane reads it back, the slot's owner writes the
        // same bytes; the last step's target is this lane's own slot)
        st16(slot0 + (size_t)rank128(erased, ts) * C, acc);
    }
}

} // namespace

#endif
