// rfec_encode.hip -- the encode kernels of the flex-FEC engine (gfx950) and their launchers; rfec_kernels.hip
// picks among them (rfec_launch_encode).
//
// Arithmetic restated from the reference (yuanrongxi/razor):
//   parity payload  = XOR of zero-padded member payloads  flex_fec_xor.c:30-32, 46-49
//   parity meta     = XOR of member headers, max data_size flex_fec_xor.c:13-26, 37-44
//
// Device layout (include/razor_fec.h): payload slots of `stride` bytes
// (multiple of 16), zero beyond data_size.  All arithmetic is wave64
// v_xor_b32 on dwordx4 registers (no MFMA: XOR is ~0.06 op/B, HBM-bound).
// Every payload load and store is non-temporal (measured best for both
// directions of the encode -> decode alternation).
//
//  encode (one launch; meta blocks at the head of the grid XOR the 20-byte
//  header records of up to 64 groups staged in LDS, one lane per (group, line)):
//    * row layouts (the sender's row layer, strip mode): k_encode_out, one
//      lane per PARITY chunk loading its row's members, XCD-swizzled blocks;
//    * the sender's full rows + columns plan (k = 6..16): k_encode_matrix_out,
//      one lane per PARITY chunk (group, line, chunk), member loads at the
//      default policy so a column's lanes re-read its members from L2 (at the
//      10 : 7 read / write mix's streaming ceiling, rfec_probe_mix);
//    * any other plan: k_encode (plan-driven).
#include "rfec_families.h"

namespace {

// ---------------------------------------------------------------------------
// Encode meta blocks: fec_meta = XOR of the member headers taken as five
// dwords (field-wise XOR, flex_fec_xor.c:13-20, 37-44), fec_data_size = max
// data_size (:22-26), status -1 where flex_fec_generate fails (:9-10, :27-28).
// ---------------------------------------------------------------------------
// (lds: kMetaDwords, 16-byte aligned; nt: the block's threads)
__device__ void meta_block_in(uint32_t* lds, uint32_t nt, uint32_t mb, const uint32_t* __restrict__ hdr_dw,
                              uint32_t* __restrict__ meta_dw, uint16_t* __restrict__ fsize,
                              int8_t* __restrict__ status, uint32_t groups, uint32_t capacity, uint32_t gpb,
                              const rfec_kplan& P)
{
    const uint32_t K = P.k, NL = P.n_lines;
    const uint32_t g0 = mb * gpb;
    const uint32_t ng = min(gpb, groups - g0);
    stage_dwords(lds, hdr_dw + (size_t)g0 * K * 5, ng * K * 5, nt);
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < ng * NL; o += nt) {
        const uint32_t gl = o / NL, l = o - gl * NL;
        const rfec_line ln = P.line[l];
        const uint32_t* h = lds + gl * K * 5;
        uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, L = 0;
        for (uint32_t q = 0; q < ln.count; ++q) {
            const uint32_t* r = h + (ln.first + q * ln.stride) * 5;
            m0 ^= r[0];
            m1 ^= r[1];
            m2 ^= r[2];
            m3 ^= r[3];
            m4 ^= r[4];
            L = max(L, r[4] >> 16);
        }
        const size_t out = (size_t)g0 * NL + o;
        uint32_t* d = meta_dw + out * 5;
        d[0] = m0;
        d[1] = m1;
        d[2] = m2;
        d[3] = m3;
        d[4] = m4;
        fsize[out] = (uint16_t)L;
        if (status)
            status[out] = (ln.count <= 1 || L > capacity) ? (int8_t)-1 : (int8_t)0;
    }
}

__device__ void meta_block(uint32_t mb, const uint32_t* __restrict__ hdr_dw, uint32_t* __restrict__ meta_dw,
                           uint16_t* __restrict__ fsize, int8_t* __restrict__ status, uint32_t groups,
                           uint32_t capacity, uint32_t gpb, const rfec_kplan& P)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[kMetaDwords];
    meta_block_in(lds, kBlock, mb, hdr_dw, meta_dw, fsize, status, groups, capacity, gpb, P);
}

// Grid of the swizzled encodes: head / 8 rounds of 8 meta blocks spread over
// the payload rounds (header_block_xcd; the payload part of the grid is whole
// rounds of 8), so the meta blocks' latency-bound header stages overlap the
// payload stream instead of holding the whole GPU at the start of the launch:
// c5 (k = 32 / 256 B, 8 % header bytes) 113.4-113.6 vs 117.9-119.4 us, c3
// 161.7-162.2 vs 162.8-163.4 us (round 5, profiles/r05/ab/enc_meta_spread/).
// Returns false for meta / padding blocks (meta work done), else the logical
// payload block.
__device__ __forceinline__ bool enc_payload_block(const EncMeta& E, uint32_t head, const rfec_kplan& P, uint32_t* b)
{
    const uint32_t n_mr = head >> 3, npay8 = gridDim.x - head;
    const uint32_t every = n_mr ? (npay8 >> 3) / n_mr : 0u;
    uint32_t mb;
    if (header_block_xcd(n_mr, every, npay8, &mb, b)) {
        if (mb < E.n_meta_blocks)
            meta_block(mb, E.hdr_dw, E.meta_dw, E.fsize, E.status, E.groups, E.capacity, E.gpb, P);
        return false;
    }
    return true;
}

// ---------------------------------------------------------------------------
// Encode payload, generic plan: one lane per (group, chunk column), every
// line's members loaded in turn.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_encode(const v4u* __restrict__ shards, v4u* __restrict__ parity,
                                                   uint32_t total, uint32_t C, FastDiv divC, EncMeta E, rfec_kplan P)
{
    if (blockIdx.x < E.n_meta_blocks) {
        meta_block(blockIdx.x, E.hdr_dw, E.meta_dw, E.fsize, E.status, E.groups, E.capacity, E.gpb, P);
        return;
    }
    const uint32_t t = (blockIdx.x - E.n_meta_blocks) * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divC);
    const uint32_t j = t - g * divC.d; // chunk column (divC.d = chunks of work per slot)
    const v4u* src = shards + (size_t)g * P.k * C + j;
    v4u* dst = parity + (size_t)g * P.n_lines * C + j;
    for (uint32_t l = 0; l < P.n_lines; ++l) {
        const rfec_line ln = P.line[l];
        const v4u* s = src + (size_t)ln.first * C;
        const size_t step = (size_t)ln.stride * C;
        v4u acc = ld16(s);
        uint32_t q = 1;
        for (; q + 4 <= ln.count; q += 4) { // four loads in flight
            const v4u a = ld16(s + q * step), b = ld16(s + (q + 1) * step);
            const v4u c = ld16(s + (q + 2) * step), d = ld16(s + (q + 3) * step);
            acc ^= (a ^ b) ^ (c ^ d);
        }
        for (; q < ln.count; ++q)
            acc ^= ld16(s + q * step);
        st16(dst + (size_t)l * C, acc);
    }
}

// ---------------------------------------------------------------------------
// Encode payload, the reference sender's full matrix plan at small k
// (flex_fec_sender.c:166-233: rows of COL consecutive segments, then columns
// strided by COL, lines with fewer than 2 members dropped), K = 6..16 (COL =
// 3 or 4, as flex_fec_sender_num_packets picks); MatrixShape (rfec_families.h)
// = its compile-time line layout.
// Output-mapped form of the full matrix encode: one lane per PARITY chunk
// (group, line, chunk column), as k_encode_out, so that every wave's store is
// 1 KiB of consecutive parity bytes (whole 128-B lines when the slots are
// packed) instead of seven 1 KiB runs that start and end inside lines shared
// with the neighbouring waves.  Each member is loaded by its row's lanes and
// again by its column's lanes one block or so later, on the same XCD, so HBM
// should still see every member once (PMC: 1.018 x algorithmic).  Row l <
// NR: members l COL + q; column c = l - NR: c + q COL (K >= 2 COL here, so no
// column has fewer than 2 members).  Loads take the default policy: the
// column lanes' second reads are meant to hit L2.  At c3 full (10 reads : 7
// writes per group) 228-230 us with the unused member slots predicated off
// through a buffer descriptor (round 5; 234-237 us when they re-read member
// 0; non-temporal loads on the rows, the columns or both: 239-242 us,
// profiles/r05/ab/encode_pred/).
// Measured slower: one lane per (group, chunk) loading each member once, all
// seven parity chunks through LDS and stored as one contiguous run per block
// (238-239 us, round 4); the same with seven direct stores per lane (252-260
// us, round 2: every 1-KiB store run starts and ends inside lines that the
// neighbouring waves write).
template <int K, int COL>
__global__ __launch_bounds__(kBlock) void k_encode_matrix_out(const v4u* __restrict__ shards,
                                                              v4u* __restrict__ parity, uint32_t total, uint32_t C,
                                                              FastDiv divC, FastDiv divLC, uint32_t head, EncMeta E,
                                                              rfec_kplan P)
{
    using Sh = MatrixShape<K, COL>;
    constexpr int NR = Sh::n_rows(), R = Sh::R, M = COL > R ? COL : R;
    static_assert(K >= 2 * COL && Sh::n_lines() == NR + COL, "every column has >= 2 members");
    uint32_t b;
    if (!enc_payload_block(E, head, P, &b))
        return;
    const uint32_t t = b * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divLC);
    const uint32_t rem = t - g * divLC.d;
    const uint32_t l = fdiv(rem, divC);
    const uint32_t j = rem - l * divC.d;
    const bool row = l < (uint32_t)NR;
    const uint32_t c = l - NR;
    const uint32_t first = row ? l * COL : c, step = row ? 1u : (uint32_t)COL;
    const uint32_t count = row ? min((uint32_t)COL, K - l * COL) : (K - c + COL - 1) / COL;
    // member loads through a descriptor over the wave's first group, an unused
    // slot predicated off (kNoLoad reads 0 without a memory access), default
    // policy: the column lanes' second reads are meant to hit L2
    const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    const __amdgpu_buffer_rsrc_t rs = wave_rsrc(shards + (size_t)gb * K * C);
    const uint32_t o0 = (((g - gb) * K + first) * C + j) * 16u;
    v4u v[M];
#pragma unroll
    for (int q = 0; q < M; ++q)
        v[q] = bld16_l2(rs, (uint32_t)q < count ? o0 + (uint32_t)q * step * C * 16u : kNoLoad);
    v4u acc = v[0];
#pragma unroll
    for (int q = 1; q < M; ++q)
        acc ^= v[q];
    st16(parity + ((size_t)g * (NR + COL) + l) * C + j, acc);
}

// ---------------------------------------------------------------------------
// Encode payload, rows-of-COL, output-mapped (default for row layouts): one
// lane per PARITY chunk (group, row, chunk column), the lane loads its row's
// COL (last row: K - (R-1)*COL) member chunks and stores one chunk.  Lane t
// writes parity chunk t when the slots are packed (stride == capacity), so
// every wave's store is 1 KiB of consecutive, 128-B-aligned parity bytes:
// whole lines, never two partial writes of one line from two waves on two
// XCDs, which a flat (group, chunk) mapping makes at every 1,200-B slot
// edge.  Row layouts have no member in two lines, so no chunk is loaded twice.
// 165-171 us vs 178-211 us flat at k = 10 / 1,200 B, equal to a 10-read :
// 3-write probe over contiguous streams; XCD-swizzled blocks: 168 vs 172 us,
// HBM traffic 1.029 vs 1.059 x algorithmic.  Round 5: the last row's absent
// members predicated off through a buffer descriptor instead of per-load
// branches: 163-166 vs 166-168 us (profiles/r05/ab/encode_pred/).
// ---------------------------------------------------------------------------
template <int K, int COL>
__global__ __launch_bounds__(kBlock) void k_encode_out(const v4u* __restrict__ shards, v4u* __restrict__ parity,
                                                       uint32_t total, uint32_t C, FastDiv divC, FastDiv divRC,
                                                       uint32_t head, EncMeta E, rfec_kplan P)
{
    constexpr int R = (K + COL - 1) / COL;
    constexpr int LAST = K - (R - 1) * COL;
    uint32_t b;
    if (!enc_payload_block(E, head, P, &b))
        return;
    const uint32_t t = b * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t g = fdiv(t, divRC);
    const uint32_t rem = t - g * divRC.d;
    const uint32_t r = fdiv(rem, divC);
    const uint32_t j = rem - r * divC.d;
    // member loads predicated through a descriptor (the last row's missing
    // members read 0 without a memory access), not per-load branches
    const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    const __amdgpu_buffer_rsrc_t rs = wave_rsrc(shards + (size_t)gb * K * C);
    const uint32_t o0 = (((g - gb) * K + r * COL) * C + j) * 16u;
    v4u v[COL];
#pragma unroll
    for (int q = 0; q < COL; ++q)
        v[q] = bld16(rs, (q < LAST || r < (uint32_t)(R - 1)) ? o0 + (uint32_t)q * C * 16u : kNoLoad);
    v4u acc = v[0];
#pragma unroll
    for (int q = 1; q < COL; ++q)
        acc ^= v[q];
    st16(parity + ((size_t)g * R + r) * C + j, acc);
}

// The same for any row layout with rows of at most CMAX members (k, col
// runtime: the strip-mode plans of flex_fec_sender_num_packets, :112-132);
// the lane's member loads stay unrolled, predicated on the row's size.
template <int CMAX>
__global__ __launch_bounds__(kBlock) void k_encode_out_rt(const v4u* __restrict__ shards, v4u* __restrict__ parity,
                                                          uint32_t total, uint32_t C, FastDiv divC, FastDiv divRC,
                                                          uint32_t K, uint32_t COL, uint32_t head, EncMeta E,
                                                          rfec_kplan P)
{
    uint32_t b;
    if (!enc_payload_block(E, head, P, &b))
        return;
    const uint32_t t = b * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t R = divRC.d / divC.d;
    const uint32_t g = fdiv(t, divRC);
    const uint32_t rem = t - g * divRC.d;
    const uint32_t r = fdiv(rem, divC);
    const uint32_t j = rem - r * divC.d;
    const uint32_t cnt = r + 1 < R ? COL : K - (R - 1) * COL;
    const v4u* s = shards + ((size_t)g * K + (size_t)r * COL) * C + j;
    v4u v[CMAX];
#pragma unroll
    for (int q = 0; q < CMAX; ++q) {
        v[q] = v4u{0, 0, 0, 0};
        if ((uint32_t)q < cnt)
            v[q] = ld16(s + (size_t)q * C);
    }
    v4u acc = v[0];
#pragma unroll
    for (int q = 1; q < CMAX; ++q)
        acc ^= v[q];
    st16(parity + ((size_t)g * R + r) * C + j, acc);
}

// the swizzled encodes' grid: the meta blocks padded to whole rounds of 8 (`head` blocks: enc_payload_block
// spreads them itself), then the payload blocks for `total` lanes in whole rounds of 8
inline Rounds8 enc_grid(const EncLaunch& a, uint32_t total) { return rounds_of_8(a.E.n_meta_blocks, blocks_for(total)); }

} // namespace

hipError_t launch_encode_rows(const EncLaunch& a, uint32_t col, bool rsrc_ok)
{
    const uint32_t K = a.P->k, R = (K + col - 1) / col, C = a.stride / 16;
    const uint32_t total = a.groups * R * a.cd; // < 2^32: checked by the caller
    const Rounds8 g = enc_grid(a, total);
    const uint32_t head = 8u * g.hdr_rounds;
    const dim3 grid(g.grid);
    const FastDiv dC = make_fastdiv(a.cd), dRC = make_fastdiv(R * a.cd);
    if (col == 4 && rsrc_ok && (K == 10 || K == 32)) {
        RFEC_TAG(RFEC_PATH_ENC_ROWS, K);
        if (K == 10)
            RFEC_LAUNCH((k_encode_out<10, 4>), grid, dim3(kBlock), 0, a.stream, a.s, a.p, total, C, dC, dRC, head, a.E,
                        *a.P);
        else
            RFEC_LAUNCH((k_encode_out<32, 4>), grid, dim3(kBlock), 0, a.stream, a.s, a.p, total, C, dC, dRC, head, a.E,
                        *a.P);
        return hipGetLastError();
    }
    // other row layouts: the same output-mapped lanes with k and col at run time
    // (an 8-wide instantiation compiled to 230 VGPRs, two waves per SIMD: 0.33 of 8 TB/s at k = 20,
    // col = 5, so rows of 5..16 take the 16-wide one, 74 VGPRs)
    RFEC_TAG(RFEC_PATH_ENC_ROWS_RT, col <= 4 ? 4 : 16);
    if (col <= 4)
        RFEC_LAUNCH((k_encode_out_rt<4>), grid, dim3(kBlock), 0, a.stream, a.s, a.p, total, C, dC, dRC, K, col, head,
                    a.E, *a.P);
    else
        RFEC_LAUNCH((k_encode_out_rt<16>), grid, dim3(kBlock), 0, a.stream, a.s, a.p, total, C, dC, dRC, K, col, head,
                    a.E, *a.P);
    return hipGetLastError();
}

hipError_t launch_encode_matrix(const EncLaunch& a)
{
    const rfec_kplan* P = a.P;
    const uint32_t nl = P->n_lines, tot = a.groups * nl * a.cd; // < 2^32: checked by the caller
    const Rounds8 g = enc_grid(a, tot);
    const uint32_t head = 8u * g.hdr_rounds;
    const dim3 grid_o(g.grid);
#define RFEC_MX(KK, CC)                                                                                           \
    case KK:                                                                                                      \
        RFEC_TAG(RFEC_PATH_ENC_MATRIX, KK);                                                                       \
        RFEC_LAUNCH((k_encode_matrix_out<KK, CC>), grid_o, dim3(kBlock), 0, a.stream, a.s, a.p, tot, a.stride / 16, \
                    make_fastdiv(a.cd), make_fastdiv(nl * a.cd), head, a.E, *P);                                  \
        return hipGetLastError();
    switch (P->k) {
        RFEC_MATRIX_SHAPES(RFEC_MX)
    default: break;
    }
#undef RFEC_MX
    return hipErrorInvalidValue; // (not reached: the dispatch sends k = 6..16 only)
}

hipError_t launch_encode_plan(const EncLaunch& a)
{
    const uint32_t total = a.groups * a.cd;
    RFEC_TAG(RFEC_PATH_ENC_PLAN, 0);
    RFEC_LAUNCH(k_encode, dim3(a.E.n_meta_blocks + blocks_for(total)), dim3(kBlock), 0, a.stream, a.s, a.p, total,
                a.stride / 16, make_fastdiv(a.cd), a.E, *a.P);
    return hipGetLastError();
}
