// rfec_deliver.hip -- CDNA4 (gfx950) kernels of rfec_recover_deliver (razor_fec.h): the dense outputs of
// rfec_recover_indexed_shapes_out -- section order, per_group out slots a row, holes where out_index is 0xFF -- into
// the list a receiver uses: one rfec_rx_seg record and one payload row per recovered segment, in window order and,
// within a group, in out-slot order.
//
// The rule is a pure function of the tables (razor_fec.h, "The rule" of rfec_recover_deliver): window group g with
// shape_of[g] = p and rank_of[g] = c < groups[p] has output row o = first[p] + c, delivers the n_g slots of that row
// whose out_index is not 0xFF, and its first entry is first_of[g], the sum of n_g' over g' < g.
//
// Three launches on the caller's stream, two for a window of at most kBlock groups; no launch has a lane read a word
// that another lane of that launch writes (a launch boundary makes the words of the launch before visible), and no
// lane waits on another workgroup:
//   k_deliver_count   one lane per window group: n_g from the row's index bytes; a scan within the workgroup (the
//                     wave's by shuffles, the workgroup's four waves through LDS) leaves the group's exclusive prefix
//                     within its block in local[g] and the block's total in blk[b].  A window of one block is done
//                     here: blk[0] = 0, first_of[G] and n_out
//   k_deliver_totals  one workgroup: blk[] (at most 256 words at 65,535 groups) to its exclusive prefix in place (a
//                     lane reads and writes its own word only), first_of[G] and n_out
//   k_deliver         one grid, header blocks then payload blocks: a lane per window group writes first_of[g] =
//                     local[g] + blk[g / kBlock]; a lane per out slot (o, e) that delivers writes the rfec_rx_seg of
//                     its entry as six words; a lane per (o, e, chunk) moves 16 bytes.  A slot lane finds its entry
//                     from the slot side: the section of o by wave-uniform compares over first[] (section_of /
//                     for_plan, as rfec_regroup_shapes.hip), g = group_of[p][o - first[p]], j = local[g] +
//                     blk[g / kBlock] + the delivering slots before e in the row.  Lanes of a 0xFF slot, of a row
//                     with no group (group_of >= G) and of an entry j >= max_out leave before any payload load.
// Payload policy: ld16 / st16 (non-temporal), the project's payload-stream policy.  Every byte is touched once here;
// the rows were written by another launch and the delivered rows are read next by a copy engine or by a consumer
// kernel on any XCD, for which a line kept in this XCD's L2 is no help, and gfx950's nt stores write through the
// same path as plain ones.  The index bytes and the two scan words are plain loads: CD lanes of a slot share them.
// The sections' group_of pointers and first[] travel as kernel arguments (392 bytes).  Row addresses are 64-bit.
#include "rfec_regroup_rules.h"

// rfec_indexed_last_path's tag (rfec_internal.h), kept in rfec_kernels.hip and declared for the other units in
// rfec_families.h, which this unit does without
#pragma GCC visibility push(hidden)
void rfec_set_indexed_path(uint32_t path);
#pragma GCC visibility pop

namespace {

constexpr uint32_t kShapes = RFEC_RECOVER_MAX_SHAPES;
constexpr uint32_t kHole = 0xFFu;
constexpr uint32_t kSegWords = 6;
static_assert(sizeof(rfec_rx_seg) == 4 * kSegWords && sizeof(rfec_hdr) == 20, "rfec_rx_seg: the header, then fec_id");
static_assert(kBlock == 4 * kWave, "k_deliver_count and k_deliver_totals scan four waves");
static_assert((65535 + kBlock - 1) / kBlock <= kBlock, "k_deliver_totals: one lane per block of k_deliver_count");

// the decode's rows: section p has output rows [first[p], first[p + 1])
struct Sect {
    const uint32_t* group_of[kShapes];
    uint32_t first[kShapes + 1];
    uint32_t n_plans;
};
struct Deliver {
    const v4u* out_sh;       // [R][E][C]
    const uint32_t* out_hdr; // [R][E][5]
    const uint8_t* out_index; // [R][E]
    uint32_t* seg;           // [max_out][6]
    v4u* pay;                // [max_out][C]
    uint32_t* first_of;      // [G + 1]
    const uint32_t* local;   // [G]: workspace
    const uint32_t* blk;     // [blocks of G]: workspace
    uint32_t G, E, C, cd, max_out, fec_id0;
    uint32_t n_slots, n_pay, hdr_blocks; // R E; R E cd; blocks of the G + R E header lanes
    FastDiv divE, divCD;
};
static_assert(sizeof(Sect) + sizeof(Deliver) <= 4096 && sizeof(Sect) + 16 * sizeof(void*) <= 4096,
              "the argument block (k_deliver; k_deliver_count)");

// the section whose rows hold row o (o < first[n_plans]; empty sections hold none)
__device__ __forceinline__ uint32_t section_of(const uint32_t* first, uint32_t n_plans, uint32_t o)
{
    uint32_t p = 0;
    while (p + 1 < n_plans && o >= first[p + 1])
        ++p;
    return p;
}
// body(p0) once per section among the wave's lanes, for the lanes of that section, with p0 wave-uniform: what body
// reads of the argument block by p0 comes through scalar loads
template <class F>
__device__ __forceinline__ void for_plan(uint32_t p, F&& body)
{
    for (;;) {
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
        if (p == p0) {
            body(p0);
            break;
        }
    }
}

// Exclusive prefix of x over the workgroup's kBlock lanes (every lane calls it) and the workgroup's total.
__device__ __forceinline__ uint32_t block_scan(uint32_t x, uint32_t* total)
{
    __shared__ uint32_t wave_sum[kBlock / kWave];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    uint32_t incl = x;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, kWave);
        if (lane >= d)
            incl += v;
    }
    if (lane == kWave - 1)
        wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kBlock / kWave; ++i) {
        const uint32_t s = wave_sum[i];
        before += i < w ? s : 0u;
        all += s;
    }
    *total = all;
    return before + incl - x;
}

// single: the window is one block, so this launch also writes what k_deliver_totals would
__global__ __launch_bounds__(kBlock) void k_deliver_count(const Sect S, uint32_t G, uint32_t E,
                                                          const uint8_t* __restrict__ shape_of,
                                                          const uint32_t* __restrict__ rank_of,
                                                          const uint8_t* __restrict__ out_index,
                                                          uint32_t* __restrict__ local, uint32_t* __restrict__ blk,
                                                          uint32_t* __restrict__ first_of, uint32_t* __restrict__ n_out,
                                                          uint32_t single)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    uint32_t n = 0;
    if (g < G) {
        const uint32_t p = shape_of[g], c = rank_of[g];
        if (p < S.n_plans)
            for_plan(p, [&](uint32_t p0) {
                const uint32_t first = S.first[p0];
                if (c >= S.first[p0 + 1] - first)
                    return; // a rank past the rows decoded (RFEC_REGROUP_NONE among them)
                const uint8_t* ix = out_index + (first + c) * E; // R E < 2^31
                for (uint32_t e = 0; e < E; ++e)
                    n += ix[e] != kHole;
            });
    }
    uint32_t total;
    const uint32_t before = block_scan(n, &total);
    if (g < G)
        local[g] = before;
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = single ? 0u : total;
        if (single) {
            first_of[G] = total;
            *n_out = total;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_deliver_totals(uint32_t* __restrict__ blk, uint32_t n_blk, uint32_t G,
                                                           uint32_t* __restrict__ first_of,
                                                           uint32_t* __restrict__ n_out)
{
    const uint32_t t = threadIdx.x;
    const uint32_t x = t < n_blk ? blk[t] : 0u;
    uint32_t total;
    const uint32_t before = block_scan(x, &total);
    if (t < n_blk)
        blk[t] = before;
    if (t == 0) {
        first_of[G] = total;
        *n_out = total;
    }
}

__global__ __launch_bounds__(kBlock) void k_deliver(const Sect S, const Deliver D)
{
    uint32_t s, chunk = 0;
    const bool header = blockIdx.x < D.hdr_blocks;
    if (header) {
        uint32_t t = blockIdx.x * kBlock + threadIdx.x;
        if (t < D.G) {
            D.first_of[t] = D.local[t] + D.blk[t / kBlock];
            return;
        }
        t -= D.G;
        if (t >= D.n_slots)
            return;
        s = t;
    } else {
        const uint32_t t = (blockIdx.x - D.hdr_blocks) * kBlock + threadIdx.x;
        if (t >= D.n_pay)
            return;
        s = fdiv(t, D.divCD);
        chunk = t - s * D.cd;
    }
    if (D.out_index[s] == kHole)
        return;
    const uint32_t o = fdiv(s, D.divE), e = s - o * D.E;
    const uint8_t* ix = D.out_index + o * D.E;
    uint32_t j = 0; // the delivering slots of the row before this one
    for (uint32_t q = 0; q < e; ++q)
        j += ix[q] != kHole;
    uint32_t g = kNone;
    for_plan(section_of(S.first, S.n_plans, o), [&](uint32_t p) { g = S.group_of[p][o - S.first[p]]; });
    if (g >= D.G)
        return; // a row past the section's groups (RFEC_REGROUP_NONE), or a broken table: nothing is read by it
    j += D.local[g] + D.blk[g / kBlock];
    if (j >= D.max_out)
        return;
    if (header) {
        const uint32_t* h = D.out_hdr + (size_t)s * 5;
        uint32_t* r = D.seg + (size_t)j * kSegWords;
#pragma unroll
        for (int q = 0; q < 5; ++q)
            r[q] = h[q];
        r[5] = fec_id_of(D.fec_id0, g); // reserved = 0 in the high half
    } else
        st16(D.pay + (size_t)j * D.C + chunk, ld16(D.out_sh + (size_t)s * D.C + chunk));
}

// rfec_recover_deliver_each: the same three launches over the outputs of rfec_recover_indexed_window_each_out, whose
// section p has E[p] out slots a row and the sections' slots packed end to end: out slot e of row c of section p is
// slot slot_first[p] + c E[p] + e, slot_first[p] the sum of groups[q] E[q] over q < p.  k_deliver_totals is the one
// above.  A slot lane finds its section by wave-uniform compares over slot_first[] and its (row, e) by the section's
// own FastDiv, read through scalar loads inside for_plan (three words and a v_mul_hi_u32; the compiler's division by
// a run-time E is a reciprocal sequence of some twenty VALU instructions per lane).
struct SectEach {
    const uint32_t* group_of[kShapes];
    uint32_t first[kShapes + 1];      // rows
    uint32_t slot_first[kShapes + 1]; // out slots
    uint32_t E[kShapes];              // out slots a row (a section without rows: 1)
    FastDiv divE[kShapes];
    uint32_t n_plans;
};
static_assert(sizeof(SectEach) + sizeof(Deliver) <= 4096 && sizeof(SectEach) + 16 * sizeof(void*) <= 4096,
              "the argument block (k_deliver_each; k_deliver_count_each)");

__global__ __launch_bounds__(kBlock) void k_deliver_count_each(const SectEach S, uint32_t G,
                                                               const uint8_t* __restrict__ shape_of,
                                                               const uint32_t* __restrict__ rank_of,
                                                               const uint8_t* __restrict__ out_index,
                                                               uint32_t* __restrict__ local, uint32_t* __restrict__ blk,
                                                               uint32_t* __restrict__ first_of,
                                                               uint32_t* __restrict__ n_out, uint32_t single)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    uint32_t n = 0;
    if (g < G) {
        const uint32_t p = shape_of[g], c = rank_of[g];
        if (p < S.n_plans)
            for_plan(p, [&](uint32_t p0) {
                if (c >= S.first[p0 + 1] - S.first[p0])
                    return; // a rank past the rows decoded (RFEC_REGROUP_NONE among them)
                const uint32_t E = S.E[p0];
                const uint8_t* ix = out_index + (S.slot_first[p0] + c * E); // slots < 2^31
                for (uint32_t e = 0; e < E; ++e)
                    n += ix[e] != kHole;
            });
    }
    uint32_t total;
    const uint32_t before = block_scan(n, &total);
    if (g < G)
        local[g] = before;
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = single ? 0u : total;
        if (single) {
            first_of[G] = total;
            *n_out = total;
        }
    }
}

// (D.E and D.divE are not used: the section's own)
__global__ __launch_bounds__(kBlock) void k_deliver_each(const SectEach S, const Deliver D)
{
    uint32_t s, chunk = 0;
    const bool header = blockIdx.x < D.hdr_blocks;
    if (header) {
        uint32_t t = blockIdx.x * kBlock + threadIdx.x;
        if (t < D.G) {
            D.first_of[t] = D.local[t] + D.blk[t / kBlock];
            return;
        }
        t -= D.G;
        if (t >= D.n_slots)
            return;
        s = t;
    } else {
        const uint32_t t = (blockIdx.x - D.hdr_blocks) * kBlock + threadIdx.x;
        if (t >= D.n_pay)
            return;
        s = fdiv(t, D.divCD);
        chunk = t - s * D.cd;
    }
    if (D.out_index[s] == kHole)
        return;
    uint32_t g = kNone, e = 0, row0 = 0; // the group of the slot's row, the slot within it, the row's first slot
    for_plan(section_of(S.slot_first, S.n_plans, s), [&](uint32_t p) {
        const uint32_t sf = S.slot_first[p], E = S.E[p], c = fdiv(s - sf, S.divE[p]);
        e = s - sf - c * E;
        row0 = s - e;
        g = S.group_of[p][c]; // c < groups[p]: s < slot_first[p + 1]
    });
    if (g >= D.G)
        return; // a row past the section's groups (RFEC_REGROUP_NONE), or a broken table: nothing is read by it
    const uint8_t* ix = D.out_index + row0;
    uint32_t j = D.local[g] + D.blk[g / kBlock]; // + the delivering slots of the row before this one
    for (uint32_t q = 0; q < e; ++q)
        j += ix[q] != kHole;
    if (j >= D.max_out)
        return;
    if (header) {
        const uint32_t* h = D.out_hdr + (size_t)s * 5;
        uint32_t* r = D.seg + (size_t)j * kSegWords;
#pragma unroll
        for (int q = 0; q < 5; ++q)
            r[q] = h[q];
        r[5] = fec_id_of(D.fec_id0, g); // reserved = 0 in the high half
    } else
        st16(D.pay + (size_t)j * D.C + chunk, ld16(D.out_sh + (size_t)s * D.C + chunk));
}

} // namespace

// The caller (rfec_recover_deliver.c) has checked n_plans in [1, 32], window_groups in [1, 65535], fec_id0 in
// [1, 65535], stride a multiple of 16, capacity <= stride, per_group >= 1, first[n_plans] * per_group * CD < 2^31 and
// the pointers (group_of of every section with rows; the decode's outputs when there are rows; seg and seg_payload
// when max_out > 0); hipErrorInvalidValue otherwise.  first: host [n_plans + 1], the prefix of the sections' rows.
// workspace: rfec_recover_deliver_workspace_size's bytes, local[G] then blk[] from the next multiple of 16.
extern "C" int rfec_launch_recover_deliver(const rfec_regroup_section* sections, uint32_t n_plans,
                                           const uint32_t* first, uint32_t groups, uint32_t fec_id0,
                                           const uint8_t* shape_of, const uint32_t* rank_of, uint32_t stride,
                                           uint32_t capacity, uint32_t per_group, const uint8_t* out_shards,
                                           const rfec_hdr* out_hdr, const uint8_t* out_index, uint32_t max_out,
                                           rfec_rx_seg* seg, uint8_t* seg_payload, uint32_t* first_of,
                                           uint32_t* n_out, void* workspace, void* stream)
{
    if (!n_plans || n_plans > kShapes || !groups || groups > 65535u || !fec_id0 || fec_id0 > 65535u || !stride ||
        stride % 16 || capacity > stride || !per_group)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    Sect S = {};
    S.n_plans = n_plans;
    for (uint32_t p = 0; p < n_plans; ++p) {
        if (first[p + 1] < first[p])
            return (int)hipErrorInvalidValue;
        S.first[p] = first[p];
        S.group_of[p] = sections[p].group_of;
    }
    const uint32_t R = S.first[n_plans] = first[n_plans];
    if ((uint64_t)R * per_group * cd >= (1ull << 31))
        return (int)hipErrorInvalidValue;
    const uint32_t n_blk = blocks_for(groups);
    uint32_t* local = static_cast<uint32_t*>(workspace);
    uint32_t* blk = local + ((groups + 3u) & ~3u);
    const uint32_t single = n_blk == 1;
    RFEC_LAUNCH(k_deliver_count, dim3(n_blk), dim3(kBlock), 0, st, S, groups, per_group, shape_of, rank_of, out_index,
                local, blk, first_of, n_out, single);
    if (!single)
        RFEC_LAUNCH(k_deliver_totals, dim3(1), dim3(kBlock), 0, st, blk, n_blk, groups, first_of, n_out);
    Deliver D = {};
    D.out_sh = reinterpret_cast<const v4u*>(out_shards);
    D.out_hdr = reinterpret_cast<const uint32_t*>(out_hdr);
    D.out_index = out_index;
    D.seg = reinterpret_cast<uint32_t*>(seg);
    D.pay = reinterpret_cast<v4u*>(seg_payload);
    D.first_of = first_of;
    D.local = local;
    D.blk = blk;
    D.G = groups;
    D.E = per_group;
    D.C = stride / 16;
    D.cd = cd;
    D.max_out = max_out;
    D.fec_id0 = fec_id0;
    D.n_slots = R * per_group;
    D.n_pay = max_out ? D.n_slots * cd : 0u; // max_out == 0: no entry is written, and the scan is all there is
    D.hdr_blocks = blocks_for((uint64_t)groups + (max_out ? D.n_slots : 0u));
    if (!max_out)
        D.n_slots = 0;
    D.divE = make_fastdiv(per_group);
    D.divCD = make_fastdiv(cd);
    RFEC_LAUNCH(k_deliver, dim3(D.hdr_blocks + blocks_for(D.n_pay)), dim3(kBlock), 0, st, S, D);
    rfec_set_indexed_path(5u | (single ? 2u : 3u) << 8);
    return (int)hipGetLastError();
}

// rfec_recover_deliver_each (rfec_recover_deliver_each.c): the caller has checked what rfec_launch_recover_deliver's
// has, per_group[p] >= 1 for every section with rows and slot_first[n_plans] * CD < 2^31; hipErrorInvalidValue
// otherwise.  first, slot_first: host [n_plans + 1], the prefixes of the sections' rows and out slots.
extern "C" int rfec_launch_recover_deliver_each(const rfec_regroup_section* sections, uint32_t n_plans,
                                                const uint32_t* first, const uint32_t* slot_first,
                                                const uint32_t* per_group, uint32_t groups, uint32_t fec_id0,
                                                const uint8_t* shape_of, const uint32_t* rank_of, uint32_t stride,
                                                uint32_t capacity, const uint8_t* out_shards, const rfec_hdr* out_hdr,
                                                const uint8_t* out_index, uint32_t max_out, rfec_rx_seg* seg,
                                                uint8_t* seg_payload, uint32_t* first_of, uint32_t* n_out,
                                                void* workspace, void* stream)
{
    if (!n_plans || n_plans > kShapes || !groups || groups > 65535u || !fec_id0 || fec_id0 > 65535u || !stride ||
        stride % 16 || capacity > stride || !first || !slot_first || !per_group)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    SectEach S = {};
    S.n_plans = n_plans;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const uint32_t rows = first[p + 1] - first[p], E = rows ? per_group[p] : 1u;
        if (first[p + 1] < first[p] || !E || (uint64_t)slot_first[p] + (uint64_t)rows * E != slot_first[p + 1])
            return (int)hipErrorInvalidValue;
        S.first[p] = first[p];
        S.slot_first[p] = slot_first[p];
        S.E[p] = E;
        S.divE[p] = make_fastdiv(E);
        S.group_of[p] = sections[p].group_of;
    }
    S.first[n_plans] = first[n_plans];
    const uint32_t n_slots = S.slot_first[n_plans] = slot_first[n_plans];
    if ((uint64_t)n_slots * cd >= (1ull << 31))
        return (int)hipErrorInvalidValue;
    const uint32_t n_blk = blocks_for(groups);
    uint32_t* local = static_cast<uint32_t*>(workspace);
    uint32_t* blk = local + ((groups + 3u) & ~3u);
    const uint32_t single = n_blk == 1;
    RFEC_LAUNCH(k_deliver_count_each, dim3(n_blk), dim3(kBlock), 0, st, S, groups, shape_of, rank_of, out_index, local,
                blk, first_of, n_out, single);
    if (!single)
        RFEC_LAUNCH(k_deliver_totals, dim3(1), dim3(kBlock), 0, st, blk, n_blk, groups, first_of, n_out);
    Deliver D = {};
    D.out_sh = reinterpret_cast<const v4u*>(out_shards);
    D.out_hdr = reinterpret_cast<const uint32_t*>(out_hdr);
    D.out_index = out_index;
    D.seg = reinterpret_cast<uint32_t*>(seg);
    D.pay = reinterpret_cast<v4u*>(seg_payload);
    D.first_of = first_of;
    D.local = local;
    D.blk = blk;
    D.G = groups;
    D.C = stride / 16;
    D.cd = cd;
    D.max_out = max_out;
    D.fec_id0 = fec_id0;
    D.n_slots = max_out ? n_slots : 0u; // max_out == 0: no entry is written, and the scan is all there is
    D.n_pay = D.n_slots * cd;
    D.hdr_blocks = blocks_for((uint64_t)groups + D.n_slots);
    D.divCD = make_fastdiv(cd);
    RFEC_LAUNCH(k_deliver_each, dim3(D.hdr_blocks + blocks_for(D.n_pay)), dim3(kBlock), 0, st, S, D);
    rfec_set_indexed_path(10u | (single ? 2u : 3u) << 8);
    return (int)hipGetLastError();
}
