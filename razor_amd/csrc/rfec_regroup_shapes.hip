// rfec_regroup_shapes.hip -- CDNA4 (gfx950) kernels of rfec_wire_regroup_shapes (razor_fec.h, wire codec): the
// records rfec_wire_parse left in arrival order, of a closed window whose groups have different shapes, into one
// dense section of rfec_recover_indexed_out's tables per shape.
//
// The rule is a pure function of the records (razor_fec.h, "The rule" of rfec_wire_regroup_shapes): a group takes
// the shape of its first accepted parity (sim_fec.c:152-163, flex_fec_receiver.c:69-78), the groups of one shape
// are ranked in window order, and within a group the placement is rfec_wire_regroup's.  "First" and "lowest" are
// minima over arrival indices, taken with atomicMin on 32-bit words; the ranks are a scan in one workgroup.
//
// Six launches on the caller's stream; no launch has a lane read, other than by an atomic, a word that another
// lane of that launch writes (a launch boundary makes the words of the launch before visible), and no lane waits
// on another workgroup:
//   k_shapes_fill     every section's src_of[cap (k + n)] and group_of[cap], and anchor_of[G] <- 0xFFFFFFFF
//   k_shapes_anchor   one lane per record: a SIM_FEC accepted by some plan does atomicMin(anchor_of[g], arrival)
//   k_shapes_shape    one lane per group: shape_of[g] from the anchor's record.  A launch of its own and not the
//                     head of the rank pass: a window's 65,535 anchors are as many gathered records, which one
//                     workgroup took 350 us to fetch and the whole device takes a few
//   k_shapes_rank     one workgroup: rank_of[g] by an exclusive scan of shape_of per shape over the window,
//                     counts[p], and group_of[rank] = g in the shape's section while there is room
//   k_shapes_contend  one lane per record: rules 1-6 with the plan of the record's group; a contender does
//                     atomicMin(src_of[slot], arrival index) in its section and notes the slot, with the plan above
//                     it, in slot_of (a refused record its code)
//   k_shapes_tables   one grid: a lane per section slot writes hdr / meta / fec_size from the winner's record, a
//                     lane per section row the two masks and base_id, a lane per record leaves a contender's
//                     slot_of as the slot alone, or as EDUP where another record won it (the plan in slot_of saves
//                     these lanes the record: they read two words each)
// Lanes of one wave mostly share a plan; where per-plan arguments are needed the wave walks its plans (for_plan),
// so that they come through scalar loads and not through a gather from the argument block.
// The plans' keys and line indices and the sections' pointers travel as kernel arguments (at most 2,888 bytes of the
// 4,096 an argument block holds, with RFEC_REGROUP_MAX_SHAPES = 32).  Record addresses are 64-bit.
#include "rfec_regroup_rules.h"

namespace {

constexpr uint32_t kShapes = RFEC_REGROUP_MAX_SHAPES;
constexpr uint32_t kNoShape = 0xFFu;
// between k_shapes_contend and k_shapes_tables a contender's slot_of holds slot | plan << kSlotBits
constexpr uint32_t kSlotBits = 24;
static_assert(65535u * (RFEC_MAX_K + RFEC_MAX_LINES) < (1u << kSlotBits) && kShapes <= (1u << (31 - kSlotBits)),
              "slot | plan << kSlotBits stays a positive int32");
// k_shapes_rank: one workgroup of kRankBlock lanes, each on kRankChunk consecutive groups of a tile
constexpr int kRankBlock = 512;
constexpr int kRankChunk = 16;
constexpr uint32_t kRankTile = kRankBlock * kRankChunk;

static_assert(kShapes * 16 == kRankBlock, "k_shapes_rank scans a shape's counters with 16 lanes");

// the window and the plans' keys
struct Win {
    const rfec_wire_rec* recs;
    uint32_t n, groups, fec_id0, capacity, n_plans;
    uint16_t rowcol[kShapes]; // plan row | col << 8
    uint8_t k[kShapes], nl[kShapes];
};
struct Lines {
    uint8_t index[kShapes][RFEC_MAX_LINES]; // plans[p].line[l].index
};
struct Out {
    uint8_t* shape_of;
    uint32_t* rank_of;
    uint32_t* anchor_of;
    uint32_t* counts;
    int32_t* slot_of;
};
struct Maps {
    uint32_t* src_of[kShapes];
    uint32_t* group_of[kShapes];
    uint32_t cap[kShapes];
};
struct Tables {
    rfec_hdr* hdr[kShapes];
    uint64_t* present[kShapes];
    rfec_hdr* meta[kShapes];
    uint16_t* fec_size[kShapes];
    uint64_t* parity_present[kShapes];
    uint32_t* base_id[kShapes];
};
// the sections' lanes in a grid: section p has slots [slot0[p], slot0[p + 1]) and rows [row0[p], row0[p + 1])
struct Offs {
    uint32_t slot0[kShapes + 1], row0[kShapes + 1];
};
static_assert(sizeof(Win) + sizeof(Lines) + sizeof(Out) + sizeof(Maps) <= 4096 &&
                  sizeof(Win) + sizeof(Out) + sizeof(Maps) + sizeof(Tables) + sizeof(Offs) <= 4096,
              "the argument block");

// the section whose lanes hold lane t (t < off[n_plans]; empty sections hold none)
__device__ __forceinline__ uint32_t section_of(const uint32_t* off, uint32_t n_plans, uint32_t t)
{
    uint32_t p = 0;
    while (p + 1 < n_plans && t >= off[p + 1])
        ++p;
    return p;
}

// (rule 1: kind_of and group_of -- rfec_regroup_rules.h)
// the plan with a SIM_FEC's (count, row, col), or kNoShape: the plans differ pairwise in them
__device__ __forceinline__ uint32_t plan_of(uint32_t count, uint32_t rowcol, const Win& W)
{
    for (uint32_t p = 0; p < W.n_plans; ++p)
        if (W.k[p] == count && W.rowcol[p] == rowcol)
            return p;
    return kNoShape;
}
// rule 2: the plan that accepts a SIM_FEC and its line there, or kNoShape (ESHAPE)
// The loops run over the plans and lines with wave-uniform counters, so the tables are read with scalar loads
// from the argument block; only the lanes whose record has plan p's key walk p's lines.
__device__ __forceinline__ uint32_t accept(const Rec& R, const Win& W, const Lines& L, uint32_t& line)
{
    if (R.data_size > W.capacity)
        return kNoShape;
    const uint32_t rowcol = R.shape & 0xFFFFu, index = R.shape >> 16;
    uint32_t found = kNoShape;
    for (uint32_t p = 0; p < W.n_plans; ++p)
        if (W.k[p] == R.count && W.rowcol[p] == rowcol) {
            const uint32_t nl = W.nl[p];
            for (uint32_t l = 0; l < nl; ++l)
                if (L.index[p][l] == index) {
                    line = l;
                    found = p;
                    break;
                }
        }
    return found;
}
// body(p0) once per plan among the wave's lanes, for the lanes of that plan, with p0 wave-uniform: what body reads
// of the argument block by p0 comes through scalar loads
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

__global__ __launch_bounds__(kBlock) void k_shapes_fill(const Maps M, const Offs O, uint32_t n_plans,
                                                        uint32_t* __restrict__ anchor_of, uint32_t groups)
{
    uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_slots = O.slot0[n_plans], n_rows = O.row0[n_plans];
    if (t < n_slots) {
        const uint32_t p = section_of(O.slot0, n_plans, t);
        M.src_of[p][t - O.slot0[p]] = kNone;
        return;
    }
    t -= n_slots;
    if (t < n_rows) {
        const uint32_t p = section_of(O.row0, n_plans, t);
        M.group_of[p][t - O.row0[p]] = kNone;
        return;
    }
    t -= n_rows;
    if (t < groups)
        anchor_of[t] = kNone;
}

__global__ __launch_bounds__(kBlock) void k_shapes_anchor(const Win W, const Lines L, uint32_t* __restrict__ anchor_of)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= W.n)
        return;
    const Rec R = load_rec(W.recs, r);
    if (kind_of(R.tag) != RFEC_WIRE_FEC)
        return;
    const uint32_t g = group_of(R.fec_id, W.fec_id0, W.groups);
    uint32_t l;
    if (g == kNone || accept(R, W, L, l) == kNoShape)
        return;
    atomicMin(anchor_of + g, r);
}

// One lane per group: the shape of the group is the plan that accepts its anchor (the plan with the anchor's key:
// the anchor pass accepted it).
__global__ __launch_bounds__(kBlock) void k_shapes_shape(const Win W, const uint32_t* __restrict__ anchor_of,
                                                         uint8_t* __restrict__ shape_of)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= W.groups)
        return;
    const uint32_t a = anchor_of[g];
    uint32_t p = kNoShape;
    if (a != kNone) {
        const v4u c = reinterpret_cast<const v4u*>(W.recs + a)[2]; // words 8-11
        p = plan_of(c.y >> 16, c.w & 0xFFFFu, W);
    }
    shape_of[g] = (uint8_t)p;
}

// One workgroup, the window in tiles of kRankTile groups, lane t on groups [t kRankChunk, (t + 1) kRankChunk) of
// the tile: its count per shape into cnt[shape][t]; an exclusive scan of each shape's kRankBlock counters (16 lanes a
// shape in use, 32 counters a lane) on top of the shape's total over the tiles before; then the lane's groups take
// cnt[shape][t], cnt[shape][t] + 1, ... in window order.  A counter row has a pad after every 32 counters, so that
// the scan's lanes, 32 counters apart, fall on different LDS banks.
__global__ __launch_bounds__(kRankBlock) void k_shapes_rank(const Win W, const Out U, const Maps M)
{
    __shared__ uint16_t cnt[kShapes][kRankBlock + kRankBlock / 32]; // ranks are below 65535
    __shared__ uint32_t run[kShapes], cap[kShapes];
    __shared__ uint32_t* group_of[kShapes];
    const uint32_t t = threadIdx.x, col = t + (t >> 5);
    if (t < kShapes) {
        run[t] = 0;
        cap[t] = t < W.n_plans ? M.cap[t] : 0u;
        group_of[t] = M.group_of[t];
    }
    const uint32_t g_last = W.groups - 1;
    for (uint32_t g0 = 0; g0 < W.groups; g0 += kRankTile) {
        const uint32_t gb = g0 + t * kRankChunk;
        uint32_t shape[kRankChunk];
#pragma unroll
        for (int j = 0; j < kRankChunk; ++j) // unconditional, so that the tile's loads are in flight together
            shape[j] = U.shape_of[min(gb + j, g_last)];
        for (uint32_t q = 0; q < W.n_plans; ++q)
            cnt[q][col] = 0; // the lane's own column: it alone touched it since the scan before
#pragma unroll
        for (int j = 0; j < kRankChunk; ++j) {
            if (gb + j >= W.groups)
                shape[j] = kNoShape;
            if (shape[j] != kNoShape)
                cnt[shape[j]][col] += 1;
        }
        __syncthreads();
        const uint32_t q = t >> 4, seg = t & 15u;
        uint32_t before = 0, total = 0;
        if (q < W.n_plans) { // whole groups of 16 lanes: the shuffles stay among active lanes
            uint16_t* c = &cnt[q][seg * 33u];
            uint32_t s = 0;
            for (int i = 0; i < 32; ++i)
                s += c[i];
            uint32_t x = s; // inclusive over the shape's 16 lanes
            for (uint32_t d = 1; d < 16; d <<= 1) {
                const uint32_t v = __shfl_up(x, d, 16);
                if (seg >= d)
                    x += v;
            }
            total = __shfl(x, 15, 16);
            before = run[q];
            uint32_t at = before + x - s;
            for (int i = 0; i < 32; ++i) {
                const uint32_t v = c[i];
                c[i] = (uint16_t)at;
                at += v;
            }
        }
        __syncthreads();
        if (seg == 0 && q < W.n_plans)
            run[q] = before + total;
#pragma unroll
        for (int j = 0; j < kRankChunk; ++j) {
            const uint32_t g = gb + j;
            if (g >= W.groups)
                break;
            uint32_t rank = kNone;
            const uint32_t p = shape[j];
            if (p != kNoShape) {
                rank = cnt[p][col];
                cnt[p][col] = (uint16_t)(rank + 1);
                if (rank < cap[p])
                    group_of[p][rank] = g;
            }
            U.rank_of[g] = rank;
        }
    }
    __syncthreads();
    if (t < W.n_plans)
        U.counts[t] = run[t];
}

__global__ __launch_bounds__(kBlock) void k_shapes_contend(const Win W, const Lines L, const Out U, const Maps M)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= W.n)
        return;
    const Rec R = load_rec(W.recs, r);
    const uint32_t kind = kind_of(R.tag);
    int32_t res;
    uint32_t g = kNone, s = kNone, p = kNoShape; // s: a segment's member index, a parity's line
    if (!kind)
        res = RFEC_REGROUP_ENOTFEC;
    else if ((g = group_of(R.fec_id, W.fec_id0, W.groups)) == kNone)
        res = RFEC_REGROUP_EWINDOW;
    else if (kind == RFEC_WIRE_FEC) {
        const uint32_t mine = accept(R, W, L, s);
        // an accepted record makes anchor_of[g] <= r, so the group has a shape
        if (mine == kNoShape || mine != (p = U.shape_of[g]))
            res = RFEC_REGROUP_ESHAPE;
        else {
            const uint32_t a = U.anchor_of[g];
            const uint32_t base = a == r ? R.base_id : base_id_of(W.recs, a);
            res = R.base_id == base ? 0 : RFEC_REGROUP_EBASE;
        }
    } else {
        const uint32_t a = U.anchor_of[g];
        if (a == kNone || (p = U.shape_of[g]) == kNoShape) // (an anchor always has a shape)
            res = RFEC_REGROUP_ENOPARITY;
        else {
            s = R.seq - base_id_of(W.recs, a); // unsigned: a packet id below the base is far above k
            res = 0;
        }
    }
    if (res == 0) {
        const uint32_t rank = U.rank_of[g];
        for_plan(p, [&](uint32_t p0) {
            const uint32_t k = W.k[p0], nl = W.nl[p0];
            if (kind == RFEC_WIRE_FEC)
                s += k;
            else if (s >= k) {
                res = RFEC_REGROUP_EBASE;
                return;
            }
            if (rank >= M.cap[p0]) {
                res = RFEC_REGROUP_EFULL;
                return;
            }
            const uint32_t slot = rank * (k + nl) + s; // < 65535 * 192 < 2^24
            atomicMin(M.src_of[p0] + slot, r);
            res = (int32_t)(slot | p0 << kSlotBits); // the plan rides along until k_shapes_tables
        });
    }
    U.slot_of[r] = res;
}

__global__ __launch_bounds__(kBlock) void k_shapes_tables(const Win W, const Out U, const Maps M, const Tables T,
                                                          const Offs O)
{
    uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_slots = O.slot0[W.n_plans], n_rows = O.row0[W.n_plans];
    if (t < n_slots) { // section slot: the winner's header record (and a parity's size)
        for_plan(section_of(O.slot0, W.n_plans, t), [&](uint32_t p) {
            const uint32_t u = t - O.slot0[p];
            const uint32_t a = M.src_of[p][u];
            if (a == kNone)
                return;
            const uint32_t k = W.k[p], nl = W.nl[p], c = u / (k + nl), s = u - c * (k + nl);
            const uint32_t* w = reinterpret_cast<const uint32_t*>(W.recs + a);
            const bool seg = s < k;
            const size_t o = seg ? (size_t)c * k + s : (size_t)c * nl + (s - k);
            place_record(w, reinterpret_cast<uint32_t*>((seg ? T.hdr[p] : T.meta[p]) + o), !seg, T.fec_size[p] + o);
        });
        return;
    }
    t -= n_slots;
    if (t < n_rows) { // section row: the masks and the anchor's base_id (an empty row: 0)
        for_plan(section_of(O.row0, W.n_plans, t), [&](uint32_t p) {
            const uint32_t c = t - O.row0[p], k = W.k[p], nl = W.nl[p];
            const SlotMasks m = slot_masks(M.src_of[p] + (size_t)c * (k + nl), k, nl);
            T.present[p][2 * (size_t)c] = m.present[0];
            T.present[p][2 * (size_t)c + 1] = m.present[1];
            T.parity_present[p][c] = m.parity_present;
            const uint32_t g = M.group_of[p][c];
            T.base_id[p][c] = g == kNone ? 0u : base_id_of(W.recs, U.anchor_of[g]);
        });
        return;
    }
    t -= n_rows;
    if (t < W.n) { // record: a contender's slot without its plan, or EDUP where it did not win the slot
        const int32_t s = U.slot_of[t];
        if (s < 0)
            return;
        const uint32_t slot = (uint32_t)s & ((1u << kSlotBits) - 1);
        for_plan((uint32_t)s >> kSlotBits, [&](uint32_t p) {
            U.slot_of[t] = M.src_of[p][slot] == t ? (int32_t)slot : RFEC_REGROUP_EDUP;
        });
    }
}

} // namespace

// The caller (rfec_wire_regroup.c) has checked the plans (k <= RFEC_MAX_K, pairwise different keys), n_plans in
// [1, 32], groups in [1, 65535], n < 2^31, cap <= groups and the pointers.  Lane counts: the sections' slots are at
// most 32 * 65535 * 192 < 2^29, with their rows and the records' lanes below 2^32.
extern "C" int rfec_launch_wire_regroup_shapes(const rfec_kplan* plans, uint32_t n_plans,
                                               const rfec_regroup_section* sections, uint32_t groups,
                                               uint32_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                                               uint32_t capacity, uint8_t* shape_of, uint32_t* rank_of,
                                               uint32_t* anchor_of, uint32_t* counts, int32_t* slot_of, void* stream)
{
    if (!n_plans || n_plans > kShapes || !groups || groups > 65535u || n > 0x7FFFFFFFu)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Win W = {};
    Lines L = {};
    Maps M = {};
    Tables T = {};
    Offs O = {};
    W.recs = recs;
    W.n = n;
    W.groups = groups;
    W.fec_id0 = fec_id0;
    W.capacity = capacity;
    W.n_plans = n_plans;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_kplan* P = plans + p;
        const rfec_regroup_section* S = sections + p;
        if (!P->k || P->k > RFEC_MAX_K || P->n_lines > RFEC_MAX_LINES || S->cap > groups)
            return (int)hipErrorInvalidValue;
        W.k[p] = (uint8_t)P->k;
        W.nl[p] = P->n_lines;
        W.rowcol[p] = (uint16_t)((uint32_t)P->row | (uint32_t)P->col << 8);
        for (uint32_t l = 0; l < P->n_lines; ++l)
            L.index[p][l] = P->line[l].index;
        M.src_of[p] = S->src_of;
        M.group_of[p] = S->group_of;
        M.cap[p] = S->cap;
        T.hdr[p] = S->hdr;
        T.present[p] = S->present;
        T.meta[p] = S->meta;
        T.fec_size[p] = S->fec_size;
        T.parity_present[p] = S->parity_present;
        T.base_id[p] = S->base_id;
        O.slot0[p + 1] = O.slot0[p] + S->cap * ((uint32_t)P->k + P->n_lines);
        O.row0[p + 1] = O.row0[p] + S->cap;
    }
    const Out U = {shape_of, rank_of, anchor_of, counts, slot_of};
    const uint64_t n_sec = (uint64_t)O.slot0[n_plans] + O.row0[n_plans];
    RFEC_LAUNCH(k_shapes_fill, dim3(blocks_for(n_sec + groups)), dim3(kBlock), 0, st, M, O, n_plans, anchor_of,
                groups);
    if (n)
        RFEC_LAUNCH(k_shapes_anchor, dim3(blocks_for(n)), dim3(kBlock), 0, st, W, L, anchor_of);
    RFEC_LAUNCH(k_shapes_shape, dim3(blocks_for(groups)), dim3(kBlock), 0, st, W, anchor_of, shape_of);
    RFEC_LAUNCH(k_shapes_rank, dim3(1), dim3(kRankBlock), 0, st, W, U, M);
    if (n)
        RFEC_LAUNCH(k_shapes_contend, dim3(blocks_for(n)), dim3(kBlock), 0, st, W, L, U, M);
    RFEC_LAUNCH(k_shapes_tables, dim3(blocks_for(n_sec + n)), dim3(kBlock), 0, st, W, U, M, T, O);
    return (int)hipGetLastError();
}
