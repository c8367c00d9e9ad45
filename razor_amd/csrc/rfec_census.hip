// rfec_census.hip -- CDNA4 (gfx950) kernels of rfec_wire_window_census (razor_fec.h, wire codec): which shapes occur
// in a parsed window, in window order, and how many groups each has, small enough to read back in one copy.  From it
// the host builds the plans and sizes the sections of rfec_wire_regroup_shapes exactly.
//
// The rule is a pure function of the records (razor_fec.h, "The rule" of rfec_wire_window_census): a group takes the
// key (count, row, col) of its first accepted parity, as in rfec_wire_regroup_shapes, where "accepted" asks the plan
// rfec_plan_from_key builds for the record's own key (rfec_census_rules.h) in place of a list of plans.
//
// Four launches on the caller's stream (three with n == 0); as in rfec_regroup_shapes.hip no launch has a lane read,
// other than by an atomic, a word that another lane of that launch writes, and no lane waits on another workgroup:
//   k_census_fill    anchor_of[G] <- 0xFFFFFFFF and the sixteen leading words of the census (g_first <- 0xFFFFFFFF)
//   k_census_anchor  a capped grid striding over the records, a lane per record and step: an accepted SIM_FEC does
//                    atomicMin(anchor_of[g], arrival); the five record counters and g_first / g_end are summed per
//                    lane, per wave (shuffles) and per block (LDS) and leave the block as five atomics
//   k_census_key     one lane per group: key_of[g] from words 8-11 of the anchor's record.  A launch of its own for
//                    the reason k_shapes_shape is one: a window's anchors are as many gathered records, which must
//                    not go through one CU
//   k_census_shapes  one workgroup over key_of in window order, a tile of kCensusTile groups at a time, one group per
//                    lane: the list of keys, their counts and first groups live in LDS; a lane looks its key up
//                    through broadcast reads; among the lanes of a tile whose key is not listed the least g wins an
//                    LDS atomicMin and appends its key, until no lane has an unlisted key or the list holds 32 (at
//                    most 32 appends over the whole window); after that an unlisted key counts into other_groups
// The matrix (row, col) of every count -- the planner's float sqrt stays on the host -- travels in the argument
// block; a wave walks the counts of its lanes (as for_plan does the plans), so the table comes through scalar loads.
#include <cstddef>

#include "rfec_census_rules.h"
#include "rfec_regroup_rules.h"

namespace {

static_assert(RFEC_CENSUS_MAX_COUNT == RFEC_MAX_K, "rfec_census_rules.h's bound on count");

constexpr uint32_t kCensusShapes = RFEC_CENSUS_MAX_SHAPES;
constexpr int kCensusTile = 1024; // k_census_shapes: lanes of its one workgroup, one group each
constexpr int kCensusAhead = 4;   // tiles whose keys a lane loads before it works on the first of them
constexpr uint32_t kAnchorBlocks = 1024; // k_census_anchor's grid at most: four blocks a CU
constexpr uint32_t kHeadWords = 16; // the census's words ahead of shape[]

static_assert(sizeof(rfec_window_census) == 4 * kHeadWords + 16 * kCensusShapes && sizeof(rfec_census_shape) == 16,
              "census layout");
static_assert(offsetof(rfec_window_census, g_first) == 12 && offsetof(rfec_window_census, n_seg) == 20 &&
                  offsetof(rfec_window_census, shape) == 4 * kHeadWords,
              "census layout");

struct CensusMatrix {
    uint32_t rc[RFEC_MAX_K + 1]; // row | col << 8 of rfec_num_packets(count, 255)
};
struct CensusWin {
    const rfec_wire_rec* recs;
    uint32_t n, groups, fec_id0, capacity;
    CensusMatrix matrix;
};
static_assert(sizeof(CensusWin) <= 1024, "the argument block");

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
        v = min(v, (uint32_t)__shfl_xor((int)v, d, kWave));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
        v += (uint32_t)__shfl_xor((int)v, d, kWave);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
        v = max(v, (uint32_t)__shfl_xor((int)v, d, kWave));
    return v;
}

__global__ __launch_bounds__(kBlock) void k_census_fill(uint32_t* __restrict__ census, uint32_t* __restrict__ anchor_of,
                                                        uint32_t groups)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < groups)
        anchor_of[t] = kNone;
    if (t < kHeadWords)
        census[t] = t == offsetof(rfec_window_census, g_first) / 4 ? kNone : 0u;
}

// A capped grid, every block striding over the records a block's worth at a time: each lane keeps its own counts
// and extent over its records, and a block leaves five atomics behind -- one for n_seg, one 64-bit add each for the
// pairs (n_fec, n_refused) and (n_notfec, n_window), a min and a max.  With a lane per record and the counters
// leaving every wave (seven atomics of 23,000 waves on one 128-byte line) the pass took 1,344 us for 1.5 M records
// against 68 us now (profiles/r22/window_census/first_form_kernel_stats.csv): the atomics on one line
// retire one after another, about 11 ns each.
// Whole waves run every step (a lane past n counts as no record): the ballots take all 64 lanes.
__global__ __launch_bounds__(kBlock) void k_census_anchor(const CensusWin W, rfec_window_census* __restrict__ census,
                                                          uint32_t* __restrict__ anchor_of)
{
    __shared__ uint32_t acc[7]; // n_seg, n_fec, n_refused, n_notfec, n_window, g_first, g_end
    if (threadIdx.x < 7)
        acc[threadIdx.x] = threadIdx.x == 5 ? kNone : 0u;
    __syncthreads();
    uint32_t c_seg = 0, c_fec = 0, c_refused = 0, c_notfec = 0, c_window = 0, lo = kNone, hi = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < W.n; base += gridDim.x * kBlock) { // the same in every lane
        const uint32_t r = base + threadIdx.x;
        const bool live = r < W.n;
        Rec R = {};
        if (live)
            R = load_rec(W.recs, r);
        const uint32_t kind = live ? kind_of(R.tag) : 0u;
        const uint32_t g = kind ? group_of(R.fec_id, W.fec_id0, W.groups) : kNone;
        const bool in_window = g != kNone;
        const bool fec = in_window && kind == RFEC_WIRE_FEC;
        const uint32_t row = R.shape & 0xFFu, col = (R.shape >> 8) & 0xFFu, index = R.shape >> 16;
        // The matrix (row, col) of the record's count, for the lanes whose answer depends on it: a column index.
        // The whole wave walks the counts of those lanes: the loop's condition and the table's index are
        // wave-uniform (a lane-divergent loop had the table read by the lane's own, equal, count: a vector load).
        uint32_t m = 0;
        const bool asks = fec && index >= 0x80u && R.count >= 6 && R.count <= RFEC_MAX_K;
        for (uint64_t todo = __ballot(asks); todo;) {
            const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)R.count, (int)__builtin_ctzll(todo));
            const uint32_t m0 = W.matrix.rc[c0];
            const bool same = asks && R.count == c0;
            m = same ? m0 : m;
            todo &= ~__ballot(same);
        }
        const bool accepted = fec && R.data_size <= W.capacity &&
                              rfec_census_line_of(R.count, row, col, index, m & 0xFFu, m >> 8) != RFEC_CENSUS_NO_LINE;
        if (accepted)
            atomicMin(anchor_of + g, r);
        c_seg += in_window && kind == RFEC_WIRE_SEG;
        c_fec += accepted;
        c_refused += fec && !accepted;
        c_notfec += live && !kind;
        c_window += kind && !in_window;
        lo = min(lo, g);
        hi = max(hi, in_window ? g + 1 : 0u);
    }
    // the block's sums: per wave through shuffles, the waves through LDS atomics
    c_seg = wave_sum(c_seg), c_fec = wave_sum(c_fec), c_refused = wave_sum(c_refused);
    c_notfec = wave_sum(c_notfec), c_window = wave_sum(c_window);
    lo = wave_min(lo), hi = wave_max(hi);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicAdd(&acc[0], c_seg);
        atomicAdd(&acc[1], c_fec);
        atomicAdd(&acc[2], c_refused);
        atomicAdd(&acc[3], c_notfec);
        atomicAdd(&acc[4], c_window);
        atomicMin(&acc[5], lo);
        atomicMax(&acc[6], hi);
    }
    __syncthreads();
    // counts stay below 2^31, so a pair of neighbouring 32-bit counters takes one 64-bit add with no carry across
    static_assert(offsetof(rfec_window_census, n_fec) % 8 == 0 && offsetof(rfec_window_census, n_notfec) % 8 == 0 &&
                      offsetof(rfec_window_census, n_refused) == offsetof(rfec_window_census, n_fec) + 4 &&
                      offsetof(rfec_window_census, n_window) == offsetof(rfec_window_census, n_notfec) + 4,
                  "the counter pairs");
    if (threadIdx.x == 0 && acc[0])
        atomicAdd(&census->n_seg, acc[0]);
    if (threadIdx.x == 1 && (acc[1] | acc[2]))
        atomicAdd(reinterpret_cast<unsigned long long*>(&census->n_fec), acc[1] | (unsigned long long)acc[2] << 32);
    if (threadIdx.x == 2 && (acc[3] | acc[4]))
        atomicAdd(reinterpret_cast<unsigned long long*>(&census->n_notfec), acc[3] | (unsigned long long)acc[4] << 32);
    if (threadIdx.x == 3 && acc[6])
        atomicMin(&census->g_first, acc[5]);
    if (threadIdx.x == 4 && acc[6])
        atomicMax(&census->g_end, acc[6]);
}

// One lane per group: the key of the group is its anchor's (count, row, col); the anchor pass accepted the record, so
// count <= RFEC_MAX_K and the key is never 0xFFFFFFFF.
__global__ __launch_bounds__(kBlock) void k_census_key(const rfec_wire_rec* __restrict__ recs, uint32_t groups,
                                                       const uint32_t* __restrict__ anchor_of,
                                                       uint32_t* __restrict__ key_of)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= groups)
        return;
    const uint32_t a = anchor_of[g];
    uint32_t key = kNone;
    if (a != kNone) {
        const v4u c = reinterpret_cast<const v4u*>(recs + a)[2]; // words 8-11
        key = c.y >> 16 | (c.w & 0xFFFFu) << 8;
    }
    key_of[g] = key;
}

// One workgroup.  Lane t takes group g0 + t of the tile at g0; the keys of kCensusAhead tiles are loaded together.
// A round of the tile: the lanes with an unlisted key do atomicMin(least[round & 1], g); after a barrier every lane
// reads the word -- 0xFFFFFFFF ends the tile -- and after another the winner appends its key and puts the word back,
// and after a third the lanes see the new entry.  The word alternates between two so that a lane one barrier ahead,
// in the next round, does not write the word the others are still reading; a tile with nothing to append takes one
// barrier.
__global__ __launch_bounds__(kCensusTile) void k_census_shapes(const uint32_t* __restrict__ key_of, uint32_t groups,
                                                               uint32_t* __restrict__ census)
{
    __shared__ uint32_t key[kCensusShapes], count[kCensusShapes], first[kCensusShapes];
    __shared__ uint32_t least[2], other, anchored;
    const uint32_t t = threadIdx.x;
    const bool lead = (t & (kWave - 1)) == 0;
    if (t < kCensusShapes)
        key[t] = count[t] = first[t] = 0;
    if (t < 2)
        least[t] = kNone;
    if (t == 0)
        other = anchored = 0;
    __syncthreads();
    uint32_t n = 0, round = 0; // the same in every lane
    const uint32_t g_last = groups - 1;
    for (uint32_t gb = 0; gb < groups; gb += kCensusAhead * kCensusTile) {
        uint32_t mine[kCensusAhead];
#pragma unroll
        for (int j = 0; j < kCensusAhead; ++j) // unconditional, so that the loads are in flight together
            mine[j] = key_of[min(gb + j * kCensusTile + t, g_last)];
#pragma unroll
        for (int j = 0; j < kCensusAhead; ++j) {
            const uint32_t g0 = gb + j * kCensusTile; // the same in every lane, and so is the break
            if (g0 >= groups)
                break;
            const uint32_t g = g0 + t;
            const uint32_t mk = g < groups ? mine[j] : kNone;
            uint32_t at = kNone;
            for (uint32_t i = 0; i < n; ++i)
                if (key[i] == mk)
                    at = i;
            while (n < kCensusShapes) {
                uint32_t* const w = &least[round & 1u];
                ++round;
                if (mk != kNone && at == kNone)
                    atomicMin(w, g);
                __syncthreads();
                const uint32_t winner = *w;
                if (winner == kNone)
                    break;
                __syncthreads();
                if (g == winner) {
                    key[n] = mk;
                    first[n] = g;
                    *w = kNone;
                }
                __syncthreads();
                if (at == kNone && key[n] == mk)
                    at = n;
                ++n;
            }
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t c = __popcll(__ballot(at == i));
                if (lead && c)
                    atomicAdd(&count[i], c);
            }
            const uint32_t a = __popcll(__ballot(mk != kNone)), o = __popcll(__ballot(mk != kNone && at == kNone));
            if (lead && a)
                atomicAdd(&anchored, a);
            if (lead && o)
                atomicAdd(&other, o);
        }
    }
    __syncthreads();
    if (t < kCensusShapes) { // entries past n: zeros
        const uint32_t k = key[t];
        const v4u e = {(k & 0xFFu) | (k >> 8 & 0xFFFFu) << 16, count[t], first[t], 0u};
        reinterpret_cast<v4u*>(census + kHeadWords)[t] = e;
    }
    if (t == 0) {
        census[0] = n;
        census[1] = other;
        census[2] = anchored;
    }
}

thread_local uint32_t t_census_path = 0;

// the planner's matrix mode for every count (meaningful from count 6): constant, so made once per process
CensusMatrix make_matrix()
{
    CensusMatrix M = {};
    for (uint32_t k = 0; k <= RFEC_MAX_K; ++k) {
        uint8_t row = 0, col = 0;
        rfec_num_packets((uint16_t)k, 255, &row, &col);
        M.rc[k] = row | (uint32_t)col << 8;
    }
    return M;
}

} // namespace

extern "C" uint32_t rfec_census_last_path(void) { return t_census_path; }
extern "C" uint32_t rfec_census_tile(void) { return kCensusTile; }

// The caller (rfec_wire_census.c) has checked groups in [1, 65535], n < 2^31, fec_id0 != 0, capacity <= 65535 and the
// pointers.
extern "C" int rfec_launch_wire_census(uint32_t groups, uint32_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                                       uint32_t capacity, rfec_window_census* census,
                                       uint32_t* anchor_of, uint32_t* key_of, void* stream)
{
    if (!groups || groups > 65535u || n > 0x7FFFFFFFu)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    CensusWin W = {};
    W.recs = recs;
    W.n = n;
    W.groups = groups;
    W.fec_id0 = fec_id0;
    W.capacity = capacity;
    static const CensusMatrix matrix = make_matrix();
    W.matrix = matrix;
    uint32_t* const words = reinterpret_cast<uint32_t*>(census);
    RFEC_LAUNCH(k_census_fill, dim3(blocks_for(groups)), dim3(kBlock), 0, st, words, anchor_of, groups);
    if (n)
        RFEC_LAUNCH(k_census_anchor, dim3(min(blocks_for(n), kAnchorBlocks)), dim3(kBlock), 0, st, W, census,
                    anchor_of);
    RFEC_LAUNCH(k_census_key, dim3(blocks_for(groups)), dim3(kBlock), 0, st, recs, groups, anchor_of, key_of);
    RFEC_LAUNCH(k_census_shapes, dim3(1), dim3(kCensusTile), 0, st, key_of, groups, words);
    t_census_path = (n ? 4u : 3u) | (groups + kCensusTile - 1) / kCensusTile << 8;
    return (int)hipGetLastError();
}
