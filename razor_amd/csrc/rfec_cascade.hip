// rfec_cascade.hip -- the cascade and matrix decodes of the flex-FEC engine (gfx950), the packed matrix
// records' packer and decode, the matrix decode through a slot map over a row pool, the decode of a window's
// sections of several shapes through that map (matrix and row-layout sections in one launch), and their launchers;
// rfec_kernels.hip picks the cascade decode (rfec_launch_recover[_out]), rfec_packed_matrix.c calls the packed
// records' shims, rfec_recover_indexed_matrix.c the indexed matrix decode's, rfec_recover_indexed_shapes.c the
// sections'.
//
// One copy of each piece: the replay and the dense tail take the received rows as a row source (BatchRows: the
// batch layout; PoolRows: a row pool through the slot map), the three matrix kernels share matrix_payload_block
// (NoPool or PoolRows) and, with the generic kernels, cascade_check_block and casc_lane; casc_out_args fills the
// dense-output arguments for the three launch paths.  Only the dependency closure over a schedule stands twice
// (k_decode_cascade and cascade_dense_tail).  The batch kernels' code is sensitive to the form of such sharing,
// not only to its content: DESIGN 7.13 lists the forms that changed it, and tools/kernel_compare.py is the check.
#include "rfec_row_blocks.h" // (the row sections of k_decode_shapes_indexed: rfec_fused.hip's bodies)
#include "rfec_matrix_wide_blocks.h" // (the wide sections of k_decode_window_indexed: rfec_matrix_wide.hip's bodies
#include "rfec_rows_wide_blocks.h"   //  and rfec_rows_wide.hip's)

namespace {

// ---------------------------------------------------------------------------
// Recover, plans with cascades (the sender's rows + columns: k <= 64, at most
// 8 lines of at most 4 members, every matrix plan of
// flex_fec_sender_num_packets up to k = 16): one launch, no workspace.
// Lanes (group, slot q, chunk column) in blocks of 256 (XCD-swizzled);
// dense output: slot q = the group's q-th erased segment, written to out slot
// q; in place: slot q = step q of the group's schedule.
// In each block one CHECKER lane per group the block touches runs the exact
// peel of that group: the canonical schedule over the masks (lines in plan
// order, repeated to a fixpoint: flex_fec_receiver.c:105-206 with the cascade
// of sim_receiver.c:780-804), then the header checks of its steps, two steps'
// loads in flight together (fec_data_size within the capacity, every member's
// size and the recovered size within fec_data_size: flex_fec_xor.c:88-89,
// 98-99).  A line that fails them is left out and the schedule recomputed:
// such a line fails every time it fires (same target, same members, same
// headers), so the exact peel is the mask peel without it.  The checker
// writes the recovered header records, the recovered mask and out_index, and
// hands the schedule to its block through LDS; after one barrier every lane
// replays the steps its slot depends on, recovered chunks of earlier steps
// kept in registers (a cascade costs loads, never another launch nor a round
// trip through another lane's output).
// ---------------------------------------------------------------------------

// A slot's task (the checker writes one per output slot of every group): the
// line and target of the step that recovers the slot's segment (dense: the
// slot's erased segment; in place: the slot-th step), bit 31 = there is one,
// bit 30 = it reads a segment recovered by an earlier step (a cascade: the
// payload lane then replays from the schedule record).
constexpr uint32_t kTaskValid = 1u << 31, kTaskCascade = 1u << 30;

// A schedule: step s = (line, target), packed so that no register array is
// indexed at run time (no scratch).  Which earlier steps a step reads follows
// from its line: its erased members other than its target were recovered
// before it.
struct CSched {
    uint32_t n;     // steps (<= 8)
    uint32_t lines; // line of step s in bits [4s, 4s + 4)
    uint64_t tg;    // target of step s in bits [8s, 8s + 8)
};

__device__ __forceinline__ uint32_t cs_line(const CSched& S, uint32_t s) { return (S.lines >> (4 * s)) & 15u; }
__device__ __forceinline__ uint32_t cs_tg(const CSched& S, uint32_t s) { return (uint32_t)(S.tg >> (8 * s)) & 0xffu; }

// Line records (first | stride << 8 | count << 16) and member masks of a plan:
// from the kernel arguments (any plan; KArgLines), from LDS copies (LdsLines),
// or arithmetic in the line index for the sender's matrix shapes (MatLines).
struct KArgLines {
    const rfec_kmask& M;
    __device__ uint32_t rec(uint32_t l) const { return reinterpret_cast<const uint32_t*>(M.plan.line)[l]; }
    __device__ uint64_t mask(uint32_t l) const { return M.mask[l][0]; }
    __device__ uint32_t nl(uint32_t n) const { return n; }
};

// The canonical schedule over the masks: a line fires with its parity
// received, exactly one member missing and one present; lines in `banned`
// never fire; dense (E > 0): only erased segments of rank < E are targets.
// MT: the mask word, uint32_t for k <= 32 (half the VALU work), else uint64_t.
template <typename MT, class Lines>
__device__ CSched cascade_schedule(const Lines& LL, uint32_t NL, MT have, uint64_t ppm, uint32_t banned, MT erased,
                                   uint32_t E)
{
    CSched S = {0, 0, 0};
    bool progress = true;
    while (progress) {
        progress = false;
        for (uint32_t l = 0; l < NL; ++l) { // uniform: the masks stay scalar kernel-argument loads (or constants)
            const MT m = (MT)LL.mask(l);
            const MT x = m & ~have;
            if (!((ppm >> l) & 1ull) || ((banned >> l) & 1u) || __popcll((uint64_t)x) != 1 || (m & have) == 0)
                continue;
            const uint32_t t = (uint32_t)__ffsll((long long)x) - 1;
            if (E && (uint32_t)__popcll((uint64_t)(erased & ((MT(1) << t) - MT(1)))) >= E)
                continue;
            S.lines |= l << (4 * S.n);
            S.tg |= (uint64_t)t << (8 * S.n);
            ++S.n;
            have |= MT(1) << t;
            progress = true;
        }
    }
    return S;
}

// the record of erased segment i's output: the dense slot of its rank, or its own slot in place
__device__ __forceinline__ uint32_t cs_slot(uint32_t E, uint64_t erased, uint32_t i)
{
    return E ? (uint32_t)__popcll(erased & ((1ull << i) - 1ull)) : i;
}

// payload lane t: (group, output slot q, chunk column j)
struct CascLane {
    uint32_t g, q, j;
};

__device__ __forceinline__ CascLane casc_lane(const CascArgs& A, uint32_t t)
{
    const uint32_t g = fdiv(t, A.divQC);
    const uint32_t rem = t - g * A.divQC.d;
    const uint32_t q = fdiv(rem, A.divC);
    return CascLane{g, q, rem - q * A.divC.d};
}

// Where a checker reads a group's masks and a step's header bytes (step =
// line l recovering target t): the batch layout's five arrays (BatchHdrs), or
// the packed matrix records (PackedMatHdrs below: the half of the target's
// slot that belongs to the line, one contiguous run).
struct BatchHdrs {
    const CascArgs& A;
    const rfec_kplan& P;
    struct Step {
        const uint32_t *gm, *gh;
        const uint16_t* gf;
        __device__ const uint32_t* meta() const { return gm; }                          // the line's fec_meta
        __device__ uint32_t size() const { return *gf; }                                // its fec_data_size
        __device__ const uint32_t* member(uint32_t, uint32_t i) const { return gh + i * 5; } // its u-th member, segment i
    };
    __device__ uint64_t present(uint32_t g) const { return A.present[2 * g]; }
    __device__ uint64_t parity_present(uint32_t g) const { return A.parity_present[g]; }
    __device__ Step step(uint32_t g, uint32_t l, uint32_t /* t */, uint64_t /* erased */) const
    {
        const uint32_t K = P.k, NL = P.n_lines;
        return Step{A.meta_dw + (size_t)g * NL * 5 + l * 5, A.hdr_dw + (size_t)g * K * 5, A.fsize + (size_t)g * NL + l};
    }
};

// The serial exact peel of group g (rare path: a header check failed): its
// header records, recovered mask and out_index written; returns the schedule.
// A step's record goes straight to its output (dense: out_hdr[g][rank], in
// place: hdr[g][t]); a later step of a cascade reads it back from there (same
// lane, same address, in order).  A line that fails its checks is left out and
// the schedule recomputed -- it would fail every time it fires (same target,
// same members, same headers), so the exact peel is the mask peel without it.
template <class Hdrs>
__device__ CSched cascade_check(const CascArgs& A, const rfec_kmask& M, const Hdrs& HS, uint32_t g)
{
    const rfec_kplan& P = M.plan;
    const uint32_t* lines = reinterpret_cast<const uint32_t*>(P.line);
    const uint32_t K = P.k, NL = P.n_lines;
    const uint64_t kmask = K >= 64 ? ~0ull : (1ull << K) - 1ull;
    const uint64_t have = HS.present(g) & kmask;
    const uint64_t erased = ~have & kmask;
    const uint64_t ppm = HS.parity_present(g);
    uint32_t* const ob = A.E ? A.out_hdr_dw + (size_t)g * A.E * 5 : A.hdr_dw + (size_t)g * K * 5;
    uint32_t banned = 0;
    CSched S;
#pragma unroll 1
    for (uint32_t attempt = 0; attempt <= NL; ++attempt) {
        S = cascade_schedule<uint64_t>(KArgLines{M}, NL, have, ppm, banned, erased, A.E);
        int bad = -1;
#pragma unroll 1
        for (uint32_t s = 0; s < S.n; ++s) {
            const uint32_t l = cs_line(S, s), t = cs_tg(S, s), ln = lines[l];
            const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
            const auto st = HS.step(g, l, t, erased);
            const uint32_t L = st.size();
            uint32_t rec[5], mem[4][5];
#pragma unroll
            for (int d = 0; d < 5; ++d)
                rec[d] = st.meta()[d];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = first + u * stride;
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    mem[u][d] = 0;
                if ((uint32_t)u < count && i != t) {
                    const uint32_t* r = ((erased >> i) & 1ull) ? ob + cs_slot(A.E, erased, i) * 5 : st.member(u, i);
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        mem[u][d] = r[d];
                }
            }
            bool ok = L <= A.capacity;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    rec[d] ^= mem[u][d];
                ok = ok && (mem[u][4] >> 16) <= L;
            }
            if (!ok || (rec[4] >> 16) > L) {
                bad = (int)s;
                break;
            }
            uint32_t* oh = ob + cs_slot(A.E, erased, t) * 5;
#pragma unroll
            for (int d = 0; d < 5; ++d)
                oh[d] = rec[d];
        }
        if (bad < 0)
            break;
        banned |= 1u << cs_line(S, (uint32_t)bad);
    }
    return S;
}

// Replays the steps in `need` (the lane's step ss and the steps it reads) over
// one chunk column; returns the result of step ss.  A step of a cascade (some
// member recovered by an earlier step) reads that member back from the slot
// where the earlier step stored it -- the dense output slot of its rank, or its
// own slot in place -- which this lane writes first (the slot's owner lane
// writes the same bytes; a lane's later load of an address it stored is
// ordered behind the store).
// Line records and masks for the replay: staged in LDS (any plan), or
// arithmetic in the line index (the sender's matrix shapes, MatLines below).
struct LdsLines {
    const uint32_t* lplan;
    const uint64_t* lmask;
    __device__ uint32_t rec(uint32_t l) const { return lplan[l]; }
    __device__ uint64_t mask(uint32_t l) const { return lmask[l]; }
};

// Where the replay reads a received member's chunk and a line's parity chunk (the chunk column folded into the
// pointers): the batch layout (grp: the group's segment 0, par: its parity line 0), or a row pool through the
// group's K + NL words of the slot map (member i in row so[i], parity line l in row so[K + l], clamped: pool_row).
struct BatchRows {
    static constexpr bool kPool = false;
    const v4u *grp, *par;
    uint32_t C;
};

struct PoolRows {
    static constexpr bool kPool = true;
    const v4u* pool;
    const uint32_t* __restrict__ so;
    uint32_t K, last, C;
};

// (the matrix kernels over the batch layout: no pool)
struct NoPool {
    static constexpr bool kPool = false;
};

template <class Rows, class Lines>
__device__ __forceinline__ v4u cascade_replay(const CSched& S, uint32_t need, uint32_t ss, uint64_t erased,
                                              const Rows& RW, v4u* slot0, uint32_t E, const Lines& LL)
{
    const uint32_t C = RW.C;
    v4u res = {0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t s = 0; s < 8; ++s) {
        if (!((need >> s) & 1u))
            continue;
        const uint32_t l = cs_line(S, s), t = cs_tg(S, s), ln = LL.rec(l);
        const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
        v4u acc, mv[4];
        if constexpr (Rows::kPool)
            acc = ld16(pool_row(RW.pool, RW.so, RW.K + l, RW.last, C));
        else
            acc = ld16(RW.par + (size_t)l * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = first + u * stride;
            mv[u] = v4u{0, 0, 0, 0};
            if ((uint32_t)u < count && i != t) {
                // (the address arithmetic stands in the ternary's arm: a call there changes the batch kernels' code)
                if constexpr (Rows::kPool)
                    mv[u] = ld16(((erased >> i) & 1ull) ? slot0 + (size_t)cs_slot(E, erased, i) * C
                                                        : pool_row(RW.pool, RW.so, i, RW.last, C));
                else
                    mv[u] = ld16(((erased >> i) & 1ull) ? slot0 + (size_t)cs_slot(E, erased, i) * C
                                                        : RW.grp + (size_t)i * C);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc ^= mv[u];
        if (s == ss) {
            res = acc;
            break;
        }
        st16(slot0 + (size_t)cs_slot(E, erased, t) * C, acc);
    }
    return res;
}

// The checker kernel, eight lanes per group (step s = lane & 7): every lane
// derives the group's mask schedule (one instruction stream for the wave's 8
// groups), lane s loads and checks step s -- fec_data_size, its meta record
// and its present members' records in one round of loads -- and forms its
// recovered header record; a member recovered by an earlier step comes from
// that step's lane (shuffles, in step order, only in waves holding a
// cascade).  When every step passes, lane s writes its record and lane 0 the
// mask, out_index and the group's schedule record (16 B: lines, targets, n);
// when one fails, lane 0 runs the serial exact peel for the group instead.
__device__ __forceinline__ v4u cs_pack(const CSched& S) { return v4u{S.lines, (uint32_t)S.tg, (uint32_t)(S.tg >> 32), S.n}; }

__device__ __forceinline__ CSched cs_unpack(const v4u r)
{
    CSched S;
    S.lines = r[0];
    S.tg = (uint64_t)r[1] | ((uint64_t)r[2] << 32);
    S.n = r[3] & 15u;
    return S;
}

// The checker, LPG lanes per group (step s = lane % LPG; the group's lanes
// [base, base + LPG) of one wave, every lane of the wave taking part): writes
// the group's header records, recovered mask and out_index, returns its
// schedule packed.  A group of more than LPG steps (more than LPG erasures
// recovered) takes the serial exact peel.  Dead lanes (live false) join the
// shuffles only.  HS: where the masks and the steps' header bytes come from.
template <typename MT, int LPG, bool kTasks, class Lines, class Hdrs>
__device__ v4u cascade_check_lanes(const CascArgs& A, const rfec_kmask& M, const Lines& LL, const Hdrs& HS, uint32_t g,
                                   bool live, uint32_t s, uint32_t base)
{
    const uint32_t gg = live ? g : 0u;
    const rfec_kplan& P = M.plan;
    const uint32_t K = P.k, NL = P.n_lines;
    const MT kmask = K >= 8 * sizeof(MT) ? ~MT(0) : (MT(1) << K) - MT(1);
    const MT have = (MT)HS.present(gg) & kmask;
    const MT erased = ~have & kmask;
    const uint64_t ppm = HS.parity_present(gg);
    const CSched S = cascade_schedule<MT>(LL, LL.nl(NL), have, ppm, 0u, erased, A.E);
    const bool on = live && s < S.n;
    const uint32_t l = on ? cs_line(S, s) : 0u, t = cs_tg(S, s);
    const uint32_t ln = LL.rec(l);
    const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
    const auto st = HS.step(gg, l, t, (uint64_t)erased);
    uint32_t L = 0, rec[5] = {0, 0, 0, 0, 0}, mem[4][5];
    if (on) {
        L = st.size();
#pragma unroll
        for (int d = 0; d < 5; ++d)
            rec[d] = st.meta()[d];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t i = first + u * stride;
#pragma unroll
        for (int d = 0; d < 5; ++d)
            mem[u][d] = 0;
        if (on && (uint32_t)u < count && i != t && ((erased >> i) & MT(1)) == 0) {
#pragma unroll
            for (int d = 0; d < 5; ++d)
                mem[u][d] = st.member(u, i)[d];
        }
    }
    bool ok = L <= A.capacity;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        ok = ok && (mem[u][4] >> 16) <= L;
#pragma unroll
        for (int d = 0; d < 5; ++d)
            rec[d] ^= mem[u][d];
    }
    // cascades: the members recovered by earlier steps, folded in step order (step r's record is
    // final before round r); only waves that hold one take the shuffles
    const MT depm = on ? ((MT)LL.mask(l) & erased & ~(MT(1) << t)) : MT(0);
    if (__ballot(depm != 0)) {
#pragma unroll
        for (int r = 0; r < LPG - 1; ++r) {
            uint32_t w[5];
#pragma unroll
            for (int d = 0; d < 5; ++d)
                w[d] = (uint32_t)__shfl((int)rec[d], (int)(base + r), kWave);
            if ((uint32_t)r < S.n && ((depm >> cs_tg(S, r)) & MT(1))) {
#pragma unroll
                for (int d = 0; d < 5; ++d)
                    rec[d] ^= w[d];
                ok = ok && (w[4] >> 16) <= L;
            }
        }
    }
    ok = !on || (ok && (rec[4] >> 16) <= L);
    uint32_t all = ok && S.n <= (uint32_t)LPG ? 1u : 0u; // every step of the group taken and passed?
#pragma unroll
    for (int m = 1; m < LPG; m <<= 1)
        all &= (uint32_t)__shfl_xor((int)all, m, kWave);
    CSched X = S;
    if (!live)
        return v4u{0, 0, 0, 0};
    if (!all) { // rare: a rejection -- the serial exact peel (it writes the header records)
        if (s != 0)
            return v4u{0, 0, 0, 0};
        X = cascade_check(A, M, HS, g);
    } else if (on) { // the recovered header record (flex_fec_xor.c:64-85)
        uint32_t* oh = (A.E ? A.out_hdr_dw + (size_t)g * A.E * 5 : A.hdr_dw + (size_t)g * K * 5) +
                       cs_slot(A.E, (uint64_t)erased, t) * 5;
#pragma unroll
        for (int d = 0; d < 5; ++d)
            oh[d] = rec[d];
    }
    if (s == 0) {
        uint64_t rm = 0;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2)
            if ((uint32_t)s2 < X.n)
                rm |= 1ull << cs_tg(X, s2);
        A.recovered[2 * g] = rm;
        A.recovered[2 * g + 1] = 0;
        // the slots' tasks (and out_index: the e-th erased segment's index where it was recovered)
        uint32_t* task = kTasks ? reinterpret_cast<uint32_t*>(A.ws + (size_t)g * A.ws_stride + 16) : nullptr;
        uint64_t m = (uint64_t)erased;
        for (uint32_t q = 0; q < A.Q; ++q) {
            uint32_t ss = 8;
            if (A.E) {
                const uint32_t i = m ? (uint32_t)__ffsll((long long)m) - 1 : 0xFFu;
                m &= m - 1;
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2)
                    if ((uint32_t)s2 < X.n && cs_tg(X, s2) == i)
                        ss = s2;
                A.out_index[(size_t)g * A.E + q] = (uint8_t)(ss < 8 ? i : 0xFFu);
            } else if (q < X.n) {
                ss = q;
            }
            uint32_t w = 0;
            if (ss < 8) {
                const uint32_t tl = cs_line(X, ss), tt = cs_tg(X, ss);
                const bool casc = (LL.mask(tl) & (uint64_t)erased & ~(1ull << tt)) != 0;
                w = kTaskValid | (casc ? kTaskCascade : 0u) | tl | (tt << 8);
            }
            if (kTasks)
                task[q] = w;
        }
    }
    return cs_pack(X);
}

// The checker, LPG = 4 lanes per group (16 groups per wave: the schedule's
// instruction stream is shared by a wave's groups, so fewer lanes per group
// means fewer waves; one round of loads covers up to 4 steps, i.e. up to 4
// erasures recovered).
constexpr int kCheckLanes = 4;

// Checker block b: lane -> (group, step s), the group's lanes from `base` of
// the wave; kTasks: the group's 16-byte schedule record and the slots' task
// words go to the workspace for the payload kernel.
template <typename MT, bool kTasks, class Lines, class Hdrs>
__device__ __forceinline__ void cascade_check_block(const CascArgs& A, const rfec_kmask& M, const Lines& LL,
                                                    const Hdrs& HS, uint32_t b)
{
    const uint32_t gt = b * kBlock + threadIdx.x;
    const uint32_t g = gt / kCheckLanes, s = gt % kCheckLanes;
    const bool live = g < A.groups;
    const v4u r = cascade_check_lanes<MT, kCheckLanes, kTasks>(A, M, LL, HS, live ? g : 0u, live, s,
                                                             (threadIdx.x & (kWave - 1)) & ~(uint32_t)(kCheckLanes - 1));
    if (kTasks && live && s == 0)
        *reinterpret_cast<v4u*>(A.ws + (size_t)g * A.ws_stride) = r;
}

// The checker kernel of the in-place decode.
template <typename MT>
__global__ __launch_bounds__(kBlock) void k_cascade_check(CascArgs A, rfec_kmask M)
{
    cascade_check_block<MT, true>(A, M, KArgLines{M}, BatchHdrs{A, M.plan}, blockIdx.x);
}

// The payload kernel: lane (group, slot, chunk column) reads its slot's task
// word and, for a single-level step (the common case), loads the line's
// parity and other members, all in flight, and stores the recovered chunk --
// no mask work, one dependent load before the payload loads.  A cascade step
// replays the steps it reads from the group's schedule record.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_cascade(CascArgs A, rfec_kmask M)
{
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    __shared__ uint64_t lmask[8];
    const rfec_kplan& P = M.plan;
    if (threadIdx.x < 8)
        lmask[threadIdx.x] = threadIdx.x < P.n_lines ? M.mask[threadIdx.x][0] : 0ull;
    stage_plan(lplan, P); // (ends in a barrier)
    // XCD-swizzled (the grid is a multiple of 8 blocks): a group's lanes share one L2
    const uint32_t t = xcd_block(blockIdx.x, gridDim.x) * kBlock + threadIdx.x;
    if (t >= A.total)
        return;
    const auto [g, q, j] = casc_lane(A, t);
    const uint32_t K = P.k, NL = P.n_lines, C = A.C;
    const uint8_t* wg = A.ws + (size_t)g * A.ws_stride;
    const uint32_t task = reinterpret_cast<const uint32_t*>(wg + 16)[q];
    if (!(task & kTaskValid))
        return;
    const uint32_t l = task & 15u, tgt = (task >> 8) & 0xffu;
    const v4u* grp = A.shards + (size_t)g * K * C + j;
    const v4u* par = A.parity + (size_t)g * NL * C + j;
    v4u* slot0 = A.E ? A.out_sh + (size_t)g * A.E * C + j : A.shards + (size_t)g * K * C + j;
    v4u* dst = slot0 + (size_t)(A.E ? q : tgt) * C;
    if (!(task & kTaskCascade)) { // single level: every other member arrived
        const uint32_t ln = lplan[l];
        const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
        v4u acc = ld16(par + (size_t)l * C);
        v4u mv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = first + u * stride;
            mv[u] = v4u{0, 0, 0, 0};
            if ((uint32_t)u < count && i != tgt)
                mv[u] = ld16(grp + (size_t)i * C);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc ^= mv[u];
        st16(dst, acc);
        return;
    }
    // a cascade: the steps it reads, transitively (a step's erased members other than its target were
    // recovered by earlier steps), replayed from the schedule record
    const uint64_t kmask = K >= 64 ? ~0ull : (1ull << K) - 1ull;
    const uint64_t erased = ~A.present[2 * g] & kmask;
    const CSched S = cs_unpack(*reinterpret_cast<const v4u*>(wg));
    uint32_t ss = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if ((uint32_t)s < S.n && cs_tg(S, s) == tgt)
            ss = s;
    uint32_t need = 1u << ss; // (the closure is cascade_dense_tail's, kept twice deliberately: DESIGN 7.13)
#pragma unroll 1
    for (int s = (int)ss; s >= 0; --s) {
        if (!((need >> s) & 1u))
            continue;
        const uint64_t dm = lmask[cs_line(S, s)] & erased & ~(1ull << cs_tg(S, s));
        for (int s2 = 0; s2 < s; ++s2)
            if ((dm >> cs_tg(S, s2)) & 1ull)
                need |= 1u << s2;
    }
    st16(dst, cascade_replay(S, need, ss, erased, BatchRows{grp, par, C}, slot0, A.E, LdsLines{lplan, lmask}));
}

// A dense payload lane whose target no line recovers at once (a cascade):
// the group's mask schedule (cascade_schedule without the header checks),
// the steps the target's step reads, transitively, replayed in registers.
// (SL: the schedule's masks -- kernel arguments or constants; LL: the replay's; RW: the received rows)
template <typename MT, class SLines, class Rows, class Lines>
__device__ __forceinline__ void cascade_dense_tail(const CascArgs& A, const SLines& SL, uint32_t NL, uint64_t have,
                                                   uint64_t erased, uint64_t ppm, uint32_t tgt, const Rows& RW,
                                                   v4u* slot0, v4u* dst, const Lines& LL)
{
    const CSched S = cascade_schedule<MT>(SL, NL, (MT)have, ppm, 0u, (MT)erased, A.E);
    uint32_t ss = 8;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if ((uint32_t)s < S.n && cs_tg(S, s) == tgt)
            ss = s;
    if (ss == 8)
        return; // not recoverable
    uint32_t need = 1u << ss; // (the closure is k_decode_cascade's, kept twice deliberately: DESIGN 7.13)
#pragma unroll 1
    for (int s = (int)ss; s >= 0; --s) {
        if (!((need >> s) & 1u))
            continue;
        const uint64_t dm = LL.mask(cs_line(S, s)) & erased & ~(1ull << cs_tg(S, s));
        for (int s2 = 0; s2 < s; ++s2)
            if ((dm >> cs_tg(S, s2)) & 1ull)
                need |= 1u << s2;
    }
    st16(dst, cascade_replay(S, need, ss, erased, RW, slot0, A.E, LL));
}

// Dense output, one launch: rounds of 8 checker blocks spread over the grid
// (header_block_xcd; they write the headers, recovered masks and out_index, no
// task words) between the payload lanes' rounds, which need nothing from them: lane
// (group, slot q, chunk column) recovers the group's q-th erased segment
// through a line that fires at once for it (parity received, every other
// member present) or, when none does, replays the group's mask schedule
// (cascade_schedule without the header checks).  Any line that recovers a
// segment gives its bytes, so the data equal the exact peel's wherever it
// recovers; a segment it leaves unrecovered (a rejected line) may still be
// written, its out_index 0xFF.  The checker's latency-bound work overlaps the
// payload traffic instead of preceding it: c3 full 128.3-128.8 us vs 131.5-131.8
// us for check + k_decode_cascade (A/Bs on one box; the checker's blocks all at
// the head of the grid: 134.6 us; spread but not XCD-aligned with the payload:
// 129.4-130.3 us; the line search through LDS copies of the masks instead of
// the kernel arguments: 131 us; checker rounds 3 or 8 rounds further ahead: no
// change).  The payload lanes wait on the masks where k_decode_cascade waited
// on its task word (L2).

template <typename MT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_cascade_dense(
    CascArgs A, rfec_kmask M, uint32_t n_hr, uint32_t every, uint32_t npay8)
{
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(n_hr, every, npay8, &hb, &pb)) { // (checker blocks XCD-aligned with the payload sweep)
        cascade_check_block<MT, false>(A, M, KArgLines{M}, BatchHdrs{A, M.plan}, hb);
        return;
    }
    __shared__ uint32_t lplan[RFEC_MAX_LINES];
    __shared__ uint64_t lmask[8];
    const rfec_kplan& P = M.plan;
    if (threadIdx.x < 8)
        lmask[threadIdx.x] = threadIdx.x < P.n_lines ? M.mask[threadIdx.x][0] : 0ull;
    stage_plan(lplan, P); // (ends in a barrier)
    const uint32_t t = pb * kBlock + threadIdx.x; // (XCD-swizzled: a group's lanes share one L2)
    if (t >= A.total)
        return;
    const auto [g, q, j] = casc_lane(A, t);
    const uint32_t K = P.k, NL = P.n_lines, C = A.C;
    // (MT: 32-bit masks for k <= 32, the low words of present / parity_present)
    constexpr uint32_t MB = 8 * sizeof(MT);
    const MT kmaskM = K >= MB ? ~(MT)0 : (((MT)1 << K) - 1);
    const MT hv = (MT)A.present[2 * g] & kmaskM, er = ~hv & kmaskM;
    const uint64_t have = hv, erased = er, ppm = (uint32_t)A.parity_present[g]; // (NL <= 8 here)
    MT e = er; // slot q: the q-th erased segment
    for (uint32_t i = 0; i < q; ++i)
        e &= e - 1;
    if (!e)
        return;
    const uint32_t tgt = MB == 32 ? (uint32_t)__ffs((int)e) - 1 : (uint32_t)__ffsll((long long)e) - 1;
    // the first line that fires at once for it (masks and line records from the
    // kernel arguments: scalar loads, no LDS round trips before the payload loads)
    uint32_t l = 0xFFu, ln = 0;
    {
        const MT tb = (MT)1 << tgt;
        const uint32_t pp = (uint32_t)ppm;
#pragma unroll
        for (int x = 7; x >= 0; --x) {
            const MT lm = (MT)M.mask[x][0];
            if ((uint32_t)x < NL && ((pp >> x) & 1u) && (lm & er) == tb && (lm & hv)) {
                l = (uint32_t)x;
                ln = reinterpret_cast<const uint32_t*>(P.line)[x];
            }
        }
    }
    const v4u* grp = A.shards + (size_t)g * K * C + j;
    const v4u* par = A.parity + (size_t)g * NL * C + j;
    v4u* slot0 = A.out_sh + (size_t)g * A.E * C + j;
    v4u* dst = slot0 + (size_t)q * C;
    if (l != 0xFFu) { // single level
        const uint32_t first = ln & 0xff, stride = (ln >> 8) & 0xff, count = (ln >> 16) & 0xff;
        v4u acc = ld16(par + (size_t)l * C);
        // members through a descriptor over the first active lane's group (wave_rsrc: no per-load
        // branch, all four loads in flight; with `if (used) load` hipcc waited on each load in turn)
        const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g); // lanes' groups ascend
        const __amdgpu_buffer_rsrc_t rs = wave_rsrc(A.shards + (size_t)gb * K * C);
        const uint32_t grp0 = ((g - gb) * K * C + j) * 16u;
        v4u mv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = first + u * stride;
            mv[u] = bld16(rs, (uint32_t)u < count && i != tgt ? grp0 + i * C * 16u : kNoLoad);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc ^= mv[u];
        st16(dst, acc);
        return;
    }
    cascade_dense_tail<MT>(A, KArgLines{M}, NL, have, erased, ppm, tgt, BatchRows{grp, par, A.C}, slot0, dst,
                           LdsLines{lplan, lmask});
}

// The sender's full matrix plans (rows of COL consecutive segments, then the
// columns, flex_fec_sender.c:166-233), K = 6..16 as
// flex_fec_sender_num_packets picks them (COL 3 for K <= 9, else 4): the dense
// cascade decode with the plan folded into the code.  A payload lane's target
// lies in exactly one row and one column, so the first line that fires at
// once for it (plan order: rows first) is its row, else its column -- two
// mask tests on masks that are shifts of constants, instead of the generic
// kernel's search over eight kernel-argument masks and line records; the
// q-th erased segment is found by clearing q low bits without a run-time
// loop for q < 4.  Cascades (no line fires at once) replay the mask schedule
// as the generic kernel does, with the line records computed from the index.
template <int K, int COL>
struct MatLines {
    using Sh = MatrixShape<K, COL>;
    static constexpr int NR = Sh::n_rows(), NL = NR + COL, MX = COL > Sh::R ? COL : Sh::R; // MX: a line's most members
    static_assert(K >= 2 * COL && K <= 16 && NL <= 8 && MX <= 4, "the cascade kernels' shapes");
    static constexpr uint32_t KM = (1u << K) - 1u, ROW = (1u << COL) - 1u;
    static constexpr uint32_t col0()
    {
        uint32_t m = 0;
        for (int r = 0; r < Sh::R; ++r)
            m |= 1u << (r * COL);
        return m;
    }
    static constexpr uint32_t COL0 = col0();
    // line l: first | stride << 8 | count << 16 (rows l < NR, then column l - NR)
    __device__ uint32_t rec(uint32_t l) const
    {
        const bool row = l < (uint32_t)NR;
        const uint32_t c = l - NR;
        const uint32_t first = row ? l * COL : c, stride = row ? 1u : (uint32_t)COL;
        const uint32_t count = row ? min((uint32_t)COL, K - l * COL) : (K - c + COL - 1) / COL;
        return first | stride << 8 | count << 16;
    }
    __device__ uint64_t mask(uint32_t l) const
    {
        return l < (uint32_t)NR ? (ROW << (l * COL)) & KM : (COL0 << (l - NR)) & KM;
    }
    __device__ uint32_t nl(uint32_t) const { return NR + COL; }
};

// The payload half of the matrix kernels, shared by the three of them (HS: where the masks come from; PL: NoPool
// for the batch layout, or the pool and the slot map -- the PoolRows of group 0 at chunk column 0).  The batch
// layout's and the pool's lanes differ in where the group's rows are, in the loads of a line that fires at once
// and in the row source they hand to the cascade tail.
template <int K, int COL, class Hdrs, class Pool>
__device__ __forceinline__ void matrix_payload_block(const CascArgs& A, const Hdrs& HS, const Pool& PL, uint32_t pb)
{
    using LL = MatLines<K, COL>;
    constexpr int NR = LL::NR, NL = LL::NL, MX = LL::MX;
    const uint32_t t = pb * kBlock + threadIdx.x; // (XCD-swizzled: a group's lanes share one L2)
    if (t >= A.total)
        return;
    const auto [g, q, j] = casc_lane(A, t);
    const uint32_t C = A.C;
    const uint32_t hv = (uint32_t)HS.present(g) & LL::KM, er = ~hv & LL::KM;
    const uint32_t pp = (uint32_t)HS.parity_present(g);
    uint32_t e = er; // slot q: the q-th erased segment
#pragma unroll
    for (int i = 0; i < 3; ++i)
        e = (uint32_t)i < q ? e & (e - 1u) : e;
    for (uint32_t i = 3; i < q; ++i)
        e &= e - 1u;
    if (!e)
        return;
    const uint32_t tgt = (uint32_t)__ffs((int)e) - 1, tb = 1u << tgt;
    const uint32_t r = tgt / COL, c = tgt - r * COL;
    const uint32_t rm = (LL::ROW << (r * COL)) & LL::KM, cm = (LL::COL0 << c) & LL::KM;
    const bool row_fires = r < (uint32_t)NR && ((pp >> r) & 1u) && (rm & er) == tb && (rm & hv);
    const bool col_fires = ((pp >> (NR + c)) & 1u) && (cm & er) == tb && (cm & hv);
    // the group's rows at chunk column j: in the batch layout (the addresses formed here, not in a row source
    // handed down: that changes the batch kernels' code), or through the group's words of the map
    const v4u *grp = nullptr, *par = nullptr;
    Pool RW = PL;
    if constexpr (Pool::kPool) {
        RW.pool += j, RW.so += (size_t)g * (K + NL);
    } else {
        grp = A.shards + (size_t)g * K * C + j;
        par = A.parity + (size_t)g * NL * C + j;
    }
    v4u* slot0 = A.out_sh + (size_t)g * A.E * C + j;
    v4u* dst = slot0 + (size_t)q * C;
    if (row_fires || col_fires) { // single level
        const uint32_t l = row_fires ? r : NR + c;
        const uint32_t first = row_fires ? r * COL : c, stride = row_fires ? 1u : (uint32_t)COL;
        const uint32_t count = row_fires ? min((uint32_t)COL, K - r * COL) : (K - c + COL - 1) / COL;
        if constexpr (Pool::kPool) {
            // the rows lie anywhere in the pool: plain 64-bit addresses -- the map words of the wanted slots first,
            // then the parity and the MX member chunks unconditionally and in flight together; a member that is not
            // wanted (past the line's end, or the target) re-reads the parity chunk and is XORed as zero
            const v4u* src[MX + 1];
            bool use[MX];
            src[MX] = pool_row(RW.pool, RW.so, K + l, RW.last, C);
#pragma unroll
            for (int u = 0; u < MX; ++u) {
                const uint32_t i = first + u * stride;
                use[u] = (uint32_t)u < count && i != tgt;
                src[u] = pool_row(RW.pool, RW.so, use[u] ? i : K + l, RW.last, C);
            }
            v4u acc = ld16(src[MX]);
            v4u mv[MX];
#pragma unroll
            for (int u = 0; u < MX; ++u)
                mv[u] = ld16(src[u]);
#pragma unroll
            for (int u = 0; u < MX; ++u)
                acc ^= use[u] ? mv[u] : v4u{0, 0, 0, 0};
            st16(dst, acc);
        } else {
            v4u acc = ld16(par + (size_t)l * C);
            // members through a descriptor over the first active lane's group (see k_decode_cascade_dense)
            const uint32_t gb = (uint32_t)__builtin_amdgcn_readfirstlane((int)g); // lanes' groups ascend
            const __amdgpu_buffer_rsrc_t rs = wave_rsrc(A.shards + (size_t)gb * K * C);
            const uint32_t grp0 = ((g - gb) * K * C + j) * 16u;
            v4u mv[MX];
#pragma unroll
            for (int u = 0; u < MX; ++u) {
                const uint32_t i = first + u * stride;
                mv[u] = bld16(rs, (uint32_t)u < count && i != tgt ? grp0 + i * C * 16u : kNoLoad);
            }
#pragma unroll
            for (int u = 0; u < MX; ++u)
                acc ^= mv[u];
            st16(dst, acc);
        }
        return;
    }
    if constexpr (Pool::kPool)
        cascade_dense_tail<uint32_t>(A, LL{}, NL, hv, er, pp, tgt, RW, slot0, dst, LL{});
    else
        cascade_dense_tail<uint32_t>(A, LL{}, NL, hv, er, pp, tgt, BatchRows{grp, par, A.C}, slot0, dst, LL{});
}

template <int K, int COL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_matrix_dense(
    CascArgs A, rfec_kmask M, uint32_t n_hr, uint32_t every, uint32_t npay8)
{
    const BatchHdrs HS{A, M.plan};
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(n_hr, every, npay8, &hb, &pb)) // the checker blocks, as the generic kernel's
        cascade_check_block<uint32_t, false>(A, M, MatLines<K, COL>{}, HS, hb);
    else
        matrix_payload_block<K, COL>(A, HS, NoPool{}, pb);
}

// The same decode from packed matrix records (rfec_recover_packed_matrix_out;
// layout in razor_fec.h): group g's record holds its two masks, then per
// output slot e (the group's e-th erased segment t, in row r and column c) a
// row half -- row r's fec_meta, fec_data_size and other members' records --
// and a column half of the same form.  A step (line l, target t) of the
// checker reads the half of slot rank(t) that belongs to l: one contiguous
// run where the batch layout costs a fec_data_size, a meta record and up to
// three member records from three arrays, in sectors shared with the lines
// that do not fire.  An erased member's position holds zeros (the checker does
// not load it; the cascade's earlier steps supply it).  The payload lanes
// read the record's first 16 bytes and no other header byte.
template <int K, int COL>
struct PackedMatHdrs {
    static constexpr uint32_t NR = MatLines<K, COL>::NR, R = MatrixShape<K, COL>::R;
    static constexpr uint32_t RH = 24 + 20 * (COL - 1), CH = 24 + 20 * (R - 1), S = RH + CH; // bytes
    const uint8_t* packed;
    uint32_t pk_stride;
    struct Step {
        const uint32_t* hs; // the half slot: meta (5 dwords), fec_data_size, the line's other members
        uint32_t t;
        __device__ const uint32_t* meta() const { return hs; }
        __device__ uint32_t size() const { return hs[5] & 0xFFFFu; }
        // the line's u-th member, segment i != t: the members after the target sit one position lower
        __device__ const uint32_t* member(uint32_t u, uint32_t i) const { return hs + 6 + 5 * (u - (i > t ? 1u : 0u)); }
    };
    __device__ const uint64_t* rec(uint32_t g) const
    {
        return reinterpret_cast<const uint64_t*>(packed + (size_t)g * pk_stride);
    }
    __device__ uint64_t present(uint32_t g) const { return rec(g)[0]; }
    __device__ uint64_t parity_present(uint32_t g) const { return rec(g)[1]; }
    __device__ Step step(uint32_t g, uint32_t l, uint32_t t, uint64_t erased) const
    {
        const uint32_t e = (uint32_t)__popcll(erased & ((1ull << t) - 1ull)); // < per_group: the schedule's targets
        return Step{reinterpret_cast<const uint32_t*>(packed + (size_t)g * pk_stride + 16 + e * S + (l < NR ? 0u : RH)), t};
    }
};

template <int K, int COL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_matrix_packed(
    CascArgs A, rfec_kmask M, uint32_t n_hr, uint32_t every, uint32_t npay8, const uint8_t* __restrict__ packed,
    uint32_t pk_stride)
{
    const PackedMatHdrs<K, COL> HS{packed, pk_stride};
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(n_hr, every, npay8, &hb, &pb))
        cascade_check_block<uint32_t, false>(A, M, MatLines<K, COL>{}, HS, hb);
    else
        matrix_payload_block<K, COL>(A, HS, NoPool{}, pb);
}

// The same decode through a slot map over a row pool (rfec_recover_indexed_matrix_out): the checker half is
// k_decode_matrix_dense's -- it reads the tables only -- and a payload lane reads member i of its group
// from row so[i] of the pool and parity line l from row so[K + l] (so: the group's K + NL words of src_of; pool:
// chunk j of row 0).  The rows lie anywhere in the pool, so no descriptor spans a wave's loads (wave_rsrc / bld16 do
// not carry over): they are plain 64-bit addresses, as in k_decode_rows_indexed -- the map words of the wanted
// slots first, then the parity and the MX member chunks unconditionally and in flight together; a member that is
// not wanted (past the line's end, or the target) re-reads the parity chunk and is XORed as zero.  A row index is
// clamped to `last` = n_rows - 1 before it is used (pool_row).  Only the entries of present members and received
// parities are read: a line fires, or takes a step of the schedule, with its parity received, and a member that
// was not received comes from the dense out slot where an earlier step stored it.  The payload block, the tail and
// the replay are the batch kernels' own, with PoolRows as their row source.
template <int K, int COL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_matrix_indexed(
    CascArgs A, rfec_kmask M, uint32_t n_hr, uint32_t every, uint32_t npay8, const v4u* rows, uint32_t last,
    const uint32_t* __restrict__ src_of)
{
    const BatchHdrs HS{A, M.plan}; // (the masks and the checker's header bytes: the tables, as the dense kernel's)
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(n_hr, every, npay8, &hb, &pb)) // the checker blocks: the tables only, never a payload row
        cascade_check_block<uint32_t, false>(A, M, MatLines<K, COL>{}, HS, hb);
    else
        matrix_payload_block<K, COL>(A, HS, PoolRows{rows, src_of, K, last, A.C}, pb);
}

// The sections of a window of several shapes (rfec_wire_regroup_shapes' dense tables, one section per shape) in
// one launch (rfec_recover_indexed_shapes_out): every section gets the grid its own call would get --
// k_decode_matrix_indexed's for a full matrix of k = 6..16, k_decode_rows_indexed<0, 4>'s for a row layout -- and
// the grids lie end to end.  Each is a whole number of rounds of 8 blocks, so a block's index within its section
// keeps its residue mod 8 and with it the XCD it has in the single call.  A block finds its section in the prefix
// of first blocks (wave-uniform: the section's arguments come through scalar loads) and runs that section's body
// on its relative index; the sections' outputs are the call's four arrays from the section's first output row on.
//
// The bodies are the single calls' own (cascade_check_block / matrix_payload_block, line_headers /
// RFEC_ROWS_INDEXED_LANE), their CascArgs / PeelArgs built in registers from the section's arguments.  The checker's
// serial peel and the header lanes index the plan's lines and masks at run time, and an argument block has no room
// for an rfec_kmask per section: a header block builds the one of its section in LDS (a matrix's lines and masks
// from MatLines, a row layout's from (k, col)) before it runs the body.  The payload lanes read none of it.
constexpr uint32_t kShapeMatrix = 1u << 24;

struct ShapeSec {
    const uint32_t* src_of;
    const uint32_t* hdr_dw;
    const uint64_t* present;
    const uint32_t* meta_dw;
    const uint16_t* fsize;
    const uint64_t* parity_present;
    uint32_t groups, first_row; // rows decoded; the first of its output rows
    uint32_t shape;             // k | col << 8 | log2 of the header lanes per group << 12 | n_lines << 16 | kShapeMatrix
    uint32_t every;             // payload rounds per header round (Rounds8)
};
static_assert(sizeof(ShapeSec) == 64, "the argument block's budget per section");

struct ShapesArgs {
    ShapeSec sec[RFEC_RECOVER_MAX_SHAPES];                // the sections with groups, in order
    uint32_t first_block[RFEC_RECOVER_MAX_SHAPES];        // of each, a multiple of 8
    uint32_t n;
    const v4u* rows;
    uint32_t last, has_rows; // n_rows - 1 (0: none); n_rows != 0 (else no payload lanes)
    uint64_t* recovered;
    v4u* out_sh;
    uint32_t* out_hdr_dw;
    uint8_t* out_index;
    uint32_t E, C, cd, capacity;
    FastDiv divC, divQC;  // cd, E * cd
    FastDiv divCol[3];    // a row layout's col = 2, 3, 4
};
static_assert(sizeof(ShapesArgs) <= 4096, "one argument block");

template <int K, int COL>
__device__ __forceinline__ void shapes_matrix_block(const CascArgs& A, rfec_kmask& sM, bool checker,
                                                    uint32_t hb, uint32_t pb, const v4u* rows, uint32_t last,
                                                    const uint32_t* __restrict__ src_of)
{
    using LL = MatLines<K, COL>;
    if (checker) {
        if (threadIdx.x == 0) {
            sM.plan.k = K;
            sM.plan.n_lines = LL::NL;
        }
        if (threadIdx.x < (uint32_t)LL::NL) { // (what the serial peel reads: KArgLines)
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = LL{}.rec(threadIdx.x);
            sM.mask[threadIdx.x][0] = LL{}.mask(threadIdx.x);
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        cascade_check_block<uint32_t, false>(A, sM, LL{}, BatchHdrs{A, sM.plan}, hb);
    } else {
        matrix_payload_block<K, COL>(A, BatchHdrs{A, sM.plan}, PoolRows{rows, src_of, K, last, A.C}, pb);
    }
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_decode_shapes_indexed(ShapesArgs S)
{
    __shared__ rfec_kmask sM;
    uint32_t p = 0;
    for (uint32_t q = 1; q < S.n; ++q) // (uniform: scalar loads and compares)
        p = blockIdx.x >= S.first_block[q] ? q : p;
    const ShapeSec& T = S.sec[p];
    const uint32_t rb = blockIdx.x - S.first_block[p];
    const uint32_t G = T.groups, K = T.shape & 0xffu, lg = (T.shape >> 12) & 15u;
    // the section's grid, as its own call lays it out (rounds_of_8): G << lg < 2^32 and total < 2^31, host-checked
    const uint32_t total = S.has_rows ? G * S.E * S.cd : 0u, hl = G << lg;
    const uint32_t n_hdr = (hl >> 8) + ((hl & 255u) != 0), npay8 = (((total + 255u) >> 8) + 7u) & ~7u;
    uint32_t hb = 0, pb = 0;
    const bool header = header_block_xcd_at(rb, (n_hdr + 7u) >> 3, T.every, npay8, &hb, &pb);
    const size_t o = T.first_row;
    if (T.shape & kShapeMatrix) {
        CascArgs A = {}; // (no shards, no parity, no workspace: rfec_launch_recover_indexed_matrix's)
        A.hdr_dw = const_cast<uint32_t*>(T.hdr_dw);
        A.meta_dw = T.meta_dw, A.fsize = T.fsize, A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = S.recovered + 2 * o;
        A.out_sh = S.out_sh + o * S.E * S.C;
        A.out_hdr_dw = S.out_hdr_dw + o * S.E * 5;
        A.out_index = S.out_index + o * S.E;
        A.E = A.Q = S.E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity;
        A.divC = S.divC, A.divQC = S.divQC;
#define RFEC_MS(KK, CC)                                                                                           \
    case KK: shapes_matrix_block<KK, CC>(A, sM, header, hb, pb, S.rows, S.last, T.src_of); break;
        switch (K) {
            RFEC_MATRIX_SHAPES(RFEC_MS)
        default: break;
        }
#undef RFEC_MS
        return;
    }
    // a row layout: k and col at run time, the masks from (k, col)
    const uint32_t col = (T.shape >> 8) & 15u, NL = (T.shape >> 16) & 0xffu;
    PeelArgs B = {};
    B.hdr = reinterpret_cast<rfec_hdr*>(const_cast<uint32_t*>(T.hdr_dw)); // dense output: hdr is only read
    B.present = T.present;
    B.meta = reinterpret_cast<const rfec_hdr*>(T.meta_dw);
    B.fsize = T.fsize, B.parity_present = T.parity_present;
    B.recovered = S.recovered + 2 * o;
    B.groups = G, B.capacity = S.capacity, B.gpb = 1, B.nlp_log2 = lg;
    B.out_hdr = reinterpret_cast<rfec_hdr*>(S.out_hdr_dw + o * S.E * 5);
    B.out_index = S.out_index + o * S.E;
    B.out_per_group = S.E;
    if (header) {
        if (hb >= n_hdr)
            return;
        if (threadIdx.x == 0) {
            sM.plan.k = (uint16_t)K;
            sM.plan.n_lines = (uint8_t)NL;
        }
        if (threadIdx.x < NL) { // row l: members l col .. of the k
            const uint32_t first = threadIdx.x * col, cnt = min(col, K - first);
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = first | 1u << 8 | cnt << 16;
            sM.mask[threadIdx.x][0] = ((1ull << cnt) - 1ull) << first;
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        [[clang::always_inline]] line_headers(B, sM, hb); // (a call would put B on the stack: scratch)
        return;
    }
    const DenseOut D = {S.out_sh + o * S.E * S.C, S.E};
    RFEC_ROWS_INDEXED_LANE(0, 4, S.rows, S.last, T.src_of, total, S.C, S.divC, S.divQC, B, D, K, col,
                           S.divCol[col - 2u], pb)
}

// The sections of a window of ANY of the planner's shapes in one launch (rfec_recover_indexed_window_out):
// k_decode_shapes_indexed's scheme -- every section the grid its own call would get, the grids end to end in whole
// rounds of 8, a block finds its section in the prefix of first blocks and builds the family's argument struct in
// registers -- over four families: (1) a full matrix of k = 6..16 and (2) a row layout of rows of <= 4 with k <= 64,
// the compiled bodies as above; (3) a full matrix of k = 17..128, k_decode_matrix_wide's bodies (one checker lane
// per group); (4) any other row layout, k_decode_rows_wide's.  A wide section keeps its own table pitch (k + n_lines
// map words, n_lines meta records per group: the bodies take NL from the section, not from ceil(k / col)).
//
// The outputs of a section are the call's four arrays from the section's first output row on: the offset goes into
// the four output BASES of the family's struct, and every body forms its addresses from those bases -- the checker's
// read-back of the record of a member recovered earlier (cascade_check's and wide_check_block's `ob`) and the
// replay's slot0 (matrix_payload_block, wide_payload_block) included -- so a cascade's intermediates stay inside
// the group's own out slots in any section.
//
// A section's entry holds what a run-time shape needs beyond ShapeSec: col in 8 bits, its FastDiv, and for a wide
// matrix the row lines and column 0's member mask.
struct WinSec {
    const uint32_t* src_of;
    const uint32_t* hdr_dw;
    const uint64_t* present;
    const uint32_t* meta_dw;
    const uint16_t* fsize;
    const uint64_t* parity_present;
    uint32_t groups, first_row; // rows decoded; the first of its output rows
    uint32_t shape;             // k | col << 8 | n_lines << 16 | log2 of the header lanes per group << 24 | family << 28
    uint32_t every;             // payload rounds per header round (Rounds8)
    FastDiv divCol;             // col
    uint32_t nr;                // family 3: the row lines (then n_lines - nr column lines)
    uint64_t col0[2];           // family 3: column 0's member mask
};
static_assert(sizeof(WinSec) == 96, "the argument block's budget per section");

struct WindowArgs {
    WinSec sec[RFEC_RECOVER_MAX_SHAPES];           // the sections with groups, in order
    uint32_t first_block[RFEC_RECOVER_MAX_SHAPES]; // of each, a multiple of 8
    uint32_t n;
    const v4u* rows;
    uint32_t last, has_rows; // n_rows - 1 (0: none); n_rows != 0 (else no payload lanes)
    uint64_t* recovered;
    v4u* out_sh;
    uint32_t* out_hdr_dw;
    uint8_t* out_index;
    uint32_t E, C, cd, capacity;
    FastDiv divC, divQC; // cd, E * cd
};
static_assert(sizeof(WindowArgs) <= 4096, "one argument block");

// (shapes_matrix_block's statements, a copy of this kernel's own: as a second caller of that function this kernel
// changed k_decode_shapes_indexed's code in the LDS fill)
template <int K, int COL>
__device__ __forceinline__ void window_matrix_block(const CascArgs& A, rfec_kmask& sM, bool checker, uint32_t hb,
                                                    uint32_t pb, const v4u* rows, uint32_t last,
                                                    const uint32_t* __restrict__ src_of)
{
    using LL = MatLines<K, COL>;
    if (checker) {
        if (threadIdx.x == 0) {
            sM.plan.k = K;
            sM.plan.n_lines = LL::NL;
        }
        if (threadIdx.x < (uint32_t)LL::NL) { // (what the serial peel reads: KArgLines)
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = LL{}.rec(threadIdx.x);
            sM.mask[threadIdx.x][0] = LL{}.mask(threadIdx.x);
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        cascade_check_block<uint32_t, false>(A, sM, LL{}, BatchHdrs{A, sM.plan}, hb);
    } else {
        matrix_payload_block<K, COL>(A, BatchHdrs{A, sM.plan}, PoolRows{rows, src_of, K, last, A.C}, pb);
    }
}

__global__ __launch_bounds__(kBlock) void k_decode_window_indexed(WindowArgs S)
{
    __shared__ rfec_kmask sM;
    uint32_t p = 0;
    for (uint32_t q = 1; q < S.n; ++q) // (uniform: scalar loads and compares)
        p = blockIdx.x >= S.first_block[q] ? q : p;
    const WinSec& T = S.sec[p];
    const uint32_t rb = blockIdx.x - S.first_block[p];
    const uint32_t G = T.groups, K = T.shape & 0xffu, col = (T.shape >> 8) & 0xffu, NL = (T.shape >> 16) & 0xffu;
    const uint32_t lg = (T.shape >> 24) & 15u, family = T.shape >> 28;
    // the section's grid, as its own call lays it out (rounds_of_8): G << lg < 2^32 and total < 2^31, host-checked
    const uint32_t total = S.has_rows ? G * S.E * S.cd : 0u, hl = G << lg;
    const uint32_t n_hdr = (hl >> 8) + ((hl & 255u) != 0), npay8 = (((total + 255u) >> 8) + 7u) & ~7u;
    uint32_t hb = 0, pb = 0;
    const bool header = header_block_xcd_at(rb, (n_hdr + 7u) >> 3, T.every, npay8, &hb, &pb);
    if (header && hb >= n_hdr) // (the round's blocks past the section's last header lane)
        return;
    const size_t o = T.first_row;
    if (family == 1) { // a full matrix of k = 6..16
        CascArgs A = {}; // (no shards, no parity, no workspace: rfec_launch_recover_indexed_matrix's)
        A.hdr_dw = const_cast<uint32_t*>(T.hdr_dw);
        A.meta_dw = T.meta_dw, A.fsize = T.fsize, A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = S.recovered + 2 * o;
        A.out_sh = S.out_sh + o * S.E * S.C;
        A.out_hdr_dw = S.out_hdr_dw + o * S.E * 5;
        A.out_index = S.out_index + o * S.E;
        A.E = A.Q = S.E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity;
        A.divC = S.divC, A.divQC = S.divQC;
#define RFEC_MW(KK, CC)                                                                                           \
    case KK: window_matrix_block<KK, CC>(A, sM, header, hb, pb, S.rows, S.last, T.src_of); break;
        switch (K) {
            RFEC_MATRIX_SHAPES(RFEC_MW)
        default: break;
        }
#undef RFEC_MW
        return;
    }
    if (family == 3) { // a full matrix of k = 17..128: k and col at run time, one checker lane per group
        WideArgs A = {};
        A.rows = S.rows, A.src_of = T.src_of, A.hdr_dw = T.hdr_dw, A.meta_dw = T.meta_dw, A.fsize = T.fsize;
        A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = S.recovered + 2 * o;
        A.out_sh = S.out_sh + o * S.E * S.C;
        A.out_hdr_dw = S.out_hdr_dw + o * S.E * 5;
        A.out_index = S.out_index + o * S.E;
        A.E = S.E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity, A.last = S.last;
        A.K = K, A.COL = col, A.NR = T.nr, A.NL = NL;
        A.col0[0] = T.col0[0], A.col0[1] = T.col0[1];
        A.divC = S.divC, A.divQC = S.divQC, A.divCol = T.divCol;
        if (header)
            wide_check_block(A, hb);
        else
            wide_payload_block(A, pb);
        return;
    }
    if (family == 4) { // a row layout of any width: k, col and the lines at run time
        RowsWideArgs A = {};
        A.rows = S.rows, A.src_of = T.src_of, A.hdr_dw = T.hdr_dw, A.meta_dw = T.meta_dw, A.fsize = T.fsize;
        A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = S.recovered + 2 * o;
        A.out_sh = S.out_sh + o * S.E * S.C;
        A.out_hdr_dw = S.out_hdr_dw + o * S.E * 5;
        A.out_index = S.out_index + o * S.E;
        A.E = S.E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity, A.last = S.last;
        A.K = K, A.COL = col, A.NL = NL, A.lg = lg, A.n_hdr = n_hdr;
        A.divC = S.divC, A.divQC = S.divQC, A.divCol = T.divCol;
        if (header)
            rows_wide_header_block(A, hb);
        else
            rows_wide_payload_block(A, pb);
        return;
    }
    // family 2, a row layout of rows of <= 4 with k <= 64: k and col at run time, the masks from (k, col)
    PeelArgs B = {};
    B.hdr = reinterpret_cast<rfec_hdr*>(const_cast<uint32_t*>(T.hdr_dw)); // dense output: hdr is only read
    B.present = T.present;
    B.meta = reinterpret_cast<const rfec_hdr*>(T.meta_dw);
    B.fsize = T.fsize, B.parity_present = T.parity_present;
    B.recovered = S.recovered + 2 * o;
    B.groups = G, B.capacity = S.capacity, B.gpb = 1, B.nlp_log2 = lg;
    B.out_hdr = reinterpret_cast<rfec_hdr*>(S.out_hdr_dw + o * S.E * 5);
    B.out_index = S.out_index + o * S.E;
    B.out_per_group = S.E;
    if (header) {
        if (threadIdx.x == 0) {
            sM.plan.k = (uint16_t)K;
            sM.plan.n_lines = (uint8_t)NL;
        }
        if (threadIdx.x < NL) { // row l: members l col .. of the k
            const uint32_t first = threadIdx.x * col, cnt = min(col, K - first);
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = first | 1u << 8 | cnt << 16;
            sM.mask[threadIdx.x][0] = ((1ull << cnt) - 1ull) << first;
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        [[clang::always_inline]] line_headers(B, sM, hb); // (a call would put B on the stack: scratch)
        return;
    }
    const DenseOut D = {S.out_sh + o * S.E * S.C, S.E};
    RFEC_ROWS_INDEXED_LANE(0, 4, S.rows, S.last, T.src_of, total, S.C, S.divC, S.divQC, B, D, K, col, T.divCol, pb)
}

// k_decode_window_indexed with an out-slot count per section (rfec_recover_indexed_window_each_out): section p's
// rows have E[p] out slots each and the sections' slots are packed end to end, so `recovered` is still indexed by
// output row first[p] + c while out_index, out_hdr and out_shards are indexed by slot slot_first[p] + c E[p] + e,
// slot_first[p] the sum of groups[q] E[q] over q < p.  The same scheme: window_section_grid with the section's own E,
// the grids end to end in whole rounds of 8.  Every family's struct already carries its own E, total and divQC and
// every body forms its addresses from the struct's bases and that E (the cascades' read-back included), so the
// section's entry gains E, its first slot and the FastDiv of E cd, the bases are taken from the first slot instead
// of first_row E, and the bodies are untouched.
struct WinSecEach {
    const uint32_t* src_of;
    const uint32_t* hdr_dw;
    const uint64_t* present;
    const uint32_t* meta_dw;
    const uint16_t* fsize;
    const uint64_t* parity_present;
    uint32_t groups, first_row; // rows decoded; the first of its output rows
    uint32_t shape;             // as WinSec's
    uint32_t every;             // payload rounds per header round (Rounds8)
    FastDiv divCol;             // col
    uint32_t nr;                // family 3: the row lines (then n_lines - nr column lines)
    uint32_t E, slot_first;     // out slots per row; the first of its out slots
    FastDiv divQC;              // E * cd
    uint64_t col0[2];           // family 3: column 0's member mask
};
static_assert(sizeof(WinSecEach) == 120, "the argument block's budget per section");

struct WindowEachArgs {
    WinSecEach sec[RFEC_RECOVER_MAX_SHAPES];       // the sections with groups, in order
    uint32_t first_block[RFEC_RECOVER_MAX_SHAPES]; // of each, a multiple of 8
    uint32_t n;
    const v4u* rows;
    uint32_t last, has_rows; // n_rows - 1 (0: none); n_rows != 0 (else no payload lanes)
    uint64_t* recovered;
    v4u* out_sh;
    uint32_t* out_hdr_dw;
    uint8_t* out_index;
    uint32_t C, cd, capacity;
    FastDiv divC; // cd
};
static_assert(sizeof(WindowEachArgs) <= 4096, "one argument block");

// (window_matrix_block's statements, a copy of this kernel's own: see there)
template <int K, int COL>
__device__ __forceinline__ void window_each_matrix_block(const CascArgs& A, rfec_kmask& sM, bool checker, uint32_t hb,
                                                         uint32_t pb, const v4u* rows, uint32_t last,
                                                         const uint32_t* __restrict__ src_of)
{
    using LL = MatLines<K, COL>;
    if (checker) {
        if (threadIdx.x == 0) {
            sM.plan.k = K;
            sM.plan.n_lines = LL::NL;
        }
        if (threadIdx.x < (uint32_t)LL::NL) { // (what the serial peel reads: KArgLines)
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = LL{}.rec(threadIdx.x);
            sM.mask[threadIdx.x][0] = LL{}.mask(threadIdx.x);
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        cascade_check_block<uint32_t, false>(A, sM, LL{}, BatchHdrs{A, sM.plan}, hb);
    } else {
        matrix_payload_block<K, COL>(A, BatchHdrs{A, sM.plan}, PoolRows{rows, src_of, K, last, A.C}, pb);
    }
}

__global__ __launch_bounds__(kBlock) void k_decode_window_each(WindowEachArgs S)
{
    __shared__ rfec_kmask sM;
    uint32_t p = 0;
    for (uint32_t q = 1; q < S.n; ++q) // (uniform: scalar loads and compares)
        p = blockIdx.x >= S.first_block[q] ? q : p;
    const WinSecEach& T = S.sec[p];
    const uint32_t rb = blockIdx.x - S.first_block[p];
    const uint32_t G = T.groups, K = T.shape & 0xffu, col = (T.shape >> 8) & 0xffu, NL = (T.shape >> 16) & 0xffu;
    const uint32_t lg = (T.shape >> 24) & 15u, family = T.shape >> 28, E = T.E;
    // the section's grid, as its own call lays it out (rounds_of_8): G << lg < 2^32 and total < 2^31, host-checked
    const uint32_t total = S.has_rows ? G * E * S.cd : 0u, hl = G << lg;
    const uint32_t n_hdr = (hl >> 8) + ((hl & 255u) != 0), npay8 = (((total + 255u) >> 8) + 7u) & ~7u;
    uint32_t hb = 0, pb = 0;
    const bool header = header_block_xcd_at(rb, (n_hdr + 7u) >> 3, T.every, npay8, &hb, &pb);
    if (header && hb >= n_hdr) // (the round's blocks past the section's last header lane)
        return;
    // the section's four output bases: its first row of `recovered`, its first slot of the three slot arrays
    const size_t sf = T.slot_first;
    uint64_t* const recovered = S.recovered + 2 * (size_t)T.first_row;
    v4u* const out_sh = S.out_sh + sf * S.C;
    uint32_t* const out_hdr_dw = S.out_hdr_dw + sf * 5;
    uint8_t* const out_index = S.out_index + sf;
    if (family == 1) { // a full matrix of k = 6..16
        CascArgs A = {}; // (no shards, no parity, no workspace: rfec_launch_recover_indexed_matrix's)
        A.hdr_dw = const_cast<uint32_t*>(T.hdr_dw);
        A.meta_dw = T.meta_dw, A.fsize = T.fsize, A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = recovered, A.out_sh = out_sh, A.out_hdr_dw = out_hdr_dw, A.out_index = out_index;
        A.E = A.Q = E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity;
        A.divC = S.divC, A.divQC = T.divQC;
#define RFEC_ME(KK, CC)                                                                                           \
    case KK: window_each_matrix_block<KK, CC>(A, sM, header, hb, pb, S.rows, S.last, T.src_of); break;
        switch (K) {
            RFEC_MATRIX_SHAPES(RFEC_ME)
        default: break;
        }
#undef RFEC_ME
        return;
    }
    if (family == 3) { // a full matrix of k = 17..128: k and col at run time, one checker lane per group
        WideArgs A = {};
        A.rows = S.rows, A.src_of = T.src_of, A.hdr_dw = T.hdr_dw, A.meta_dw = T.meta_dw, A.fsize = T.fsize;
        A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = recovered, A.out_sh = out_sh, A.out_hdr_dw = out_hdr_dw, A.out_index = out_index;
        A.E = E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity, A.last = S.last;
        A.K = K, A.COL = col, A.NR = T.nr, A.NL = NL;
        A.col0[0] = T.col0[0], A.col0[1] = T.col0[1];
        A.divC = S.divC, A.divQC = T.divQC, A.divCol = T.divCol;
        if (header)
            wide_check_block(A, hb);
        else
            wide_payload_block(A, pb);
        return;
    }
    if (family == 4) { // a row layout of any width: k, col and the lines at run time
        RowsWideArgs A = {};
        A.rows = S.rows, A.src_of = T.src_of, A.hdr_dw = T.hdr_dw, A.meta_dw = T.meta_dw, A.fsize = T.fsize;
        A.present = T.present, A.parity_present = T.parity_present;
        A.recovered = recovered, A.out_sh = out_sh, A.out_hdr_dw = out_hdr_dw, A.out_index = out_index;
        A.E = E, A.groups = G, A.total = total, A.C = S.C, A.capacity = S.capacity, A.last = S.last;
        A.K = K, A.COL = col, A.NL = NL, A.lg = lg, A.n_hdr = n_hdr;
        A.divC = S.divC, A.divQC = T.divQC, A.divCol = T.divCol;
        if (header)
            rows_wide_header_block(A, hb);
        else
            rows_wide_payload_block(A, pb);
        return;
    }
    // family 2, a row layout of rows of <= 4 with k <= 64: k and col at run time, the masks from (k, col)
    PeelArgs B = {};
    B.hdr = reinterpret_cast<rfec_hdr*>(const_cast<uint32_t*>(T.hdr_dw)); // dense output: hdr is only read
    B.present = T.present;
    B.meta = reinterpret_cast<const rfec_hdr*>(T.meta_dw);
    B.fsize = T.fsize, B.parity_present = T.parity_present;
    B.recovered = recovered;
    B.groups = G, B.capacity = S.capacity, B.gpb = 1, B.nlp_log2 = lg;
    B.out_hdr = reinterpret_cast<rfec_hdr*>(out_hdr_dw);
    B.out_index = out_index;
    B.out_per_group = E;
    if (header) {
        if (threadIdx.x == 0) {
            sM.plan.k = (uint16_t)K;
            sM.plan.n_lines = (uint8_t)NL;
        }
        if (threadIdx.x < NL) { // row l: members l col .. of the k
            const uint32_t first = threadIdx.x * col, cnt = min(col, K - first);
            reinterpret_cast<uint32_t*>(sM.plan.line)[threadIdx.x] = first | 1u << 8 | cnt << 16;
            sM.mask[threadIdx.x][0] = ((1ull << cnt) - 1ull) << first;
            sM.mask[threadIdx.x][1] = 0;
        }
        __syncthreads();
        [[clang::always_inline]] line_headers(B, sM, hb); // (a call would put B on the stack: scratch)
        return;
    }
    const DenseOut D = {out_sh, E};
    RFEC_ROWS_INDEXED_LANE(0, 4, S.rows, S.last, T.src_of, total, S.C, S.divC, T.divQC, B, D, K, col, T.divCol, pb)
}

// The batch layout -> packed matrix records (rfec_pack_erasures_matrix): one
// lane per (group, 16-byte chunk of the record), so every byte of a record --
// masks, slots, zeros and padding -- leaves in whole 16-byte stores (slots
// start on 4-byte boundaries only: lanes per slot could store dwords at best).
// A dword of slot e belongs to the row half or the column half of the group's
// e-th erased segment t: the line's meta record, its fec_data_size, or the
// record of one of its other members (zeros for an erased member, past the
// line's end, for a row without a line and where the group has no e-th erased
// segment).
struct PackMatArgs {
    const uint32_t* hdr;
    const uint64_t* present;
    const uint32_t* meta;
    const uint16_t* fsize;
    const uint64_t* parity_present;
    uint32_t groups, K, COL, NR, E, RHd, Sd; // RHd, Sd: dwords of a row half and of a slot
    uint32_t total;                          // groups x chunks per record
    FastDiv divChunks;
};

__device__ __forceinline__ uint32_t pack_matrix_dword(const PackMatArgs& P, uint32_t g, uint64_t h, uint32_t w)
{
    const uint32_t e = w / P.Sd;
    if (e >= P.E)
        return 0; // padding
    uint32_t m = ~(uint32_t)h & ((1u << P.K) - 1u);
    for (uint32_t u = 0; u < e; ++u)
        m &= m - 1u;
    if (!m)
        return 0;
    const uint32_t t = (uint32_t)__ffs((int)m) - 1, r = t / P.COL, c = t - r * P.COL;
    uint32_t x = w - e * P.Sd, l, first, stride, count;
    if (x < P.RHd) {
        if (r >= P.NR)
            return 0; // a last row of one member has no line
        l = r, first = r * P.COL, stride = 1, count = min(P.COL, P.K - first);
    } else {
        x -= P.RHd;
        l = P.NR + c, first = c, stride = P.COL, count = (P.K - c + P.COL - 1) / P.COL;
    }
    const size_t gl = (size_t)g * (P.NR + P.COL) + l;
    if (x < 5)
        return P.meta[gl * 5 + x];
    if (x == 5)
        return P.fsize[gl];
    const uint32_t pos = (x - 6) / 5, d = x - 6 - pos * 5, ut = (t - first) / stride;
    const uint32_t u = pos < ut ? pos : pos + 1, i = first + u * stride;
    if (u >= count || !((h >> i) & 1ull))
        return 0;
    return P.hdr[((size_t)g * P.K + i) * 5 + d];
}

__global__ __launch_bounds__(kBlock) void k_pack_matrix(v4u* __restrict__ packed, PackMatArgs P)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.total)
        return;
    const uint32_t g = fdiv(t, P.divChunks), ch = t - g * P.divChunks.d;
    const uint64_t h = P.present[2 * g];
    v4u v;
    if (ch == 0) {
        const uint64_t pp = P.parity_present[g];
        v = v4u{(uint32_t)h, (uint32_t)(h >> 32), (uint32_t)pp, (uint32_t)(pp >> 32)};
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d)
            v[d] = pack_matrix_dword(P, g, h, ch * 4 - 4 + d);
    }
    packed[t] = v; // record g, chunk ch: the records are contiguous
}

// the payload lanes: Q slots per group, cd chunks of work per slot (groups * Q * cd < 2^32: checked by the callers)
void casc_lanes(CascArgs* A, uint32_t groups, uint32_t Q, uint32_t cd)
{
    A->Q = Q;
    A->groups = groups;
    A->total = groups * Q * cd;
    A->divC = make_fastdiv(cd);
    A->divQC = make_fastdiv(Q * cd);
}

// the dense decodes' grid: rounds of 8 checker blocks spread over the payload's; these kernels take the ROUNDS
Rounds8 casc_dense_grid(const CascArgs& A)
{
    return rounds_of_8(blocks_for((uint64_t)A.groups * kCheckLanes), blocks_for(A.total));
}

} // namespace

// the dense-output half of A (out null or per_group 0: in place), with the payload stride and capacity
void casc_out_args(CascArgs* A, const rfec_dense_out* out, uint32_t stride, uint32_t capacity)
{
    const bool dense = out && out->per_group;
    A->out_sh = dense ? reinterpret_cast<v4u*>(out->shards) : nullptr;
    A->out_hdr_dw = dense ? reinterpret_cast<uint32_t*>(out->hdr) : nullptr;
    A->out_index = dense ? out->index : nullptr;
    A->E = dense ? out->per_group : 0u;
    A->C = stride / 16;
    A->capacity = capacity;
}

// cascade decode, dense: one launch (k_decode_cascade_dense, or k_decode_matrix_dense for the sender's full
// matrix plans); in place: the checker (schedule records and task words into the workspace), then the payload
// lanes, Q slots per group (one per possible step)
void launch_cascade(CascArgs A, const rfec_kmask& M, uint32_t groups, uint32_t cd, void* ws, uint32_t ws_stride,
                    hipStream_t st, bool matrix)
{
    casc_lanes(&A, groups, A.E ? A.E : (M.plan.n_lines < M.plan.k ? M.plan.n_lines : M.plan.k), cd);
    A.ws = reinterpret_cast<uint8_t*>(ws);
    A.ws_stride = ws_stride;
    if (A.E) { // dense: one launch, the checker's blocks spread over the payload's
        const Rounds8 g = casc_dense_grid(A);
        if (matrix) {
#define RFEC_MD(KK, CC)                                                                                           \
    case KK:                                                                                                      \
        RFEC_TAG(RFEC_PATH_MATRIX_DENSE, KK);                                                                     \
        RFEC_LAUNCH((k_decode_matrix_dense<KK, CC>), dim3(g.grid), dim3(kBlock), 0, st, A, M, g.hdr_rounds, g.every, \
                    g.npay8);                                                                                     \
        return;
            switch (M.plan.k) {
                RFEC_MATRIX_SHAPES(RFEC_MD)
            default: break;
            }
#undef RFEC_MD
        }
        RFEC_TAG(RFEC_PATH_CASCADE_DENSE, M.plan.k <= 32 ? 32 : 64);
        if (M.plan.k <= 32)
            RFEC_LAUNCH(k_decode_cascade_dense<uint32_t>, dim3(g.grid), dim3(kBlock), 0, st, A, M, g.hdr_rounds,
                        g.every, g.npay8);
        else
            RFEC_LAUNCH(k_decode_cascade_dense<uint64_t>, dim3(g.grid), dim3(kBlock), 0, st, A, M, g.hdr_rounds,
                        g.every, g.npay8);
        return;
    }
    const dim3 gc(blocks_for((uint64_t)groups * kCheckLanes));
    RFEC_TAG(RFEC_PATH_CASCADE, M.plan.k <= 32 ? 32 : 64);
    if (M.plan.k <= 32)
        RFEC_LAUNCH(k_cascade_check<uint32_t>, gc, dim3(kBlock), 0, st, A, M);
    else
        RFEC_LAUNCH(k_cascade_check<uint64_t>, gc, dim3(kBlock), 0, st, A, M);
    const uint32_t nb = (blocks_for(A.total) + 7u) & ~7u; // whole rounds of 8 (XCD swizzle)
    RFEC_LAUNCH(k_decode_cascade, dim3(nb), dim3(kBlock), 0, st, A, M);
}

extern "C" {

int rfec_launch_pack_matrix(const rfec_kplan* P, uint32_t groups, const rfec_hdr* hdr, const uint64_t* present,
                            const rfec_hdr* meta, const uint16_t* fsize, const uint64_t* parity_present,
                            uint32_t per_group, uint8_t* packed, uint32_t pk_stride, void* stream)
{
    const uint32_t col = (uint32_t)rfec_packed_matrix_col(P);
    if (!col || pk_stride % 16)
        return (int)hipErrorInvalidValue;
    const uint32_t R = (P->k + col - 1) / col, NR = P->n_lines - col;
    PackMatArgs A = {reinterpret_cast<const uint32_t*>(hdr), present, reinterpret_cast<const uint32_t*>(meta), fsize,
                     parity_present, groups, P->k, col, NR, per_group, 6u + 5u * (col - 1u),
                     12u + 5u * (col - 1u) + 5u * (R - 1u), groups * (pk_stride / 16), // < 2^32: host-checked
                     make_fastdiv(pk_stride / 16)};
    RFEC_TAG(RFEC_PATH_PACK_MATRIX, 0);
    RFEC_LAUNCH(k_pack_matrix, dim3(blocks_for(A.total)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<v4u*>(packed), A);
    return (int)hipGetLastError();
}

int rfec_launch_recover_packed_matrix(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                      const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                                      uint32_t pk_stride, uint64_t* recovered, const rfec_dense_out* out, void* stream)
{
    if (!rfec_packed_matrix_col(&M->plan))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    CascArgs A = {}; // (no header arrays, no workspace: the records carry the checker's input)
    A.shards = const_cast<v4u*>(reinterpret_cast<const v4u*>(shards));
    A.parity = reinterpret_cast<const v4u*>(parity);
    A.recovered = recovered;
    casc_out_args(&A, out, stride, capacity);
    casc_lanes(&A, groups, A.E, capacity ? (capacity + 15) / 16 : 1); // < 2^32 lanes: host-checked
    const Rounds8 g = casc_dense_grid(A);
#define RFEC_MP(KK, CC)                                                                                           \
    case KK:                                                                                                      \
        RFEC_TAG(RFEC_PATH_MATRIX_PACKED, KK);                                                                    \
        RFEC_LAUNCH((k_decode_matrix_packed<KK, CC>), dim3(g.grid), dim3(kBlock), 0, st, A, *M, g.hdr_rounds, g.every, \
                    g.npay8, packed, pk_stride);                                                                  \
        break;
    switch (M->plan.k) {
        RFEC_MATRIX_SHAPES(RFEC_MP)
    default: break;
    }
#undef RFEC_MP
    return (int)hipGetLastError();
}

// rfec_recover_indexed_matrix_out (rfec_recover_indexed_matrix.c): one launch of k_decode_matrix_indexed, no
// workspace.  n_rows == 0 (no slot can be present): the checker blocks alone, with zero payload lanes -- they
// still write recovered, out_hdr and out_index, and no row is dereferenced.
int rfec_launch_recover_indexed_matrix(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                       const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                       const rfec_hdr* hdr, const uint64_t* present, const rfec_hdr* meta,
                                       const uint16_t* fsize, const uint64_t* parity_present, uint64_t* recovered,
                                       const rfec_dense_out* out, void* stream)
{
    const rfec_kplan& P = M->plan;
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0;
    if (!rfec_packed_matrix_col(&P) || !groups || !stride || stride % 16 || capacity > stride || !E || E > P.k ||
        (uint64_t)groups * E * cd >= (1ull << 31) || (uint64_t)groups * kCheckLanes >= (1ull << 32))
        return (int)hipErrorInvalidValue;
    CascArgs A = {}; // (no shards, no parity, no workspace: the payload lanes read the pool through src_of)
    A.hdr_dw = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(hdr)); // dense output: hdr is only read
    A.meta_dw = reinterpret_cast<const uint32_t*>(meta);
    A.fsize = fsize, A.present = present, A.parity_present = parity_present, A.recovered = recovered;
    casc_out_args(&A, out, stride, capacity);
    casc_lanes(&A, groups, E, cd);
    if (!n_rows)
        A.total = 0;
    const Rounds8 g = casc_dense_grid(A);
#define RFEC_MI(KK, CC)                                                                                           \
    case KK:                                                                                                      \
        rfec_set_indexed_path(3u | (uint32_t)KK << 8);                                                            \
        RFEC_LAUNCH((k_decode_matrix_indexed<KK, CC>), dim3(g.grid), dim3(kBlock), 0,                             \
                    reinterpret_cast<hipStream_t>(stream), A, *M, g.hdr_rounds, g.every, g.npay8,                 \
                    reinterpret_cast<const v4u*>(rows), n_rows ? n_rows - 1 : 0u, src_of);                        \
        break;
    switch (P.k) {
        RFEC_MATRIX_SHAPES(RFEC_MI)
    default: break;
    }
#undef RFEC_MI
    return (int)hipGetLastError();
}

// A section's part of k_decode_shapes_indexed's grid: rfec_launch_recover_indexed_matrix's (the checker's lanes per
// group) or launch_rows_indexed's (header lanes per (group, line)); with n_rows == 0 the header rounds alone.
static bool shapes_section_grid(const rfec_kplan* P, uint32_t groups, uint32_t E, uint32_t cd, uint32_t n_rows,
                                uint32_t* lg, Rounds8* g)
{
    const bool matrix = rfec_packed_matrix_col(P) != 0;
    if (!matrix && !rfec_rows_indexed_col(P))
        return false;
    *lg = matrix ? rfec_ceil_log2(kCheckLanes) : rfec_header_lanes_log2(P->n_lines);
    *g = rounds_of_8(blocks_for((uint64_t)groups << *lg), blocks_for(n_rows ? (uint64_t)groups * E * cd : 0));
    return true;
}

uint32_t rfec_recover_shapes_blocks(const rfec_kplan* P, uint32_t groups, uint32_t per_group, uint32_t cd,
                                    uint32_t n_rows)
{
    uint32_t lg;
    Rounds8 g;
    return shapes_section_grid(P, groups, per_group, cd, n_rows, &lg, &g) ? g.grid : 0u;
}

// rfec_recover_indexed_shapes_out (rfec_recover_indexed_shapes.c): one launch of k_decode_shapes_indexed over the
// sections with groups, no workspace.
int rfec_launch_recover_indexed_shapes(const rfec_kplan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                                       const uint32_t* groups, uint32_t stride, uint32_t capacity, const uint8_t* rows,
                                       uint32_t n_rows, uint64_t* recovered, const rfec_dense_out* out, void* stream)
{
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0;
    if (!plans || !sections || !n_plans || n_plans > RFEC_RECOVER_MAX_SHAPES || !stride || stride % 16 ||
        capacity > stride || !E)
        return (int)hipErrorInvalidValue;
    ShapesArgs S = {};
    uint64_t blocks = 0, first_row = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_kplan* P = plans + p;
        const uint32_t G = groups ? groups[p] : sections[p].cap;
        if (!G)
            continue;
        uint32_t lg;
        Rounds8 g;
        if (!shapes_section_grid(P, G, E, cd, n_rows, &lg, &g) || E > P->k || (uint64_t)G * E * cd >= (1ull << 31) ||
            ((uint64_t)G << lg) >= (1ull << 32))
            return (int)hipErrorInvalidValue;
        const rfec_regroup_section& s = sections[p];
        const uint32_t mcol = (uint32_t)rfec_packed_matrix_col(P);
        ShapeSec& T = S.sec[S.n];
        T.src_of = s.src_of, T.hdr_dw = reinterpret_cast<const uint32_t*>(s.hdr), T.present = s.present;
        T.meta_dw = reinterpret_cast<const uint32_t*>(s.meta), T.fsize = s.fec_size;
        T.parity_present = s.parity_present;
        T.groups = G, T.first_row = (uint32_t)first_row, T.every = g.every;
        T.shape = P->k | (mcol ? mcol : (uint32_t)rfec_rows_indexed_col(P)) << 8 | lg << 12 |
                  (uint32_t)P->n_lines << 16 | (mcol ? kShapeMatrix : 0u);
        S.first_block[S.n++] = (uint32_t)blocks;
        blocks += g.grid;
        first_row += G;
        if (blocks >= (1ull << 31) || first_row >= (1ull << 32))
            return (int)hipErrorInvalidValue;
    }
    if (!S.n)
        return (int)hipSuccess;
    S.rows = reinterpret_cast<const v4u*>(rows);
    S.last = n_rows ? n_rows - 1 : 0u, S.has_rows = n_rows != 0;
    S.recovered = recovered;
    S.out_sh = reinterpret_cast<v4u*>(out->shards);
    S.out_hdr_dw = reinterpret_cast<uint32_t*>(out->hdr);
    S.out_index = out->index;
    S.E = E, S.C = stride / 16, S.cd = cd, S.capacity = capacity;
    S.divC = make_fastdiv(cd), S.divQC = make_fastdiv(E * cd);
    for (uint32_t c = 2; c <= 4; ++c)
        S.divCol[c - 2] = make_fastdiv(c);
    rfec_set_indexed_path(4u | S.n << 8);
    RFEC_LAUNCH(k_decode_shapes_indexed, dim3((uint32_t)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                S);
    return (int)hipGetLastError();
}

// The family of a section of k_decode_window_indexed, the first predicate that holds: 1 the compiled full matrix
// (k = 6..16), 2 the compiled row layout (rows of <= 4, k <= 64), 3 the planner's full matrix of k = 17..128 in rows
// of rfec_num_packets' col (rfec_recover_indexed_matrix_wide.c's wide_col and its launcher's bounds), 4 any other
// row layout (rfec_rows_wide_col and its launcher's bounds); 0: none.
int rfec_recover_window_family(const rfec_kplan* P)
{
    if (rfec_packed_matrix_col(P))
        return 1;
    if (rfec_rows_indexed_col(P))
        return 2;
    uint8_t row = 0, col = 0;
    if (P->k >= 6 && P->k <= RFEC_MAX_K && rfec_num_packets(P->k, 255, &row, &col) == 1 && col >= 2 && col <= 20 &&
        P->n_lines <= kWideSteps && rfec_full_matrix(P, col))
        return 3;
    if (P->k >= 2 && P->k <= RFEC_MAX_K && P->n_lines <= RFEC_MAX_LINES && rfec_rows_wide_col(P))
        return 4;
    return 0;
}

// A section's part of k_decode_window_indexed's grid, the one its own call takes: header (or checker) lanes per
// group 4 (family 1), 2^rfec_header_lanes_log2(n_lines) (families 2 and 4) or 1 (family 3); with n_rows == 0 the
// header rounds alone.
static int window_section_grid(const rfec_kplan* P, uint32_t groups, uint32_t E, uint32_t cd, uint32_t n_rows,
                               uint32_t* lg, Rounds8* g)
{
    const int family = rfec_recover_window_family(P);
    if (!family)
        return 0;
    *lg = family == 1 ? rfec_ceil_log2(kCheckLanes) : family == 3 ? 0u : rfec_header_lanes_log2(P->n_lines);
    *g = rounds_of_8(blocks_for((uint64_t)groups << *lg), blocks_for(n_rows ? (uint64_t)groups * E * cd : 0));
    return family;
}

uint32_t rfec_recover_window_blocks(const rfec_kplan* P, uint32_t groups, uint32_t per_group, uint32_t cd,
                                    uint32_t n_rows)
{
    uint32_t lg;
    Rounds8 g;
    return window_section_grid(P, groups, per_group, cd, n_rows, &lg, &g) ? g.grid : 0u;
}

// rfec_recover_indexed_window_out (rfec_recover_indexed_window.c): one launch of k_decode_window_indexed over the
// sections with groups, no workspace.
int rfec_launch_recover_indexed_window(const rfec_kplan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                                       const uint32_t* groups, uint32_t stride, uint32_t capacity, const uint8_t* rows,
                                       uint32_t n_rows, uint64_t* recovered, const rfec_dense_out* out, void* stream)
{
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0;
    if (!plans || !sections || !n_plans || n_plans > RFEC_RECOVER_MAX_SHAPES || !stride || stride % 16 ||
        capacity > stride || !E)
        return (int)hipErrorInvalidValue;
    WindowArgs S = {};
    uint64_t blocks = 0, first_row = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_kplan* P = plans + p;
        const uint32_t G = groups ? groups[p] : sections[p].cap;
        if (!G)
            continue;
        uint32_t lg;
        Rounds8 g;
        const int family = window_section_grid(P, G, E, cd, n_rows, &lg, &g);
        if (!family || E > P->k || (uint64_t)G * E * cd >= (1ull << 31) || ((uint64_t)G << lg) >= (1ull << 32))
            return (int)hipErrorInvalidValue;
        const rfec_regroup_section& s = sections[p];
        WinSec& T = S.sec[S.n];
        T.src_of = s.src_of, T.hdr_dw = reinterpret_cast<const uint32_t*>(s.hdr), T.present = s.present;
        T.meta_dw = reinterpret_cast<const uint32_t*>(s.meta), T.fsize = s.fec_size;
        T.parity_present = s.parity_present;
        T.groups = G, T.first_row = (uint32_t)first_row, T.every = g.every;
        uint32_t col = 0;
        if (family == 1) {
            col = (uint32_t)rfec_packed_matrix_col(P);
        } else if (family == 2) {
            col = (uint32_t)rfec_rows_indexed_col(P);
        } else if (family == 3) {
            uint8_t row = 0, c = 0;
            rfec_num_packets(P->k, 255, &row, &c);
            col = c;
            const uint32_t R = (P->k + col - 1) / col;
            T.nr = P->k - (R - 1) * col >= 2 ? R : R - 1; // a last row of one member has no line
            for (uint32_t i = 0; i < P->k; i += col)
                T.col0[i >> 6] |= 1ull << (i & 63u);
        } else {
            col = (uint32_t)rfec_rows_wide_col(P);
        }
        T.divCol = make_fastdiv(col);
        T.shape = P->k | col << 8 | (uint32_t)P->n_lines << 16 | lg << 24 | (uint32_t)family << 28;
        S.first_block[S.n++] = (uint32_t)blocks;
        blocks += g.grid;
        first_row += G;
        if (blocks >= (1ull << 31) || first_row >= (1ull << 32))
            return (int)hipErrorInvalidValue;
    }
    if (!S.n)
        return (int)hipSuccess;
    S.rows = reinterpret_cast<const v4u*>(rows);
    S.last = n_rows ? n_rows - 1 : 0u, S.has_rows = n_rows != 0;
    S.recovered = recovered;
    S.out_sh = reinterpret_cast<v4u*>(out->shards);
    S.out_hdr_dw = reinterpret_cast<uint32_t*>(out->hdr);
    S.out_index = out->index;
    S.E = E, S.C = stride / 16, S.cd = cd, S.capacity = capacity;
    S.divC = make_fastdiv(cd), S.divQC = make_fastdiv(E * cd);
    rfec_set_indexed_path(8u | S.n << 8);
    RFEC_LAUNCH(k_decode_window_indexed, dim3((uint32_t)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                S);
    return (int)hipGetLastError();
}

// rfec_recover_indexed_window_each_out (rfec_recover_indexed_window_each.c): one launch of k_decode_window_each over
// the sections with groups, section p with per_group[p] out slots a row, the slots packed end to end; no workspace.
int rfec_launch_recover_indexed_window_each(const rfec_kplan* plans, uint32_t n_plans,
                                            const rfec_regroup_section* sections, const uint32_t* groups,
                                            uint32_t stride, uint32_t capacity, const uint8_t* rows, uint32_t n_rows,
                                            uint64_t* recovered, const uint32_t* per_group, uint8_t* out_shards,
                                            rfec_hdr* out_hdr, uint8_t* out_index, void* stream)
{
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    if (!plans || !sections || !n_plans || n_plans > RFEC_RECOVER_MAX_SHAPES || !stride || stride % 16 ||
        capacity > stride || !per_group)
        return (int)hipErrorInvalidValue;
    WindowEachArgs S = {};
    uint64_t blocks = 0, first_row = 0, slot_first = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_kplan* P = plans + p;
        const uint32_t G = groups ? groups[p] : sections[p].cap;
        if (!G)
            continue;
        const uint32_t E = per_group[p];
        uint32_t lg;
        Rounds8 g;
        const int family = E ? window_section_grid(P, G, E, cd, n_rows, &lg, &g) : 0;
        if (!family || E > P->k || (uint64_t)G * E * cd >= (1ull << 31) || ((uint64_t)G << lg) >= (1ull << 32))
            return (int)hipErrorInvalidValue;
        const rfec_regroup_section& s = sections[p];
        WinSecEach& T = S.sec[S.n];
        T.src_of = s.src_of, T.hdr_dw = reinterpret_cast<const uint32_t*>(s.hdr), T.present = s.present;
        T.meta_dw = reinterpret_cast<const uint32_t*>(s.meta), T.fsize = s.fec_size;
        T.parity_present = s.parity_present;
        T.groups = G, T.first_row = (uint32_t)first_row, T.every = g.every;
        T.E = E, T.slot_first = (uint32_t)slot_first, T.divQC = make_fastdiv(E * cd);
        uint32_t col = 0;
        if (family == 1) {
            col = (uint32_t)rfec_packed_matrix_col(P);
        } else if (family == 2) {
            col = (uint32_t)rfec_rows_indexed_col(P);
        } else if (family == 3) {
            uint8_t row = 0, c = 0;
            rfec_num_packets(P->k, 255, &row, &c);
            col = c;
            const uint32_t R = (P->k + col - 1) / col;
            T.nr = P->k - (R - 1) * col >= 2 ? R : R - 1; // a last row of one member has no line
            for (uint32_t i = 0; i < P->k; i += col)
                T.col0[i >> 6] |= 1ull << (i & 63u);
        } else {
            col = (uint32_t)rfec_rows_wide_col(P);
        }
        T.divCol = make_fastdiv(col);
        T.shape = P->k | col << 8 | (uint32_t)P->n_lines << 16 | lg << 24 | (uint32_t)family << 28;
        S.first_block[S.n++] = (uint32_t)blocks;
        blocks += g.grid;
        first_row += G;
        slot_first += (uint64_t)G * E;
        if (blocks >= (1ull << 31) || first_row >= (1ull << 32) || slot_first * cd >= (1ull << 31))
            return (int)hipErrorInvalidValue;
    }
    if (!S.n)
        return (int)hipSuccess;
    S.rows = reinterpret_cast<const v4u*>(rows);
    S.last = n_rows ? n_rows - 1 : 0u, S.has_rows = n_rows != 0;
    S.recovered = recovered;
    S.out_sh = reinterpret_cast<v4u*>(out_shards);
    S.out_hdr_dw = reinterpret_cast<uint32_t*>(out_hdr);
    S.out_index = out_index;
    S.C = stride / 16, S.cd = cd, S.capacity = capacity;
    S.divC = make_fastdiv(cd);
    rfec_set_indexed_path(9u | S.n << 8);
    RFEC_LAUNCH(k_decode_window_each, dim3((uint32_t)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                S);
    return (int)hipGetLastError();
}

} // extern "C"
