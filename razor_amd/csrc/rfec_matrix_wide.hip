// rfec_matrix_wide.hip -- the one-launch decode of the sender's full row + column plans of any k = 6..128 through
// a slot map over a row pool (rfec_recover_indexed_matrix_wide_out, rfec_recover_indexed_matrix_wide.c), gfx950.
//
// The plan's shape (k, col) is a run-time argument: one kernel serves every k, its masks two 64-bit words.  Line l
// of the plan is row l for l < NR (members l col .., a last row of one member has no line) and column l - NR after
// that, so a line's record and member mask are arithmetic in (k, col, l) -- nothing is read from a plan in memory.
//
// The grid is k_decode_matrix_indexed's (rfec_cascade.hip): rounds of 8 checker blocks spread between the payload
// blocks' rounds (header_block_xcd), payload lanes (group, out slot q, chunk j) in XCD-swizzled blocks; the
// payload lanes need nothing from the checker lanes, and no workgroup waits on another.
//
// Checker: ONE lane per group runs the group's exact peel serially -- lines in plan order to a fixpoint over the
// 128-bit masks; a line that fires is checked there and then (fec_data_size within the capacity, every member's
// size and the recovered size within fec_data_size: flex_fec_xor.c:88-89, 98-99), its loads in rounds of four
// member records in flight together; a line that fails is banned (it would fail every time it fires: same
// target, same members, same headers), which is cascade_check's "left out and the schedule recomputed" without
// the recomputation: the steps before it are the same with or without it.  So the checker keeps no schedule at
// all (a schedule of these plans has up to 23 steps), and a cascade of any depth costs it nothing extra: the
// record of a member recovered earlier is read back from the out slot this lane wrote.  Lanes per step with
// shuffles (cascade_check_lanes) would need 32 lanes per group for 23 steps and a serial fallback besides.
//
// Payload lane: its target, the group's q-th erased segment, lies in one row and one column; the row's line is
// taken if it fires at once (plan order: rows first), else the column's.  When neither does (a cascade) the lane
// recomputes the group's mask schedule -- (line, target) per step packed into three 128-bit words, no array --
// forms the dependency closure of its target's step and replays it in step order, intermediate results through
// the group's own out slots as cascade_replay does.
#include "rfec_matrix_wide_blocks.h" // (the bodies: k_decode_window_indexed runs them too)

namespace {

__global__ __launch_bounds__(kBlock) void k_decode_matrix_wide(WideArgs A)
{
    uint32_t hb = 0, pb = 0;
    if (header_block_xcd(A.n_hr, A.every, A.npay8, &hb, &pb)) // the checker blocks: the tables only, never a row
        wide_check_block(A, hb);
    else
        wide_payload_block(A, pb);
}

} // namespace

extern "C" {

// rfec_recover_indexed_matrix_wide_out (rfec_recover_indexed_matrix_wide.c): one launch of k_decode_matrix_wide, no
// workspace.  n_rows == 0 (no slot can be present): the checker blocks alone, with zero payload lanes -- they
// still write recovered, out_hdr and out_index, and no row is dereferenced.
int rfec_launch_recover_indexed_matrix_wide(const rfec_kplan* P, uint32_t col, uint32_t groups, uint32_t stride,
                                            uint32_t capacity, const uint8_t* rows, uint32_t n_rows,
                                            const uint32_t* src_of, const rfec_hdr* hdr, const uint64_t* present,
                                            const rfec_hdr* meta, const uint16_t* fsize,
                                            const uint64_t* parity_present, uint64_t* recovered,
                                            const rfec_dense_out* out, void* stream)
{
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1, E = out ? out->per_group : 0, K = P->k;
    if (K < 6 || K > RFEC_MAX_K || col < 2 || col > 20 || !rfec_full_matrix(P, col) || P->n_lines > kWideSteps ||
        !groups || !stride || stride % 16 || capacity > stride || !E || E > K ||
        (uint64_t)groups * E * cd >= (1ull << 31))
        return (int)hipErrorInvalidValue;
    WideArgs A = {};
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
    const uint32_t R = (K + col - 1) / col;
    A.NR = K - (R - 1) * col >= 2 ? R : R - 1; // a last row of one member has no line
    for (uint32_t i = 0; i < K; i += col)
        A.col0[i >> 6] |= 1ull << (i & 63u);
    A.divC = make_fastdiv(cd), A.divQC = make_fastdiv(E * cd), A.divCol = make_fastdiv(col);
    // one checker lane per group (groups < 2^31 by the bound above)
    const Rounds8 g = rounds_of_8(blocks_for(groups), blocks_for(A.total));
    A.n_hr = g.hdr_rounds, A.every = g.every, A.npay8 = g.npay8;
    rfec_set_indexed_path(6u | K << 8);
    RFEC_LAUNCH(k_decode_matrix_wide, dim3(g.grid), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), A);
    return (int)hipGetLastError();
}

} // extern "C"
