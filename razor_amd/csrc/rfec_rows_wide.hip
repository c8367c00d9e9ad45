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
// contiguous run of count x 20 bytes, the target's among them) are loaded in rounds of kRowsRound in flight, the target
// skipped in the numbering.
//
// Payload lane: its target is the group's q-th erased segment over both mask words, the target's row tgt / col; the
// lane exits unless that row has a line, misses exactly that member and has its parity.  Loads as wide_line<false>
// (rfec_matrix_wide_blocks.h): the parity chunk, then rounds of kRowsRound members -- the round's map words first, then the
// chunks unconditionally and in flight together; a position past the line's end re-reads the parity chunk and is
// XORed as zero.
#include "rfec_rows_wide_blocks.h" // (the bodies: k_decode_window_indexed runs them too)

namespace {

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
