// rfec_families.h -- what the kernel families of the flex-FEC engine share (C++ only).  Not installed.
//
// rfec_kernels.hip holds the dispatch (which family a plan takes) and reaches each family's launchers -- a
// family's kernels live with their launches in one unit -- through the plain host functions declared at the end.
// Here: the argument structs that cross from the dispatch to a launcher (PeelArgs, DenseOut and CascArgs go on
// to the kernels by value: their layout is part of the kernels), and the small forced-inline device helpers
// that more than one family uses.
#ifndef RFEC_FAMILIES_H_
#define RFEC_FAMILIES_H_

#include "rfec_device.h"

constexpr int kMetaDwords = 4096; // 16 KiB of LDS for the meta blocks' header stage

struct EncMeta {
    const uint32_t* hdr_dw;
    uint32_t* meta_dw;
    uint16_t* fsize;
    int8_t* status;
    uint32_t groups, capacity, gpb, n_meta_blocks;
};

struct EncLaunch {
    const rfec_kplan* P;
    uint32_t groups, stride, cd; // cd = 16-B chunks of work per slot, ceil(capacity / 16)
    const v4u* s;
    v4u* p;
    EncMeta E;
    hipStream_t stream;
};

// the compile-time line layout of the reference sender's full matrix plan (flex_fec_sender.c:166-233)
template <int K, int COL>
struct MatrixShape {
    static constexpr int R = (K + COL - 1) / COL;
    static constexpr int row_count(int r) { return (r * COL + COL <= K) ? COL : K - r * COL; }
    static constexpr int col_count(int c) { return (K - c + COL - 1) / COL; }
    static constexpr int n_rows()
    {
        int n = 0;
        for (int r = 0; r < R; ++r)
            n += row_count(r) >= 2;
        return n;
    }
    static constexpr int n_lines()
    {
        int n = n_rows();
        for (int c = 0; c < COL; ++c)
            n += col_count(c) >= 2;
        return n;
    }
};

struct PeelArgs {
    rfec_hdr* hdr;
    const uint64_t* present;
    const rfec_hdr* meta;
    const uint16_t* fsize;
    const uint64_t* parity_present;
    uint64_t* recovered;
    uint8_t* sched;
    uint32_t groups, capacity, gpb, rec_bytes, disjoint;
    uint32_t nlp_log2; // fused disjoint decodes: header lanes per group (line_headers)
    // dense output (rfec_recover_batch_out): recovered segment e of group g
    // (the e-th erased one in index order, e < out_per_group) goes to
    // out_hdr[g * out_per_group + e]; out_per_group == 0: in place
    rfec_hdr* out_hdr;
    uint8_t* out_index;
    uint32_t out_per_group;
    // packed erasure records (rfec_recover_packed_out): group g's record at
    // packed + g * pk_stride, slot e's at + 16 + e * pk_slot; null: the batch layout
    const uint8_t* packed;
    uint32_t pk_stride, pk_slot;
};

// Payload side of the dense output: out slot (g * E + e) of `sh` (E == 0: in place).
struct DenseOut {
    v4u* sh;
    uint32_t E;
};

// rank of erased segment t among the group's erased segments (index order)
__device__ __forceinline__ uint32_t missing_rank(uint64_t h0, uint64_t h1, uint32_t t)
{
    return t < 64 ? (uint32_t)__popcll(~h0 & ((1ull << t) - 1ull))
                  : (uint32_t)__popcll(~h0) + (uint32_t)__popcll(~h1 & ((1ull << (t - 64)) - 1ull));
}

__device__ __forceinline__ bool has_bit(uint64_t h0, uint64_t h1, uint32_t i)
{
    return ((i < 64 ? h0 >> i : h1 >> (i - 64)) & 1ull) != 0;
}

__device__ __forceinline__ void stage_plan(uint32_t* lplan, const rfec_kplan& P)
{
    if (threadIdx.x < P.n_lines)
        lplan[threadIdx.x] = reinterpret_cast<const uint32_t*>(P.line)[threadIdx.x];
    __syncthreads();
}

// row so[slot] of a row pool (chunk 0), the index clamped to `last` = n_rows - 1 (a broken map stays in the pool)
__device__ __forceinline__ const v4u* pool_row(const v4u* rows, const uint32_t* __restrict__ so, uint32_t slot,
                                               uint32_t last, uint32_t C)
{
    return rows + (size_t)min(so[slot], last) * C;
}

struct CascArgs {
    v4u* shards;              // in place: the erased slots are written; dense: read only
    const v4u* parity;
    uint32_t* hdr_dw;         // [G][K][5]
    const uint32_t* meta_dw;  // [G][NL][5]
    const uint16_t* fsize;    // [G][NL]
    const uint64_t* present;  // [G][2]
    const uint64_t* parity_present;
    uint64_t* recovered;      // [G][2]
    v4u* out_sh;              // dense: [G][E][C]
    uint32_t* out_hdr_dw;     // dense: [G][E][5]
    uint8_t* out_index;       // dense: [G][E]
    uint32_t E;               // dense slots per group; 0 = in place
    uint32_t groups, total, C, capacity;
    FastDiv divC, divQC;      // cd, Q * cd (Q = slots per group)
    uint8_t* ws;              // per group (ws_stride bytes): the schedule record, then Q task words
    uint32_t ws_stride, Q;
};

struct FusedArgs {
    v4u* shards;
    const v4u* parity;
    uint32_t total, C;
    FastDiv f;
    uint32_t n_hdr;
    hipStream_t stream;
    DenseOut D; // recovered payloads in place (E == 0) or to the dense output
};

// K = 6..16 of the sender's full matrix plans with the COL flex_fec_sender_num_packets picks (3 for K <= 9)
#define RFEC_MATRIX_SHAPES(X) X(6, 3) X(7, 3) X(8, 3) X(9, 3) X(10, 4) X(11, 4) X(12, 4) X(13, 4) X(14, 4) X(15, 4) X(16, 4)

#pragma GCC visibility push(hidden)

void rfec_set_path(uint32_t path);
#define RFEC_TAG(kind, arg) rfec_set_path(RFEC_PATH(kind, arg)) // the dispatch tag, kept in rfec_kernels.hip
void rfec_set_indexed_path(uint32_t path); // rfec_indexed_last_path's tag (rfec_internal.h), kept there too

// rfec_encode.hip: a row layout of rows of col <= 16 (rsrc_ok: a wave's groups fit one buffer descriptor), the
// full matrix plan of k = 6..16, any plan
hipError_t launch_encode_rows(const EncLaunch& a, uint32_t col, bool rsrc_ok);
hipError_t launch_encode_matrix(const EncLaunch& a);
hipError_t launch_encode_plan(const EncLaunch& a);

// rfec_peel.hip.  peel_args fills B for the batch layout (in place when out is null or per_group 0) from the
// call's pointers and the plan: lines pairwise disjoint, the most members of a line, k_peel_lds' groups per block
struct PeelGeom {
    uint32_t disjoint, maxc, gpb;
};
PeelGeom peel_args(PeelArgs* B, const rfec_kmask& M, uint32_t groups, uint32_t capacity, rfec_hdr* hdr,
                   const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                   const uint64_t* parity_present, uint64_t* recovered, void* ws, const rfec_dense_out* out);
void launch_peel(const PeelArgs& B, const rfec_kmask& M, hipStream_t st);
void launch_replay_flat(const PeelArgs& B, const rfec_kplan& P, v4u* shards, const v4u* parity, uint32_t C,
                        uint32_t cd, uint32_t maxc, const DenseOut& D, hipStream_t st);
void launch_replay_indexed(const PeelArgs& B, const rfec_kplan& P, const v4u* pool, uint32_t last,
                           const uint32_t* src_of, uint32_t C, uint32_t cd, uint32_t maxc, const DenseOut& D,
                           hipStream_t st);

// rfec_fused.hip (cd: chunks of work per slot; slots: lanes per dense output slot; the indexed form takes C,
// n_hdr, the stream and D from F)
void launch_fused_flat(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t maxc);
void launch_fused_out(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t cd, bool slots,
                      uint32_t maxc);
void launch_fused_rows(const FusedArgs& F, const PeelArgs& B, const rfec_kmask& M, uint32_t cd, bool slots,
                       uint32_t col);
void launch_rows_indexed(const v4u* pool, uint32_t last, const uint32_t* src_of, const FusedArgs& F,
                         const PeelArgs& B, const rfec_kmask& M, uint32_t cd, uint32_t col);

// rfec_cascade.hip (casc_out_args: the dense-output fields of A, E and the out pointers, from the call's `out` --
// null or per_group 0: in place -- with C = stride / 16 and the capacity; matrix: the plan is a full matrix of
// k = 6..16, a dense output takes k_decode_matrix_dense)
void casc_out_args(CascArgs* A, const rfec_dense_out* out, uint32_t stride, uint32_t capacity);
void launch_cascade(CascArgs A, const rfec_kmask& M, uint32_t groups, uint32_t cd, void* ws, uint32_t ws_stride,
                    hipStream_t st, bool matrix);

#pragma GCC visibility pop

#endif
