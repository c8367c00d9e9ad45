/* rfec_internal.h -- contract between the C host layer (rfec_host.c) and the
 * HIP launch shims (rfec_kernels.hip: the batched encode / recover dispatch; the other .hip units: their own).
 * Not installed. */
#ifndef RFEC_INTERNAL_H_
#define RFEC_INTERNAL_H_

#include "razor_fec.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef rfec_plan rfec_kplan;

/* plan + per-line member bitmasks (bit i of mask[l] = segment i on line l) */
typedef struct {
    rfec_kplan plan;
    uint64_t mask[RFEC_MAX_LINES][2];
} rfec_kmask;

/* the least lg with 2^lg >= x (0 for x <= 1): lanes per group of the header and pack kernels */
static inline uint32_t rfec_ceil_log2(uint32_t x)
{
    uint32_t lg = 0;
    while ((1ull << lg) < x)
        ++lg;
    return lg;
}
/* the fused decodes' header lanes per group: a power of two >= n_lines, at least 2 */
static inline uint32_t rfec_header_lanes_log2(uint32_t n_lines) { return n_lines > 2 ? rfec_ceil_log2(n_lines) : 1u; }

/* kernel flags == the RFEC_TUNE_* bits of razor_fec.h */
#define RFEC_KFLAG_GENERIC RFEC_TUNE_GENERIC
#define RFEC_KFLAG_MATRIX_GENERIC RFEC_TUNE_PLAN_CASCADE

int rfec_launch_encode(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                       const uint8_t* shards, const rfec_hdr* hdr, uint8_t* parity, rfec_hdr* meta,
                       uint16_t* fsize, int8_t* status, void* stream, unsigned flags);
int rfec_launch_recover(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                        uint8_t* shards, rfec_hdr* hdr, const uint64_t* present, const uint8_t* parity,
                        const rfec_hdr* meta, const uint16_t* fsize, const uint64_t* parity_present,
                        uint64_t* recovered, void* ws, void* stream, unsigned flags);

/* dense output of rfec_recover_batch_out (device pointers; per_group > 0) */
typedef struct {
    uint8_t* shards;  /* [G][per_group][stride] */
    rfec_hdr* hdr;    /* [G][per_group] */
    uint8_t* index;   /* [G][per_group] */
    uint32_t per_group;
} rfec_dense_out;
int rfec_launch_recover_out(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                            const uint8_t* shards, const rfec_hdr* hdr, const uint64_t* present,
                            const uint8_t* parity, const rfec_hdr* meta, const uint16_t* fsize,
                            const uint64_t* parity_present, uint64_t* recovered, void* ws, void* stream,
                            unsigned flags, const rfec_dense_out* out);

/* The dispatch tag: which kernel the calling thread's last batched launch (the shims above and the packed ones
 * below) took, RFEC_PATH(kind, arg).  Host-side and thread-local: one store per launch, no device code.  For
 * tests, which assert the path a case means to exercise; not part of razor_fec.h.  arg:
 *   ENC_ROWS          K of k_encode_out<K, 4> (10, 32)
 *   ENC_ROWS_RT       CMAX of k_encode_out_rt<CMAX> (4, 16)
 *   ENC_MATRIX        k of k_encode_matrix_out<k, c> (6..16)
 *   ENC_PLAN          0 (k_encode)
 *   DEC_ROWS          K of k_decode_rows<K, 4, ...> (0, 10, 32) | RFEC_PATH_SLOTS | RFEC_PATH_PACKED
 *   DEC_OUT           MAXC of k_decode_out<MAXC, slots> (4, 8) | RFEC_PATH_SLOTS
 *   DEC_FLAT          MAXC of k_decode_disjoint<MAXC> (4, 8)
 *   CASCADE           mask bits of k_cascade_check<u32 / u64> + k_decode_cascade (32, 64)
 *   CASCADE_DENSE     mask bits of k_decode_cascade_dense<u32 / u64> (32, 64)
 *   MATRIX_DENSE      k of k_decode_matrix_dense<k, c> (6..16)
 *   PEEL_FLAT         MAXC of k_peel_lds + k_recover_flat<4, 2> / <8, 1> (4, 8) | RFEC_PATH_FAST | RFEC_PATH_DENSE
 *   PACK_ROWS / PACK_MATRIX   0 (k_pack_rows / k_pack_matrix)
 *   MATRIX_PACKED     k of k_decode_matrix_packed<k, c> (6..16) */
enum {
    RFEC_PATH_NONE = 0,
    RFEC_PATH_ENC_ROWS,
    RFEC_PATH_ENC_ROWS_RT,
    RFEC_PATH_ENC_MATRIX,
    RFEC_PATH_ENC_PLAN,
    RFEC_PATH_DEC_ROWS,
    RFEC_PATH_DEC_OUT,
    RFEC_PATH_DEC_FLAT,
    RFEC_PATH_CASCADE,
    RFEC_PATH_CASCADE_DENSE,
    RFEC_PATH_MATRIX_DENSE,
    RFEC_PATH_PEEL_FLAT,
    RFEC_PATH_PACK_ROWS,
    RFEC_PATH_PACK_MATRIX,
    RFEC_PATH_MATRIX_PACKED
};
#define RFEC_PATH_SLOTS 0x40u  /* lanes per dense output slot */
#define RFEC_PATH_PACKED 0x80u /* header input from the packed erasure records */
#define RFEC_PATH_FAST 0x40u   /* the replay's single-level fast form (lines of <= 8 members) */
#define RFEC_PATH_DENSE 0x80u  /* dense output */
#define RFEC_PATH(kind, arg) ((uint32_t)(kind) | (uint32_t)(arg) << 8)
uint32_t rfec_last_path(void);

/* recover workspace, per group: the generic peel's schedule record (step
 * count, single-level flag, then a (line, target) byte pair per step), or the
 * cascade decode's 16-byte schedule record followed by one 4-byte task word
 * per output slot (max(k, n_lines) of them); 16-byte multiple */
static inline uint32_t rfec_sched_record_bytes(uint32_t k, uint32_t n_lines)
{
    const uint32_t peel = 2u + 2u * n_lines, casc = 16u + 4u * (k > n_lines ? k : n_lines);
    return ((peel > casc ? peel : casc) + 15u) & ~15u;
}
static inline size_t rfec_ws_bytes(uint32_t k, uint32_t n_lines, uint32_t groups)
{
    return (size_t)groups * rfec_sched_record_bytes(k, n_lines);
}
/* packed erasure records (rfec_pack_erasures / rfec_recover_packed_out): row layouts, rows of `col` <= 4,
 * k <= 64; group records of pk_stride bytes, slot records of pk_slot = 24 + 20 (col - 1) bytes */
int rfec_launch_pack_rows(const rfec_kplan* P, uint32_t col, uint32_t groups, const rfec_hdr* hdr,
                          const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                          const uint64_t* parity_present, uint32_t per_group, uint8_t* packed, uint32_t pk_stride,
                          uint32_t pk_slot, void* stream);
int rfec_launch_recover_packed(const rfec_kmask* M, uint32_t col, uint32_t groups, uint32_t stride,
                               uint32_t capacity, const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                               uint32_t pk_stride, uint32_t pk_slot, uint64_t* recovered,
                               const rfec_dense_out* out, void* stream);
/* packed matrix records (rfec_pack_erasures_matrix / rfec_recover_packed_matrix_out, rfec_packed_matrix.c): the
 * sender's full row + column plans of k = 6..16, the shapes k_decode_matrix_dense is compiled for.
 * rfec_packed_matrix_col: the plan's row width (3 for k <= 9, else 4), 0 for any other plan. */
int rfec_packed_matrix_col(const rfec_kplan* P);
int rfec_launch_pack_matrix(const rfec_kplan* P, uint32_t groups, const rfec_hdr* hdr, const uint64_t* present,
                            const rfec_hdr* meta, const uint16_t* fsize, const uint64_t* parity_present,
                            uint32_t per_group, uint8_t* packed, uint32_t pk_stride, void* stream);
int rfec_launch_recover_packed_matrix(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                      const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                                      uint32_t pk_stride, uint64_t* recovered, const rfec_dense_out* out,
                                      void* stream);
int rfec_launch_wire_frame_fec(uint32_t count, uint32_t stride, uint32_t capacity, const uint8_t* parity,
                               const rfec_hdr* meta, const uint16_t* fec_size, const int8_t* status,
                               const rfec_fec_stamp* stamps, const uint32_t* order, uint32_t dstride,
                               uint8_t* dgram, uint16_t* dlen, void* stream);
int rfec_launch_wire_frame_seg(uint32_t count, uint32_t stride, uint32_t capacity, const uint8_t* shards,
                               const rfec_hdr* hdr, const rfec_seg_stamp* stamps, const uint32_t* order,
                               uint32_t dstride, uint8_t* dgram, uint16_t* dlen, uint32_t rows_out, void* stream);
/* rfec_wire_encode_fec (rfec_wire_fused.c): one launch of the fused encode + SIM_FEC framing over `groups` groups,
 * datagram g * n_lines + l -> slot order[...] (or its own index) of `dgram`, which holds rows_out slots.  The
 * caller keeps (groups * k + 4) * stride + 1280, groups * k * 20 and rows_out * dstride below 0xFFFFFFF0
 * (32-bit buffer offsets) and dstride <= 1280; hipErrorInvalidValue otherwise. */
int rfec_launch_wire_encode_fec(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                                const uint8_t* shards, const rfec_hdr* hdr, const rfec_fec_stamp* stamps,
                                const uint32_t* order, uint32_t dstride, uint8_t* dgram, uint16_t* dlen,
                                uint32_t rows_out, void* stream);
/* rfec_wire_encode_send (rfec_wire_fused.c): one launch of the fused SIM_SEG framing + encode + SIM_FEC framing
 * over `groups` groups; segment g * k + i -> slot seg_order[...] (or its own index) of seg_dgram, which holds
 * seg_rows_out slots, datagram g * n_lines + l likewise into fec_dgram's fec_rows_out slots.  The caller keeps
 * (groups * k + 4) * stride + 1280, groups * k * 20 and both rows_out * dstride below 0xFFFFFFF0 and
 * dstride <= 1280, stride a multiple of 16; hipErrorInvalidValue otherwise.  With n_lines == 0 the FEC pointers
 * are not touched. */
int rfec_launch_wire_encode_send(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                                 const uint8_t* shards, const rfec_hdr* hdr, const rfec_seg_stamp* seg_stamps,
                                 const uint32_t* seg_order, uint8_t* seg_dgram, uint16_t* seg_dlen,
                                 uint32_t seg_rows_out, const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order,
                                 uint8_t* fec_dgram, uint16_t* fec_dlen, uint32_t fec_rows_out, uint32_t dstride,
                                 void* stream);
/* rfec_wire_encode_send_shapes's plans as its kernel takes them, in the argument block: the lines of every plan,
 * shape after shape, one dword each (first | stride << 8 | count << 16: an rfec_line), and per shape
 * k | n_lines << 8 | the index of its first line << 16. */
typedef struct {
    uint32_t n_plans;
    uint32_t shape[RFEC_SEND_MAX_SHAPES];
    uint32_t line[RFEC_SEND_MAX_LINES];
} rfec_send_shapes;
/* rfec_wire_encode_send_shapes (rfec_wire_fused.c): its one launch.  The caller has checked the plans
 * (check_plan, their lines' sum) and keeps (n_rows + 4) * stride + 1280, n_rows * 20, n_rows * dstride,
 * n_fec * dstride, n_fec * 24 and groups * 16 below 0xFFFFFFF0, dstride <= 1280 and stride a multiple of 16;
 * hipErrorInvalidValue otherwise.  With n_fec == 0 the FEC pointers are not touched. */
int rfec_launch_wire_encode_send_shapes(const rfec_send_shapes* S, uint32_t groups, const rfec_send_group* group,
                                        uint32_t n_rows, uint32_t n_fec, uint32_t stride, uint32_t capacity,
                                        const uint8_t* shards, const rfec_hdr* hdr, const rfec_seg_stamp* seg_stamps,
                                        const uint32_t* seg_order, uint8_t* seg_dgram, uint16_t* seg_dlen,
                                        const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order,
                                        uint8_t* fec_dgram, uint16_t* fec_dlen, uint32_t dstride, void* stream);
/* rfec_wire_regroup (rfec_wire_regroup.c, kernels in rfec_regroup.hip): the call's four launches on `stream`.  The
 * caller has checked the arguments (groups in [1, 65535], k <= RFEC_MAX_K, n < 2^31, stride a multiple of 16 up to
 * 2,048, capacity <= stride, the pointers); hipErrorInvalidValue otherwise. */
int rfec_launch_wire_regroup(const rfec_kplan* P, uint32_t groups, uint32_t fec_id0, uint32_t n,
                             const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride, uint32_t capacity,
                             uint8_t* shards, rfec_hdr* hdr, uint64_t* present, uint8_t* parity, rfec_hdr* meta,
                             uint16_t* fec_size, uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                             int32_t* slot_of, void* stream);
/* rfec_wire_regroup_index (rfec_wire_regroup.c): the same four launches, k_regroup_place with no row lane; the
 * caller has checked the same arguments but for the stride. */
int rfec_launch_wire_regroup_index(const rfec_kplan* P, uint32_t groups, uint32_t fec_id0, uint32_t n,
                                   const rfec_wire_rec* recs, uint32_t capacity, rfec_hdr* hdr, uint64_t* present,
                                   rfec_hdr* meta, uint16_t* fec_size, uint64_t* parity_present, uint32_t* base_id,
                                   uint32_t* src_of, int32_t* slot_of, void* stream);
/* rfec_wire_regroup_shapes (rfec_wire_regroup.c, kernels in rfec_regroup_shapes.hip): the call's six launches on
 * `stream` (four with n == 0).  The caller has checked the arguments (n_plans in [1, RFEC_REGROUP_MAX_SHAPES], every
 * plan with k <= RFEC_MAX_K and its own (k, row, col), groups in [1, 65535], n < 2^31, cap <= groups, the pointers of
 * the sections with cap > 0); hipErrorInvalidValue otherwise. */
int rfec_launch_wire_regroup_shapes(const rfec_kplan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                                    uint32_t groups, uint32_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                                    uint32_t capacity, uint8_t* shape_of, uint32_t* rank_of, uint32_t* anchor_of,
                                    uint32_t* counts, int32_t* slot_of, void* stream);
/* rfec_wire_window_census (rfec_wire_census.c, kernels in rfec_census.hip): the call's four launches on `stream`
 * (three with n == 0: no record pass).  The matrix (row, col) of every count, from rfec_num_packets(count, 255), is
 * made once per process and travels in the argument block.  The caller has checked groups in [1, 65535], n < 2^31,
 * fec_id0 != 0, capacity <= 65535 and the pointers; hipErrorInvalidValue otherwise. */
int rfec_launch_wire_census(uint32_t groups, uint32_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                            uint32_t capacity, rfec_window_census* census, uint32_t* anchor_of, uint32_t* key_of,
                            void* stream);
/* For tests: the line of rfec_plan_from_key's plan that each SIM_FEC index 0..255 names under the key (count, row,
 * col), or 0xFF -- rfec_census_rules.h's rule as the census kernels apply it; an unplannable key has no lines. */
void rfec_census_lines_of_key(uint16_t count, uint8_t row, uint8_t col, uint8_t line_of[256]);
/* For tests: the groups of one tile of k_census_shapes (one workgroup, a group per lane), and which launches the
 * calling thread's last rfec_launch_wire_census made: launches (4, or 3 with n == 0) | tiles << 8, tiles =
 * ceil(groups / tile); 0 before the first (host-side, thread-local, apart from the other tags). */
uint32_t rfec_census_tile(void);
uint32_t rfec_census_last_path(void);
/* rfec_recover_indexed_out (rfec_recover_indexed.c, kernels in rfec_fused.hip / rfec_peel.hip): the dense decode with member and
 * parity rows read from rows [n_rows][stride] through src_of [G (k + n_lines)].  The caller has checked the plan
 * (k <= RFEC_MAX_K), stride a multiple of 16, capacity <= stride, out->per_group in [1, k],
 * groups * per_group * CD < 2^31, groups << ceil(log2 n_lines) < 2^32 and the pointers; hipErrorInvalidValue
 * otherwise.  flags: RFEC_KFLAG_GENERIC sends a row layout down the peel + replay too. */
int rfec_launch_recover_indexed(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of, const rfec_hdr* hdr,
                                const uint64_t* present, const rfec_hdr* meta, const uint16_t* fsize,
                                const uint64_t* parity_present, uint64_t* recovered, void* ws, void* stream,
                                unsigned flags, const rfec_dense_out* out);
/* rfec_recover_indexed_matrix_out (rfec_recover_indexed_matrix.c, kernel in rfec_cascade.hip): the same decode for
 * the sender's full row + column plans of k = 6..16 (rfec_packed_matrix_col != 0) in one launch of
 * k_decode_matrix_indexed<k, col>, no workspace; with n_rows == 0 the checker blocks alone.  The caller has checked
 * what rfec_launch_recover_indexed's has, the plan's shape, and groups * 4 < 2^32 (the checker's lanes) in place of
 * the header lanes; hipErrorInvalidValue otherwise.  No flags: rfec_set_tuning does not reach this call. */
int rfec_launch_recover_indexed_matrix(const rfec_kmask* M, uint32_t groups, uint32_t stride, uint32_t capacity,
                                       const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                       const rfec_hdr* hdr, const uint64_t* present, const rfec_hdr* meta,
                                       const uint16_t* fsize, const uint64_t* parity_present, uint64_t* recovered,
                                       const rfec_dense_out* out, void* stream);
/* 1 when P is the sender's full row + column plan of its k in rows of `col` (is_full_matrix, rfec_kernels.hip: the
 * rows of col consecutive segments in plan order, then the columns, lines of fewer than 2 members dropped), else 0 */
int rfec_full_matrix(const rfec_kplan* P, uint32_t col);
/* rfec_recover_indexed_matrix_wide_out (rfec_recover_indexed_matrix_wide.c, kernel in rfec_matrix_wide.hip): the
 * same decode for the sender's full row + column plan of any k in [6, RFEC_MAX_K] in rows of `col`, the planner's
 * (rfec_full_matrix(P, col) != 0, col in [3, 20], at most 23 lines), in one launch of k_decode_matrix_wide, which
 * takes (k, col) at run time; no workspace; with n_rows == 0 the checker blocks alone.  The caller has checked
 * what rfec_launch_recover_indexed_matrix's has, with one checker lane per group (groups < 2^32 as it stands);
 * hipErrorInvalidValue otherwise.  No flags: rfec_set_tuning does not reach this call. */
int rfec_launch_recover_indexed_matrix_wide(const rfec_kplan* P, uint32_t col, uint32_t groups, uint32_t stride,
                                            uint32_t capacity, const uint8_t* rows, uint32_t n_rows,
                                            const uint32_t* src_of, const rfec_hdr* hdr, const uint64_t* present,
                                            const rfec_hdr* meta, const uint16_t* fsize,
                                            const uint64_t* parity_present, uint64_t* recovered,
                                            const rfec_dense_out* out, void* stream);
/* rfec_recover_indexed_rows_wide_out (rfec_recover_indexed_rows_wide.c, kernel in rfec_rows_wide.hip): the same
 * decode for a row layout of any width in one launch of k_decode_rows_wide, which takes (k, col, n_lines) at run
 * time; no workspace; with n_rows == 0 the header blocks alone.  rfec_rows_wide_col is the predicate: the row width
 * col = line[0].count >= 2 when line l is (l col, stride 1, min(col, k - l col)) for every l < n_lines and n_lines is
 * ceil(k / col), or one less when the last row has one segment (it has no line); 0 for any other plan.  The tables'
 * pitch is k + n_lines (src_of) and n_lines (meta, fsize).  The caller has checked what
 * rfec_launch_recover_indexed's has (groups << rfec_header_lanes_log2(n_lines) < 2^32 among it);
 * hipErrorInvalidValue otherwise.  No flags: rfec_set_tuning does not reach this call. */
int rfec_rows_wide_col(const rfec_kplan* P);
int rfec_launch_recover_indexed_rows_wide(const rfec_kplan* P, uint32_t groups, uint32_t stride, uint32_t capacity,
                                          const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                          const rfec_hdr* hdr, const uint64_t* present, const rfec_hdr* meta,
                                          const uint16_t* fsize, const uint64_t* parity_present, uint64_t* recovered,
                                          const rfec_dense_out* out, void* stream);
/* The plans rfec_launch_recover_indexed runs in one launch of k_decode_rows_indexed: the row width of a row layout
 * with rows of <= 4 segments and k <= 64, 0 for any other plan. */
int rfec_rows_indexed_col(const rfec_kplan* P);
/* rfec_recover_indexed_shapes_out (rfec_recover_indexed_shapes.c, kernel in rfec_cascade.hip): the sections of
 * rfec_wire_regroup_shapes decoded in one launch of k_decode_shapes_indexed, section p's first groups[p] rows
 * (groups NULL: sections[p].cap) as rfec_launch_recover_indexed_matrix (rfec_packed_matrix_col != 0) or as
 * rfec_launch_recover_indexed's one launch (rfec_rows_indexed_col != 0) decodes them, into output rows
 * first[p] + c of out and recovered, first[p] the sum of the groups before p.  The caller has checked n_plans in
 * [1, RFEC_RECOVER_MAX_SHAPES], each plan, that every section with groups[p] > 0 has one of the two shapes and the
 * two calls' bounds for it (out->per_group <= k among them), its pointers, and that the sections' blocks
 * (rfec_recover_shapes_blocks) sum to less than 2^31; hipErrorInvalidValue otherwise.  All groups[p] == 0: no
 * launch.  No flags: rfec_set_tuning does not reach this call. */
int rfec_launch_recover_indexed_shapes(const rfec_kplan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                                       const uint32_t* groups, uint32_t stride, uint32_t capacity, const uint8_t* rows,
                                       uint32_t n_rows, uint64_t* recovered, const rfec_dense_out* out, void* stream);
/* the blocks of one section's part of that launch's grid, a multiple of 8: the grid its own call would take (cd:
 * 16-byte chunks of work per slot); 0 for a plan of neither shape */
uint32_t rfec_recover_shapes_blocks(const rfec_kplan* P, uint32_t groups, uint32_t per_group, uint32_t cd,
                                    uint32_t n_rows);
/* rfec_recover_indexed_window_out (rfec_recover_indexed_window.c, kernel in rfec_cascade.hip): the same sections in
 * one launch of k_decode_window_indexed, for any of the planner's shapes.  rfec_recover_window_family is the rule, the
 * first predicate that holds: 1 rfec_packed_matrix_col != 0 (as rfec_launch_recover_indexed_matrix decodes it),
 * 2 rfec_rows_indexed_col != 0 (as rfec_launch_recover_indexed's one launch), 3 the planner's full matrix of
 * k = 17..128 (rfec_num_packets' col in [2, 20], rfec_full_matrix, at most 23 lines: as
 * rfec_launch_recover_indexed_matrix_wide), 4 rfec_rows_wide_col != 0 with k >= 2 (as
 * rfec_launch_recover_indexed_rows_wide); 0: refused.  The caller has checked what
 * rfec_launch_recover_indexed_shapes' has, with every section's family and that family's bounds;
 * hipErrorInvalidValue otherwise.  All groups[p] == 0: no launch.  No flags: rfec_set_tuning does not reach this
 * call. */
int rfec_recover_window_family(const rfec_kplan* P);
int rfec_launch_recover_indexed_window(const rfec_kplan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                                       const uint32_t* groups, uint32_t stride, uint32_t capacity, const uint8_t* rows,
                                       uint32_t n_rows, uint64_t* recovered, const rfec_dense_out* out, void* stream);
/* the blocks of one section's part of that launch's grid, a multiple of 8: the grid its family's own call would take
 * (header or checker lanes per group: 4, 2^rfec_header_lanes_log2(n_lines), 1, 2^rfec_header_lanes_log2(n_lines));
 * 0 for a refused plan */
uint32_t rfec_recover_window_blocks(const rfec_kplan* P, uint32_t groups, uint32_t per_group, uint32_t cd,
                                    uint32_t n_rows);
/* rfec_recover_indexed_window_each_out (rfec_recover_indexed_window_each.c, kernel in rfec_cascade.hip): that launch
 * with per_group[p] out slots a row in section p (host [n_plans]; read only where groups[p] > 0), the sections' slots
 * packed end to end: one launch of k_decode_window_each.  The caller has checked what rfec_launch_recover_indexed_window's
 * has, per section with its own per_group[p] in [1, k], and the slots' total x CD < 2^31; hipErrorInvalidValue
 * otherwise. */
int rfec_launch_recover_indexed_window_each(const rfec_kplan* plans, uint32_t n_plans,
                                            const rfec_regroup_section* sections, const uint32_t* groups,
                                            uint32_t stride, uint32_t capacity, const uint8_t* rows, uint32_t n_rows,
                                            uint64_t* recovered, const uint32_t* per_group, uint8_t* out_shards,
                                            rfec_hdr* out_hdr, uint8_t* out_index, void* stream);
/* rfec_recover_deliver (rfec_recover_deliver.c, kernels in rfec_deliver.hip): the outputs of
 * rfec_launch_recover_indexed_shapes as a dense list in window order, in three launches on `stream` (k_deliver_count,
 * k_deliver_totals, k_deliver), two when groups <= 256 (one block counts the window and writes the totals).  first:
 * host [n_plans + 1], the prefix of the sections' rows as that decode numbers them; workspace: local[groups] u32,
 * then from the next multiple of 16 bytes one u32 per 256 groups.  The caller has checked n_plans in
 * [1, RFEC_RECOVER_MAX_SHAPES], groups in [1, 65535], fec_id0 != 0, stride a multiple of 16, capacity <= stride,
 * per_group >= 1, first[n_plans] * per_group * CD < 2^31 and the pointers; hipErrorInvalidValue otherwise. */
int rfec_launch_recover_deliver(const rfec_regroup_section* sections, uint32_t n_plans, const uint32_t* first,
                                uint32_t groups, uint32_t fec_id0, const uint8_t* shape_of, const uint32_t* rank_of,
                                uint32_t stride, uint32_t capacity, uint32_t per_group, const uint8_t* out_shards,
                                const rfec_hdr* out_hdr, const uint8_t* out_index, uint32_t max_out, rfec_rx_seg* seg,
                                uint8_t* seg_payload, uint32_t* first_of, uint32_t* n_out, void* workspace,
                                void* stream);
/* rfec_recover_deliver_each (rfec_recover_deliver_each.c, kernels in rfec_deliver.hip): rfec_launch_recover_deliver
 * over the outputs of rfec_launch_recover_indexed_window_each: k_deliver_count_each, k_deliver_totals, k_deliver_each,
 * the same launches and workspace.  first, slot_first: host [n_plans + 1], the prefixes of the sections' rows and of
 * their out slots; per_group: host [n_plans], read only for a section with rows and there >= 1.  The caller has
 * checked what rfec_launch_recover_deliver's has, with slot_first[n_plans] * CD < 2^31; hipErrorInvalidValue
 * otherwise. */
int rfec_launch_recover_deliver_each(const rfec_regroup_section* sections, uint32_t n_plans, const uint32_t* first,
                                     const uint32_t* slot_first, const uint32_t* per_group, uint32_t groups,
                                     uint32_t fec_id0, const uint8_t* shape_of, const uint32_t* rank_of,
                                     uint32_t stride, uint32_t capacity, const uint8_t* out_shards,
                                     const rfec_hdr* out_hdr, const uint8_t* out_index, uint32_t max_out,
                                     rfec_rx_seg* seg, uint8_t* seg_payload, uint32_t* first_of, uint32_t* n_out,
                                     void* workspace, void* stream);
/* Which kernels the calling thread's last rfec_launch_recover_indexed, rfec_launch_recover_indexed_matrix,
 * rfec_launch_recover_indexed_matrix_wide, rfec_launch_recover_indexed_rows_wide, rfec_launch_recover_indexed_shapes,
 * rfec_launch_recover_indexed_window, rfec_launch_recover_deliver, rfec_launch_recover_indexed_window_each or
 * rfec_launch_recover_deliver_each took (host-side, thread-local, for tests; apart from rfec_last_path, whose kinds
 * are a closed table): 0 none yet,
 * 1 | K << 8 one launch of k_decode_rows_indexed<K, 4> (K = 10, 32, or 0 for k and col at run time), 2 | MAXC << 8
 * k_peel_lds + k_recover_indexed<MAXC, ...> (MAXC = 4, 8), 3 | K << 8 one launch of k_decode_matrix_indexed<K, col>
 * (K = 6..16; rfec_launch_recover_indexed_matrix only), 4 | n << 8 one launch of k_decode_shapes_indexed over n
 * sections with groups (rfec_launch_recover_indexed_shapes only), 5 | n << 8 the n = 2 or 3 launches of
 * rfec_launch_recover_deliver (k_deliver_count, k_deliver_totals for a window of more than 256 groups, k_deliver),
 * 6 | k << 8 one launch of k_decode_matrix_wide (k = 6..128; rfec_launch_recover_indexed_matrix_wide only),
 * 7 | k << 8 | col << 16 one launch of k_decode_rows_wide (k = 2..128 in rows of col = 2..128;
 * rfec_launch_recover_indexed_rows_wide only), 8 | n << 8 one launch of k_decode_window_indexed over n sections
 * with groups (rfec_launch_recover_indexed_window only), 9 | n << 8 one launch of k_decode_window_each over n
 * sections with groups (rfec_launch_recover_indexed_window_each only), 10 | n << 8 the n = 2 or 3 launches of
 * rfec_launch_recover_deliver_each (k_deliver_count_each, k_deliver_totals for a window of more than 256 groups,
 * k_deliver_each). */
uint32_t rfec_indexed_last_path(void);
/* Which kernel the calling thread's last wire-codec launch (rfec_wire.hip: the rfec_launch_wire_* shims) took, and on
 * how many blocks: kernel id | grid blocks << 8, 0 before the first (host-side, thread-local, for tests; apart from
 * rfec_last_path and rfec_indexed_last_path, which keep their own tags).  A wave of the kernel then strides over its
 * units by nw = 16 * blocks.  A call that takes several launches (the fused encodes split a batch past 32-bit
 * offsets) leaves its last launch's tag.  The ids:
 *   FRAME_FEC_32 / FRAME_SEG_32    k_frame_fec<32> / k_frame_seg<32>: dstride > 1,280, a datagram per wave step
 *   PARSE_20 / PARSE_32            k_parse<20> / k_parse<32>: a datagram per wave step (RFEC_TUNE_WAVE_PARSE, or
 *                                  slots or payload slots past 1,280 bytes)
 *   FRAME_SEG_Q / FRAME_FEC_Q      k_frame_seg_q / k_frame_fec_q: a quad of 4 datagrams per wave step
 *   PARSE_Q                        k_parse_q: a quad per wave step, header batches of 16 quads
 *   ENCODE_FEC_Q                   k_encode_frame_fec_q (rfec_wire_encode_fec): a quad of SIM_FEC per wave step
 *   ENCODE_SEND_Q / _Q2            k_encode_send_q<., 5> / <., 2> (dstride <= 512): 4 groups per wave step
 *   ENCODE_SEND_SHAPES_Q / _Q2     k_encode_send_shapes_q<., 5> / <., 2> (dstride <= 512): 4 descriptors per step */
enum {
    RFEC_WIRE_K_NONE = 0,
    RFEC_WIRE_K_FRAME_FEC_32 = 1,
    RFEC_WIRE_K_FRAME_SEG_32 = 3,
    RFEC_WIRE_K_PARSE_20 = 4,
    RFEC_WIRE_K_PARSE_32 = 5,
    RFEC_WIRE_K_FRAME_SEG_Q = 6,
    RFEC_WIRE_K_FRAME_FEC_Q = 7,
    RFEC_WIRE_K_PARSE_Q = 8,
    RFEC_WIRE_K_ENCODE_FEC_Q = 9,
    RFEC_WIRE_K_ENCODE_SEND_Q = 10,
    RFEC_WIRE_K_ENCODE_SEND_Q2 = 11,
    RFEC_WIRE_K_ENCODE_SEND_SHAPES_Q = 12,
    RFEC_WIRE_K_ENCODE_SEND_SHAPES_Q2 = 13
};
uint32_t rfec_wire_last_path(void);
/* For tests: at most `blocks` blocks for every wire-codec launch from now on, in every thread (0, the default: none
 * -- the grid is the resident blocks or what the batch needs, whichever is less; the cap is taken after that).  A
 * small cap makes a small batch walk the persistent loops as deep as a large batch does on the whole device.  One
 * word, read once per launch; no environment variable. */
void rfec_wire_set_grid_cap(uint32_t blocks);
/* max_len: the longest datagram when the caller knows it (host-side lengths), else 0; slots
 * wider than 1,280 B still take the 20-byte-lane parse when every datagram fits 1,280 B */
int rfec_launch_wire_parse(uint32_t n, uint32_t dstride, const uint8_t* dgram, const uint16_t* dlen,
                           uint32_t stride, uint32_t capacity, rfec_wire_rec* recs, uint8_t* payload,
                           uint32_t max_len, void* stream);
int rfec_launch_gather_rows(uint8_t* dst, const uint8_t* src, const int32_t* map, uint32_t rows, uint32_t stride,
                            void* stream);
/* the receiver session's device stage (rfec_rx_dev.c rx_device): dst row r <- src row map[r] (zeros for
 * map[r] < 0; `map` may be pinned host memory), and tbytes (a multiple of 16) of tables tsrc -> tdst */
int rfec_launch_rx_stage(uint8_t* dst, const uint8_t* src, const int32_t* map, uint32_t rows, uint32_t stride,
                         void* tdst, const void* tsrc, size_t tbytes, void* stream);
/* The receiver session's batch split, per parsed record (rfec_rx_plane.c rx_phase0): its shard (fec_id % T, a
 * segment outside FEC by packet id; 0xFF: no effect on the control plane), its kind (RX_SPLIT_*) and the
 * value the replay's max_ts rules read (a segment's timestamp, a parity's send_ts + 3000). */
#define RX_SPLIT_NONE 0
#define RX_SPLIT_SEG_TS 1 /* SIM_SEG with fec_id and packet id: may raise max_ts */
#define RX_SPLIT_SEG 2
#define RX_SPLIT_FEC 3
typedef struct {
    uint8_t shard, kind;
    uint16_t reserved;
    uint32_t value;
} rfec_rx_split; /* 8 bytes */
int rfec_launch_rx_split(const rfec_wire_rec* recs, uint32_t n, uint32_t T, rfec_rx_split* out, void* stream);
/* rfec_launch_wire_parse with the receiver session's split entries of the parsed records (T shards) written
 * beside them (the quarter-wave parse writes them itself; the wave parses are followed by k_rx_split) */
int rfec_launch_wire_parse_split(uint32_t n, uint32_t dstride, const uint8_t* dgram, const uint16_t* dlen,
                                 uint32_t stride, uint32_t capacity, rfec_wire_rec* recs, uint8_t* payload,
                                 uint32_t max_len, rfec_rx_split* split, uint32_t shards, void* stream);
/* receiver groups above RFEC_MAX_K segments: out row = parity row ^ member rows (one dependency level per call) */
typedef struct {
    int32_t out;       /* output row */
    int32_t parity;    /* row of `rows` holding the line's parity */
    uint32_t member0;  /* first member code in the member list */
    uint32_t n_members;
} rfec_line_job;
int rfec_launch_line_jobs(const rfec_line_job* jobs, uint32_t n_jobs, const int32_t* members, const uint8_t* rows,
                          uint8_t* outrows, uint32_t stride, void* stream);
int rfec_launch_zero_tails(uint32_t slots, uint32_t stride, uint8_t* shards, const rfec_hdr* hdr, void* stream);
/* rfec_hostio.hip: razor's structs in device-mapped host memory <-> the slot
 * layout (pointer tables hold device addresses, 0 = a lost struct, bit 0 set =
 * header only: the payload is not read and its slot is zeroed).  One launch
 * gathers ns sim_segment_t (-> shards + header records) and nf sim_fec_t (->
 * parity slots + fec_meta records + fec_data_size + fec_id; nf may be 0) and
 * copies aux_n u64 words aux_src -> aux_dst (may be 0: none). */
int rfec_launch_host_gather(const uint64_t* sptrs, uint32_t ns, uint8_t* shards, rfec_hdr* hdr,
                            const uint64_t* fptrs, uint32_t nf, uint8_t* parity, rfec_hdr* meta, uint16_t* fsize,
                            uint16_t* fecid, uint32_t stride, uint32_t video, const uint64_t* aux_src,
                            uint64_t* aux_dst, uint32_t aux_n, void* stream);
/* sender staging (rfec_sender.c): slot s of `stride` bytes <- src[s] (device address of host bytes, any
 * alignment; 0: zeros) for size[s] bytes, zeros past them */
int rfec_launch_send_gather(const uint64_t* src, const uint16_t* size, uint32_t slots, uint32_t stride, uint8_t* dst,
                            void* stream);
/* parity slots of `groups` groups -> their sim_fec_t, stamped as flex_fec_sender_update does */
int rfec_launch_host_scatter_fec(const uint64_t* fptrs, uint32_t groups, const rfec_kplan* P, uint32_t stride,
                                 const uint8_t* parity, const rfec_hdr* meta, const uint16_t* fsize,
                                 const int8_t* status, const rfec_hdr* hdr, uint16_t fec_id0, uint32_t g0,
                                 uint32_t video, void* stream);
/* dense recover output -> the callers' out_seg structs (flex_fec_recover's
 * fields + fec_id); out_index and the recovered masks into oidx_host / rec_host */
int rfec_launch_host_scatter_seg(const uint64_t* optrs, uint32_t groups, uint32_t E, uint32_t stride,
                                 const uint8_t* out_shards, const rfec_hdr* out_hdr, const uint8_t* out_index,
                                 const uint16_t* fecid, const uint64_t* ppm, uint32_t n_lines, uint32_t video,
                                 uint8_t* oidx_host, const uint64_t* recovered, uint64_t* rec_host, void* stream);
const char* rfec_hip_error_string(int code);

/* Group-level drop-in (rfec_flex.c) over the per-thread pinned, device-mapped
 * staging area of the single-call path (rfec_host.c): one launch and one
 * stream sync per call.  Both return RFEC_OK once the device work is done
 * (per-item results in rets[]), or an error code with rfec_last_error set. */
#define RFEC_DI_GROUPS 8 /* one-line recover jobs per launch */
typedef struct {
    sim_segment_t* const* segs; /* the present members */
    int count;
    sim_fec_t* fec;
    sim_segment_t* out;
} rfec_di_recover_job;
__attribute__((visibility("hidden"))) int rfec_di_generate_group(sim_segment_t* const* segs, int k,
                                                                 const rfec_plan* plan, sim_fec_t* const* outs,
                                                                 int* rets);
__attribute__((visibility("hidden"))) int rfec_di_recover_lines(const rfec_di_recover_job* jobs, int n, int* rets);
/* The resident service (rfec_service.hip): one workgroup polling a doorbell for
 * the drop-in's jobs.  Two control blocks of this layout: the request side
 * (bell, stop, quit, job; the staging slots follow it) in host-mapped device
 * memory or pinned host memory, the results side (done, alive, out; the output
 * slots follow it) in pinned host memory; with a host-memory request side
 * they are one block.  A job's payloads sit in staging slots 0..n_slots-1
 * (LDS slot s = staging slot s), zero-filled to the slot's end; its outputs go
 * to the output slots (encode: line l, recover: job g). */
#define RFEC_SVC_ENCODE 1u
#define RFEC_SVC_RECOVER 2u
#define RFEC_SVC_SLOTS 264 /* an encode group (<= 255 members) or the recover jobs' members + parities */
#define RFEC_SVC_MAX_GROUPS 8 /* workgroups of the service, each on its share of the chunk columns */
/* the doorbell word: job sequence number | n_slots << 32 | op << 48 */
#define RFEC_SVC_BELL(seq, ns, op) ((uint64_t)(uint32_t)(seq) | (uint64_t)(ns) << 32 | (uint64_t)(op) << 48)
typedef struct {
    uint32_t op, n_slots, groups, capacity;
    rfec_kplan plan;                   /* encode: the group's lines over slots 0..k-1 */
    uint16_t slot0[RFEC_DI_GROUPS];    /* recover job g: its first slot (members, then its parity) and the
                                        * first of its header records (the parity's meta, then the members') */
    uint16_t count[RFEC_DI_GROUPS];    /* present members */
    uint16_t fsize[RFEC_DI_GROUPS];    /* fec_data_size */
    uint16_t pad[RFEC_DI_GROUPS];
    uint8_t slot_nck[RFEC_SVC_SLOTS];  /* 16-byte chunks of the slot that hold its bytes (zeros follow) */
    uint32_t hdr[RFEC_SVC_SLOTS * 5];  /* encode: member i at 5 i; recover: as slot0 */
} rfec_svc_job;
typedef struct {
    uint64_t bell;                 /* host-written: RFEC_SVC_BELL, written last */
    uint32_t stop, pad0[13];       /* host-written: leave now */
    uint32_t done[RFEC_SVC_MAX_GROUPS], pad1[16 - RFEC_SVC_MAX_GROUPS]; /* device-written: workgroup w's last job */
    uint32_t alive, quit, pad2[14]; /* alive: 1 set by the host before a launch, 0 by workgroup 0 as it leaves;
                                     * quit: set by workgroup 0 before that, the others leave on it */
    struct {
        uint32_t meta[RFEC_MAX_LINES][5]; /* encode: line l's meta; recover: job g's recovered header */
        uint16_t fsize[RFEC_MAX_LINES];
        int8_t status[RFEC_MAX_LINES];    /* flex_fec_generate / flex_fec_recover's 0 / -1 */
        uint64_t t[2][4]; /* s_memrealtime of job seq at [seq & 1]: bell seen, job staged, results stored,
                           * drained; written after its `done` (the next job's drain lands it) */
    } out;
    rfec_svc_job job;
} rfec_svc_ctl;
int rfec_launch_service(rfec_svc_ctl* ctl, rfec_svc_ctl* in, const uint8_t* shards, uint8_t* out, uint32_t stride,
                        uint64_t idle_ticks, uint64_t life_ticks, uint32_t groups, void* stream);

__attribute__((visibility("hidden"))) int rfec_set_error(int code, const char* what);
__attribute__((visibility("hidden"))) double now_us(void); /* rfec_host.c: CLOCK_MONOTONIC, microseconds */
/* sets rfec_last_error() from an errno value (0: `what` alone); returns code */
int rfec_set_error_sys(int code, const char* what, int err);

#ifdef __cplusplus
}
#endif

#endif
