/*
 * razor_fec.h -- C ABI of the MI355X-native flex-FEC engine.
 *
 * Two layers, both exported from librazor_fec.so:
 *
 *  1. Drop-in symbols with the reference signatures (link-compatible with the
 *     callers in sim_transport/fec/flex_fec_sender.c:175,219 and
 *     flex_fec_receiver.c:144,200):
 *        flex_fec_generate   replaces sim_transport/fec/flex_fec_xor.h:7 (.c:4-53)
 *        flex_fec_recover    replaces sim_transport/fec/flex_fec_xor.h:8 (.c:55-104)
 *     Each call runs on the GPU (one launch over a zero-copy staging area).
 *
 *  2. A batched, device-resident API (rfec_*): many independent FEC groups laid
 *     out structure-of-arrays in HBM, encoded / recovered by one kernel launch
 *     each.  The plan (which segments every parity line covers) restates
 *     flex_fec_sender_num_packets / flex_fec_sender_update
 *     (sim_transport/fec/flex_fec_sender.c:81-135, 146-245).
 *
 * All pointers passed to rfec_*_batch are DEVICE pointers; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  Nothing in this
 * header needs HIP headers.
 */
#ifndef RAZOR_FEC_H_
#define RAZOR_FEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Reference ABI types (sim_transport/sim_proto.h:54, 80-99, 145-174).       */
/* When the reference's own sim_proto.h is already included, its definitions */
/* are used and these are skipped; the layouts are identical.                */
/* ------------------------------------------------------------------------ */
#ifndef SIM_VIDEO_SIZE
#define SIM_VIDEO_SIZE 1000 /* sim_proto.h:54 */
#endif

#ifndef __sim_proto_h_001__
typedef struct {
    uint32_t packet_id;     /* offset  0 */
    uint32_t fid;           /* offset  4 */
    uint32_t timestamp;     /* offset  8 */
    uint16_t index;         /* offset 12 */
    uint16_t total;         /* offset 14 */
    uint8_t ftype;          /* offset 16 */
    uint8_t payload_type;   /* offset 17 */
    uint8_t remb;           /* offset 18 */
    uint16_t fec_id;        /* offset 20 */
    uint16_t send_ts;       /* offset 22 */
    uint16_t transport_seq; /* offset 24 */
    uint32_t send_id;       /* offset 28 */
    uint16_t data_size;     /* offset 32 */
    uint8_t data[SIM_VIDEO_SIZE]; /* offset 34 (not 16-B aligned) */
} sim_segment_t;

typedef struct {
    uint32_t seq;  /* XOR of packet_id */
    uint32_t fid;
    uint32_t ts;   /* XOR of timestamp */
    uint16_t index;
    uint16_t total;
    uint8_t ftype;
    uint8_t payload_type;
    uint16_t size; /* XOR of data_size */
} sim_fec_meta_t;

typedef struct {
    uint16_t fec_id;        /* offset  0 */
    uint8_t row;            /* offset  2 */
    uint8_t col;            /* offset  3 */
    uint8_t index;          /* offset  4: row r, or 0x80|c for column c */
    uint16_t count;         /* offset  6 */
    uint32_t base_id;       /* offset  8 */
    uint32_t send_ts;       /* offset 12 */
    uint16_t transport_seq; /* offset 16 */
    sim_fec_meta_t fec_meta; /* offset 20 */
    uint16_t fec_data_size; /* offset 40 */
    uint8_t fec_data[SIM_VIDEO_SIZE]; /* offset 42 */
} sim_fec_t;
#endif /* __sim_proto_h_001__ */

/* Drop-in entry points: same names, argument meaning and 0 / -1 returns as
 * flex_fec_xor.c:4-53 and :55-104 (see DESIGN.md for the side effects kept). */
int flex_fec_generate(sim_segment_t* segs[], int segs_count, sim_fec_t* fec);
int flex_fec_recover(sim_segment_t* segs[], int segs_count, sim_fec_t* fec, sim_segment_t* out_seg);

/* SIM_VIDEO_SIZE this library's drop-in symbols were compiled with. */
int rfec_sim_video_size(void);

/* ABI version of this header / library.  A caller compiled against one
 * header checks rfec_abi_version() == RFEC_ABI_VERSION before using structs
 * whose size changed.  History: 5 -- rfec_host_timing grew from 48 to 56
 * bytes (zero_copy, reserved); 6 -- rfec_abi_version, rfec_rx_session_info grew
 * from 24 to 88 bytes (threads, batches_*, the host time split),
 * rfec_rx_session_set_threads; 7 -- rfec_send_report grew from 64 to 72 bytes
 * (zero_copy, reserved). */
#define RFEC_ABI_VERSION 7
uint32_t rfec_abi_version(void);

/* ------------------------------------------------------------------------ */
/* Batched device API                                                        */
/* ------------------------------------------------------------------------ */
#define RFEC_MAX_K 128     /* segments per group in recovery (sim_sender.c:370 flushes at 100) */
#define RFEC_MAX_K_ENCODE 255 /* segments per group in an encode plan (rfec_line's 8-bit fields; razor's
                                 flex sender keeps row and col in uint8_t, so no line exceeds it) */
#define RFEC_MAX_LINES 64  /* parity lines per group */

#define RFEC_OK 0
#define RFEC_EINVAL (-1)
#define RFEC_EDEVICE (-2)
#define RFEC_ENOMEM (-3)

/* 20-byte header record.  Field order and widths are sim_fec_meta_t's, so the
 * XOR of several records, taken as five 32-bit words, is the record of the
 * XORed fields (flex_fec_xor.c:13-20, 37-44, 64-85). */
typedef struct {
    uint32_t seq;   /* packet_id */
    uint32_t fid;
    uint32_t ts;    /* timestamp */
    uint16_t index;
    uint16_t total;
    uint8_t ftype;
    uint8_t payload_type;
    uint16_t size;  /* data_size */
} rfec_hdr;

/* One parity line: members first, first+stride, ..., first+(count-1)*stride. */
typedef struct {
    uint8_t first;
    uint8_t stride;
    uint8_t count;
    uint8_t index; /* sim_fec_t.index: row r, or 0x80|c (flex_fec_sender.c:180,224) */
} rfec_line;

#define RFEC_LAYER_ROWS 1u
#define RFEC_LAYER_COLS 2u

typedef struct {
    uint16_t k;        /* segments per group */
    uint8_t row, col;  /* matrix shape (flex_fec_sender_t.row/.col) */
    uint8_t rc;        /* 1 when the planner chose matrix mode */
    uint8_t n_lines;   /* parity lines emitted (lines with <2 members dropped) */
    uint8_t n_row_lines;
    uint8_t reserved;
    rfec_line line[RFEC_MAX_LINES]; /* rows first, then columns, reference order */
} rfec_plan;

/* Restates flex_fec_sender_num_packets (flex_fec_sender.c:81-135).  Writes
 * row/col and returns rc (0 strip mode, 1 matrix mode); k==0 -> (0,0). */
int rfec_num_packets(uint16_t k, uint8_t protect_fraction, uint8_t* row, uint8_t* col);

/* Plan of flex_fec_sender_update (flex_fec_sender.c:146-245) for a group of
 * k segments at the given protect_fraction, restricted to `layers`.  Lines
 * whose flex_fec_generate would fail (fewer than 2 members) are dropped, as
 * the reference drops them.  Returns RFEC_OK or RFEC_EINVAL. */
int rfec_plan_from_fraction(uint16_t k, uint8_t protect_fraction, unsigned layers, rfec_plan* plan);

/* Plan for an explicit row x col matrix over k segments (rows of `col`
 * consecutive segments, columns strided by `col`). */
int rfec_plan_matrix(uint16_t k, uint8_t row, uint8_t col, unsigned layers, rfec_plan* plan);

/* The plan a receiver takes for a SIM_FEC's (count, row, col), the only place
 * a group's shape reaches it (rfec_wire_window_census reports these keys).  A
 * key is plannable when 1 <= count <= RFEC_MAX_K, row >= 1, col >= 2 and
 * row * col >= count; any other key gets RFEC_EINVAL.  If count >= 6 and
 * rfec_num_packets(count, 255, ...) returns exactly (row, col) -- the planner's
 * matrix-mode shape, the matrix key of count -- the plan is
 * rfec_plan_matrix(count, row, col, RFEC_LAYER_ROWS | RFEC_LAYER_COLS); for any
 * other key it is rfec_plan_matrix(count, row, col, RFEC_LAYER_ROWS).  A
 * strip-mode sender whose key coincides with the matrix key gets the full
 * matrix: its column parities simply never arrive, and the recovery is the
 * same.  A plannable key whose plan has no lines (count 1) returns RFEC_OK with
 * n_lines == 0. */
int rfec_plan_from_key(uint16_t count, uint8_t row, uint8_t col, rfec_plan* plan);

/*
 * Device layout (G groups, k segments, n = plan->n_lines):
 *   shards  [G][k][stride] u8    payloads, bytes beyond data_size MUST be 0
 *   hdr     [G][k]         rfec_hdr
 *   parity  [G][n][stride] u8    fec_data (see "Slot tails")
 *   meta    [G][n]         rfec_hdr  (fec_meta)
 *   fec_size[G][n]         u16   (fec_data_size)
 *   status  [G][n]         i8    0, or -1 where flex_fec_generate returns -1
 * stride is a multiple of 16 and >= capacity; capacity plays SIM_VIDEO_SIZE.
 *
 * Alignment.  The minimum alignment of every device pointer of the batched
 * API (this call, rfec_recover_batch[_out], the packed calls), as the kernels
 * access them; a sub-allocated arena may place each buffer at exactly this.
 * The entry points return RFEC_EINVAL for less:
 *   16 bytes  shards, parity, out_shards (payload chunks move as 16-byte
 *             vectors), workspace, packed (records are read as 16-byte vectors)
 *    8 bytes  present, parity_present, recovered (64-bit words)
 *    4 bytes  hdr, meta, out_hdr (rfec_hdr records move as five 32-bit words;
 *             a 16-byte aligned array is staged with wider loads, a 4-byte
 *             aligned one with 32-bit loads, same result)
 *    2 bytes  fec_size
 *    1 byte   status, out_index
 * (rfec_wire_encode_fec and rfec_wire_encode_send, the wire-codec calls that
 * check alignment: 16 bytes shards and the datagram slots, 4 bytes hdr, stamps
 * and orders, 2 bytes the lengths; rfec_wire_regroup: the batch layout's as
 * above, 16 bytes recs and payload, 4 bytes base_id, src_of and slot_of;
 * rfec_wire_regroup_index and rfec_recover_indexed_out: the same, 16 bytes
 * rows; rfec_wire_regroup_shapes: the same per section, 4 bytes group_of,
 * rank_of, anchor_of and counts)
 *
 * Slot tails.  Every call works on the CD = ceil(capacity / 16) leading
 * 16-byte chunks of a slot (CD = 1 for capacity 0) and touches no byte of any
 * slot from 16 * CD to the stride, under every kernel selection
 * (rfec_set_tuning).  Of a slot a call writes:
 *   parity line        [0, fec_data_size) the XOR of the members, [fec_data_size,
 *                      16 * CD) zero, [16 * CD, stride) not written (they keep
 *                      what the buffer held; a reader takes fec_data_size bytes)
 *   recovered segment  (in place, or a dense out slot whose out_index is not
 *                      0xFF) [0, 16 * CD) the XOR of the line's parity and its
 *                      other members over whole chunks: [0, data_size) the
 *                      segment, [data_size, 16 * CD) zero whenever the line's
 *                      inputs are zero beyond their sizes (parities as encoded
 *                      here, headers as sent); [16 * CD, stride) not written
 * The inputs' bytes from 16 * CD to the stride are not read.
 */
int rfec_encode_batch(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                      const uint8_t* shards, const rfec_hdr* hdr, uint8_t* parity, rfec_hdr* meta,
                      uint16_t* fec_size, int8_t* status, void* stream);

/*
 * Peeling recovery (flex_fec_receiver.c:105-206 + the cascade of
 * sim_receiver.c:780-804), batched:
 *   shards/hdr       in/out: erased slots are filled with the recovered segment
 *   present          [G][2] u64: bit i = segment i was received
 *   parity/meta/fec_size as produced by rfec_encode_batch
 *   parity_present   [G] u64: bit l = parity line l was received
 *   recovered        [G][2] u64 out: bit i = segment i was recovered here
 *   workspace        rfec_recover_workspace_size(plan, G) bytes of device memory
 *                    (one peeling-schedule record per group, used by the
 *                    generic peel + replay), 16-byte aligned; its contents
 *                    need no initialisation
 * A line recovers its single missing member only under the conditions of
 * flex_recover_row/col and flex_fec_recover (sizes within fec_data_size).
 * `recovered` is authoritative: an erased slot whose bit stays clear holds
 * unspecified bytes in [0, 16 * CD) afterwards (the fused decode may have
 * written it).  A received segment (present bit set) is only read: its slot and
 * header are byte-identical afterwards, as are present, parity, meta, fec_size
 * and parity_present.  What a recovered slot holds: "Slot tails" above.
 */
size_t rfec_recover_workspace_size(const rfec_plan* plan, uint32_t groups);
int rfec_recover_batch(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                       uint8_t* shards, rfec_hdr* hdr, const uint64_t* present,
                       const uint8_t* parity, const rfec_hdr* meta, const uint16_t* fec_size,
                       const uint64_t* parity_present, uint64_t* recovered, void* workspace,
                       void* stream);

/*
 * Recovery into a dense output, as flex_fec_recover writes each recovered
 * segment into a caller-allocated out_seg (flex_fec_xor.c:55-104,
 * flex_fec_receiver.c:142-143): the shards and headers are only read.  The
 * e-th erased segment of group g (e-th in segment-index order among the
 * segments whose present bit is clear, e < per_group) goes to
 *   out_shards [g*per_group + e][stride]   its payload ("Slot tails" above: chunks
 *                                          [0, 16 * CD) written, the rest kept)
 *   out_hdr    [g*per_group + e]           its recovered header record
 *   out_index  [g*per_group + e]           its segment index, or 0xFF where
 *                                          that erased segment was not recovered
 *                                          (its out_shards slot then holds
 *                                          unspecified bytes)
 * and `recovered` gets its bit as in rfec_recover_batch.  Any plan: where
 * lines cascade (rows + columns), a recovered segment feeds the lines after
 * it as in place.  Only erased segments of rank < per_group are recovered
 * (they are the ones with an output slot), so with per_group at least the
 * group's erasure count the result is rfec_recover_batch's; with fewer slots
 * the peel runs as if the segments of higher rank could not be recovered.
 * Same workspace as rfec_recover_batch.
 */
int rfec_recover_batch_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                           const uint8_t* shards, const rfec_hdr* hdr, const uint64_t* present,
                           const uint8_t* parity, const rfec_hdr* meta, const uint16_t* fec_size,
                           const uint64_t* parity_present, uint64_t* recovered, uint32_t per_group,
                           uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index, void* workspace,
                           void* stream);

/*
 * Packed erasure records: the header input of rfec_recover_batch_out for row
 * layouts (rows of `col` consecutive segments and no columns -- strip mode or
 * the row layer alone, flex_fec_sender.c:166-190; k <= 64, col <= 4) laid out
 * per erased segment, so a decode reads one contiguous run per group instead
 * of the present / parity_present / fec_size / meta / hdr arrays, whose
 * sectors it shares with the rows that do not fire.  Group g's record,
 * rfec_packed_stride(plan, per_group) bytes (a multiple of 64) at
 * packed + g * stride:
 *   +0   u64 present         bit i = segment i was received
 *   +8   u64 parity_present  bit r = row r's parity was received
 *   +16 + e * S, e < per_group, S = 24 + 20 (col - 1): the group's e-th erased
 *        segment (index order), in row r:
 *        rfec_hdr meta of row r; u16 fec_data_size of row r; u16 0;
 *        rfec_hdr of row r's other members in index order (zeros past the
 *        row's end).  All zeros where the group has fewer than e + 1 erasures.
 *   zeros up to the stride.
 * A receiver that knows the plan can write these as segments and parities
 * arrive (each segment's record goes to the slot of every erased segment of
 * its row); rfec_pack_erasures builds them from the batch layout.
 * rfec_recover_packed_out then gives rfec_recover_batch_out's results for the
 * same batch (out_shards, out_hdr, out_index, recovered) with no workspace.
 * rfec_packed_stride returns 0 for a plan outside the row layouts above or a
 * per_group outside [1, k].  (razor's flex_fec_receiver.c:105-206 reads the
 * same fields per line; the layout is this library's.)
 */
size_t rfec_packed_stride(const rfec_plan* plan, uint32_t per_group);
int rfec_pack_erasures(const rfec_plan* plan, uint32_t groups, const rfec_hdr* hdr, const uint64_t* present,
                       const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                       uint32_t per_group, uint8_t* packed, void* stream);
int rfec_recover_packed_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                            const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                            uint64_t* recovered, uint32_t per_group, uint8_t* out_shards, rfec_hdr* out_hdr,
                            uint8_t* out_index, void* stream);

/*
 * Packed matrix records: the same idea for the sender's full row + column
 * plans of k = 6..16 (flex_fec_sender_num_packets' matrix: rows of COL
 * consecutive segments, COL = 3 for k <= 9, else 4, R = ceil(k / COL) <= 4
 * rows; the row lines first, then the COL column lines; a last row of one
 * member has no line, so there are NR = R or R - 1 row lines), which the
 * row-layout calls above refuse.  A segment t lies in row r = t / COL and
 * column c = t % COL, and either line may recover it -- at once or after a
 * cascade -- so a slot carries both.  Group g's record,
 * rfec_packed_matrix_stride(plan, per_group) bytes (a multiple of 64) at
 * packed + g * stride (16-byte aligned):
 *   +0   u64 present
 *   +8   u64 parity_present  bit l = plan line l (rows first)
 *   +16 + e * S, e < per_group, S = RH + CH, RH = 24 + 20 (COL - 1),
 *        CH = 24 + 20 (R - 1): the group's e-th erased segment t (index order):
 *        row half, RH bytes: rfec_hdr meta of row line r; u16 fec_data_size
 *          of row r; u16 0; rfec_hdr of row r's other members in index order.
 *          All zeros when row r has no line.
 *        column half, CH bytes: the same for line NR + c and column c's other
 *          members in index order.
 *        In both halves a member that was not received holds zeros (not
 *        whatever the hdr array held: a receiver that never saw the header
 *        writes the same bytes), as do the positions past the line's end.
 *        All zeros where the group has fewer than e + 1 erasures.
 *   zeros up to the stride.
 *   (k = 10: COL 4, R 3, S = 84 + 64 = 148; 192 bytes at per_group 1, 320 at 2.)
 * A line only ever fires for a target of rank < per_group, whose slot holds
 * the line's meta, size and received members; members recovered earlier in a
 * cascade come from the earlier step: the records carry the exact peel's whole
 * input, rejected lines and their rescheduling included.
 * rfec_pack_erasures_matrix builds the records from the batch layout (every
 * byte of every record is written); rfec_recover_packed_matrix_out gives
 * rfec_recover_batch_out's out_shards, out_hdr, out_index and recovered for
 * the batch the records describe, with no workspace (payload bytes over
 * [0, ceil(capacity / 16) * 16) of every slot whose out_index is not 0xFF; the
 * bytes of an unrecovered slot are unspecified).  rfec_packed_matrix_stride
 * returns 0, and the two calls RFEC_EINVAL, for any other plan or a per_group
 * outside [1, k].
 */
size_t rfec_packed_matrix_stride(const rfec_plan* plan, uint32_t per_group);
int rfec_pack_erasures_matrix(const rfec_plan* plan, uint32_t groups, const rfec_hdr* hdr, const uint64_t* present,
                              const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                              uint32_t per_group, uint8_t* packed, void* stream);
int rfec_recover_packed_matrix_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                   const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                                   uint64_t* recovered, uint32_t per_group, uint8_t* out_shards, rfec_hdr* out_hdr,
                                   uint8_t* out_index, void* stream);

/*
 * Host-resident batch: the path that starts and ends in host memory (segments
 * built from UDP socket buffers, sim_session.c).  Gathers G groups of
 * sim_segment_t (segs[g*k + i], this library's SIM_VIDEO_SIZE layout) into a
 * pinned structure-of-arrays staging area, copies it to HBM, runs
 * rfec_encode_batch, copies the parities back and scatters them into the
 * caller's sim_fec_t (fecs[g*n + l]) stamped like flex_fec_sender_update
 * (flex_fec_sender.c:176-181, 220-225: fec_id = fec_id0 + g, base_id = the
 * group's smallest packet_id, row, col, index, count).  A line whose
 * flex_fec_generate would fail gets fec_data_size = 0xFFFF and no payload.
 * `timing` (may be NULL) receives the per-stage wall times in microseconds.
 * Staging is per calling thread and grows on demand.
 *
 * Zero copy: when every segs / fecs pointer lies inside one block from
 * rfec_pinned_alloc (and RFEC_HOST_ZEROCOPY is not "0"), no host gather or
 * scatter runs -- the device reads the sim_segment_t and writes the sim_fec_t
 * through the block's device mapping over PCIe, and only the pointer tables
 * are staged (timing->zero_copy = 1; gather_us is then the host's table
 * build, h2d_us the device's gathers over PCIe, kernel_us the encode / decode,
 * d2h_us the device's scatter, scatter_us the copy of out_index / recovered).
 */
typedef struct {
    double gather_us, h2d_us, kernel_us, d2h_us, scatter_us, total_us;
    uint32_t zero_copy, reserved;
} rfec_host_timing;

int rfec_host_encode_groups(const rfec_plan* plan, uint32_t groups, sim_segment_t* const* segs,
                            sim_fec_t* const* fecs, uint16_t fec_id0, rfec_host_timing* timing);

/*
 * The receive direction of rfec_host_encode_groups: G groups in host memory,
 * segs[g*k + i] the received sim_segment_t of member i or NULL where it was
 * lost, fecs[g*n + l] the received sim_fec_t of line l or NULL.  Gathers them
 * into the pinned staging (payload slots, header records, the present and
 * parity-present masks, the parities' meta / fec_data_size / payload), copies
 * it to HBM, runs rfec_recover_batch_out with per_group dense slots, copies
 * the recovered slots back and scatters them like flex_fec_recover's out_seg
 * (flex_fec_xor.c:64-101): out[g*per_group + e] receives the group's e-th
 * erased segment (index order) when the peel recovered it -- header fields,
 * data_size, SIM_VIDEO_SIZE bytes of data (zero past the recovering line's
 * fec_data_size), fec_id of the group's parities -- and out_index[g*per_group
 * + e] its member index, 0xFF when it was not recovered (out[...] untouched).
 * recovered (may be NULL): [G][2] masks.  Chunked and double-buffered as the
 * encode; k <= RFEC_MAX_K.  timing: gather = staging, scatter = delivery.
 */
int rfec_host_recover_groups(const rfec_plan* plan, uint32_t groups, sim_segment_t* const* segs,
                             sim_fec_t* const* fecs, uint32_t per_group, sim_segment_t* const* out,
                             uint8_t* out_index, uint64_t* recovered, rfec_host_timing* timing);

/* Kernel timing for benches: the next kernel this thread launches through the
 * batched API (rfec_encode_batch, rfec_recover_batch[_out], rfec_zero_tails,
 * rfec_wire_frame_fec / _seg, rfec_wire_encode_fec, rfec_wire_encode_send, rfec_wire_encode_send_shapes, rfec_wire_parse, rfec_wire_regroup[_index], rfec_recover_indexed_out, rfec_recover_indexed_matrix_out, rfec_recover_indexed_matrix_wide_out, rfec_recover_indexed_rows_wide_out, rfec_recover_indexed_shapes_out, rfec_recover_indexed_window_out, rfec_recover_indexed_window_each_out, rfec_recover_deliver, rfec_recover_deliver_each) records its own start / stop on these hipEvent_t (either may be NULL), via
 * hipExtLaunchKernel; the setting is consumed by that launch.
 * rfec_timing_launches: kernels launched by this thread since the last
 * rfec_timing_events (a call that launched more than one kernel timed only
 * its first). */
int rfec_timing_events(void* start, void* stop);
uint32_t rfec_timing_launches(void);

/* Zero bytes [data_size, stride) of every shard (establishes the layout
 * invariant for callers that cannot guarantee it). */
int rfec_zero_tails(uint32_t groups, uint32_t k, uint32_t stride, uint8_t* shards,
                    const rfec_hdr* hdr, void* stream);

/* ------------------------------------------------------------------------ */
/* Wire codec, batched on the device: the SIM_FEC / SIM_SEG datagrams of     */
/* sim_encode_msg / sim_decode_header + sim_decode_msg (sim_proto.c:13-146,  */
/* sim_proto.inl:83-179, 244-307), big-endian fields (cf_stream.c:328-414),  */
/* CRC32 trailer (cf_crc32.c:56-68, seed 0x0e3dfc0a, sim_proto.c:11).        */
/*                                                                          */
/* A datagram is: ver, mid, uid (6 B, sim_proto.c:13-18) | body | crc32 of   */
/* everything before it, big-endian (sim_proto.c:92-94).  Datagram slots are */
/* [N][dstride] bytes, dstride a multiple of 16 in [64, 2048]; lengths are   */
/* u16 per slot.  Bytes of a slot beyond its length are written as 0.        */
/* ------------------------------------------------------------------------ */
#define RFEC_WIRE_VER 0x01        /* protocol_ver, sim_proto.h:39 */
#define RFEC_WIRE_SEG 0x17        /* SIM_SEG, sim_proto.h:17-29 */
#define RFEC_WIRE_FEC 0x1c        /* SIM_FEC, sim_proto.h:34 */
#define RFEC_WIRE_MIN_MID 0x10    /* MIN_MSG_ID */
#define RFEC_WIRE_MAX_MID 0x1d    /* MAX_MSG_ID (accepted, sim_session.c:594) */
#define RFEC_WIRE_CRC_SEED 0x0e3dfc0au
#define RFEC_WIRE_FEC_OVERHEAD 49 /* 6 + 17 + 20 + 2 + 4 bytes around fec_data */
#define RFEC_WIRE_MAX_DSTRIDE 2048

/* Per-datagram fields of a SIM_FEC the FEC engine does not produce: the
 * session uid (sim_proto.c:13-18) and the sim_fec_t stamps of the sender
 * (flex_fec_sender.c:176-181, 220-225; sim_sender.c:112-113). */
typedef struct {
    uint32_t uid;
    uint32_t base_id;
    uint32_t send_ts;
    uint16_t fec_id;
    uint16_t count;
    uint16_t transport_seq;
    uint8_t row, col, index;
    uint8_t reserved;
    uint8_t pad[2];
} rfec_fec_stamp; /* 24 bytes */

/* Per-datagram fields of a SIM_SEG beyond rfec_hdr (sim_sender.c:88-91, 335-351). */
typedef struct {
    uint32_t uid;
    uint16_t fec_id;
    uint16_t send_ts;
    uint16_t transport_seq;
    uint8_t remb;
    uint8_t reserved;
} rfec_seg_stamp; /* 12 bytes */

/* SIM_FEC datagrams (sim_sender.c:118-119 + sim_fec_encode,
 * sim_proto.inl:270-285) of `count` parity slots laid out as rfec_encode_batch
 * wrote them (slot g*n + l = line l of group g): datagram i -> dgram slot i.
 * `status` may be NULL; a slot with status -1 gets length 0 (the reference
 * never emits that parity).  `order` may be NULL; otherwise datagram i is
 * written to slot order[i] of dgram / dlen (a permutation).  Needs
 * fec_size <= capacity <= stride and dstride >= capacity + 49.
 * Alignment (RFEC_EINVAL for less): 16 bytes parity and dgram, 4 bytes meta,
 * stamps and order, 2 bytes fec_size and dlen (status: any).  Datagram
 * slots whose stride is a multiple of 128 bytes (1,280 for 1,200-byte
 * payloads) are written in whole 128-byte lines: 0.60 of HBM peak against
 * 0.52 for the minimal 16-byte multiples, whose slot edges split lines
 * (DESIGN.md §4). */
int rfec_wire_frame_fec(uint32_t count, uint32_t stride, uint32_t capacity, const uint8_t* parity,
                        const rfec_hdr* meta, const uint16_t* fec_size, const int8_t* status,
                        const rfec_fec_stamp* stamps, const uint32_t* order, uint32_t dstride, uint8_t* dgram,
                        uint16_t* dlen, void* stream);

/* SIM_SEG datagrams (sim_sender.c:96-97 + sim_segment_encode,
 * sim_proto.inl:83-125; header widths follow the value ranges) of `count`
 * segments: shards [count][stride], hdr [count]; `order` as for
 * rfec_wire_frame_fec.  Needs data_size <= capacity <= stride and
 * dstride >= capacity + 36.
 * Alignment (RFEC_EINVAL for less): 16 bytes shards and dgram, 4 bytes hdr,
 * stamps and order, 2 bytes dlen. */
int rfec_wire_frame_seg(uint32_t count, uint32_t stride, uint32_t capacity, const uint8_t* shards,
                        const rfec_hdr* hdr, const rfec_seg_stamp* stamps, const uint32_t* order, uint32_t dstride,
                        uint8_t* dgram, uint16_t* dlen, void* stream);

/* A batch of groups straight into its SIM_FEC datagrams, the encode and the
 * framing in one kernel: with count = groups * plan->n_lines, dgram
 * [count][dstride] and dlen [count] are byte for byte what
 *   rfec_encode_batch(plan, groups, stride, capacity, shards, hdr, parity,
 *                     meta, fec_size, status, ...), then
 *   rfec_wire_frame_fec(count, stride, capacity, parity, meta, fec_size,
 *                       status, stamps, order, dstride, dgram, dlen, ...)
 * write on the same inputs (datagram g*n + l = line l of group g; a line
 * whose flex_fec_generate would fail -- fewer than 2 members, or a member's
 * data_size above capacity -- gets length 0 and a zero slot; `order` as for
 * rfec_wire_frame_fec), without the parity, meta, fec_size and status arrays:
 * every member is read once per line it sits on and nothing but the datagram
 * slots and lengths is written ("Slot tails": the shards' bytes from 16 * CD
 * to the stride are not read).  k <= RFEC_MAX_K_ENCODE.
 * Alignment (RFEC_EINVAL for less): 16 bytes shards and dgram, 4 bytes hdr,
 * stamps and order, 2 bytes dlen.
 * Datagram slots up to 1,280 bytes only (both SIM_VIDEO_SIZEs fit: 1,000 + 49
 * and 1,200 + 49): dstride > 1280 returns RFEC_EINVAL -- use the two calls
 * above.  A batch of any size is taken (shards beyond 4 GiB are split over
 * several launches); with `order`, count * dstride must stay below 4 GiB
 * (RFEC_EINVAL).  RFEC_WIRE_ENCODE_CHUNK_GROUPS (environment, for tests) caps
 * the groups per launch. */
int rfec_wire_encode_fec(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                         const uint8_t* shards, const rfec_hdr* hdr, const rfec_fec_stamp* stamps,
                         const uint32_t* order, uint32_t dstride, uint8_t* dgram, uint16_t* dlen, void* stream);

/* Every datagram of a batch of groups in one kernel: the k SIM_SEG datagrams
 * of each group and its n_lines SIM_FEC datagrams.  With ns = groups * plan->k
 * and nf = groups * plan->n_lines, seg_dgram [ns][dstride] / seg_dlen [ns] are
 * byte for byte what
 *   rfec_wire_frame_seg(ns, stride, capacity, shards, hdr, seg_stamps,
 *                       seg_order, dstride, seg_dgram, seg_dlen, ...)
 * writes and fec_dgram [nf][dstride] / fec_dlen [nf] what
 *   rfec_wire_encode_fec(plan, groups, stride, capacity, shards, hdr,
 *                        fec_stamps, fec_order, dstride, fec_dgram, fec_dlen, ...)
 * writes on the same inputs, whole slots (a segment whose data_size exceeds
 * capacity gets length 0 and a zero slot; a line is refused as there).  Every
 * member is read once per line it sits on -- on a rows-only plan once, for its
 * SIM_SEG and its row's parity together -- and a member that sits on no line
 * once, for its SIM_SEG ("Slot tails": the shards' bytes from 16 * CD to the
 * stride are not read).  Any plan with k <= RFEC_MAX_K_ENCODE; with
 * n_lines == 0 only the segments are framed and the four SIM_FEC pointers are
 * not touched (they may be NULL).  groups == 0 touches nothing: every pointer
 * may be NULL.  Each order may be NULL, as for rfec_wire_frame_fec.
 * The four outputs must not overlap each other or any input (not checked).
 * Alignment (RFEC_EINVAL for less): 16 bytes shards, seg_dgram and fec_dgram,
 * 4 bytes hdr, both stamp arrays and both orders, 2 bytes seg_dlen and
 * fec_dlen.  dstride >= capacity + 49 (the SIM_FEC overhead, which covers the
 * SIM_SEG's 36) and dstride <= 1280: above that RFEC_EINVAL -- use
 * rfec_wire_frame_seg + rfec_wire_encode_fec.  A batch of any size is taken
 * (split over several launches so that every launch keeps 32-bit buffer
 * offsets); with seg_order, ns * dstride must stay below 4 GiB, with
 * fec_order nf * dstride (RFEC_EINVAL).  RFEC_WIRE_ENCODE_CHUNK_GROUPS caps
 * the groups per launch as for rfec_wire_encode_fec. */
int rfec_wire_encode_send(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                          const uint8_t* shards, const rfec_hdr* hdr,
                          const rfec_seg_stamp* seg_stamps, const uint32_t* seg_order,
                          uint8_t* seg_dgram, uint16_t* seg_dlen,
                          const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order,
                          uint8_t* fec_dgram, uint16_t* fec_dlen,
                          uint32_t dstride, void* stream);

/* rfec_wire_encode_send over a send window whose groups have different shapes
 * (the flex sender closes a group per frame, so k and row x col follow the
 * frame size), in one launch: the sender-side counterpart of
 * rfec_wire_regroup_shapes.  The window's member rows lie in shards / hdr /
 * seg_stamps [n_rows] in any layout, its SIM_FEC stamps in fec_stamps [n_fec];
 * group g of the call is a descriptor. */
#define RFEC_SEND_MAX_SHAPES 32
#define RFEC_SEND_MAX_LINES  512   /* sum of n_lines over the call's plans */

typedef struct {          /* one group of the window; DEVICE array */
    uint32_t row0;        /* first member row: members are rows row0 .. row0 + k_p - 1 */
    uint32_t line0;       /* first SIM_FEC index: lines are line0 .. line0 + n_p - 1 */
    uint32_t shape;       /* index into plans; >= n_plans: the group is skipped */
    uint32_t reserved;    /* 0 */
} rfec_send_group;        /* 16 bytes */

/* Equivalence.  For every group g that is not skipped, with p = group[g].shape,
 * k_p = plans[p].k and n_p = plans[p].n_lines, the call writes byte for byte
 * what rfec_wire_encode_send(&plans[p], 1, ...) writes for the same rows,
 * headers and stamps, whole slots: the SIM_SEG slots and lengths of rows
 * row0 .. row0 + k_p - 1 (seg_dgram / seg_dlen [n_rows]) and the SIM_FEC slots
 * and lengths of lines line0 .. line0 + n_p - 1 (fec_dgram / fec_dlen
 * [n_fec]); with the orders, through seg_order[row0 + i] / fec_order[line0 + l]
 * (permutations of [0, n_rows) / [0, n_fec), each may be NULL).  So a segment
 * above `capacity` gets length 0 and a zero slot, a refused line likewise, and
 * a plan without lines frames only segments.
 * Skipped groups.  A group is skipped when shape >= n_plans, or
 * row0 + k_p > n_rows, or line0 + n_p > n_fec: it reads nothing and writes
 * nothing (the device cannot return RFEC_EINVAL for a bad descriptor, so this
 * is the rule).  Rows and lines that no group covers keep what their slots
 * held.
 * Overlap.  Overlapping row or line ranges of two groups are the caller's
 * fault: the result for those slots is unspecified; nothing is accessed outside
 * the buffers.
 * Descriptor order is free and need not follow row order.  A wave takes four
 * consecutive descriptors: four of one shape run at rfec_wire_encode_send's
 * rate, a mixed four costs one pass per distinct shape.  So a caller who sorts
 * the descriptors by shape -- not the rows -- gets full lanes and still gets
 * the datagrams in send order.
 * "Slot tails": the shards' bytes from 16 * CD to the stride are not read.
 * One launch, always: the call is not split, so the 32-bit buffer offsets are
 * argument checks (RFEC_EINVAL, "split the window"): (n_rows + 4) * stride +
 * 1280, n_rows * 20, n_rows * dstride, n_fec * dstride, n_fec * 24 and
 * groups * 16 must each stay below 0xFFFFFFF0.
 * Checked before any runtime call (RFEC_EINVAL, rfec_last_error names the
 * argument): plans (NULL, n_plans in [1, RFEC_SEND_MAX_SHAPES], every plan as
 * for rfec_wire_encode_send with k <= RFEC_MAX_K_ENCODE, the sum of n_lines
 * <= RFEC_SEND_MAX_LINES); stride / capacity / dstride as for
 * rfec_wire_encode_send (dstride >= capacity + 49, dstride <= 1280); NULL
 * pointers (the four SIM_FEC pointers may be NULL when n_fec == 0, each order
 * always); alignment: 16 bytes shards, seg_dgram and fec_dgram, 4 bytes group,
 * hdr, both stamp arrays and both orders, 2 bytes seg_dlen and fec_dlen.
 * groups == 0 touches nothing: every pointer but plans may be NULL.
 * The call allocates nothing, copies nothing from the host (the plans travel
 * in the kernel's argument block), does not synchronise and launches only on
 * `stream`.  The four outputs must not overlap each other or any input (not
 * checked). */
int rfec_wire_encode_send_shapes(const rfec_plan* plans, uint32_t n_plans,       /* host */
                                 uint32_t groups, const rfec_send_group* group,  /* device [groups] */
                                 uint32_t n_rows, uint32_t n_fec,
                                 uint32_t stride, uint32_t capacity,
                                 const uint8_t* shards, const rfec_hdr* hdr,     /* [n_rows] */
                                 const rfec_seg_stamp* seg_stamps, const uint32_t* seg_order,
                                 uint8_t* seg_dgram, uint16_t* seg_dlen,         /* [n_rows] */
                                 const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order,
                                 uint8_t* fec_dgram, uint16_t* fec_dlen,         /* [n_fec] */
                                 uint32_t dstride, void* stream);

/* Parse status (rfec_wire_rec.status). */
#define RFEC_WIRE_OK 0         /* SIM_SEG / SIM_FEC decoded (a SEG with a bad data length decodes
                                  with data_size 0, as sim_segment_decode does) */
#define RFEC_WIRE_OTHER 1      /* valid control message (CONNECT, PING, ...): header only */
#define RFEC_WIRE_EBADCRC (-1) /* sim_decode_header: CRC mismatch, or shorter than the trailer */
#define RFEC_WIRE_EMID (-2)    /* mid outside [MIN_MSG_ID, MAX_MSG_ID] (sim_session.c:594) */
#define RFEC_WIRE_EBODY (-3)   /* sim_fec_decode returned -1 (fec_data length invalid) */

/* One parsed datagram.  SIM_SEG: hdr = the segment's header (seq=packet_id,
 * fid, ts=timestamp, index, total, ftype, payload_type, size=data_size),
 * fec_id, send_ts (u16 widened), transport_seq, remb.  SIM_FEC: hdr = fec_meta,
 * the sim_fec_t fields, data_size = fec_data_size. */
typedef struct {
    int8_t status;
    uint8_t ver, mid, remb;
    uint32_t uid;
    rfec_hdr hdr;
    uint32_t base_id;
    uint32_t send_ts;
    uint16_t fec_id;
    uint16_t count;
    uint16_t transport_seq;
    uint16_t data_size;
    uint8_t row, col, index;
    uint8_t reserved[17];
} rfec_wire_rec; /* 64 bytes */

/* Decode N received datagrams (sim_session.c:587-653 -> sim_decode_header,
 * sim_decode_msg) into recs [N] and their payloads into slots [N][stride]
 * (zero beyond data_size: the layout rfec_recover_batch expects).  `capacity`
 * plays SIM_VIDEO_SIZE in the length checks (cf_stream.c:342-355,
 * sim_proto.inl:301-305); capacity <= stride.
 * Alignment (RFEC_EINVAL for less): 16 bytes dgram, recs and payload, 2 bytes
 * dlen. */
int rfec_wire_parse(uint32_t n, uint32_t dstride, const uint8_t* dgram, const uint16_t* dlen,
                    uint32_t stride, uint32_t capacity, rfec_wire_rec* recs, uint8_t* payload,
                    void* stream);

/*
 * Parsed datagrams into recover's batch layout, on the device: recs [n] and
 * payload [n][stride] as rfec_wire_parse wrote them, in arrival order, placed
 * into shards [G][k][stride], hdr, present, parity [G][n_l][stride], meta,
 * fec_size and parity_present of rfec_encode_batch / rfec_recover_batch for
 * `plan` and `groups` (k = plan->k, n_l = plan->n_lines).  For a receiver of
 * groups of one shape: one call per shape, the records of other shapes and
 * windows get ESHAPE / EWINDOW.  Group g has k + n_l slots: slot s < k is
 * member s, slot k + l is parity line l.  All pointers are device pointers.
 *
 * One call is one closed window, and stateless: the timing rules of sim_fec.c
 * -- the 3 s parity drop (:148), max_ts, eviction (:209-241) -- do not apply
 * and are not modelled; nor is arrival order beyond "the first wins" (the
 * reference delivers a segment recovered before its own late arrival; here
 * that segment is present).  rfec_rx_recover and the receiver session replay
 * those.
 *
 * The placement rule, independent of how the device schedules the work:
 *  1. ENOTFEC.  A record with status != RFEC_WIRE_OK, or whose mid is neither
 *     SIM_SEG nor SIM_FEC, gets ENOTFEC.
 *  2. Group index.  fec_id == 0 gets EWINDOW.  Otherwise
 *     g = fec_id >= fec_id0 ? fec_id - fec_id0 : fec_id + 65535 - fec_id0, the
 *     sender's succession 65535 -> 1, skipping 0 (flex_fec_sender.c:241-243);
 *     g >= groups gets EWINDOW.
 *  3. Shape.  A SIM_FEC is shape-accepted when count == k, row == plan->row,
 *     col == plan->col, index == plan->line[l].index for some l (the first
 *     such l) and data_size <= capacity; otherwise it gets ESHAPE.
 *  4. Anchor.  The group's anchor is its shape-accepted SIM_FEC with the
 *     lowest arrival index; base_id[g] is the anchor's base_id (sim_fec.c:
 *     152-163, flex_fec_receiver.c:69-78, :255-266).  With no anchor,
 *     base_id[g] is 0.
 *  5. Parity base.  A shape-accepted SIM_FEC whose base_id differs from
 *     base_id[g] gets EBASE.  The others contend for slot k + l.
 *  6. Segments.  A SIM_SEG in a group with no anchor gets ENOPARITY.
 *     Otherwise i = (uint32_t)(hdr.seq - base_id[g]); i >= k gets EBASE;
 *     otherwise the segment contends for slot i.
 *  7. Winner.  The lowest arrival index wins a slot (first-arrival dedupe,
 *     sim_fec.c:180-182, flex_fec_receiver.c:222-224, :258-260).  For the
 *     winner d, slot_of[d] = g (k + n_l) + s.  Every other contender gets
 *     EDUP.  src_of[g (k + n_l) + s] is the winner's arrival index, or
 *     RFEC_REGROUP_NONE for an empty slot.
 *
 * Written: every element of slot_of [n] (the slot, or the negative code),
 * src_of [G (k + n_l)], base_id [G], present [G][2] (bit i: member slot i is
 * filled) and parity_present [G] (bit l: parity slot l is filled).  For each
 * filled member slot, bytes [0, 16 CD) of its shards row, copied from the
 * winner's payload row (CD: "Slot tails"), and hdr[g k + i] = rec.hdr; for each
 * filled parity slot, bytes [0, 16 CD) of its parity row, meta = rec.hdr and
 * fec_size = rec.data_size.  Nothing else: the rows and records of empty slots
 * and bytes [16 CD, stride) of every row keep what they held, the inputs are
 * untouched.  The outputs are then a complete input of rfec_recover_batch /
 * rfec_recover_batch_out on the same buffers (recs, payload and src_of tell
 * where every slot came from).
 *
 * Checked before any runtime call (RFEC_EINVAL): the plan (k <= RFEC_MAX_K),
 * stride a multiple of 16 (at most 2,048, as rfec_wire_parse's),
 * capacity <= stride, fec_id0 != 0, groups <= 65535, n <= 0x7FFFFFFF, NULL
 * pointers, and alignment: 16 bytes recs, payload, shards, parity; 8 bytes
 * present, parity_present; 4 bytes hdr, meta, base_id, src_of, slot_of; 2
 * bytes fec_size.  groups == 0 touches nothing: every pointer may be NULL.
 * n == 0 writes the masks (0), src_of (NONE) and base_id (0); recs, payload
 * and slot_of may then be NULL.  n_lines == 0 is legal (parity, meta and
 * fec_size may be NULL): no group has an anchor, so every candidate segment
 * gets ENOPARITY.  The outputs must not overlap each other or the inputs (not
 * checked).  The call allocates nothing, does not synchronise, launches only
 * on `stream` and addresses rows with 64 bits (n * stride may pass 4 GiB).
 * base_id holds intermediate values until the call's last kernel has run.
 */
#define RFEC_REGROUP_NONE      0xFFFFFFFFu
#define RFEC_REGROUP_ENOTFEC   (-1)
#define RFEC_REGROUP_EWINDOW   (-2)
#define RFEC_REGROUP_ESHAPE    (-3)
#define RFEC_REGROUP_ENOPARITY (-4)
#define RFEC_REGROUP_EBASE     (-5)
#define RFEC_REGROUP_EDUP      (-6)

int rfec_wire_regroup(const rfec_plan* plan, uint32_t groups, uint16_t fec_id0,
                      uint32_t n, const rfec_wire_rec* recs, const uint8_t* payload,
                      uint32_t stride, uint32_t capacity,
                      uint8_t* shards, rfec_hdr* hdr, uint64_t* present,
                      uint8_t* parity, rfec_hdr* meta, uint16_t* fec_size, uint64_t* parity_present,
                      uint32_t* base_id, uint32_t* src_of, int32_t* slot_of, void* stream);

/*
 * rfec_wire_regroup without the row copy: the same records, the same placement
 * rule (`capacity` is rule 3's bound) and the same four launches, and exactly
 * what rfec_wire_regroup writes to hdr, present, meta, fec_size,
 * parity_present, base_id, src_of and slot_of -- no payload row is read or
 * written, so payload, stride, shards and parity are not arguments.  src_of is
 * then the slot map of rfec_recover_indexed_out over rfec_wire_parse's payload
 * rows where they lie.  The argument checks (no stride), the optional pointers
 * (n == 0: recs, slot_of; n_lines == 0: meta, fec_size), groups == 0 and the
 * guarantees (no allocation, no synchronisation, launches only on `stream`)
 * are rfec_wire_regroup's.
 */
int rfec_wire_regroup_index(const rfec_plan* plan, uint32_t groups, uint16_t fec_id0,
                            uint32_t n, const rfec_wire_rec* recs, uint32_t capacity,
                            rfec_hdr* hdr, uint64_t* present, rfec_hdr* meta, uint16_t* fec_size,
                            uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                            int32_t* slot_of, void* stream);

/*
 * rfec_wire_regroup_index for a window whose groups have different shapes: the
 * flex sender closes a group per frame, so k, and with it row x col
 * (rfec_num_packets), follows the frame size.  One call classifies every group
 * of the closed window by the shape of its first accepted parity, the rule by
 * which the reference creates a flex (sim_fec.c:152-163,
 * flex_fec_receiver.c:69-78), compacts the groups of each shape in window order
 * and writes, per shape, one dense section of exactly the tables
 * rfec_recover_indexed_out reads.  plans [n_plans] and sections [n_plans] are
 * host arrays (sections: of device pointers), section p belonging to plans[p]
 * (k_p = plans[p].k, n_p = plans[p].n_lines); everything else is a device
 * pointer.  More than RFEC_REGROUP_MAX_SHAPES shapes need more than one call
 * over the window.
 *
 * The rule, independent of how the device schedules the work:
 *  1. ENOTFEC, EWINDOW.  Rules 1 and 2 of rfec_wire_regroup, unchanged: the
 *     group index g counts from fec_id0 in the succession 65535 -> 1, and
 *     fec_id == 0 gets EWINDOW.
 *  2. Shape.  A SIM_FEC is accepted by plan p when count == plans[p].k, row and
 *     col equal the plan's, index == plans[p].line[l].index for some l (the
 *     first such l) and data_size <= capacity.  The plans of one call differ
 *     pairwise in (k, row, col), so at most one p accepts a record.  A SIM_FEC
 *     accepted by no plan gets ESHAPE.
 *  3. Anchor and shape of a group.  anchor_of[g] is the lowest arrival index
 *     among the accepted SIM_FECs of group g, of any plan, or
 *     RFEC_REGROUP_NONE.  shape_of[g] is the plan that accepts the anchor, or
 *     0xFF.  The group's base_id is the anchor's.  A SIM_FEC accepted by a plan
 *     other than shape_of[g] gets ESHAPE: the reference's flex keeps the
 *     geometry of its first parity.
 *  4. Rank.  rank_of[g] is the number of g' < g with shape_of[g'] ==
 *     shape_of[g] -- window order, not arrival order -- or RFEC_REGROUP_NONE
 *     for a group with no anchor.  counts[p] is the number of groups of shape
 *     p in the window; it is not clamped to cap.
 *  5. Parity base and segments.  Rules 5 and 6 of rfec_wire_regroup with k and
 *     the lines of plans[shape_of[g]]: EBASE, ENOPARITY, and the slot s (member
 *     i: s = i; parity line l: s = k_p + l).
 *  6. Room.  A record that reaches contention in a group with rank_of[g] >=
 *     sections[shape_of[g]].cap gets EFULL and contends for nothing.  A caller
 *     sees the overflow as counts[p] > cap.
 *  7. Winner.  The lowest arrival index wins a slot, as rule 7 of
 *     rfec_wire_regroup.  For the winner d, slot_of[d] = rank_of[g] (k_p + n_p)
 *     + s within the section of p = shape_of[g].  Every other contender gets
 *     EDUP.  The section's src_of holds the winner's arrival index, or
 *     RFEC_REGROUP_NONE.
 *
 * Written: every element of shape_of [G], rank_of [G], anchor_of [G], counts
 * [n_plans] and slot_of [n].  In section p, for every row c < cap: present
 * [c][2], parity_present [c], base_id [c], group_of [c] (the window index g of
 * the group with rank c) and the row's k_p + n_p entries of src_of; rows with
 * c >= counts[p] are empty: masks 0, base_id 0, group_of and src_of
 * RFEC_REGROUP_NONE.  For each filled slot, hdr / meta / fec_size from the
 * winner's record, as rfec_wire_regroup_index writes them.  Nothing else: the
 * records of empty slots keep what they held, recs is untouched.  Section p
 * with groups = min(counts[p], cap) -- or cap, without reading counts back: the
 * trailing rows decode to nothing -- is then a complete input of
 * rfec_recover_indexed_out over rfec_wire_parse's payload rows.
 *
 * Equivalence: for every g with shape_of[g] == p and rank_of[g] < cap, row
 * rank_of[g] of section p (hdr, present, meta, fec_size, parity_present,
 * base_id, src_of) equals row g of what rfec_wire_regroup_index(&plans[p], ...)
 * writes for the same records, and every record of such a group has the same
 * slot_of, rebased by (g - rank_of[g]) (k_p + n_p) when it is not negative.
 *
 * Checked before any runtime call (RFEC_EINVAL, rfec_last_error names the
 * argument): each plan (k <= RFEC_MAX_K), n_plans in [1,
 * RFEC_REGROUP_MAX_SHAPES], no two plans with one (k, row, col), fec_id0 != 0,
 * groups <= 65535, n <= 0x7FFFFFFF, cap <= groups, NULL pointers (a section
 * with cap == 0 may hold NULLs; a plan with n_lines == 0 may have NULL meta /
 * fec_size, its section stays empty; recs and slot_of may be NULL when n == 0)
 * and alignment: 16 bytes recs; 8 bytes present, parity_present; 4 bytes hdr,
 * meta, base_id, src_of, group_of, rank_of, anchor_of, counts, slot_of; 2 bytes
 * fec_size.  groups == 0 touches nothing: every pointer but plans may be NULL.
 * The buffers must not overlap (not checked).  The call allocates nothing,
 * copies nothing from the host (plans and sections travel as kernel arguments,
 * which is what bounds RFEC_REGROUP_MAX_SHAPES), does not synchronise and
 * launches only on `stream`: six launches (four with n == 0), none waiting on
 * another workgroup.  slot_of holds intermediate values until the last one has
 * run.
 */
#define RFEC_REGROUP_MAX_SHAPES 32
#define RFEC_REGROUP_EFULL (-7)

typedef struct {            /* host struct of DEVICE pointers: one shape's section */
    uint32_t cap;           /* groups the section has room for, 0..groups */
    uint32_t reserved;
    rfec_hdr* hdr;              /* [cap][k]      */
    uint64_t* present;          /* [cap][2]      */
    rfec_hdr* meta;             /* [cap][n_l]    */
    uint16_t* fec_size;         /* [cap][n_l]    */
    uint64_t* parity_present;   /* [cap]         */
    uint32_t* base_id;          /* [cap]         */
    uint32_t* src_of;           /* [cap (k+n_l)] */
    uint32_t* group_of;         /* [cap]: the window index g of the section's row */
} rfec_regroup_section;

int rfec_wire_regroup_shapes(const rfec_plan* plans, uint32_t n_plans,
                             const rfec_regroup_section* sections,
                             uint32_t groups, uint16_t fec_id0,
                             uint32_t n, const rfec_wire_rec* recs, uint32_t capacity,
                             uint8_t* shape_of, uint32_t* rank_of, uint32_t* anchor_of,
                             uint32_t* counts, int32_t* slot_of, void* stream);

/*
 * The census of a parsed window, on the device: which shapes occur in it, in
 * window order, and how many groups each has -- what rfec_wire_regroup_shapes
 * and the decodes behind it take as host arguments (plans, cap, groups), and
 * what a receiver cannot know ahead: the flex sender picks (k, row, col) per
 * frame, and the shape reaches the receiver only inside the SIM_FEC records.
 * The census is 576 bytes: one small copy to the host replaces the copy of the
 * n 64-byte records, or sections sized for the worst case and a read-back of
 * counts.  From it the host builds the plans (rfec_plan_from_key of each
 * shape), sizes every section exactly (cap = groups[p] = shape[p].groups) and
 * runs the rest of the chain with no further read-back.
 *
 * (fec_id0, groups) is the caller's admission window, as rfec_wire_regroup_shapes
 * takes it: the next expected id, and up to 65,535 groups.  recs [n], census,
 * anchor_of [groups] and key_of [groups] are device pointers.
 *
 * The rule, independent of how the device schedules the work:
 *  1. ENOTFEC, EWINDOW.  Rules 1 and 2 of rfec_wire_regroup, unchanged.
 *     n_notfec and n_window count those records.
 *  2. In-window records.  An in-window SIM_SEG counts in n_seg.  An in-window
 *     SIM_FEC is accepted when its key (count, row, col) is plannable
 *     (rfec_plan_from_key), its index is the index of a line of the key's plan
 *     and data_size <= capacity.  Accepted records count in n_fec, the others
 *     in n_refused.
 *  3. Window extent.  g_first is the least group index over all in-window
 *     records, or RFEC_REGROUP_NONE with none; g_end is 1 + the greatest, or 0
 *     with none.  The caller tightens (fec_id0, groups) with them.
 *  4. Anchor and key.  anchor_of[g] is the lowest arrival index among group
 *     g's accepted SIM_FECs, or RFEC_REGROUP_NONE.  key_of[g] is
 *     k | row << 8 | col << 16 of that record, or RFEC_REGROUP_NONE.  anchored
 *     is the number of groups with an anchor.
 *  5. Shapes.  The distinct keys among key_of are ordered by first_g, the least
 *     g with that key -- window order, not arrival order.  n_shapes =
 *     min(distinct, RFEC_CENSUS_MAX_SHAPES); shape[i] for i < n_shapes are the
 *     keys with the least first_g, in that order; shape[i].groups is the number
 *     of groups with that key.  other_groups counts the anchored groups whose
 *     key is not listed: other_groups > 0 means more than 32 shapes (key_of
 *     lets a caller run a second pass).  Entries i >= n_shapes and all reserved
 *     words are 0: the whole struct is written on every call.
 *
 * Equivalence.  When other_groups == 0, take plans[i] =
 * rfec_plan_from_key(shape[i]) in any order.  rfec_wire_regroup_shapes on the
 * same (groups, fec_id0, n, recs, capacity) then writes the same anchor_of; its
 * shape_of[g] is the index of key_of[g]'s plan, and 0xFF where the key is NONE;
 * its counts[p] equals the groups of plans[p]'s shape.  (The regroup's accepted
 * set is a subset of the census's, and every census anchor's key is among the
 * plans: so each group's lowest accepted arrival is the same record.)
 *
 * Checked before any runtime call (RFEC_EINVAL, rfec_last_error names the
 * argument): fec_id0 != 0, groups <= 65535, n <= 0x7FFFFFFF, capacity <= 65535,
 * NULL pointers (recs may be NULL when n == 0) and alignment: 16 bytes recs and
 * census, 4 bytes anchor_of and key_of.  groups == 0 touches nothing: every
 * pointer may be NULL.  n == 0 writes the empty census (g_first NONE, all else
 * 0) and both arrays (NONE).  The buffers must not overlap (not checked).  The
 * call allocates nothing, copies nothing from the host, does not synchronise
 * and launches only on `stream`: at most four launches (three with n == 0),
 * none waiting on another workgroup.  census holds intermediate values until
 * the last one has run.
 */
#define RFEC_CENSUS_MAX_SHAPES 32
typedef struct {
    uint16_t k;           /* the key: SIM_FEC count, row, col */
    uint8_t row, col;
    uint32_t groups;      /* groups of the window with this key */
    uint32_t first_g;     /* the least of them */
    uint32_t reserved;
} rfec_census_shape; /* 16 bytes */
typedef struct {
    uint32_t n_shapes, other_groups, anchored, g_first, g_end;
    uint32_t n_seg, n_fec, n_refused, n_notfec, n_window, reserved[6];
    rfec_census_shape shape[RFEC_CENSUS_MAX_SHAPES];
} rfec_window_census; /* 64 + 512 bytes, DEVICE */

int rfec_wire_window_census(uint32_t groups, uint16_t fec_id0,
                            uint32_t n, const rfec_wire_rec* recs, uint32_t capacity,
                            rfec_window_census* census,
                            uint32_t* anchor_of, uint32_t* key_of, void* stream);

/*
 * rfec_recover_batch_out with shards and parity replaced by a row pool and a
 * slot map: rows [n_rows][stride], src_of [G (k + n_l)] u32; slot s < k of
 * group g is member s, slot k + l is parity line l, and slot s of group g is
 * row src_of[g (k + n_l) + s] of the pool.  This is the layout
 * rfec_wire_regroup[_index] writes, though any producer may write it.  hdr,
 * present, meta, fec_size and parity_present are the batch layout's.
 *
 * Consistency is the caller's to keep: a member or parity whose present /
 * parity_present bit is set has src_of < n_rows.  The entries of absent slots
 * are never read.  The kernels clamp a row index to n_rows - 1 before they use
 * it: a broken map gives unspecified bytes for that group, never a read
 * outside rows.
 *
 * Results: recovered, out_index, out_hdr, and out_shards over [0, 16 CD) of
 * every slot whose out_index is not 0xFF, are byte for byte what
 * rfec_recover_batch_out writes on the batch obtained by copying row
 * src_of[slot] into each present slot -- for any plan with k <= RFEC_MAX_K,
 * cascades included, and under every kernel selection (rfec_set_tuning).
 * "Slot tails": bytes [16 CD, stride) of every out slot are not written and
 * bytes [16 CD, stride) of the rows are not read; every input is untouched.
 * Row addresses are 64-bit (n_rows * stride may pass 4 GiB).
 *
 * workspace: rfec_recover_workspace_size(plan, G) bytes, 16-byte aligned, as
 * for rfec_recover_batch_out (row layouts of rows of <= 4 segments, k <= 64,
 * run in one launch and leave it alone).
 *
 * Checked before any runtime call (RFEC_EINVAL, rfec_last_error names the
 * argument): the plan, stride a positive multiple of 16, capacity <= stride,
 * per_group in [1, k], groups * per_group * CD < 2^31, NULL pointers (rows may
 * be NULL when n_rows == 0; meta and fec_size when n_lines == 0), and
 * alignment: 16 bytes rows, out_shards and workspace; 8 bytes present,
 * parity_present and recovered; 4 bytes src_of, hdr, meta and out_hdr; 2 bytes
 * fec_size.  groups == 0 touches nothing: every pointer may be NULL.  The
 * call allocates nothing, does not synchronise and launches only on `stream`.
 */
int rfec_recover_indexed_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                             const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                             const rfec_hdr* hdr, const uint64_t* present,
                             const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                             uint64_t* recovered, uint32_t per_group,
                             uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index,
                             void* workspace, void* stream);

/*
 * rfec_recover_indexed_out without `workspace`, for the sender's full row +
 * column plans of k = 6..16 (the plans of rfec_plan_from_fraction's matrix mode
 * with both layers, every frame of 6..16 segments): one launch, nothing
 * staged.  rfec_packed_matrix_stride(plan, 1) != 0 is the predicate; any other
 * plan gets RFEC_EINVAL, and its caller uses rfec_recover_indexed_out, which
 * takes every plan and keeps its own kernel selection for these.
 *
 * Results: recovered, out_index, out_hdr, and out_shards over [0, 16 CD) of
 * every slot whose out_index is not 0xFF, are byte for byte what
 * rfec_recover_indexed_out writes for the same arguments (so what
 * rfec_recover_batch_out writes on the gathered batch: cascades, lines the
 * header checks refuse and the rescheduling around them included).  Bytes
 * [16 CD, stride) of every out slot are not written; payload bytes of a slot
 * whose out_index is 0xFF are unspecified (as for
 * rfec_recover_packed_matrix_out).  Every input is untouched; the map's
 * consistency rule, the clamp of a row index to n_rows - 1 and the 64-bit row
 * addresses are rfec_recover_indexed_out's.  With n_rows == 0 no row is read:
 * recovered, out_hdr and out_index are still written.  rfec_set_tuning does
 * not reach this call.
 *
 * Checked before any runtime call (RFEC_EINVAL), in rfec_recover_indexed_out's
 * order: the plan and its shape, stride a positive multiple of 16,
 * capacity <= stride, per_group in [1, k], groups * per_group * CD < 2^31,
 * NULL pointers (rows may be NULL when n_rows == 0), alignment: 16 bytes rows
 * and out_shards; 8 bytes present, parity_present and recovered; 4 bytes
 * src_of, hdr, meta and out_hdr; 2 bytes fec_size, and groups * 4 < 2^32.
 * groups == 0 touches nothing: every pointer may be NULL.  The call allocates
 * nothing, does not synchronise and launches only on `stream`.
 */
int rfec_recover_indexed_matrix_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                    const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                    const rfec_hdr* hdr, const uint64_t* present,
                                    const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                                    uint64_t* recovered, uint32_t per_group,
                                    uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index, void* stream);

/*
 * rfec_recover_indexed_matrix_out for the sender's full row + column plan of
 * any k in [6, RFEC_MAX_K]: the plan rfec_plan_from_fraction(k, pf >= 10,
 * RFEC_LAYER_ROWS | RFEC_LAYER_COLS) returns -- rows of `col` consecutive
 * segments, then the `col` columns, col from rfec_num_packets (3..12; a last
 * row of one segment has no line: up to 23 lines of up to 12 members).  That
 * is every frame of 6 or more segments once protect_fraction >= 10, an
 * I-frame of 100 segments included.  One launch, no workspace, nothing
 * staged; the shape is taken at run time (one kernel for every k, masks of
 * two 64-bit words).  Any other plan gets RFEC_EINVAL -- a full matrix in rows
 * of another width, rows or columns alone, a row layout, a strip plan -- and
 * its caller uses rfec_recover_indexed_out, which takes every plan.
 * rfec_recover_indexed_matrix_out (k = 6..16, the shape compiled in) and
 * rfec_recover_indexed_shapes_out keep their own answers.
 *
 * Results: recovered (both words: k may pass 64), out_index, out_hdr, and
 * out_shards over [0, 16 CD) of every slot whose out_index is not 0xFF, are
 * byte for byte what rfec_recover_indexed_out writes for the same arguments
 * (so what rfec_recover_batch_out writes on the gathered batch: cascades of
 * any depth, lines the header checks refuse and the rescheduling around them,
 * and dense mode's rule that only erased segments of rank < per_group are
 * targets, included).  Bytes [16 CD, stride) of every out slot are not
 * written; payload bytes of a slot whose out_index is 0xFF are unspecified.
 * Every input is untouched; the map's consistency rule, the clamp of a row
 * index to n_rows - 1 and the 64-bit row addresses are
 * rfec_recover_indexed_out's.  With n_rows == 0 no row is read: recovered,
 * out_hdr and out_index are still written.  rfec_set_tuning does not reach
 * this call.
 *
 * Checked before any runtime call (RFEC_EINVAL), in
 * rfec_recover_indexed_matrix_out's order: the plan and its shape, stride a
 * positive multiple of 16, capacity <= stride, per_group in [1, k],
 * groups * per_group * CD < 2^31, NULL pointers (rows may be NULL when
 * n_rows == 0), alignment: 16 bytes rows and out_shards; 8 bytes present,
 * parity_present and recovered; 4 bytes src_of, hdr, meta and out_hdr; 2 bytes
 * fec_size (one checker lane per group: their count is bounded with the
 * groups).  groups == 0 touches nothing: every pointer may be NULL.  The call allocates
 * nothing, does not synchronise and launches only on `stream`; no workgroup
 * waits on another.
 */
int rfec_recover_indexed_matrix_wide_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                         const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                         const rfec_hdr* hdr, const uint64_t* present,
                                         const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                                         uint64_t* recovered, uint32_t per_group,
                                         uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index, void* stream);

/*
 * rfec_recover_indexed_out without `workspace` and in one launch for a row
 * layout of any width: with col = line[0].count >= 2, line l is (first l col,
 * stride 1, count min(col, k - l col)) for l = 0 .. n_lines - 1, and n_lines
 * is ceil(k / col) -- or one less when the last row has one segment: that row
 * has no line and its segment is never recovered.  k in [2, RFEC_MAX_K], col
 * up to 128, up to RFEC_MAX_LINES rows.  That is every strip-mode plan of
 * rfec_plan_from_fraction (protect_fraction < 10, and every group of fewer
 * than 6 segments: one parity over the frame, or rows of ceil(k / lines)
 * segments), rfec_plan_matrix(k, row, col, RFEC_LAYER_ROWS), the rows-only
 * layer of a full matrix, and the row layouts rfec_recover_indexed_out itself
 * decodes in one launch.  The shape is taken at run time (one kernel, masks of
 * two 64-bit words).  Any other plan gets RFEC_EINVAL -- a full matrix, columns
 * alone, a plan without lines, rows with a gap or of unequal width, a
 * hand-made plan -- and its caller uses rfec_recover_indexed_out, which takes
 * every plan.  rfec_recover_indexed_out, rfec_recover_indexed_shapes_out and
 * both matrix entries keep their own answers and kernels for every plan.
 *
 * Results: recovered (both words), out_index, out_hdr, and out_shards over
 * [0, 16 CD) of every slot whose out_index is not 0xFF, are byte for byte what
 * rfec_recover_indexed_out writes for the same arguments (dense mode's rule
 * that only erased segments of rank < per_group are targets, and lines the
 * header checks refuse, included).  Bytes [16 CD, stride) of every out slot
 * are not written; payload bytes of a slot whose out_index is 0xFF are
 * unspecified.  Every input is untouched; the map's consistency rule, the
 * clamp of a row index to n_rows - 1 and the 64-bit row addresses are
 * rfec_recover_indexed_out's.  With n_rows == 0 no row is read: recovered,
 * out_hdr and out_index are still written.  rfec_set_tuning does not reach
 * this call.
 *
 * In a window of several shapes (rfec_wire_regroup_shapes) a section with such
 * a plan that rfec_recover_indexed_shapes_out does not take is decoded as a
 * wide matrix section is: groups[p] = 0 in the window decode, this call on the
 * section's tables with its outputs at row first[p] of the same dense arrays
 * (recovered + 2 first[p], out_index + first[p] per_group, ...), then
 * rfec_recover_deliver with groups[p] = min(counts[p], cap).
 *
 * Checked before any runtime call (RFEC_EINVAL), in rfec_recover_indexed_out's
 * order and with its messages: the plan and, right after it, its shape;
 * stride a positive multiple of 16, capacity <= stride, per_group in [1, k],
 * groups * per_group * CD < 2^31, NULL pointers (rows may be NULL when
 * n_rows == 0; meta and fec_size are never optional), alignment: 16 bytes rows
 * and out_shards; 8 bytes present, parity_present and recovered; 4 bytes
 * src_of, hdr, meta and out_hdr; 2 bytes fec_size, and last the header lanes'
 * bound, groups * 2^ceil(log2(max(n_lines, 2))) < 2^32.  groups == 0 touches
 * nothing: every pointer may be NULL.  The call allocates nothing, does not
 * synchronise and launches only on `stream`; no workgroup waits on another.
 */
int rfec_recover_indexed_rows_wide_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                       const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                       const rfec_hdr* hdr, const uint64_t* present,
                                       const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                                       uint64_t* recovered, uint32_t per_group,
                                       uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index, void* stream);

/*
 * The decode behind rfec_wire_regroup_shapes: the sections of a closed window
 * of several shapes in one launch and without a workspace, so that the receive
 * chain of such a window is parse -> one regroup -> one decode.  plans
 * [n_plans] and sections [n_plans] are the host arrays given to
 * rfec_wire_regroup_shapes; of section p the call reads hdr, present, meta,
 * fec_size, parity_present and src_of (base_id and group_of are ignored).
 * groups [n_plans] is a host array, groups[p] <= sections[p].cap the number of
 * rows of section p to decode -- min(counts[p], cap) for a caller that read the
 * counts back -- or NULL for sections[p].cap: the trailing empty rows then
 * decode to nothing.
 *
 * Output rows are dense over the call: row c of section p is output row
 * o = first[p] + c, first[p] the sum of groups[q] over q < p.  recovered is
 * indexed by o; out_index, out_hdr and out_shards by (o, e) with one
 * per_group = E for the whole call.
 *
 * Plans accepted for a section with groups[p] > 0: the sender's full row +
 * column plans of k = 6..16 (rfec_packed_matrix_stride(plan, 1) != 0), and the
 * row layouts rfec_recover_indexed_out runs in one launch (rows of <= 4
 * segments, k <= 64).  Any other plan gets RFEC_EINVAL, rfec_last_error names
 * its index: give that section groups[p] == 0 and decode it with
 * rfec_recover_indexed_out (an I-frame's strip plan, say).  A section with
 * groups[p] == 0 only has to hold a valid plan; its tables may be NULL.
 *
 * Results: for every p with groups[p] > 0, output rows [first[p], first[p] +
 * groups[p]) hold byte for byte what rfec_recover_indexed_matrix_out (a full
 * matrix) or rfec_recover_indexed_out (a row layout) writes into arrays of its
 * own for (&plans[p], groups[p], stride, capacity, rows, n_rows, section p's
 * tables, per_group): recovered, out_index, out_hdr, and out_shards over
 * [0, 16 CD) of every slot whose out_index is not 0xFF.  Bytes [16 CD, stride)
 * of every out slot are not written; the payload of a 0xFF slot is
 * unspecified; every input is untouched.  The clamp of a row index to
 * n_rows - 1, the 64-bit row addresses and n_rows == 0 (no row is read:
 * recovered, out_hdr and out_index are still written) are those calls'.
 * rfec_set_tuning does not reach this call.
 *
 * Checked before any runtime call (RFEC_EINVAL), in rfec_recover_indexed_out's
 * order: n_plans in [1, RFEC_RECOVER_MAX_SHAPES], each plan and, with
 * groups[p] > 0, its shape; stride a positive multiple of 16,
 * capacity <= stride, per_group in [1, the least k of the sections with
 * groups]; per section groups[p] <= cap, groups[p] * per_group * CD < 2^31 and
 * the header lanes' bound of its own call (groups * 4, or groups x the least
 * power of two >= n_lines, < 2^32); the launch's blocks (the sections' own
 * grids, end to end) < 2^31 and its output rows < 2^32.  All groups[p] == 0
 * touches nothing: every other pointer may be NULL.  Then NULL pointers (rows
 * may be NULL when n_rows == 0) and alignment: 16 bytes rows and out_shards;
 * 8 bytes present, parity_present and recovered; 4 bytes src_of, hdr, meta and
 * out_hdr; 2 bytes fec_size.  The call allocates nothing, copies nothing from
 * the host (the sections travel as kernel arguments), does not synchronise and
 * makes exactly one launch on `stream`.
 */
#define RFEC_RECOVER_MAX_SHAPES RFEC_REGROUP_MAX_SHAPES
int rfec_recover_indexed_shapes_out(const rfec_plan* plans, uint32_t n_plans,
                                    const rfec_regroup_section* sections,
                                    const uint32_t* groups, /* host [n_plans], or NULL: sections[p].cap */
                                    uint32_t stride, uint32_t capacity,
                                    const uint8_t* rows, uint32_t n_rows,
                                    uint64_t* recovered, uint32_t per_group,
                                    uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index,
                                    void* stream);

/*
 * rfec_recover_indexed_shapes_out for a window of ANY of the planner's shapes:
 * the same arguments, the same output numbering (row c of section p is output
 * row first[p] + c, one per_group for the call, recovered indexed by output
 * row) and the same NULL rules, so rfec_recover_deliver takes its outputs
 * unchanged, with the same plans, sections, groups and per_group.  No section
 * of a planner plan has to sit in the window with groups[p] = 0 and take a
 * launch of its own: strip-mode frames and the frames above 16 segments decode
 * in the window's one launch.
 *
 * The family of a section with groups[p] > 0 is the first of these that holds:
 *  1. the sender's full row + column plan of k = 6..16
 *     (rfec_packed_matrix_stride(plan, 1) != 0), decoded as
 *     rfec_recover_indexed_matrix_out decodes it (the shape compiled in);
 *  2. a row layout of rows of <= 4 segments with k <= 64, as
 *     rfec_recover_indexed_out decodes it in one launch;
 *  3. the sender's full row + column plan of k = 17..128 in rows of
 *     rfec_num_packets' col (at most 23 lines), as
 *     rfec_recover_indexed_matrix_wide_out decodes it;
 *  4. any other row layout -- k in [2, RFEC_MAX_K], rows of 2..128, a last row
 *     of one segment without a line -- as rfec_recover_indexed_rows_wide_out
 *     decodes it.
 * Any other plan gets RFEC_EINVAL and rfec_last_error names plans[p]: a
 * hand-made plan, columns alone, rows with a gap or of unequal width, a plan
 * without lines.  Give that section groups[p] == 0 and decode it with
 * rfec_recover_indexed_out.  A section with groups[p] == 0 only has to hold a
 * valid plan; its tables may be NULL.
 *
 * Results: for every p with groups[p] > 0, output rows [first[p], first[p] +
 * groups[p]) hold byte for byte what its family's single-shape call (above)
 * writes into arrays of its own for (&plans[p], groups[p], stride, capacity,
 * rows, n_rows, section p's tables, per_group): recovered, out_index, out_hdr,
 * and out_shards over [0, 16 CD) of every slot whose out_index is not 0xFF.
 * Bytes [16 CD, stride) of every out slot are not written; the payload of a
 * 0xFF slot is unspecified; every input is untouched.  The clamp of a row
 * index to n_rows - 1, the 64-bit row addresses and n_rows == 0 (only the
 * header and checker lanes run, no row is read: recovered, out_hdr and
 * out_index are still written) are those calls'.  A wide section keeps its
 * table pitch: k + n_lines map words and n_lines meta records per group.
 * rfec_set_tuning does not reach this call.
 *
 * Checked before any runtime call (RFEC_EINVAL), in
 * rfec_recover_indexed_shapes_out's order: plans not NULL, n_plans in [1,
 * RFEC_RECOVER_MAX_SHAPES], sections not NULL, each plan and, with
 * groups[p] > 0, its family; stride a positive multiple of 16,
 * capacity <= stride, per_group in [1, the least k of the sections with
 * groups]; per section groups[p] <= cap, groups[p] * per_group * CD < 2^31 and
 * the header lanes' bound of its family (1: groups * 4 < 2^32; 2 and 4:
 * groups * 2^ceil(log2(max(n_lines, 2))) < 2^32; 3: one checker lane per group,
 * no further bound); the launch's blocks (the sections' own grids, end to end)
 * < 2^31 and its output rows < 2^32.  All groups[p] == 0 touches nothing:
 * every other pointer may be NULL.  Then NULL pointers (rows may be NULL when
 * n_rows == 0) and alignment: 16 bytes rows and out_shards; 8 bytes present,
 * parity_present and recovered; 4 bytes src_of, hdr, meta and out_hdr; 2 bytes
 * fec_size.  The call uses no workspace, allocates nothing, copies nothing from
 * the host (the sections travel as kernel arguments), does not synchronise and
 * makes exactly one launch on `stream`; no workgroup waits on another.
 */
int rfec_recover_indexed_window_out(const rfec_plan* plans, uint32_t n_plans,
                                    const rfec_regroup_section* sections,
                                    const uint32_t* groups, /* host [n_plans], or NULL: sections[p].cap */
                                    uint32_t stride, uint32_t capacity,
                                    const uint8_t* rows, uint32_t n_rows,
                                    uint64_t* recovered, uint32_t per_group,
                                    uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index,
                                    void* stream);

/*
 * rfec_recover_indexed_window_out with an out-slot count per section: the same
 * arguments with per_group a host array [n_plans], so that a window's small
 * groups do not bound what its large ones deliver.  With one per_group for the
 * call a window of 1 x 3 P-frame groups and a 100-segment I-frame gets 3 out
 * slots per group; here the I-frame's section takes per_group[p] = 10 (or up
 * to 100) beside the P-frames' 3.  The families, the NULL rules and what a
 * section with groups[p] == 0 may hold are rfec_recover_indexed_window_out's.
 *
 * Output numbering ("the ragged numbering"): first[p] is the sum of groups[q]
 * over q < p and slot_first[p] the sum of groups[q] * per_group[q] over q < p,
 * groups[p] = sections[p].cap when groups is NULL.  Row c of section p is
 * output row o = first[p] + c; recovered is indexed by o.  out_index, out_hdr
 * and out_shards are indexed by slot: out slot e < per_group[p] of that row is
 * slot slot_first[p] + c * per_group[p] + e.  Section p's rows have
 * per_group[p] slots each and the sections' slots are packed end to end:
 * S = slot_first[n_plans] = rfec_recover_window_slots(...) slots in all, so
 * out_index holds S bytes, out_hdr S records and out_shards S * stride bytes.
 *
 * Results: for every p with groups[p] > 0, rows [first[p], first[p] +
 * groups[p]) of recovered and slots [slot_first[p], slot_first[p + 1]) of
 * out_index, out_hdr and out_shards hold byte for byte what its family's
 * single-shape call writes into arrays of its own for (&plans[p], groups[p],
 * stride, capacity, rows, n_rows, section p's tables, per_group[p]): recovered,
 * out_index, out_hdr, and out_shards over [0, 16 CD) of every slot whose
 * out_index is not 0xFF.  "Slot tails": bytes [16 CD, stride) of every out slot
 * are not written; the payload of a 0xFF slot is unspecified; every input is
 * untouched.  Everything else rfec_recover_indexed_window_out says of its
 * results holds.  With every per_group[p] equal to E the outputs are byte for
 * byte those of rfec_recover_indexed_window_out(..., E, ...).
 *
 * Checked before any runtime call (RFEC_EINVAL), in
 * rfec_recover_indexed_window_out's order with per_group where it stands
 * there: plans not NULL, n_plans in [1, RFEC_RECOVER_MAX_SHAPES], sections not
 * NULL, each plan and, with groups[p] > 0, its family; stride a positive
 * multiple of 16, capacity <= stride; per_group not NULL and, for each section
 * with groups[p] > 0, per_group[p] in [1, plans[p].k] (rfec_last_error names
 * per_group[p]; per_group[p] of a section with groups[p] == 0 is not read for
 * range and may be anything, 0 included); per section groups[p] <= cap,
 * groups[p] * per_group[p] * CD < 2^31 and the header lanes' bound of its
 * family; the launch's blocks < 2^31, its output rows < 2^32 and S * CD <
 * 2^31.  All groups[p] == 0 touches nothing: every other pointer may be NULL.
 * Then NULL pointers and alignment as rfec_recover_indexed_window_out.  The
 * call uses no workspace, allocates nothing, copies nothing from the host (the
 * sections and their per_group travel as kernel arguments), does not
 * synchronise and makes exactly one launch on `stream`; no workgroup waits on
 * another.
 */
int rfec_recover_indexed_window_each_out(const rfec_plan* plans, uint32_t n_plans,
                                         const rfec_regroup_section* sections,
                                         const uint32_t* groups, /* host [n_plans], or NULL: sections[p].cap */
                                         uint32_t stride, uint32_t capacity,
                                         const uint8_t* rows, uint32_t n_rows,
                                         uint64_t* recovered,
                                         const uint32_t* per_group, /* host [n_plans] */
                                         uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index,
                                         void* stream);

/* S of the ragged numbering: the sum over p of groups[p] * per_group[p]
 * (groups[p] = sections[p].cap when groups is NULL; per_group[p] of a section
 * with groups[p] == 0 is not read), the out slots the three slot arrays of
 * rfec_recover_indexed_window_each_out hold.  Host arithmetic only: no device,
 * no checks; 0 when per_group is NULL, or groups and sections both. */
uint64_t rfec_recover_window_slots(const rfec_regroup_section* sections, uint32_t n_plans,
                                   const uint32_t* groups, const uint32_t* per_group);

/* One delivered segment, as every call that hands recovered segments back
 * writes it (rfec_recover_deliver below; rfec_rx_recover, the rx session). */
typedef struct {
    rfec_hdr hdr;     /* recovered header (flex_fec_xor.c:64-85) */
    uint16_t fec_id;  /* out_seg->fec_id = fec->fec_id (:101) */
    uint16_t reserved;
} rfec_rx_seg; /* 24 bytes */

/*
 * The last stage of a closed window's receive chain: what
 * rfec_recover_indexed_shapes_out wrote -- dense over the sections, per_group
 * out slots a row, a hole wherever out_index is 0xFF, the rows in section order
 * -- as the list a receiver uses: one rfec_rx_seg and one payload row per
 * recovered segment, in window order.  plans, sections, groups and per_group
 * are exactly the arguments given to rfec_recover_indexed_shapes_out (of
 * section p the call reads cap and group_of); window_groups = G, fec_id0,
 * shape_of and rank_of are those of rfec_wire_regroup_shapes.  plans, sections
 * and groups are host arrays, everything else is a device pointer.
 *
 * The rule, independent of how the device schedules the work:
 *  1. Output rows.  first[p] is the sum of groups[q] over q < p, groups[p] =
 *     sections[p].cap when groups is NULL; R = first[n_plans].  This is the
 *     decode's own numbering.
 *  2. Decoded groups.  Window group g in [0, G) is decoded when p = shape_of[g]
 *     < n_plans and c = rank_of[g] < groups[p]; its output row is o(g) =
 *     first[p] + c.  Any other group delivers nothing: RFEC_REGROUP_NONE, shape
 *     0xFF, a rank past the rows decoded, a section left to the generic call
 *     (groups[p] == 0).
 *  3. Counts.  n_g is the number of e < per_group with out_index[o(g) per_group
 *     + e] != 0xFF; 0 for a group that is not decoded.
 *  4. Prefix.  first_of[g] is the sum of n_g' over g' < g, first_of[G] the
 *     total T, and *n_out = T.  Neither is clamped to max_out, as counts is not
 *     clamped to cap: a caller sees overflow as *n_out > max_out.
 *  5. Order.  Window order and, within a group, out-slot order (ascending
 *     segment index): out slot e of group g is entry j = first_of[g] + the
 *     number of e' < e with out_index[o(g) per_group + e'] != 0xFF.
 *  6. Entries.  For j < max_out: seg[j].hdr is out_hdr[o per_group + e],
 *     seg[j].fec_id = ((fec_id0 - 1 + g) % 65535) + 1 (the regroup's succession
 *     65535 -> 1), seg[j].reserved = 0, and row j of seg_payload over [0, 16 CD)
 *     is the out slot's bytes.  "Slot tails": bytes [16 CD, stride) of a
 *     delivered row are not written.
 *  7. Overflow.  Entries with j >= max_out are not written anywhere.
 *
 * Written: first_of [G + 1], *n_out, and seg / seg_payload as rule 6 says.
 * Nothing else: entries at and past min(T, max_out) keep what they held, every
 * input is untouched, and the payload bytes of an out slot whose out_index is
 * 0xFF are not read.  Consistency of the tables is the caller's to keep: as
 * rfec_wire_regroup_shapes writes them, sections[p].group_of[rank_of[g]] == g
 * for every decoded g.  The delivery goes by group_of: a value >= G there
 * (RFEC_REGROUP_NONE, as the rows past counts[p] hold) delivers nothing, and a
 * row that disagrees with rank_of gives unspecified entries -- never a read or
 * a write outside the arrays as sized here.
 *
 * workspace: rfec_recover_deliver_workspace_size(G) bytes (a multiple of 16),
 * 16-byte aligned; it needs no initialisation.
 *
 * Checked before any runtime call (RFEC_EINVAL, rfec_last_error names the
 * argument), in this order: plans not NULL; n_plans in [1,
 * RFEC_RECOVER_MAX_SHAPES]; sections not NULL (but see window_groups == 0);
 * each plan; window_groups <= 65535; fec_id0 != 0; stride a positive multiple
 * of 16; capacity <= stride; per_group >= 1; groups[p] <= sections[p].cap;
 * R * per_group * CD < 2^31 and R < 2^32.  window_groups == 0 then touches
 * nothing: every pointer but plans may be NULL.  Then NULL pointers (seg and
 * seg_payload may be NULL when max_out == 0; out_shards, out_hdr and out_index
 * when R == 0; sections[p].group_of when groups[p] == 0) and alignment: 16
 * bytes out_shards, seg_payload and workspace; 4 bytes out_hdr, seg, rank_of,
 * first_of, n_out and every group_of.  With G > 0 and R == 0 the call still
 * writes first_of[0..G] = 0 and *n_out = 0.  The buffers must not overlap (not
 * checked).  The call allocates nothing, copies nothing from the host (the
 * sections' group_of pointers and first[] travel as kernel arguments), does
 * not synchronise and launches only on `stream`: three launches, two when
 * window_groups <= 256, none waiting on another workgroup.
 */
size_t rfec_recover_deliver_workspace_size(uint32_t window_groups);

int rfec_recover_deliver(const rfec_plan* plans, uint32_t n_plans,            /* host */
                         const rfec_regroup_section* sections,                /* host, of device pointers: group_of is read */
                         const uint32_t* groups,                              /* host [n_plans] or NULL: sections[p].cap */
                         uint32_t window_groups, uint16_t fec_id0,
                         const uint8_t* shape_of, const uint32_t* rank_of,    /* device [G], as regroup_shapes wrote them */
                         uint32_t stride, uint32_t capacity, uint32_t per_group,
                         const uint8_t* out_shards, const rfec_hdr* out_hdr,  /* device: the decode's outputs */
                         const uint8_t* out_index,
                         uint32_t max_out,
                         rfec_rx_seg* seg, uint8_t* seg_payload,              /* device [max_out], [max_out][stride] */
                         uint32_t* first_of,                                  /* device [G + 1] */
                         uint32_t* n_out,                                     /* device [1] */
                         void* workspace, void* stream);

/*
 * rfec_recover_deliver over what rfec_recover_indexed_window_each_out wrote:
 * the same arguments with per_group the host array [n_plans] given to that
 * decode, the slot arrays in the ragged numbering (slot_first[p] the sum of
 * groups[q] * per_group[q] over q < p; out slot e < per_group[p] of row c of
 * section p is slot slot_first[p] + c * per_group[p] + e).  The rule is
 * rfec_recover_deliver's except in two places:
 *  3. Counts.  For a decoded group g with p = shape_of[g] and c = rank_of[g],
 *     n_g is the number of e < per_group[p] with out_index[slot_first[p] +
 *     c * per_group[p] + e] != 0xFF.
 *  5, 6. Order and entries read that slot: out slot e of group g is entry j =
 *     first_of[g] + the number of e' < e whose slot is not 0xFF, seg[j].hdr is
 *     out_hdr of the slot and row j of seg_payload over [0, 16 CD) its bytes.
 * With every per_group[p] equal to E all six outputs are byte for byte those of
 * rfec_recover_deliver(..., E, ...).  What is written, the tables' consistency,
 * the workspace (rfec_recover_deliver_workspace_size(G)) and the launches
 * (three, two when window_groups <= 256) are rfec_recover_deliver's.
 *
 * Checked before any runtime call (RFEC_EINVAL), in rfec_recover_deliver's
 * order with per_group where it stands there: per_group not NULL and
 * per_group[p] >= 1 for every section with groups[p] > 0 (rfec_last_error
 * names per_group[p]; not read where groups[p] == 0, nor when sections is NULL
 * with window_groups == 0); groups[p] <= sections[p].cap; S * CD < 2^31 with
 * S = slot_first[n_plans], and R < 2^32.  Everything else as
 * rfec_recover_deliver.
 */
int rfec_recover_deliver_each(const rfec_plan* plans, uint32_t n_plans,       /* host */
                              const rfec_regroup_section* sections,           /* host, of device pointers: group_of is read */
                              const uint32_t* groups,                         /* host [n_plans] or NULL: sections[p].cap */
                              uint32_t window_groups, uint16_t fec_id0,
                              const uint8_t* shape_of, const uint32_t* rank_of, /* device [G], as regroup_shapes wrote them */
                              uint32_t stride, uint32_t capacity,
                              const uint32_t* per_group,                      /* host [n_plans] */
                              const uint8_t* out_shards, const rfec_hdr* out_hdr, /* device: the decode's outputs */
                              const uint8_t* out_index,
                              uint32_t max_out,
                              rfec_rx_seg* seg, uint8_t* seg_payload,         /* device [max_out], [max_out][stride] */
                              uint32_t* first_of,                             /* device [G + 1] */
                              uint32_t* n_out,                                /* device [1] */
                              void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Sender staging: sim_sender_put (sim_sender.c:306-377) with sim_split_frame */
/* (:254-284) and the flex sender's grouping (flex_fec_sender.c:49-78,       */
/* 137-245), as a plan over a batch of frames, then frame bytes copied       */
/* straight into pinned structure-of-arrays slots.                          */
/* ------------------------------------------------------------------------ */
typedef struct {
    const uint8_t* data;      /* frame bytes (host) */
    uint32_t size;
    uint8_t payload_type, ftype;
    uint8_t protect_fraction; /* s->loss_fraction when the frame is put (sim_sender.c:291) */
    uint8_t reserved;
    int64_t now_ms;           /* GET_SYS_MS() during sim_sender_put */
} rfec_frame;

/* The sim_sender_t / flex_fec_sender_t fields that shape segments and groups. */
typedef struct {
    uint32_t packet_id_seed, send_id_seed, frame_id_seed;
    int64_t first_ts;   /* -1 before the first frame (sim_sender.c:333-338) */
    int64_t fec_ts;     /* flex->fec_ts (0 = unset) */
    uint32_t base_id;   /* flex->base_id */
    int32_t open_seg;   /* the open group's first segment, relative to the next batch (<= 0) */
    uint16_t fec_id;    /* flex->fec_id, starts at 1, skips 0 */
    uint16_t segs_count;
    int32_t first;      /* flex->first */
    uint32_t transport_seq_seed; /* sender->transport_seq_seed (sim_sender.c:90, 112), u16 on the wire */
} rfec_sender_state;

/* One segment the sender builds (sim_sender.c:341-363). */
typedef struct {
    uint32_t frame;        /* index into the frame batch */
    uint32_t offset;       /* byte offset in the frame */
    uint32_t packet_id, send_id, fid, timestamp;
    uint16_t index, total, data_size, fec_id;
    uint8_t ftype, payload_type;
    uint8_t reserved[2];
    int32_t group;         /* group index in this batch, -1 if never protected */
} rfec_seg_plan; /* 40 bytes */

/* One protected group: a flex_fec_sender_update that emitted parities. */
typedef struct {
    int32_t first_seg;     /* segments [first_seg, first_seg + count) of the batch; negative:
                              the first -first_seg were planned by the previous call */
    uint16_t count, fec_id;
    uint32_t base_id;      /* smallest packet_id of the group */
    uint32_t fec_send_id0; /* send ids of its parities: fec_send_id0 + line (sim_sender.c:295-296) */
    uint32_t fec_ts;       /* now_ms - first_ts when it closed (sim_sender.c:299) */
    uint8_t protect_fraction, n_lines;
    uint8_t reserved[2];
} rfec_group_plan; /* 24 bytes */

void rfec_sender_init(rfec_sender_state* st);
/* Plans `n` frames: the segments sim_sender_put builds (segs, at most
 * max_segs) and the groups flex_fec_sender_update protects (groups, at most
 * max_groups), in creation order; `st` carries the sender across calls.  A
 * group still open after the last frame stays open in `st` (its segments have
 * group -2); the call that closes it reports a negative first_seg.
 * seg_size = the sender's SIM_VIDEO_SIZE.  Returns RFEC_OK, or RFEC_EINVAL
 * when an output array is too small (nothing is consumed then). */
int rfec_sender_plan(rfec_sender_state* st, const rfec_frame* frames, uint32_t n, uint32_t seg_size,
                     rfec_seg_plan* segs, uint32_t max_segs, uint32_t* n_segs, rfec_group_plan* groups,
                     uint32_t max_groups, uint32_t* n_groups);

/* Frames in, datagrams out (host memory both ends): rfec_sender_plan, the
 * frame bytes copied once into pinned structure-of-arrays slots (groups of
 * one shape contiguous, so each shape is one rfec_encode_batch), one H2D
 * copy, the encode, rfec_wire_frame_seg / _fec, one D2H copy per datagram
 * kind.  Datagrams come out in creation order: seg_dgram[i] is segs[i]'s
 * SIM_SEG, fec_dgram holds the parities group by group, lines in plan order.
 * transport_seq counts datagrams in creation order (a group's parities right
 * after the segment that closed it); send_ts is that of an immediate send
 * (sim_sender.c:88-91, 111-113).  seg_size is this library's SIM_VIDEO_SIZE;
 * the segments of a group still open at the end are kept (per calling thread)
 * and encoded by the call that closes it.
 *
 * Zero copy (RFEC_HOST_ZEROCOPY not "0"): when every frame's bytes lie inside
 * one rfec_pinned_alloc block, the device reads the segments out of the frames
 * itself (no host copy into the staging slots, no bulk H2D: h2d_us is then the
 * tables' copy and the device's reads); when the four datagram outputs lie in
 * such blocks, the framing writes the datagrams there (no D2H; the writes fall
 * in kernel_us).  report->zero_copy: bit 0 input, bit 1 output. */
typedef struct {
    uint32_t n_segs, n_groups, n_parities, n_shapes;
    double plan_us, stage_us, h2d_us, kernel_us, d2h_us, total_us;
    uint32_t zero_copy, reserved;
} rfec_send_report;

int rfec_host_send_frames(rfec_sender_state* st, const rfec_frame* frames, uint32_t n_frames, uint32_t uid,
                          rfec_seg_plan* segs, uint32_t max_segs, rfec_group_plan* groups, uint32_t max_groups,
                          uint32_t dstride, uint8_t* seg_dgram, uint16_t* seg_dlen, uint8_t* fec_dgram,
                          uint16_t* fec_dlen, uint32_t max_parities, rfec_send_report* report);

/* ------------------------------------------------------------------------ */
/* Receiver ingestion: the receiver-side FEC of one session over a batch of */
/* parsed datagrams in arrival order (sim_receiver_put / _put_fec,          */
/* sim_receiver.c:780-838 -> sim_fec_put_segment / sim_fec_put_fec_packet,  */
/* sim_fec.c:104-207 -> flex receiver, flex_fec_receiver.c:69-280).         */
/* The control plane replays the reference event by event over the 64-byte  */
/* records on the host: first-arrival dedupe, max_ts (raised by recovered   */
/* segments too), the 3000 ms parity drop (sim_fec.c:148), flex creation    */
/* from the first admitted parity and removal when full, and which line     */
/* recovers which packet and when (so a packet recovered before its own     */
/* late arrival is delivered, as the reference does).  The bytes stay on    */
/* the device: every group is peeled by rfec_recover_batch from its arrived */
/* members and registered parities, and the delivered rows are gathered.    */
/* Not modelled (counted in n_unmodelled, never delivered wrong): the       */
/* wall-clock eviction of sim_fec_evict, parity lines outside the sender's  */
/* row/column plan, geometries the planner cannot express (count > 128 or   */
/* row * col < count) and parities inconsistent with their members.         */
/* Output: the recovered segments, ascending packet_id.                     */
/* ------------------------------------------------------------------------ */
/* (rfec_rx_seg, the record of a delivered segment: above, at rfec_recover_deliver) */

typedef struct {
    uint32_t n_groups, n_shapes, n_recovered, n_fec_dropped, n_unmodelled, reserved;
    double host_us, h2d_us, kernel_us, d2h_us, total_us;
} rfec_rx_report;

/* recs / payload: DEVICE (rfec_wire_parse output), n records in arrival
 * order, payload rows of `stride` bytes.  max_ts: in/out
 * (sim_receiver_fec_t.max_ts).  out / out_payload: HOST, up to max_out
 * recovered segments (payload rows of `stride`, zero beyond data_size). */
int rfec_rx_recover(uint32_t n, const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride,
                    uint32_t capacity, uint32_t* max_ts, rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out,
                    uint32_t* n_out, rfec_rx_report* report, void* stream);

/* ------------------------------------------------------------------------ */
/* Batched UDP I/O: the datagram path of sim_session (sim_session.c:286-296 */
/* send, :321-364 receive loop) over posix.c's socket calls (su_udp_create  */
/* :133-170, su_udp_send :240-243, su_udp_recv :245-275), moved from one    */
/* sendto / select+recvfrom per datagram to sendmmsg / recvmmsg over the    */
/* [N][dstride] datagram slots the wire codec reads and writes.  Host-only  */
/* (no HIP); slot buffers are best pinned (hipHostMalloc) so the same block */
/* is the DMA source / target of the H2D / D2H copies.                      */
/* ------------------------------------------------------------------------ */
#define RFEC_EAGAIN (-4)           /* the socket stayed blocked for wait_ms */
#define RFEC_EIO (-5)              /* a socket call failed (errno in rfec_last_error) */
#define RFEC_UDP_SERVER 1u         /* SU_SERVER build: 1 MiB buffers, non-blocking (posix.c:135-160) */
#define RFEC_UDP_RECV_BYTES 1500u  /* receive buffer per datagram (sim_session.c:333) */
#define RFEC_UDP_MIN_DGRAM 6u      /* SIM_HEADER_SIZE: shorter datagrams are ignored (sim_session.c:339) */

typedef struct {
    uint32_t ip;   /* host byte order */
    uint16_t port; /* host byte order */
    uint16_t reserved;
} rfec_udp_addr;

typedef struct {
    uint64_t datagrams;  /* sent / received (kept) datagrams: s->scount / s->rcount */
    uint64_t bytes;      /* their bytes: s->sbandwidth / s->rbandwidth (sim_session.c:291, 343) */
    uint64_t skipped;    /* send: slots of length 0 (sim_session_network_send returns -1, :287-288) */
    uint64_t dropped;    /* recv: datagrams shorter than RFEC_UDP_MIN_DGRAM */
    uint64_t truncated;  /* recv: datagrams longer than the slot (MSG_TRUNC; their CRC then fails) */
    uint64_t syscalls;   /* sendmmsg / recvmmsg calls */
    uint64_t stalls;     /* send: waits for buffer space; recv: waits for data */
} rfec_udp_stats;

/* su_udp_create (posix.c:133-170): a UDP socket bound to ip:port (ip NULL or
 * "" = INADDR_ANY, port 0 = any), SO_SNDBUF / SO_RCVBUF = buf_bytes (0 = the
 * reference's 1 MiB with RFEC_UDP_SERVER, 128 KiB without), non-blocking
 * with RFEC_UDP_SERVER.  `bound` (may be NULL) receives the bound address. */
int rfec_udp_open(const char* ip, uint16_t port, unsigned flags, uint32_t buf_bytes, int* fd, rfec_udp_addr* bound);
void rfec_udp_close(int fd);
/* su_set_addr (posix.c:282-288) */
int rfec_udp_addr_of(const char* ip, uint16_t port, rfec_udp_addr* addr);

/* Sends slots [0, n) of dgram ([n][dstride], lengths dlen) to `peer` in slot
 * order, up to 1024 per sendmmsg; slots of length 0 are skipped.  When the
 * socket is full it waits for space up to wait_ms per stall (0: no wait) and
 * then returns RFEC_EAGAIN; *n_done (may be NULL) = slots consumed so far, so
 * the call can be resumed at that slot.  `st` (may be NULL) accumulates. */
int rfec_udp_send_batch(int fd, const rfec_udp_addr* peer, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                        const uint16_t* dlen, uint32_t wait_ms, uint32_t* n_done, rfec_udp_stats* st);

/* Receives up to `max` datagrams into consecutive slots of dgram ([max][dstride],
 * at most RFEC_UDP_RECV_BYTES of each datagram; slot bytes past the length
 * are not written) with their lengths in dlen and sources in `from` (may be
 * NULL).  Waits up to wait_ms for the first datagram, as su_udp_recv's select
 * does (0: no wait), then takes what is queued without waiting.  Datagrams
 * shorter than RFEC_UDP_MIN_DGRAM are dropped, as the session loop does.
 * *n = datagrams stored (0 after a quiet wait_ms: RFEC_OK). */
int rfec_udp_recv_batch(int fd, uint32_t max, uint32_t dstride, uint8_t* dgram, uint16_t* dlen, rfec_udp_addr* from,
                        uint32_t wait_ms, uint32_t* n, rfec_udp_stats* st);

/* Received datagrams in host memory -> recovered segments in host memory: one
 * H2D of the slots, rfec_wire_parse, rfec_rx_recover (arrival order = slot
 * order).  recs_out (HOST, may be NULL) receives the n parse records.  The
 * device staging is per calling thread.  rfec_rx_report.h2d_us includes the
 * datagram H2D; parse time is in kernel_us. */
int rfec_host_recv_datagrams(uint32_t n, uint32_t dstride, const uint8_t* dgram, const uint16_t* dlen,
                             uint32_t stride, uint32_t capacity, uint32_t* max_ts, rfec_wire_rec* recs_out,
                             rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                             rfec_rx_report* report);

/* Pinned host memory the device maps (hipHostMalloc / hipHostFree): datagram
 * slots, and struct pools for the zero-copy form of rfec_host_encode_groups /
 * rfec_host_recover_groups (each block is registered with its device address
 * until rfec_pinned_free). */
void* rfec_pinned_alloc(size_t bytes);
void rfec_pinned_free(void* p);

/* ------------------------------------------------------------------------ */
/* Receiver session: the receiver-side FEC state of one sim_session          */
/* (sim_receiver_fec_t, sim_fec.c) kept from one batch of datagrams to the   */
/* next -- open flex receivers, the segment cache, max_ts, first-arrival     */
/* dedupe -- with every cached segment's and registered parity's payload row */
/* held in HBM, so a group whose datagrams straddle batches recovers exactly */
/* as in one stream.  rfec_rx_session_evict is sim_fec_evict (sim_fec.c:    */
/* 209-241) for the caller's heartbeat (sim_receiver_timer, sim_receiver.c: */
/* 880, every >= 300 ms): stale or full flexes in fec_id order, cached      */
/* segments older than 6 s in packet_id order; then the held rows are       */
/* compacted.  Pushing a stream in any batches, with evictions between      */
/* batches, delivers what rfec_rx_recover delivers on the whole stream with */
/* the same evictions.  One session per calling thread at a time.           */
/* ------------------------------------------------------------------------ */
typedef struct rfec_rx_session rfec_rx_session;

typedef struct {
    uint32_t max_ts;          /* sim_receiver_fec_t.max_ts */
    uint32_t open_flexes;     /* skiplist_size(f->flexes) */
    uint32_t cached_segments; /* skiplist_size(f->segs_cache) */
    uint32_t records_held;    /* parsed records kept for open state */
    uint32_t rows_held;       /* HBM payload rows allocated */
    uint32_t pending;         /* datagrams of the batch the last _async call
                                 started: the records its next call writes */
    uint32_t threads;         /* control-plane shards (1: serial) */
    uint32_t batches_parallel;    /* batches replayed by the shards in parallel */
    uint32_t batches_serial;      /* batches replayed in arrival order */
    uint32_t batches_rolled_back; /* parallel replays undone (then replayed in order) */
    uint32_t reserved;
    /* host time, microseconds, summed over the session's batches: */
    double split_us;   /* the batch split over the shards (serial) */
    double replay_us;  /* the control plane's replay (the shards in parallel, or in order) */
    double verify_us;  /* the packet-id ownership check (parallel) */
    double tables_us;  /* the device tables of the delivering groups (rx_device, host part) */
    double compact_us; /* record / row compaction (rfec_rx_session_evict, and when the arena fills) */
} rfec_rx_session_info;

/* NULL on bad arguments (stride % 16, capacity > stride) or no memory.
 *
 * The control plane is sharded by fec_id over RFEC_RX_THREADS (default 8)
 * shards, each replayed in arrival order by its own thread: groups are
 * independent in the reference (sim_fec.c:141-207 keys a flex by fec_id).
 * Deliveries are those of the serial replay, always: a batch runs in parallel
 * only while every packet id belongs to one fec_id and no parity of the batch
 * can meet the 3 s drop (sim_fec.c:148) through max_ts; one that breaks either
 * is rolled back and replayed in arrival order (a packet id under two fec_ids
 * merges the shards into one for the rest of the session). */
rfec_rx_session* rfec_rx_session_create(uint32_t stride, uint32_t capacity);
/* Control-plane shards / threads (1..64) of a session that has not been
 * pushed to yet; 1 = the serial replay. */
int rfec_rx_session_set_threads(rfec_rx_session* s, uint32_t threads);
void rfec_rx_session_destroy(rfec_rx_session* s);
/* recs / payload: DEVICE (rfec_wire_parse output, rows of the session's
 * stride), n records in arrival order; out / out_payload: HOST, the segments
 * recovered by this batch, ascending packet_id.  As rfec_rx_recover. */
int rfec_rx_session_push(rfec_rx_session* s, uint32_t n, const rfec_wire_rec* recs, const uint8_t* payload,
                         rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                         rfec_rx_report* report, void* stream);
/* Received datagram slots in HOST memory (rfec_udp_recv_batch's output):
 * rfec_wire_parse, rfec_rx_session_push.  Pinned slots (rfec_pinned_alloc)
 * are read by the parse kernel itself, pageable ones copied first; a pinned
 * out_payload is gathered into directly.  recs_out (HOST, may be NULL)
 * receives the n parse records.  Refused while a pipelined batch is pending. */
int rfec_rx_session_push_datagrams(rfec_rx_session* s, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                                   const uint16_t* dlen, rfec_wire_rec* recs_out, rfec_rx_seg* out,
                                   uint8_t* out_payload, uint32_t max_out, uint32_t* n_out, rfec_rx_report* report);
/* Pipelined form, one batch of latency: starts the parse of these n
 * datagrams on the session's own stream, then ingests the batch the previous
 * call started (control plane, peel) while the device parses this one, and
 * returns THAT batch's recovered segments.  recs_out (HOST, may be NULL)
 * receives THAT batch's records too, so it must hold the PREVIOUS call's n
 * records (rfec_rx_session_get_info's `pending`), not this call's.  dgram /
 * dlen must stay unchanged until the next call on the session returns.
 * n == 0 only ingests the pending batch (the flush).  Deliveries, in total
 * and in order, equal rfec_rx_session_push_datagrams over the same batches;
 * rfec_rx_session_evict may come between calls. */
int rfec_rx_session_push_datagrams_async(rfec_rx_session* s, uint32_t n, uint32_t dstride, const uint8_t* dgram,
                                         const uint16_t* dlen, rfec_wire_rec* recs_out, rfec_rx_seg* out,
                                         uint8_t* out_payload, uint32_t max_out, uint32_t* n_out,
                                         rfec_rx_report* report);
int rfec_rx_session_evict(rfec_rx_session* s, void* stream);
int rfec_rx_session_get_info(const rfec_rx_session* s, rfec_rx_session_info* info);

/* Kernel selection, for tests: 0 = the default kernels (specialised where the
 * plan allows); RFEC_TUNE_GENERIC = the plan-driven kernels for every plan
 * (encode: one lane per (group, chunk column) over the plan's lines; recover
 * in place: the LDS peel + schedule replay), the cross-check of the
 * specialised ones.  Other bits: below, or ignored. */
#define RFEC_TUNE_GENERIC 1u
/* RFEC_TUNE_PLAN_CASCADE: a dense recover of the sender's matrix plan
 * (k = 6..16) takes the plan-driven cascade kernel instead of the one
 * compiled for its shape (the A/B and cross-check of the latter). */
#define RFEC_TUNE_PLAN_CASCADE (1u << 2)
/* RFEC_TUNE_WAVE_PARSE: rfec_wire_parse takes the wave-per-datagram kernel
 * instead of the quarter-wave one (the A/B and cross-check of the latter). */
#define RFEC_TUNE_WAVE_PARSE (1u << 3)
/* RFEC_TUNE_NO_SERVICE: the drop-in symbols (flex_fec_generate / _recover, the
 * group-level sender and receiver) launch their kernels per call instead of
 * posting to the resident service (process-wide; also RFEC_SERVICE=0 in the
 * environment).  Bit 30, so that no value of the round-1/2 tuning bits
 * (1u << 1 .. 1u << 24, now ignored) turns the service off. */
#define RFEC_TUNE_NO_SERVICE (1u << 30)
void rfec_set_tuning(unsigned flags);
unsigned rfec_get_tuning(void);

/* The drop-in's resident service: RFEC_SERVICE_GROUPS (default 1, at most 8)
 * workgroups that stay on the device and take the drop-in symbols' jobs from
 * a doorbell (no launch, no stream synchronisation per call), each on its
 * share of a job's 16-byte columns.  It starts on the
 * first drop-in call and leaves the device by itself after RFEC_SERVICE_IDLE_US
 * (default 2000) microseconds without a job, after RFEC_SERVICE_LIFE_US (default
 * 4000) in total (the next call starts it again) and at exit.  The request side
 * (doorbell, job, staged segments) sits in device memory the host writes
 * through its mapping when the runtime maps it (large-BAR hosts), else in
 * pinned host memory (also with RFEC_SERVICE_STAGE=host).  rfec_service_stop() makes it leave
 * now and waits for it; it returns RFEC_OK (also when it was not running) or
 * RFEC_EDEVICE.  rfec_service_get_info reports the calls served, the
 * launches made and where a call's time goes (means over the calls served). */
typedef struct {
    uint64_t jobs;       /* drop-in calls served */
    uint64_t launches;   /* workgroup launches (the first call, then after each idle exit) */
    double stage_host_us; /* mean, per job: the host copying the segments next to the doorbell */
    double wait_us;      /* doorbell written -> `done` seen by the host */
    double dev_stage_us; /* on the device: doorbell seen -> the job's slots in LDS */
    double dev_work_us;  /* -> results stored */
    double dev_release_us; /* -> the results' stores acknowledged, before `done` */
    uint32_t request_in_device; /* 1: the request side is in host-mapped device memory */
    uint32_t reserved;
} rfec_service_info;
int rfec_service_stop(void);
int rfec_service_get_info(rfec_service_info* info);

/* HBM ceiling probes (measurement only, not on the FEC path): streaming
 * read / copy / write of `bytes` (multiple of 16) in the FEC kernels' access
 * shape.  flags bit0 = non-temporal, bit1 = 4 vectors per lane.  `sink` of
 * rfec_probe_read needs 16 KiB.  Return 0 or a HIP error code. */
int rfec_probe_read(const void* src, size_t bytes, void* sink, unsigned flags, void* stream);
int rfec_probe_copy(const void* src, void* dst, size_t bytes, unsigned flags, void* stream);
int rfec_probe_write(void* dst, size_t bytes, unsigned flags, void* stream);
/* r read streams : w write streams of stream_bytes each (src holds r, dst w
 * streams back to back), lane i XORs chunk i of every read stream into chunk
 * i of every write stream, non-temporal: the ceiling of the encodes' read /
 * write mixes.  (r, w) in {(10, 3), (10, 7), (4, 1), (1, 1)}, else -1. */
int rfec_probe_mix(const void* src, void* dst, size_t stream_bytes, unsigned r, unsigned w, void* stream);

/* Synthetic inputs of SURVEY.md §8(d) (bench and tests only, not on the FEC
 * path): payload slots of groups [g0, g0 + groups) of the xorshift64*
 * stream seeded 0x52415A4F52464543 ^ config_id, filled group-major and
 * shard-major, S bytes per slot from ceil(S / 8) outputs (little endian),
 * zero to `stride`.  The slice is reached by jump-ahead, so a rank fills its
 * own part of a batch without the outputs before it.  Synchronises `stream`.
 * Returns RFEC_OK, RFEC_EINVAL or RFEC_EDEVICE. */
int rfec_fill_xorshift(uint8_t* shards, uint64_t config_id, uint64_t g0, uint32_t groups, uint32_t k, uint32_t S,
                       uint32_t stride, void* stream);
/* The xorshift64* state n steps after x (GF(2) jump-ahead; host only). */
uint64_t rfec_xorshift_jump(uint64_t x, uint64_t n);

/* Last HIP error string seen by this thread (for diagnostics). */
const char* rfec_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* RAZOR_FEC_H_ */
