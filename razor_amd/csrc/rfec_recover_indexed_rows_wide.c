/*
 * rfec_recover_indexed_rows_wide.c -- rfec_recover_indexed_rows_wide_out
 * (razor_fec.h): rfec_recover_indexed_out for a row layout of any width (the
 * sender's strip-mode plans, the rows-only layer of a matrix) in one launch
 * and without a workspace: argument checks, all before any runtime call and in
 * rfec_recover_indexed.c's order, then the launch through
 * rfec_launch_recover_indexed_rows_wide (rfec_rows_wide.hip).
 * rfec_recover_indexed_out, rfec_recover_indexed_shapes_out and the matrix
 * entries keep their own answers for these plans.
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

int rfec_recover_indexed_rows_wide_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                       const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of,
                                       const rfec_hdr* hdr, const uint64_t* present, const rfec_hdr* meta,
                                       const uint16_t* fec_size, const uint64_t* parity_present, uint64_t* recovered,
                                       uint32_t per_group, uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index,
                                       void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K);
    if (rc)
        return rc;
    if (!rfec_rows_wide_col(plan))
        return set_err(RFEC_EINVAL,
                       "plan is not a row layout (rows of line[0].count >= 2 consecutive segments in order, a last "
                       "row of one segment without a line): use rfec_recover_indexed_out",
                       0);
    if (stride == 0 || stride % 16)
        return set_err(RFEC_EINVAL, "stride must be a positive multiple of 16", 0);
    if (capacity > stride)
        return set_err(RFEC_EINVAL, "capacity must be <= stride", 0);
    if (per_group == 0 || per_group > plan->k)
        return set_err(RFEC_EINVAL, "per_group must be in [1, k]", 0);
    /* one lane per (group, out slot, chunk), 32-bit lane index and fast division */
    if ((uint64_t)groups * per_group * (capacity ? (capacity + 15) / 16 : 1) >= (1ull << 31))
        return set_err(RFEC_EINVAL, "batch too large for one launch (groups x per_group x chunks)", 0);
    if (groups == 0)
        return RFEC_OK;
    /* (these plans have lines: meta and fec_size are never optional) */
    if (!src_of || !hdr || !present || !parity_present || !recovered || !out_shards || !out_hdr || !out_index ||
        (n_rows && !rows) || !meta || !fec_size)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (misaligned(rows, 16) || misaligned(out_shards, 16))
        return set_err(RFEC_EINVAL, "rows and out_shards must be 16-byte aligned", 0);
    if (misaligned(present, 8) || misaligned(parity_present, 8) || misaligned(recovered, 8))
        return set_err(RFEC_EINVAL, "present, parity_present and recovered must be 8-byte aligned", 0);
    if (misaligned(src_of, 4) || misaligned(hdr, 4) || misaligned(meta, 4) || misaligned(out_hdr, 4))
        return set_err(RFEC_EINVAL, "src_of, hdr, meta and out_hdr must be 4-byte aligned", 0);
    if (misaligned(fec_size, 2))
        return set_err(RFEC_EINVAL, "fec_size must be 2-byte aligned", 0);
    /* header lanes: one per (group, line slot), 32-bit lane index */
    if (((uint64_t)groups << rfec_header_lanes_log2(plan->n_lines)) >= (1ull << 32))
        return set_err(RFEC_EINVAL, "batch too large for one launch (groups x lines)", 0);
    const rfec_dense_out D = {out_shards, out_hdr, out_index, per_group};
    const int e = rfec_launch_recover_indexed_rows_wide(plan, groups, stride, capacity, rows, n_rows, src_of, hdr,
                                                        present, meta, fec_size, parity_present, recovered, &D, stream);
    return e ? set_err(RFEC_EDEVICE, "recover_indexed_rows_wide launch", e) : RFEC_OK;
}
