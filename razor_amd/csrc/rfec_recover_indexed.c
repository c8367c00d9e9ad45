/*
 * rfec_recover_indexed.c -- rfec_recover_indexed_out (razor_fec.h): the dense
 * decode of rfec_recover_batch_out with the payload rows read through a slot
 * map from a row pool (rfec_wire_parse's rows where they lie, src_of as
 * rfec_wire_regroup[_index] writes it): argument checks, all before any
 * runtime call, then the launches through rfec_launch_recover_indexed
 * (rfec_kernels.hip).
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

int rfec_recover_indexed_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                             const uint8_t* rows, uint32_t n_rows, const uint32_t* src_of, const rfec_hdr* hdr,
                             const uint64_t* present, const rfec_hdr* meta, const uint16_t* fec_size,
                             const uint64_t* parity_present, uint64_t* recovered, uint32_t per_group,
                             uint8_t* out_shards, rfec_hdr* out_hdr, uint8_t* out_index, void* workspace,
                             void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K);
    if (rc)
        return rc;
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
    if (!src_of || !hdr || !present || !parity_present || !recovered || !workspace || !out_shards || !out_hdr ||
        !out_index || (n_rows && !rows) || (plan->n_lines && (!meta || !fec_size)))
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (misaligned(rows, 16) || misaligned(out_shards, 16) || misaligned(workspace, 16))
        return set_err(RFEC_EINVAL, "rows, out_shards and workspace must be 16-byte aligned", 0);
    if (misaligned(present, 8) || misaligned(parity_present, 8) || misaligned(recovered, 8))
        return set_err(RFEC_EINVAL, "present, parity_present and recovered must be 8-byte aligned", 0);
    if (misaligned(src_of, 4) || misaligned(hdr, 4) || misaligned(meta, 4) || misaligned(out_hdr, 4))
        return set_err(RFEC_EINVAL, "src_of, hdr, meta and out_hdr must be 4-byte aligned", 0);
    if (misaligned(fec_size, 2))
        return set_err(RFEC_EINVAL, "fec_size must be 2-byte aligned", 0);
    /* header lanes: one per (group, line slot), 32-bit lane index */
    if (((uint64_t)groups << rfec_header_lanes_log2(plan->n_lines)) >= (1ull << 32))
        return set_err(RFEC_EINVAL, "batch too large for one launch (groups x lines)", 0);
    static __thread rfec_kmask M; /* 1.3 KB: keep it off the stack */
    make_masks(plan, &M);
    const rfec_dense_out D = {out_shards, out_hdr, out_index, per_group};
    const int e = rfec_launch_recover_indexed(&M, groups, stride, capacity, rows, n_rows, src_of, hdr, present, meta,
                                              fec_size, parity_present, recovered, workspace, stream, g_tuning, &D);
    return e ? set_err(RFEC_EDEVICE, "recover_indexed launch", e) : RFEC_OK;
}
