/*
 * rfec_packed_matrix.c -- packed erasure records for the sender's full row +
 * column plans of k = 6..16 (razor_fec.h: rfec_packed_matrix_stride,
 * rfec_pack_erasures_matrix, rfec_recover_packed_matrix_out): argument
 * checks, then the launches through the shims in rfec_cascade.hip.  The
 * row-layout records' entry points (rfec_host.c) keep refusing these plans.
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

/* bytes of one slot: a row half (meta, fec_data_size, col - 1 members) and a column half (rows - 1 members) */
static uint32_t slot_bytes(uint32_t k, uint32_t col)
{
    const uint32_t rows = (k + col - 1) / col;
    return (24u + 20u * (col - 1u)) + (24u + 20u * (rows - 1u));
}

size_t rfec_packed_matrix_stride(const rfec_plan* plan, uint32_t per_group)
{
    if (!plan || plan->n_lines > RFEC_MAX_LINES)
        return 0;
    const uint32_t col = (uint32_t)rfec_packed_matrix_col(plan);
    if (!col || per_group == 0 || per_group > plan->k)
        return 0;
    return ((16u + per_group * slot_bytes(plan->k, col)) + 63u) & ~(size_t)63u;
}

/* the checks both entry points share (rfec_host.c packed_check's); sets *pk_stride */
static int matrix_check(const rfec_plan* plan, uint32_t groups, uint32_t per_group, const void* packed,
                        size_t* pk_stride)
{
    int rc = check_plan(plan, RFEC_MAX_K);
    if (rc)
        return rc;
    if (!rfec_packed_matrix_col(plan))
        return set_err(RFEC_EINVAL, "packed matrix records need the sender's full row + column plan of k = 6..16", 0);
    if (per_group == 0 || per_group > plan->k)
        return set_err(RFEC_EINVAL, "per_group must be in [1, k]", 0);
    *pk_stride = rfec_packed_matrix_stride(plan, per_group);
    /* (the pack kernel's lanes: one per 16 bytes of the records) */
    if (((uint64_t)groups << rfec_ceil_log2(per_group)) >= (1ull << 32) || (uint64_t)groups * *pk_stride >= (1ull << 40) ||
        (uint64_t)groups * (*pk_stride / 16) >= (1ull << 32))
        return set_err(RFEC_EINVAL, "batch too large for one launch (groups x slots)", 0);
    if (groups && (!packed || (uintptr_t)packed % 16))
        return set_err(RFEC_EINVAL, "packed records: NULL or not 16-byte aligned", 0);
    return RFEC_OK;
}

int rfec_pack_erasures_matrix(const rfec_plan* plan, uint32_t groups, const rfec_hdr* hdr, const uint64_t* present,
                              const rfec_hdr* meta, const uint16_t* fec_size, const uint64_t* parity_present,
                              uint32_t per_group, uint8_t* packed, void* stream)
{
    size_t pks;
    int rc = matrix_check(plan, groups, per_group, packed, &pks);
    if (rc)
        return rc;
    if (groups == 0)
        return RFEC_OK;
    if (!hdr || !present || !meta || !fec_size || !parity_present)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if ((rc = check_align_in(NULL, hdr, NULL, meta, fec_size)) ||
        (rc = check_align_masks(present, parity_present, NULL)))
        return rc;
    const int e = rfec_launch_pack_matrix(plan, groups, hdr, present, meta, fec_size, parity_present, per_group,
                                          packed, (uint32_t)pks, stream);
    return e ? set_err(RFEC_EDEVICE, "pack launch", e) : RFEC_OK;
}

int rfec_recover_packed_matrix_out(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                                   const uint8_t* shards, const uint8_t* parity, const uint8_t* packed,
                                   uint64_t* recovered, uint32_t per_group, uint8_t* out_shards, rfec_hdr* out_hdr,
                                   uint8_t* out_index, void* stream)
{
    size_t pks;
    int rc = matrix_check(plan, groups, per_group, packed, &pks);
    if (rc)
        return rc;
    if ((rc = check_geometry(groups, stride, capacity, plan->k)))
        return rc;
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    /* 32-bit lane index; a wave's groups are addressed through one buffer descriptor (as rfec_recover_packed_out) */
    if ((uint64_t)groups * per_group * cd >= (1ull << 32) || (uint64_t)65 * plan->k * stride >= 0x7FFFFFF0ull)
        return set_err(RFEC_EINVAL, "batch too large for one launch (groups x slots x chunks)", 0);
    if (groups == 0)
        return RFEC_OK;
    if (!shards || !parity || !recovered || !out_shards || !out_hdr || !out_index)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if ((rc = check_align_in(shards, NULL, parity, NULL, NULL)) || (rc = check_align_masks(NULL, NULL, recovered)) ||
        (rc = check_align_out(out_shards, out_hdr)))
        return rc;
    static __thread rfec_kmask M; /* 1.3 KB: keep it off the stack */
    make_masks(plan, &M);
    const rfec_dense_out D = {out_shards, out_hdr, out_index, per_group};
    const int e = rfec_launch_recover_packed_matrix(&M, groups, stride, capacity, shards, parity, packed,
                                                    (uint32_t)pks, recovered, &D, stream);
    return e ? set_err(RFEC_EDEVICE, "recover launch", e) : RFEC_OK;
}
