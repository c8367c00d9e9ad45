/*
 * rfec_recover_deliver_each.c -- rfec_recover_deliver_each (razor_fec.h):
 * rfec_recover_deliver over the outputs of
 * rfec_recover_indexed_window_each_out, whose section p has per_group[p] out
 * slots a row and whose slots are packed end to end.  Argument checks, all
 * before any runtime call and in rfec_recover_deliver.c's order with per_group
 * where it stands there, the prefixes of the sections' rows and slots, then
 * the launches through rfec_launch_recover_deliver_each (rfec_deliver.hip).
 * The workspace is rfec_recover_deliver_workspace_size's.
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include <stdio.h>

#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

static int section_err(const char* array, uint32_t p, const char* what)
{
    char msg[160];
    snprintf(msg, sizeof(msg), "%s[%u]%s", array, (unsigned)p, what);
    return set_err(RFEC_EINVAL, msg, 0);
}

int rfec_recover_deliver_each(const rfec_plan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                              const uint32_t* groups, uint32_t window_groups, uint16_t fec_id0,
                              const uint8_t* shape_of, const uint32_t* rank_of, uint32_t stride, uint32_t capacity,
                              const uint32_t* per_group, const uint8_t* out_shards, const rfec_hdr* out_hdr,
                              const uint8_t* out_index, uint32_t max_out, rfec_rx_seg* seg, uint8_t* seg_payload,
                              uint32_t* first_of, uint32_t* n_out, void* workspace, void* stream)
{
    if (!plans)
        return set_err(RFEC_EINVAL, "plans is NULL", 0);
    if (n_plans < 1 || n_plans > RFEC_RECOVER_MAX_SHAPES)
        return set_err(RFEC_EINVAL, "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]", 0);
    if (!sections && window_groups)
        return set_err(RFEC_EINVAL, "sections is NULL", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const int rc = check_plan(plans + p, RFEC_MAX_K);
        if (rc)
            return rc;
    }
    if (window_groups > 65535)
        return set_err(RFEC_EINVAL, "window_groups must be <= 65535", 0);
    if (fec_id0 == 0)
        return set_err(RFEC_EINVAL, "fec_id0 must not be 0", 0);
    if (stride == 0 || stride % 16)
        return set_err(RFEC_EINVAL, "stride must be a positive multiple of 16", 0);
    if (capacity > stride)
        return set_err(RFEC_EINVAL, "capacity must be <= stride", 0);
    if (!per_group)
        return set_err(RFEC_EINVAL, "per_group is NULL", 0);
    for (uint32_t p = 0; sections && p < n_plans; ++p)
        if ((groups ? groups[p] : sections[p].cap) && per_group[p] == 0)
            return section_err("per_group", p, " must be >= 1");
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    uint32_t first[RFEC_RECOVER_MAX_SHAPES + 1], slot_first[RFEC_RECOVER_MAX_SHAPES + 1];
    uint64_t rows = 0, slots = 0;
    int too_large = 0;
    first[0] = slot_first[0] = 0;
    for (uint32_t p = 0; sections && p < n_plans; ++p) {
        const uint32_t g = groups ? groups[p] : sections[p].cap;
        if (g > sections[p].cap)
            return section_err("groups", p, " must be <= sections[p].cap");
        rows += g;
        if (g)
            slots += (uint64_t)g * per_group[p];
        too_large |= slots >= (1ull << 31); /* (the sum stays far below 2^64: 32 terms below 2^64 / 32 each) */
        first[p + 1] = (uint32_t)rows; /* (checked below) */
        slot_first[p + 1] = (uint32_t)slots;
    }
    /* one lane per (out slot, chunk), 32-bit lane index and fast division */
    if (rows >= (1ull << 32) || too_large || slots * cd >= (1ull << 31))
        return set_err(RFEC_EINVAL, "window too large for one launch (the sections' slots x chunks, or their rows)", 0);
    if (window_groups == 0)
        return RFEC_OK;
    if (!shape_of || !rank_of || !first_of || !n_out || !workspace)
        return set_err(RFEC_EINVAL, "NULL buffer (shape_of, rank_of, first_of, n_out, workspace)", 0);
    if (max_out && (!seg || !seg_payload))
        return set_err(RFEC_EINVAL, "NULL buffer (seg, seg_payload)", 0);
    if (rows && (!out_shards || !out_hdr || !out_index))
        return set_err(RFEC_EINVAL, "NULL buffer (out_shards, out_hdr, out_index)", 0);
    for (uint32_t p = 0; p < n_plans; ++p)
        if (first[p + 1] != first[p] && !sections[p].group_of)
            return section_err("sections", p, ".group_of is NULL");
    if (misaligned(out_shards, 16) || misaligned(seg_payload, 16) || misaligned(workspace, 16))
        return set_err(RFEC_EINVAL, "out_shards, seg_payload and workspace must be 16-byte aligned", 0);
    if (misaligned(out_hdr, 4) || misaligned(seg, 4) || misaligned(rank_of, 4) || misaligned(first_of, 4) ||
        misaligned(n_out, 4))
        return set_err(RFEC_EINVAL, "out_hdr, seg, rank_of, first_of and n_out must be 4-byte aligned", 0);
    for (uint32_t p = 0; p < n_plans; ++p)
        if (first[p + 1] != first[p] && misaligned(sections[p].group_of, 4))
            return section_err("sections", p, ".group_of must be 4-byte aligned");
    const int e = rfec_launch_recover_deliver_each(sections, n_plans, first, slot_first, per_group, window_groups,
                                                   fec_id0, shape_of, rank_of, stride, capacity, out_shards, out_hdr,
                                                   out_index, max_out, seg, seg_payload, first_of, n_out, workspace,
                                                   stream);
    return e ? set_err(RFEC_EDEVICE, "recover_deliver_each launch", e) : RFEC_OK;
}
