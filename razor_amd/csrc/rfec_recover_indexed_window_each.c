/*
 * rfec_recover_indexed_window_each.c -- rfec_recover_indexed_window_each_out
 * and rfec_recover_window_slots (razor_fec.h):
 * rfec_recover_indexed_window_out with an out-slot count per section.
 * per_group is a host array [n_plans]; section p's rows have per_group[p] out
 * slots each and the sections' slots are packed end to end, so a window's
 * small groups no longer bound what its large ones deliver.  Argument checks,
 * all before any runtime call and in rfec_recover_indexed_window.c's order
 * with per_group where it stands there, then the launch through
 * rfec_launch_recover_indexed_window_each (rfec_cascade.hip).
 * rfec_recover_indexed_window_out keeps its own answers and its kernel.
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
    char msg[200];
    snprintf(msg, sizeof(msg), "%s[%u]%s", array, (unsigned)p, what);
    return set_err(RFEC_EINVAL, msg, 0);
}

uint64_t rfec_recover_window_slots(const rfec_regroup_section* sections, uint32_t n_plans, const uint32_t* groups,
                                   const uint32_t* per_group)
{
    uint64_t slots = 0;
    if (!per_group || (!groups && !sections))
        return 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const uint32_t g = groups ? groups[p] : sections[p].cap;
        if (g)
            slots += (uint64_t)g * per_group[p];
    }
    return slots;
}

int rfec_recover_indexed_window_each_out(const rfec_plan* plans, uint32_t n_plans,
                                         const rfec_regroup_section* sections, const uint32_t* groups, uint32_t stride,
                                         uint32_t capacity, const uint8_t* rows, uint32_t n_rows, uint64_t* recovered,
                                         const uint32_t* per_group, uint8_t* out_shards, rfec_hdr* out_hdr,
                                         uint8_t* out_index, void* stream)
{
    if (!plans)
        return set_err(RFEC_EINVAL, "plans is NULL", 0);
    if (n_plans < 1 || n_plans > RFEC_RECOVER_MAX_SHAPES)
        return set_err(RFEC_EINVAL, "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]", 0);
    if (!sections)
        return set_err(RFEC_EINVAL, "sections is NULL", 0);
    uint32_t n_launched = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const int rc = check_plan(plans + p, RFEC_MAX_K);
        if (rc)
            return rc;
        if (!(groups ? groups[p] : sections[p].cap))
            continue; /* left to the generic call: any plan */
        if (!rfec_recover_window_family(plans + p))
            return section_err("plans", p,
                               " is neither the sender's full row + column plan of k = 6..128 nor a row layout (rows "
                               "of line[0].count >= 2 consecutive segments in order): use rfec_recover_indexed_out");
        ++n_launched;
    }
    if (stride == 0 || stride % 16)
        return set_err(RFEC_EINVAL, "stride must be a positive multiple of 16", 0);
    if (capacity > stride)
        return set_err(RFEC_EINVAL, "capacity must be <= stride", 0);
    if (!per_group)
        return set_err(RFEC_EINVAL, "per_group is NULL", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        if (!(groups ? groups[p] : sections[p].cap))
            continue; /* not read for range */
        if (per_group[p] == 0 || per_group[p] > plans[p].k)
            return section_err("per_group", p, " must be in [1, plans[p].k]");
    }
    const uint32_t cd = capacity ? (capacity + 15) / 16 : 1;
    uint64_t blocks = 0, out_rows = 0, slots = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const uint32_t g = groups ? groups[p] : sections[p].cap;
        if (g > sections[p].cap)
            return section_err("groups", p, " must be <= sections[p].cap");
        if (!g)
            continue;
        /* one lane per (group, out slot, chunk), 32-bit lane index and fast division */
        if ((uint64_t)g * per_group[p] * cd >= (1ull << 31))
            return section_err("groups", p, ": section too large for one launch (groups x per_group x chunks)");
        /* checker lanes: four per group (family 1) or one (family 3: bounded with the groups already); header lanes:
         * one per (group, line slot) (families 2 and 4); 32-bit lane index */
        const int family = rfec_recover_window_family(plans + p);
        if (family == 1 ? (uint64_t)g * 4 >= (1ull << 32)
                        : family != 3 && ((uint64_t)g << rfec_header_lanes_log2(plans[p].n_lines)) >= (1ull << 32))
            return section_err("groups", p, ": section too large for one launch (groups x header lanes)");
        blocks += rfec_recover_window_blocks(plans + p, g, per_group[p], cd, n_rows);
        out_rows += g;
        slots += (uint64_t)g * per_group[p];
    }
    if (blocks >= (1ull << 31) || out_rows >= (1ull << 32) || slots * cd >= (1ull << 31))
        return set_err(RFEC_EINVAL,
                       "window too large for one launch (the sections' blocks, their rows, or their slots x chunks)", 0);
    if (!n_launched)
        return RFEC_OK;
    if (!recovered || !out_shards || !out_hdr || !out_index || (n_rows && !rows))
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_regroup_section* s = sections + p;
        if (!(groups ? groups[p] : s->cap))
            continue; /* nothing of it is touched */
        /* (these plans have lines: meta and fec_size are never optional) */
        if (!s->src_of || !s->hdr || !s->present || !s->parity_present || !s->meta || !s->fec_size)
            return section_err("sections", p, ": NULL buffer");
    }
    if (misaligned(rows, 16) || misaligned(out_shards, 16))
        return set_err(RFEC_EINVAL, "rows and out_shards must be 16-byte aligned", 0);
    if (misaligned(recovered, 8))
        return set_err(RFEC_EINVAL, "recovered must be 8-byte aligned", 0);
    if (misaligned(out_hdr, 4))
        return set_err(RFEC_EINVAL, "out_hdr must be 4-byte aligned", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_regroup_section* s = sections + p;
        if (!(groups ? groups[p] : s->cap))
            continue;
        if (misaligned(s->present, 8) || misaligned(s->parity_present, 8))
            return section_err("sections", p, ": present and parity_present must be 8-byte aligned");
        if (misaligned(s->src_of, 4) || misaligned(s->hdr, 4) || misaligned(s->meta, 4))
            return section_err("sections", p, ": src_of, hdr and meta must be 4-byte aligned");
        if (misaligned(s->fec_size, 2))
            return section_err("sections", p, ": fec_size must be 2-byte aligned");
    }
    const int e = rfec_launch_recover_indexed_window_each(plans, n_plans, sections, groups, stride, capacity, rows,
                                                          n_rows, recovered, per_group, out_shards, out_hdr, out_index,
                                                          stream);
    return e ? set_err(RFEC_EDEVICE, "recover_indexed_window_each launch", e) : RFEC_OK;
}
