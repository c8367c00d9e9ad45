/*
 * rfec_wire_regroup.c -- rfec_wire_regroup (razor_fec.h, wire codec): the
 * parsed datagrams of one closed window, in arrival order, into the batch
 * layout of rfec_recover_batch[_out] (rfec_regroup.hip): argument checks, all
 * before any runtime call, then the launches through rfec_launch_wire_regroup;
 * and rfec_wire_regroup_shapes, the index-only form over a window of several
 * shapes (rfec_regroup_shapes.hip).
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include <stdio.h>

#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

static int check_window(uint16_t fec_id0, uint32_t groups, uint32_t n)
{
    if (fec_id0 == 0)
        return set_err(RFEC_EINVAL, "fec_id0 must not be 0 (the sender skips it)", 0);
    if (groups > 65535u)
        return set_err(RFEC_EINVAL, "groups must be <= 65535 (the fec_ids of one succession)", 0);
    if (n > 0x7FFFFFFFu)
        return set_err(RFEC_EINVAL, "n must be <= 0x7FFFFFFF", 0);
    return RFEC_OK;
}

int rfec_wire_regroup(const rfec_plan* plan, uint32_t groups, uint16_t fec_id0, uint32_t n,
                      const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride, uint32_t capacity,
                      uint8_t* shards, rfec_hdr* hdr, uint64_t* present, uint8_t* parity, rfec_hdr* meta,
                      uint16_t* fec_size, uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                      int32_t* slot_of, void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K);
    if (rc)
        return rc;
    /* rfec_wire_parse's geometry: rows of at most 2,048 bytes */
    if (stride == 0 || stride % 16 || stride > RFEC_WIRE_MAX_DSTRIDE)
        return set_err(RFEC_EINVAL, "stride must be a positive multiple of 16, at most 2048", 0);
    if (capacity > stride)
        return set_err(RFEC_EINVAL, "capacity must be <= stride", 0);
    if ((rc = check_window(fec_id0, groups, n)) != RFEC_OK)
        return rc;
    if (groups == 0)
        return RFEC_OK;
    const int nl = plan->n_lines;
    if (!shards || !hdr || !present || !parity_present || !base_id || !src_of)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (nl && (!parity || !meta || !fec_size))
        return set_err(RFEC_EINVAL, "NULL buffer (parity, meta, fec_size)", 0);
    if (n && (!recs || !payload || !slot_of))
        return set_err(RFEC_EINVAL, "NULL buffer (recs, payload, slot_of)", 0);
    if (misaligned(recs, 16) || misaligned(payload, 16) || misaligned(shards, 16) || misaligned(parity, 16))
        return set_err(RFEC_EINVAL, "recs, payload, shards and parity must be 16-byte aligned", 0);
    if (misaligned(present, 8) || misaligned(parity_present, 8))
        return set_err(RFEC_EINVAL, "present and parity_present must be 8-byte aligned", 0);
    if (misaligned(hdr, 4) || misaligned(meta, 4) || misaligned(base_id, 4) || misaligned(src_of, 4) ||
        misaligned(slot_of, 4))
        return set_err(RFEC_EINVAL, "hdr, meta, base_id, src_of and slot_of must be 4-byte aligned", 0);
    if (misaligned(fec_size, 2))
        return set_err(RFEC_EINVAL, "fec_size must be 2-byte aligned", 0);
    const int e = rfec_launch_wire_regroup(plan, groups, fec_id0, n, recs, payload, stride, capacity, shards, hdr,
                                           present, parity, meta, fec_size, parity_present, base_id, src_of, slot_of,
                                           stream);
    return e ? set_err(RFEC_EDEVICE, "wire_regroup launch", e) : RFEC_OK;
}

/* rfec_wire_regroup without the row copy: the tables alone (src_of is the row map of rfec_recover_indexed_out) */
int rfec_wire_regroup_index(const rfec_plan* plan, uint32_t groups, uint16_t fec_id0, uint32_t n,
                            const rfec_wire_rec* recs, uint32_t capacity, rfec_hdr* hdr, uint64_t* present,
                            rfec_hdr* meta, uint16_t* fec_size, uint64_t* parity_present, uint32_t* base_id,
                            uint32_t* src_of, int32_t* slot_of, void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K);
    if (rc)
        return rc;
    if ((rc = check_window(fec_id0, groups, n)) != RFEC_OK)
        return rc;
    if (groups == 0)
        return RFEC_OK;
    const int nl = plan->n_lines;
    if (!hdr || !present || !parity_present || !base_id || !src_of)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (nl && (!meta || !fec_size))
        return set_err(RFEC_EINVAL, "NULL buffer (meta, fec_size)", 0);
    if (n && (!recs || !slot_of))
        return set_err(RFEC_EINVAL, "NULL buffer (recs, slot_of)", 0);
    if (misaligned(recs, 16))
        return set_err(RFEC_EINVAL, "recs must be 16-byte aligned", 0);
    if (misaligned(present, 8) || misaligned(parity_present, 8))
        return set_err(RFEC_EINVAL, "present and parity_present must be 8-byte aligned", 0);
    if (misaligned(hdr, 4) || misaligned(meta, 4) || misaligned(base_id, 4) || misaligned(src_of, 4) ||
        misaligned(slot_of, 4))
        return set_err(RFEC_EINVAL, "hdr, meta, base_id, src_of and slot_of must be 4-byte aligned", 0);
    if (misaligned(fec_size, 2))
        return set_err(RFEC_EINVAL, "fec_size must be 2-byte aligned", 0);
    const int e = rfec_launch_wire_regroup_index(plan, groups, fec_id0, n, recs, capacity, hdr, present, meta,
                                                 fec_size, parity_present, base_id, src_of, slot_of, stream);
    return e ? set_err(RFEC_EDEVICE, "wire_regroup_index launch", e) : RFEC_OK;
}

/* rfec_wire_regroup_shapes's argument errors name the plan or section: "sections[3].hdr is NULL" */
static int shapes_err(const char* array, uint32_t p, const char* what)
{
    char msg[128];
    snprintf(msg, sizeof(msg), "%s[%u]%s", array, (unsigned)p, what);
    return set_err(RFEC_EINVAL, msg, 0);
}

/* One regroup pass over a window whose groups have different shapes: a dense section of
 * rfec_wire_regroup_index's tables per plan (razor_fec.h, "The rule" of rfec_wire_regroup_shapes). */
int rfec_wire_regroup_shapes(const rfec_plan* plans, uint32_t n_plans, const rfec_regroup_section* sections,
                             uint32_t groups, uint16_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                             uint32_t capacity, uint8_t* shape_of, uint32_t* rank_of, uint32_t* anchor_of,
                             uint32_t* counts, int32_t* slot_of, void* stream)
{
    if (!plans)
        return set_err(RFEC_EINVAL, "plans is NULL", 0);
    if (n_plans < 1 || n_plans > RFEC_REGROUP_MAX_SHAPES)
        return set_err(RFEC_EINVAL, "n_plans must be in [1, RFEC_REGROUP_MAX_SHAPES]", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const int rc = check_plan(plans + p, RFEC_MAX_K);
        if (rc)
            return rc;
        for (uint32_t q = 0; q < p; ++q)
            if (plans[q].k == plans[p].k && plans[q].row == plans[p].row && plans[q].col == plans[p].col)
                return shapes_err("plans", p, " repeats the (k, row, col) of an earlier plan");
    }
    const int rc = check_window(fec_id0, groups, n);
    if (rc)
        return rc;
    for (uint32_t p = 0; sections && p < n_plans; ++p)
        if (sections[p].cap > groups)
            return shapes_err("sections", p, ".cap must be <= groups");
    if (groups == 0)
        return RFEC_OK;
    if (!sections)
        return set_err(RFEC_EINVAL, "sections is NULL", 0);
    if (n && (!recs || !slot_of))
        return set_err(RFEC_EINVAL, "NULL buffer (recs, slot_of)", 0);
    if (misaligned(recs, 16))
        return set_err(RFEC_EINVAL, "recs must be 16-byte aligned", 0);
    if (misaligned(rank_of, 4) || misaligned(anchor_of, 4) || misaligned(counts, 4) || misaligned(slot_of, 4))
        return set_err(RFEC_EINVAL, "rank_of, anchor_of, counts and slot_of must be 4-byte aligned", 0);
    for (uint32_t p = 0; p < n_plans; ++p) {
        const rfec_regroup_section* s = sections + p;
        if (s->cap == 0)
            continue; /* nothing of it is touched */
        if (!s->hdr || !s->present || !s->parity_present || !s->base_id || !s->src_of || !s->group_of)
            return shapes_err("sections", p, ": NULL buffer");
        if (plans[p].n_lines && (!s->meta || !s->fec_size))
            return shapes_err("sections", p, ": NULL buffer (meta, fec_size)");
        if (misaligned(s->present, 8) || misaligned(s->parity_present, 8))
            return shapes_err("sections", p, ": present and parity_present must be 8-byte aligned");
        if (misaligned(s->hdr, 4) || misaligned(s->meta, 4) || misaligned(s->base_id, 4) || misaligned(s->src_of, 4) ||
            misaligned(s->group_of, 4))
            return shapes_err("sections", p, ": hdr, meta, base_id, src_of and group_of must be 4-byte aligned");
        if (misaligned(s->fec_size, 2))
            return shapes_err("sections", p, ": fec_size must be 2-byte aligned");
    }
    if (!shape_of || !rank_of || !anchor_of || !counts)
        return set_err(RFEC_EINVAL, "NULL buffer (shape_of, rank_of, anchor_of, counts)", 0);
    const int e = rfec_launch_wire_regroup_shapes(plans, n_plans, sections, groups, fec_id0, n, recs, capacity,
                                                  shape_of, rank_of, anchor_of, counts, slot_of, stream);
    return e ? set_err(RFEC_EDEVICE, "wire_regroup_shapes launch", e) : RFEC_OK;
}
