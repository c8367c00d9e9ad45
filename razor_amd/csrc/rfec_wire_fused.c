/*
 * rfec_wire_fused.c -- rfec_wire_encode_fec (razor_fec.h, wire codec): a
 * batch of groups straight into SIM_FEC datagrams, the encode and the framing
 * in one kernel (k_encode_frame_fec_q, rfec_wire.hip): argument checks, then
 * the launches through rfec_launch_wire_encode_fec, split over groups so that
 * every launch keeps 32-bit buffer offsets.  rfec_wire_encode_send: the same
 * for the batch's SIM_SEG and SIM_FEC datagrams in one kernel
 * (k_encode_send_q); rfec_wire_encode_send_shapes: that kernel's form for a
 * window of several shapes (k_encode_send_shapes_q), one launch.
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include <stdio.h>
#include <stdlib.h>

#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

#define WEF_MAX_DSTRIDE 1280u        /* the quarter-wave window */
#define WEF_OFFSETS 0xFFFFFFF0ull    /* buffer offsets stay below this */

/* The most groups one launch takes: (groups k + 4) stride + 1280 (the bound the quarter-wave framing states for
 * its input slots), the header records' groups k 20 bytes and, when the launch's output is its own slice of
 * dgram (own_out), groups n dstride, all below WEF_OFFSETS.  At least 1: a group is at most 255 slots of 2 KiB. */
static uint32_t groups_per_launch(const rfec_plan* p, uint32_t stride, uint32_t dstride, int own_out)
{
    const uint64_t k = p->k, n = p->n_lines;
    uint64_t g = ((WEF_OFFSETS - 1 - WEF_MAX_DSTRIDE) / stride - 4) / k;
    const uint64_t gh = (WEF_OFFSETS - 1) / (k * sizeof(rfec_hdr));
    g = gh < g ? gh : g;
    if (own_out) {
        const uint64_t go = (WEF_OFFSETS - 1) / (n * dstride);
        g = go < g ? go : g;
    }
    const char* v = getenv("RFEC_WIRE_ENCODE_CHUNK_GROUPS"); /* tests: a cap, to split a small batch */
    if (v && atoi(v) > 0 && (uint64_t)atoi(v) < g)
        g = (uint64_t)atoi(v);
    return (uint32_t)(g < 1 ? 1 : g);
}

int rfec_wire_encode_fec(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                         const uint8_t* shards, const rfec_hdr* hdr, const rfec_fec_stamp* stamps,
                         const uint32_t* order, uint32_t dstride, uint8_t* dgram, uint16_t* dlen, void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K_ENCODE);
    if (rc)
        return rc;
    const uint32_t n = plan->n_lines;
    if ((uint64_t)groups * n > 0xFFFFFFFFull)
        return set_err(RFEC_EINVAL, "groups * n_lines overflows", 0);
    if ((rc = check_wire(groups * n, stride, capacity, dstride, RFEC_WIRE_FEC_OVERHEAD)))
        return rc;
    if (dstride > WEF_MAX_DSTRIDE)
        return set_err(RFEC_EINVAL,
                       "rfec_wire_encode_fec takes dstride <= 1280: use rfec_encode_batch + rfec_wire_frame_fec", 0);
    if (groups == 0 || n == 0)
        return RFEC_OK;
    if (!shards || !hdr || !stamps || !dgram || !dlen)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (misaligned(shards, 16) || misaligned(dgram, 16))
        return set_err(RFEC_EINVAL, "shards and dgram must be 16-byte aligned", 0);
    if (misaligned(hdr, 4) || misaligned(stamps, 4) || misaligned(order, 4))
        return set_err(RFEC_EINVAL, "hdr, stamps and order must be 4-byte aligned", 0);
    if (misaligned(dlen, 2))
        return set_err(RFEC_EINVAL, "dlen must be 2-byte aligned", 0);
    const uint32_t count = groups * n;
    if (order && (uint64_t)count * dstride >= WEF_OFFSETS)
        return set_err(RFEC_EINVAL, "with order, the datagram slots must stay below 4 GiB", 0);
    const uint32_t per = groups_per_launch(plan, stride, dstride, order == NULL);
    for (uint32_t g0 = 0; g0 < groups; g0 += per) {
        const uint32_t ng = groups - g0 < per ? groups - g0 : per;
        const size_t r0 = (size_t)g0 * plan->k, d0 = (size_t)g0 * n;
        /* without order a launch writes its own slots; with it, anywhere in the batch's */
        const int e = rfec_launch_wire_encode_fec(plan, ng, stride, capacity, shards + r0 * stride, hdr + r0,
                                                  stamps + d0, order ? order + d0 : NULL, dstride,
                                                  order ? dgram : dgram + d0 * dstride, order ? dlen : dlen + d0,
                                                  order ? count : ng * n, stream);
        if (e)
            return set_err(RFEC_EDEVICE, "wire_encode_fec launch", e);
    }
    return RFEC_OK;
}

/* groups_per_launch for rfec_wire_encode_send: the SIM_FEC output as there (own_fec), and groups k dstride of
 * the SIM_SEG output below WEF_OFFSETS when the launch's slots are its own slice of seg_dgram (own_seg). */
static uint32_t send_groups_per_launch(const rfec_plan* p, uint32_t stride, uint32_t dstride, int own_seg,
                                       int own_fec)
{
    uint64_t g = groups_per_launch(p, stride, dstride, own_fec && p->n_lines > 0);
    if (own_seg) {
        const uint64_t gs = (WEF_OFFSETS - 1) / ((uint64_t)p->k * dstride);
        g = gs < g ? gs : g;
    }
    return (uint32_t)(g < 1 ? 1 : g);
}

int rfec_wire_encode_send(const rfec_plan* plan, uint32_t groups, uint32_t stride, uint32_t capacity,
                          const uint8_t* shards, const rfec_hdr* hdr, const rfec_seg_stamp* seg_stamps,
                          const uint32_t* seg_order, uint8_t* seg_dgram, uint16_t* seg_dlen,
                          const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order, uint8_t* fec_dgram,
                          uint16_t* fec_dlen, uint32_t dstride, void* stream)
{
    int rc = check_plan(plan, RFEC_MAX_K_ENCODE);
    if (rc)
        return rc;
    const uint32_t k = plan->k, n = plan->n_lines;
    if ((uint64_t)groups * k > 0xFFFFFFFFull || (uint64_t)groups * n > 0xFFFFFFFFull)
        return set_err(RFEC_EINVAL, "groups * k or groups * n_lines overflows", 0);
    const uint32_t ns = groups * k, nf = groups * n;
    /* the SIM_FEC overhead covers the SIM_SEG's 36 */
    if ((rc = check_wire(ns > nf ? ns : nf, stride, capacity, dstride, RFEC_WIRE_FEC_OVERHEAD)))
        return rc;
    if (dstride > WEF_MAX_DSTRIDE)
        return set_err(RFEC_EINVAL,
                       "rfec_wire_encode_send takes dstride <= 1280: use rfec_wire_frame_seg + rfec_wire_encode_fec",
                       0);
    if (groups == 0)
        return RFEC_OK;
    if (!shards || !hdr || !seg_stamps || !seg_dgram || !seg_dlen)
        return set_err(RFEC_EINVAL, "NULL buffer", 0);
    if (n && (!fec_stamps || !fec_dgram || !fec_dlen))
        return set_err(RFEC_EINVAL, "NULL buffer (SIM_FEC)", 0);
    if (misaligned(shards, 16) || misaligned(seg_dgram, 16) || (n && misaligned(fec_dgram, 16)))
        return set_err(RFEC_EINVAL, "shards, seg_dgram and fec_dgram must be 16-byte aligned", 0);
    if (misaligned(hdr, 4) || misaligned(seg_stamps, 4) || misaligned(seg_order, 4) ||
        (n && (misaligned(fec_stamps, 4) || misaligned(fec_order, 4))))
        return set_err(RFEC_EINVAL, "hdr, the stamps and the orders must be 4-byte aligned", 0);
    if (misaligned(seg_dlen, 2) || (n && misaligned(fec_dlen, 2)))
        return set_err(RFEC_EINVAL, "seg_dlen and fec_dlen must be 2-byte aligned", 0);
    if (n == 0)
        fec_order = NULL;
    if (seg_order && (uint64_t)ns * dstride >= WEF_OFFSETS)
        return set_err(RFEC_EINVAL, "with seg_order, the SIM_SEG slots must stay below 4 GiB", 0);
    if (fec_order && (uint64_t)nf * dstride >= WEF_OFFSETS)
        return set_err(RFEC_EINVAL, "with fec_order, the SIM_FEC slots must stay below 4 GiB", 0);
    const uint32_t per = send_groups_per_launch(plan, stride, dstride, seg_order == NULL, fec_order == NULL);
    for (uint32_t g0 = 0; g0 < groups; g0 += per) {
        const uint32_t ng = groups - g0 < per ? groups - g0 : per;
        const size_t r0 = (size_t)g0 * k, d0 = (size_t)g0 * n;
        /* without an order a launch writes its own slots; with it, anywhere in the batch's */
        const int e = rfec_launch_wire_encode_send(
            plan, ng, stride, capacity, shards + r0 * stride, hdr + r0, seg_stamps + r0,
            seg_order ? seg_order + r0 : NULL, seg_order ? seg_dgram : seg_dgram + r0 * dstride,
            seg_order ? seg_dlen : seg_dlen + r0, seg_order ? ns : ng * k, n ? fec_stamps + d0 : NULL,
            fec_order ? fec_order + d0 : NULL, fec_order || !n ? fec_dgram : fec_dgram + d0 * dstride,
            fec_order || !n ? fec_dlen : fec_dlen + d0, fec_order ? nf : ng * n, dstride, stream);
        if (e)
            return set_err(RFEC_EDEVICE, "wire_encode_send launch", e);
    }
    return RFEC_OK;
}

static int send_shapes_err(const char* what, const char* tail)
{
    char msg[160];
    snprintf(msg, sizeof(msg), "%s%s", what, tail);
    return set_err(RFEC_EINVAL, msg, 0);
}

/* rfec_wire_encode_send over a window of several shapes (razor_fec.h): the checks, the plans compacted into the
 * kernel's argument block, one launch. */
int rfec_wire_encode_send_shapes(const rfec_plan* plans, uint32_t n_plans, uint32_t groups,
                                 const rfec_send_group* group, uint32_t n_rows, uint32_t n_fec, uint32_t stride,
                                 uint32_t capacity, const uint8_t* shards, const rfec_hdr* hdr,
                                 const rfec_seg_stamp* seg_stamps, const uint32_t* seg_order, uint8_t* seg_dgram,
                                 uint16_t* seg_dlen, const rfec_fec_stamp* fec_stamps, const uint32_t* fec_order,
                                 uint8_t* fec_dgram, uint16_t* fec_dlen, uint32_t dstride, void* stream)
{
    static const char split[] = " must stay below 0xFFFFFFF0 (32-bit buffer offsets): split the window";
    if (!plans)
        return set_err(RFEC_EINVAL, "plans is NULL", 0);
    if (n_plans < 1 || n_plans > RFEC_SEND_MAX_SHAPES)
        return set_err(RFEC_EINVAL, "n_plans must be in [1, RFEC_SEND_MAX_SHAPES]", 0);
    rfec_send_shapes S;
    uint32_t lines = 0;
    S.n_plans = n_plans;
    for (uint32_t p = 0; p < RFEC_SEND_MAX_SHAPES; ++p)
        S.shape[p] = 0;
    for (uint32_t p = 0; p < n_plans; ++p) {
        const int rc = check_plan(plans + p, RFEC_MAX_K_ENCODE);
        if (rc)
            return rc;
        const uint32_t n = plans[p].n_lines;
        if (lines + n > RFEC_SEND_MAX_LINES)
            return set_err(RFEC_EINVAL, "plans: the sum of n_lines must be <= RFEC_SEND_MAX_LINES", 0);
        S.shape[p] = (uint32_t)plans[p].k | n << 8 | lines << 16;
        for (uint32_t l = 0; l < n; ++l) {
            const rfec_line* ln = &plans[p].line[l];
            S.line[lines + l] = (uint32_t)ln->first | (uint32_t)ln->stride << 8 | (uint32_t)ln->count << 16;
        }
        lines += n;
    }
    for (uint32_t l = lines; l < RFEC_SEND_MAX_LINES; ++l)
        S.line[l] = 0;
    /* the SIM_FEC overhead covers the SIM_SEG's 36 */
    const int rc = check_wire(n_rows > n_fec ? n_rows : n_fec, stride, capacity, dstride, RFEC_WIRE_FEC_OVERHEAD);
    if (rc)
        return rc;
    if (dstride > WEF_MAX_DSTRIDE)
        return set_err(RFEC_EINVAL,
                       "rfec_wire_encode_send_shapes takes dstride <= 1280: use rfec_wire_frame_seg + "
                       "rfec_wire_encode_fec per shape",
                       0);
    if (((uint64_t)n_rows + 4) * stride + WEF_MAX_DSTRIDE >= WEF_OFFSETS)
        return send_shapes_err("(n_rows + 4) * stride + 1280", split);
    if ((uint64_t)n_rows * sizeof(rfec_hdr) >= WEF_OFFSETS)
        return send_shapes_err("n_rows * 20", split);
    if ((uint64_t)n_rows * dstride >= WEF_OFFSETS)
        return send_shapes_err("n_rows * dstride", split);
    if ((uint64_t)n_fec * sizeof(rfec_fec_stamp) >= WEF_OFFSETS)
        return send_shapes_err("n_fec * 24", split);
    if ((uint64_t)n_fec * dstride >= WEF_OFFSETS)
        return send_shapes_err("n_fec * dstride", split);
    if ((uint64_t)groups * sizeof(rfec_send_group) >= WEF_OFFSETS)
        return send_shapes_err("groups * 16", split);
    if (groups == 0)
        return RFEC_OK;
    if (!group)
        return set_err(RFEC_EINVAL, "group is NULL", 0);
    if (!shards || !hdr || !seg_stamps || !seg_dgram || !seg_dlen)
        return set_err(RFEC_EINVAL, "NULL buffer (shards, hdr, seg_stamps, seg_dgram, seg_dlen)", 0);
    if (n_fec && (!fec_stamps || !fec_dgram || !fec_dlen))
        return set_err(RFEC_EINVAL, "NULL buffer (fec_stamps, fec_dgram, fec_dlen)", 0);
    if (misaligned(shards, 16) || misaligned(seg_dgram, 16) || (n_fec && misaligned(fec_dgram, 16)))
        return set_err(RFEC_EINVAL, "shards, seg_dgram and fec_dgram must be 16-byte aligned", 0);
    if (misaligned(group, 4) || misaligned(hdr, 4) || misaligned(seg_stamps, 4) || misaligned(seg_order, 4) ||
        (n_fec && (misaligned(fec_stamps, 4) || misaligned(fec_order, 4))))
        return set_err(RFEC_EINVAL, "group, hdr, seg_stamps, seg_order, fec_stamps and fec_order must be 4-byte aligned",
                       0);
    if (misaligned(seg_dlen, 2) || (n_fec && misaligned(fec_dlen, 2)))
        return set_err(RFEC_EINVAL, "seg_dlen and fec_dlen must be 2-byte aligned", 0);
    if (n_fec == 0)
        fec_order = NULL;
    const int e = rfec_launch_wire_encode_send_shapes(&S, groups, group, n_rows, n_fec, stride, capacity, shards, hdr,
                                                      seg_stamps, seg_order, seg_dgram, seg_dlen, fec_stamps, fec_order,
                                                      fec_dgram, fec_dlen, dstride, stream);
    return e ? set_err(RFEC_EDEVICE, "wire_encode_send_shapes launch", e) : RFEC_OK;
}
