// rfec_regroup_rules.h -- the placement rules of razor_fec.h ("The placement rule") as device code, one copy for
// rfec_regroup.hip (one shape) and rfec_regroup_shapes.hip (a window of several): how a parsed record is read,
// which records take part, the group a fec_id names, and what the winner of a slot and the slots of a group leave
// in the tables.  rfec_deliver.hip takes the window's succession of fec_ids from here.  C++ only, not installed;
// everything is forced inline.
#ifndef RFEC_REGROUP_RULES_H_
#define RFEC_REGROUP_RULES_H_

#include "rfec_device.h"

constexpr uint32_t kNone = RFEC_REGROUP_NONE;

static_assert(sizeof(rfec_wire_rec) == 64 && sizeof(rfec_hdr) == 20, "record layouts");
// rfec_wire_rec as sixteen 32-bit words (razor_fec.h): 0 status | ver | mid | remb, 2-6 hdr (2 = seq), 7 base_id,
// 9 fec_id | count, 10 transport_seq | data_size, 11 row | col | index
struct Rec {
    uint32_t tag, seq, base_id, fec_id, count, data_size, shape; // shape: row | col << 8 | index << 16
};
__device__ __forceinline__ Rec load_rec(const rfec_wire_rec* __restrict__ recs, uint32_t r)
{
    const v4u* p = reinterpret_cast<const v4u*>(recs + r); // 16-byte aligned (checked by the entry point)
    const v4u a = p[0], b = p[1], c = p[2];
    Rec R;
    R.tag = a.x;
    R.seq = a.z;
    R.base_id = b.w;
    R.fec_id = c.y & 0xFFFFu;
    R.count = c.y >> 16;
    R.data_size = c.z >> 16;
    R.shape = c.w & 0xFFFFFFu;
    return R;
}

// the base_id of record a (an anchor)
__device__ __forceinline__ uint32_t base_id_of(const rfec_wire_rec* __restrict__ recs, uint32_t a)
{
    return reinterpret_cast<const uint32_t*>(recs + a)[7];
}

// 0 = ENOTFEC, else the mid (status == RFEC_WIRE_OK and SIM_SEG or SIM_FEC)
__device__ __forceinline__ uint32_t kind_of(uint32_t tag)
{
    const uint32_t mid = (tag >> 16) & 0xFFu;
    return (tag & 0xFFu) == RFEC_WIRE_OK && (mid == RFEC_WIRE_SEG || mid == RFEC_WIRE_FEC) ? mid : 0u;
}

// the window rule: the group index of fec_id counted from fec_id0 in the sender's succession, or kNone (EWINDOW)
__device__ __forceinline__ uint32_t group_of(uint32_t fec_id, uint32_t fec_id0, uint32_t groups)
{
    if (fec_id == 0)
        return kNone;
    const uint32_t g = fec_id >= fec_id0 ? fec_id - fec_id0 : fec_id + 65535u - fec_id0;
    return g < groups ? g : kNone;
}

// its inverse: the fec_id of window group g < 65535, ((fec_id0 - 1 + g) % 65535) + 1 (rfec_recover_deliver's entries)
__device__ __forceinline__ uint32_t fec_id_of(uint32_t fec_id0, uint32_t g)
{
    const uint32_t id = fec_id0 + g;
    return id > 65535u ? id - 65535u : id;
}

// a slot's lane: the header record of the slot's winner (w: the winner's record as words) to h, and a parity's
// size to *fec_size
__device__ __forceinline__ void place_record(const uint32_t* w, uint32_t* h, bool parity, uint16_t* fec_size)
{
#pragma unroll
    for (int q = 0; q < 5; ++q)
        h[q] = w[2 + q];
    if (parity)
        *fec_size = (uint16_t)(w[10] >> 16);
}

// a group's lane: present[2] and parity_present from the group's k + n_lines words of src_of
// (returned, not stored: the callers load their table pointers after the loops, as the loops need the registers)
struct SlotMasks {
    uint64_t present[2], parity_present;
};
__device__ __forceinline__ SlotMasks slot_masks(const uint32_t* so, uint32_t k, uint32_t n_lines)
{
    uint64_t m0 = 0, m1 = 0, pp = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t bit = so[i] != kNone;
        if (i < 64)
            m0 |= bit << i;
        else
            m1 |= bit << (i - 64);
    }
    for (uint32_t l = 0; l < n_lines; ++l)
        pp |= (uint64_t)(so[k + l] != kNone) << l;
    return SlotMasks{{m0, m1}, pp};
}

#endif
