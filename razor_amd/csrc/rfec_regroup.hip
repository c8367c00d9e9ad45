// rfec_regroup.hip -- CDNA4 (gfx950) kernels of rfec_wire_regroup (razor_fec.h, wire codec): the records and
// payload rows rfec_wire_parse left in arrival order, placed into the batch layout rfec_recover_batch[_out]
// reads (shards / hdr / present, parity / meta / fec_size / parity_present), on the device.
//
// The placement is a pure function of the records (razor_fec.h, "The placement rule"): group = fec_id counted
// from fec_id0 in the sender's succession (flex_fec_sender.c:241-243), member = packet_id - base_id, line = the
// SIM_FEC's index, base_id from the group's first shape-accepted parity (sim_fec.c:152-163,
// flex_fec_receiver.c:69-78, :255-266), the lowest arrival index winning a slot (sim_fec.c:180-182,
// flex_fec_receiver.c:222-224, :258-260).  "First" and "lowest" are minima over arrival indices, so they are
// taken with atomicMin on 32-bit words and come out the same however the lanes are scheduled.
//
// Four launches on the caller's stream; no launch has a lane read, other than by an atomic, a word that another
// lane of that launch writes (a launch boundary makes the words of the launch before visible):
//   k_regroup_fill     src_of[G (k + n)] and the anchor word of every group (base_id[g], scratch until the last
//                      launch) <- 0xFFFFFFFF
//   k_regroup_anchor   one lane per record: a shape-accepted SIM_FEC does atomicMin(anchor[g], arrival index)
//   k_regroup_contend  one lane per record: rules 1-6 with the anchor's base_id; a contender does
//                      atomicMin(src_of[slot], arrival index) and notes its slot in slot_of (a refused record its
//                      code)
//   k_regroup_place    the hot path, one grid: a lane per (slot, 16-byte chunk j < CD) copies the winner's payload
//                      row into the slot (src_of is the row map: the lanes of a slot read one word, then stream
//                      the row; the destination is walked in order, the source gathered); ahead of them in the
//                      grid, so that their scattered accesses run beside the rows' streams and not after them
//                      (1-4 % of the call), a lane per slot writes hdr / meta / fec_size from the winner's record,
//                      a lane per group the two masks and base_id, a lane per record turns a beaten contender's
//                      slot_of into EDUP
// rfec_wire_regroup_index is the same call without the row lanes: the tables alone, src_of then being the row map
// of rfec_recover_indexed_out.
// The rows are loaded non-temporally (each is read once) and stored with the default policy: the decode reads
// them next.  Row and record addresses are 64-bit (records x stride passes 4 GiB on the large shapes).
#include "rfec_regroup_rules.h"

namespace {

struct RgArgs {
    const rfec_wire_rec* recs;
    uint32_t n, groups, fec_id0, capacity;
    uint32_t k, n_lines, slots; // slots = k + n_lines per group
    uint32_t rowcol;            // plan row | col << 8
    uint32_t* anchor;           // base_id[G], the anchors' arrival indices until k_regroup_place
    uint32_t* src_of;
    int32_t* slot_of;
    uint8_t index[RFEC_MAX_LINES]; // plan->line[l].index
};

// (rule 1: kind_of; rule 2: group_of -- rfec_regroup_rules.h)
// rule 3: the line of a shape-accepted SIM_FEC, or kNone (ESHAPE)
__device__ __forceinline__ uint32_t line_of(const Rec& R, const RgArgs& A)
{
    if (R.count != A.k || (R.shape & 0xFFFFu) != A.rowcol || R.data_size > A.capacity)
        return kNone;
    const uint32_t index = R.shape >> 16;
    for (uint32_t l = 0; l < A.n_lines; ++l)
        if (A.index[l] == index)
            return l;
    return kNone;
}

__global__ __launch_bounds__(kBlock) void k_regroup_fill(uint32_t* __restrict__ src_of, uint32_t n_src,
                                                         uint32_t* __restrict__ anchor, uint32_t groups)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < n_src)
        src_of[t] = kNone;
    else if (t - n_src < groups)
        anchor[t - n_src] = kNone;
}

__global__ __launch_bounds__(kBlock) void k_regroup_anchor(const RgArgs A)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= A.n)
        return;
    const Rec R = load_rec(A.recs, r);
    if (kind_of(R.tag) != RFEC_WIRE_FEC)
        return;
    const uint32_t g = group_of(R.fec_id, A.fec_id0, A.groups);
    if (g == kNone || line_of(R, A) == kNone)
        return;
    atomicMin(A.anchor + g, r);
}

__global__ __launch_bounds__(kBlock) void k_regroup_contend(const RgArgs A)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= A.n)
        return;
    const Rec R = load_rec(A.recs, r);
    const uint32_t kind = kind_of(R.tag);
    int32_t res;
    uint32_t g = kNone, s = kNone;
    if (!kind)
        res = RFEC_REGROUP_ENOTFEC;
    else if ((g = group_of(R.fec_id, A.fec_id0, A.groups)) == kNone)
        res = RFEC_REGROUP_EWINDOW;
    else if (kind == RFEC_WIRE_FEC) {
        const uint32_t l = line_of(R, A);
        if (l == kNone)
            res = RFEC_REGROUP_ESHAPE;
        else {
            const uint32_t a = A.anchor[g]; // <= r: this record is shape-accepted itself
            const uint32_t base = a == r ? R.base_id : base_id_of(A.recs, a);
            res = R.base_id == base ? 0 : RFEC_REGROUP_EBASE;
            s = A.k + l;
        }
    } else {
        const uint32_t a = A.anchor[g];
        if (a == kNone)
            res = RFEC_REGROUP_ENOPARITY;
        else {
            s = R.seq - base_id_of(A.recs, a); // unsigned: a packet id below the base is far above k
            res = s < A.k ? 0 : RFEC_REGROUP_EBASE;
        }
    }
    if (res == 0) {
        const uint32_t slot = g * A.slots + s; // < 65535 * 192
        atomicMin(A.src_of + slot, r);
        res = (int32_t)slot;
    }
    A.slot_of[r] = res;
}

struct PlaceArgs {
    const v4u* payload;
    v4u* shards;
    v4u* parity;
    rfec_hdr* hdr;
    rfec_hdr* meta;
    uint16_t* fec_size;
    uint64_t* present;
    uint64_t* parity_present;
    uint32_t C, CD;        // 16-byte chunks per row, and of them the ones a call works on
    uint32_t n_rows, n_slots; // n_slots = G (k + n), n_rows = n_slots CD
    FastDiv divCD, divSlots;
};

__global__ __launch_bounds__(kBlock) void k_regroup_place(const RgArgs A, const PlaceArgs P)
{
    uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n_tab = P.n_slots + A.groups + A.n; // the tables' lanes lead the grid
    if (t >= n_tab) { // (slot, chunk): the winner's row into the slot
        t -= n_tab;
        if (t >= P.n_rows)
            return;
        const uint32_t slot = fdiv(t, P.divCD), j = t - slot * P.CD;
        const uint32_t a = A.src_of[slot];
        if (a == kNone)
            return;
        const uint32_t g = fdiv(slot, P.divSlots), s = slot - g * A.slots;
        const v4u v = ld16(P.payload + (size_t)a * P.C + j);
        v4u* dst = s < A.k ? P.shards + ((size_t)g * A.k + s) * P.C : P.parity + ((size_t)g * A.n_lines + (s - A.k)) * P.C;
        dst[j] = v;
        return;
    }
    if (t < P.n_slots) { // slot: the winner's header record (and a parity's size)
        const uint32_t a = A.src_of[t];
        if (a == kNone)
            return;
        const uint32_t g = fdiv(t, P.divSlots), s = t - g * A.slots;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(A.recs + a);
        const bool seg = s < A.k;
        const size_t o = seg ? (size_t)g * A.k + s : (size_t)g * A.n_lines + (s - A.k);
        place_record(w, reinterpret_cast<uint32_t*>((seg ? P.hdr : P.meta) + o), !seg, P.fec_size + o);
        return;
    }
    t -= P.n_slots;
    if (t < A.groups) { // group: the masks, and the anchor's base_id in place of its arrival index
        const SlotMasks m = slot_masks(A.src_of + (size_t)t * A.slots, A.k, A.n_lines);
        P.present[2 * (size_t)t] = m.present[0];
        P.present[2 * (size_t)t + 1] = m.present[1];
        P.parity_present[t] = m.parity_present;
        const uint32_t a = A.anchor[t];
        A.anchor[t] = a == kNone ? 0u : base_id_of(A.recs, a);
        return;
    }
    t -= A.groups;
    if (t < A.n) { // record: a contender that did not win its slot
        const int32_t s = A.slot_of[t];
        if (s >= 0 && A.src_of[s] != t)
            A.slot_of[t] = RFEC_REGROUP_EDUP;
    }
}

} // namespace

// The caller (rfec_wire_regroup.c) has checked the plan (k <= RFEC_MAX_K), groups in [1, 65535], n < 2^31, stride a
// multiple of 16, capacity <= stride and the pointers.  Lane counts: G (k + n_lines) CD < 65535 * 192 * 128 < 2^31
// (the dividends of the fast divisions), and with the slots', the groups' and the records' lanes below 2^32.
//
// copy_rows false (rfec_wire_regroup_index): the same four launches with no (slot, chunk) lane in k_regroup_place's
// grid, so no payload row is read or written (payload, shards, parity and stride are not used).
static int launch_regroup(const rfec_kplan* P, uint32_t groups, uint32_t fec_id0, uint32_t n,
                          const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride, uint32_t capacity,
                          uint8_t* shards, rfec_hdr* hdr, uint64_t* present, uint8_t* parity, rfec_hdr* meta,
                          uint16_t* fec_size, uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                          int32_t* slot_of, void* stream, bool copy_rows)
{
    const uint32_t k = P->k, nl = P->n_lines, slots = k + nl;
    if (!groups || groups > 65535u || !k || k > RFEC_MAX_K || nl > RFEC_MAX_LINES || n > 0x7FFFFFFFu ||
        (copy_rows && (!stride || stride % 16 || capacity > stride || stride > 16u * 128u)))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t C = stride / 16, CD = copy_rows && capacity ? (capacity + 15) / 16 : 1;
    RgArgs A;
    A.recs = recs;
    A.n = n;
    A.groups = groups;
    A.fec_id0 = fec_id0;
    A.capacity = capacity;
    A.k = k;
    A.n_lines = nl;
    A.slots = slots;
    A.rowcol = (uint32_t)P->row | (uint32_t)P->col << 8;
    A.anchor = base_id;
    A.src_of = src_of;
    A.slot_of = slot_of;
    for (uint32_t l = 0; l < RFEC_MAX_LINES; ++l)
        A.index[l] = l < nl ? P->line[l].index : 0;
    const uint32_t n_slots = groups * slots;
    RFEC_LAUNCH(k_regroup_fill, dim3(blocks_for((uint64_t)n_slots + groups)), dim3(kBlock), 0, st, src_of, n_slots,
                base_id, groups);
    if (n) {
        RFEC_LAUNCH(k_regroup_anchor, dim3(blocks_for(n)), dim3(kBlock), 0, st, A);
        RFEC_LAUNCH(k_regroup_contend, dim3(blocks_for(n)), dim3(kBlock), 0, st, A);
    }
    PlaceArgs Q;
    Q.payload = reinterpret_cast<const v4u*>(payload);
    Q.shards = reinterpret_cast<v4u*>(shards);
    Q.parity = reinterpret_cast<v4u*>(parity);
    Q.hdr = hdr;
    Q.meta = meta;
    Q.fec_size = fec_size;
    Q.present = present;
    Q.parity_present = parity_present;
    Q.C = C;
    Q.CD = CD;
    Q.n_slots = n_slots;
    Q.n_rows = copy_rows ? n_slots * CD : 0u;
    Q.divCD = make_fastdiv(CD);
    Q.divSlots = make_fastdiv(slots);
    RFEC_LAUNCH(k_regroup_place, dim3(blocks_for((uint64_t)Q.n_rows + n_slots + groups + n)), dim3(kBlock), 0, st, A,
                Q);
    return (int)hipGetLastError();
}

extern "C" int rfec_launch_wire_regroup(const rfec_kplan* P, uint32_t groups, uint32_t fec_id0, uint32_t n,
                                        const rfec_wire_rec* recs, const uint8_t* payload, uint32_t stride,
                                        uint32_t capacity, uint8_t* shards, rfec_hdr* hdr, uint64_t* present,
                                        uint8_t* parity, rfec_hdr* meta, uint16_t* fec_size,
                                        uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                                        int32_t* slot_of, void* stream)
{
    return launch_regroup(P, groups, fec_id0, n, recs, payload, stride, capacity, shards, hdr, present, parity, meta,
                          fec_size, parity_present, base_id, src_of, slot_of, stream, true);
}

extern "C" int rfec_launch_wire_regroup_index(const rfec_kplan* P, uint32_t groups, uint32_t fec_id0, uint32_t n,
                                              const rfec_wire_rec* recs, uint32_t capacity, rfec_hdr* hdr,
                                              uint64_t* present, rfec_hdr* meta, uint16_t* fec_size,
                                              uint64_t* parity_present, uint32_t* base_id, uint32_t* src_of,
                                              int32_t* slot_of, void* stream)
{
    return launch_regroup(P, groups, fec_id0, n, recs, nullptr, 0, capacity, nullptr, hdr, present, nullptr, meta,
                          fec_size, parity_present, base_id, src_of, slot_of, stream, false);
}
