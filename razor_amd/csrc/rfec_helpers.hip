// rfec_helpers.hip -- the receiver's helper kernels (gfx950) and their extern "C" launch shims: the batch split
// of parsed records, the row gathers, the ingestion stage, the line jobs of groups above RFEC_MAX_K segments
// and the zeroing of slot tails.  Payload rows move as 16-byte chunks, one lane per chunk.
#include "rfec_device.h"

namespace {

// The receiver session's batch split (rfec_rx.c rx_phase0), one lane per
// parsed record: the host then reads 8 bytes per record instead of the 64-B
// records the parse just wrote (cache-cold on the host), and the replay
// threads take those cache misses in parallel.  Reads only the fields the
// split needs (status, mid, seq, ts, send_ts, fec_id; rfec_wire_rec layout).
__global__ __launch_bounds__(kBlock) void k_rx_split(const rfec_wire_rec* __restrict__ recs, uint32_t n, uint32_t T,
                                                    rfec_rx_split* __restrict__ out)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n)
        return;
    static_assert(offsetof(rfec_wire_rec, mid) == 2 && offsetof(rfec_wire_rec, hdr) == 8 &&
                      offsetof(rfec_wire_rec, send_ts) == 32 && offsetof(rfec_wire_rec, fec_id) == 36 &&
                      sizeof(rfec_rx_split) == 8,
                  "record layout");
    const uint32_t* r = reinterpret_cast<const uint32_t*>(recs + p);
    const uint32_t w0 = r[0], seq = r[2], ts = r[4], send_ts = r[8], fec_id = r[9] & 0xFFFFu;
    const int8_t status = (int8_t)(w0 & 0xFFu);
    const uint32_t mid = (w0 >> 16) & 0xFFu;
    uint32_t shard = 0xFFu, kind = RX_SPLIT_NONE, value = 0;
    if (status == RFEC_WIRE_OK && mid == RFEC_WIRE_SEG) {
        shard = (fec_id ? fec_id : seq) % T;
        kind = fec_id && seq ? RX_SPLIT_SEG_TS : RX_SPLIT_SEG;
        value = ts;
    } else if (status == RFEC_WIRE_OK && mid == RFEC_WIRE_FEC) {
        shard = fec_id % T;
        kind = RX_SPLIT_FEC;
        value = send_ts + 3000u;
    }
    uint2 o;
    o.x = shard | kind << 8;
    o.y = value;
    *reinterpret_cast<uint2*>(out + p) = o;
}

// dst row r <- src row map[r] (all `C` 16-B chunks), or zeros for map[r] < 0:
// the receiver's scatter of parsed payloads into group slots and its gather
// of recovered segments.  One lane per chunk, streaming.
__global__ __launch_bounds__(kBlock) void k_gather_rows(v4u* __restrict__ dst, const v4u* __restrict__ src,
                                                        const int32_t* __restrict__ map, uint32_t total, uint32_t C,
                                                        FastDiv divC)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t r = fdiv(t, divC);
    const uint32_t j = t - r * C;
    const int32_t s = map[r];
    const v4u v = s >= 0 ? ld16(src + (size_t)s * C + j) : v4u{0, 0, 0, 0};
    st16(dst + (size_t)r * C + j, v);
}

// The receiver session's device stage of one ingestion call (rfec_rx.c
// rx_device): the delivering groups' member and parity rows gathered from the
// row arena by a map the host wrote into pinned memory (read over PCIe by the
// lanes themselves), and, by the lanes after them, the host's tables (header
// records, masks, sizes, the output map) copied from pinned into device
// memory -- one launch where an H2D copy and two gathers ran in sequence (each
// step a few us of dispatch latency for ~5 MB of rows per 4,096-datagram
// batch).  The rows are stored with the default policy: the decode reads them
// next.
__global__ __launch_bounds__(kBlock) void k_rx_stage(v4u* __restrict__ dst, const v4u* __restrict__ src,
                                                     const int32_t* __restrict__ map, uint32_t total, uint32_t C,
                                                     FastDiv divC, v4u* __restrict__ tdst,
                                                     const v4u* __restrict__ tsrc, uint32_t tchunks)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < total) {
        const uint32_t r = fdiv(t, divC);
        const uint32_t j = t - r * C;
        const int32_t s = map[r];
        dst[(size_t)r * C + j] = s >= 0 ? ld16(src + (size_t)s * C + j) : v4u{0, 0, 0, 0};
        return;
    }
    const uint32_t u = t - total;
    if (u < tchunks)
        tdst[u] = tsrc[u];
}

// Receiver groups above RFEC_MAX_K segments (a foreign peer's flexes): one
// line job per recovered segment, recovered = parity ^ the line's present
// members (flex_fec_xor.c:73-95), the host's peel in dependency levels (one
// launch per level: a job reads only arrived rows and outputs of earlier
// levels).  One lane per (job, 16-byte column); member code m >= 0: row m of
// `rows`, m < 0: output row -1 - m.
__global__ __launch_bounds__(kBlock) void k_line_jobs(const rfec_line_job* __restrict__ jobs,
                                                      const int32_t* __restrict__ members,
                                                      const v4u* __restrict__ rows, v4u* outrows, uint32_t total,
                                                      uint32_t C, FastDiv divC)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t q = fdiv(t, divC);
    const uint32_t j = t - q * C;
    const rfec_line_job J = jobs[q];
    v4u acc = ld16(rows + (size_t)J.parity * C + j);
    uint32_t i = 0;
    for (; i + 4 <= J.n_members; i += 4) { // four loads in flight
        v4u v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t m = members[J.member0 + i + u];
            v[u] = m >= 0 ? rows[(size_t)m * C + j] : outrows[(size_t)(-1 - m) * C + j];
        }
        acc ^= (v[0] ^ v[1]) ^ (v[2] ^ v[3]);
    }
    for (; i < J.n_members; ++i) {
        const int32_t m = members[J.member0 + i];
        acc ^= m >= 0 ? rows[(size_t)m * C + j] : outrows[(size_t)(-1 - m) * C + j];
    }
    outrows[(size_t)J.out * C + j] = acc;
}

// Zero bytes [data_size, stride) of every slot.
__global__ __launch_bounds__(kBlock) void k_zero_tails(v4u* shards, const rfec_hdr* __restrict__ hdr,
                                                       uint32_t total, uint32_t C, FastDiv divC)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total)
        return;
    const uint32_t slot = fdiv(t, divC);
    const uint32_t j = t - slot * C;
    const uint32_t size = hdr[slot].size;
    const uint32_t b0 = j * 16;
    if (b0 + 16 <= size)
        return;
    v4u* p = shards + (size_t)slot * C + j;
    if (b0 >= size) {
        *p = v4u{0, 0, 0, 0};
        return;
    }
    v4u v = *p;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = b0 + 4 * i;
        if (lo >= size)
            v[i] = 0;
        else if (lo + 4 > size)
            v[i] &= (1u << (8 * (size - lo))) - 1u;
    }
    *p = v;
}

} // namespace

extern "C" {

int rfec_launch_line_jobs(const rfec_line_job* jobs, uint32_t n_jobs, const int32_t* members, const uint8_t* rows,
                          uint8_t* outrows, uint32_t stride, void* stream)
{
    if (n_jobs == 0)
        return 0;
    const uint32_t C = stride / 16, total = n_jobs * C; // n_jobs * C < 2^32: host-bounded
    RFEC_LAUNCH(k_line_jobs, dim3(blocks_for(total)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), jobs,
                members, reinterpret_cast<const v4u*>(rows), reinterpret_cast<v4u*>(outrows), total, C,
                make_fastdiv(C));
    return (int)hipGetLastError();
}

int rfec_launch_gather_rows(uint8_t* dst, const uint8_t* src, const int32_t* map, uint32_t rows, uint32_t stride,
                            void* stream)
{
    const uint32_t C = stride / 16;
    const uint32_t total = rows * C;
    if (!total)
        return 0;
    RFEC_LAUNCH(k_gather_rows, dim3(blocks_for(total)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<v4u*>(dst), reinterpret_cast<const v4u*>(src), map, total, C, make_fastdiv(C));
    return (int)hipGetLastError();
}

int rfec_launch_rx_stage(uint8_t* dst, const uint8_t* src, const int32_t* map, uint32_t rows, uint32_t stride,
                         void* tdst, const void* tsrc, size_t tbytes, void* stream)
{
    const uint32_t C = stride / 16;
    const uint64_t total = (uint64_t)rows * C, tchunks = (tbytes + 15) / 16;
    if (total + tchunks >= (1ull << 32) || stride % 16)
        return (int)hipErrorInvalidValue;
    if (!(total + tchunks))
        return 0;
    RFEC_LAUNCH(k_rx_stage, dim3(blocks_for(total + tchunks)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<v4u*>(dst), reinterpret_cast<const v4u*>(src), map, (uint32_t)total, C,
                make_fastdiv(C ? C : 1), reinterpret_cast<v4u*>(tdst), reinterpret_cast<const v4u*>(tsrc),
                (uint32_t)tchunks);
    return (int)hipGetLastError();
}

int rfec_launch_rx_split(const rfec_wire_rec* recs, uint32_t n, uint32_t T, rfec_rx_split* out, void* stream)
{
    if (!n)
        return 0;
    RFEC_LAUNCH(k_rx_split, dim3(blocks_for(n)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), recs, n, T,
                out);
    return (int)hipGetLastError();
}

int rfec_launch_zero_tails(uint32_t slots, uint32_t stride, uint8_t* shards, const rfec_hdr* hdr, void* stream)
{
    const uint32_t C = stride / 16;
    const uint32_t total = slots * C;
    RFEC_LAUNCH(k_zero_tails, dim3(blocks_for(total)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<v4u*>(shards), hdr, total, C, make_fastdiv(C));
    return (int)hipGetLastError();
}

} // extern "C"
