// rfec_device.h -- the device and launch helpers every 256-lane HIP unit shares (C++ only).  Not installed.
// Everything here is forced inline or static: a unit that includes this header gets no symbol from it.
// (rfec_wire.hip runs 1,024-lane blocks and keeps its own definitions.)
#ifndef RFEC_DEVICE_H_
#define RFEC_DEVICE_H_

#include <hip/hip_runtime.h>

#include "rfec_internal.h"
#include "rfec_launch.h"

constexpr int kBlock = 256;
constexpr int kWave = 64;

// CUTLASS-style fast unsigned division for dividends < 2^31.
struct FastDiv {
    uint32_t d, m, s;
};

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f)
{
    uint64_t hi = __umulhi(n, f.m);
    return (uint32_t)((hi + n) >> f.s);
}

// native 16-byte vector (the nontemporal builtins need a clang vector type)
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// payload streams: non-temporal loads and stores (every byte is touched once)
__device__ __forceinline__ v4u ld16(const v4u* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st16(v4u* p, v4u v) { __builtin_nontemporal_store(v, p); }

// Predicated member loads of the decodes: a buffer descriptor over the wave's
// first group (wave-uniform base, made provably uniform by readfirstlane) and
// per-lane byte offsets; a load that is not wanted takes kNoLoad, past the
// descriptor's range, and returns zeros without touching memory.  No branch
// and no redundant request: with per-load branches hipcc waited on each load
// before the next (c3 decode 130 us), with loads redirected to an address
// already in flight it issued 25-150 % more requests (127 us).
constexpr uint32_t kNoLoad = 0x7FFFFFF0u;
constexpr int kAuxNT = 2; // gfx950 cache-policy bits: nt
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_rsrc(const void* p)
{
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((uint64_t)hi << 32 | lo), 0, (int)kNoLoad,
                                             0x00020000);
}
__device__ __forceinline__ v4u bld16(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    return __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kAuxNT));
}
__device__ __forceinline__ v4u bld16_l2(__amdgpu_buffer_rsrc_t r, uint32_t off) // default policy (kept in L2)
{
    return __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

// Payload-block index, XCD-swizzled.  Workgroups are dispatched round-robin
// over the 8 XCDs (block b runs on XCD b % 8, each XCD with its own L2); the
// swizzle gives every XCD one contiguous range of logical blocks, so a cache
// line shared by neighbouring blocks is fetched into one L2.  The tail beyond
// the last multiple of 8 keeps the identity mapping (a bijection).
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb)
{
    const uint32_t nb8 = nb & ~7u;
    if (b >= nb8)
        return b;
    return (b & 7u) * (nb8 >> 3) + (b >> 3);
}

// Header / meta blocks spread in rounds of 8 blocks (one per XCD: block b runs on XCD
// b % 8) for the XCD-swizzled decodes: the first round of every (every + 1) is
// a round of 8 header blocks until n_hr of them ran, so the payload blocks fill
// whole rounds and payload block p (in payload order) runs on XCD p % 8; it
// then takes logical block xcd_block(p): consecutive logical blocks share an
// XCD's L2 (the 128-B lines split between neighbouring slots are fetched once)
// and XCD x sweeps its eighth of the groups in order.  XCD x's header blocks
// are x n_hr + 0, 1, ...: the groups its own payload rounds reach next, so the
// header blocks' reads of the masks come in through the same L2 just before
// the payload lanes read them (the cascade decode: 128.3-128.8 vs 129.4-130.3
// us with header block per * 8 + x, last in each period).
// npay8: payload blocks rounded up to a multiple of 8.
__device__ __forceinline__ bool header_block_xcd(uint32_t n_hr, uint32_t every, uint32_t npay8, uint32_t* hb,
                                                 uint32_t* pb)
{
    const uint32_t R = blockIdx.x >> 3, x = blockIdx.x & 7u;
    uint32_t pr;
    if (!every) {
        if (R < n_hr) {
            *hb = x * n_hr + R;
            return true;
        }
        pr = R - n_hr;
    } else {
        const uint32_t per = R / (every + 1);
        if (per < n_hr && R == per * (every + 1)) {
            *hb = x * n_hr + per;
            return true;
        }
        pr = R - min(per + 1, n_hr);
    }
    *pb = xcd_block(pr * 8u + x, npay8);
    return false;
}

// header_block_xcd for a grid that starts at a multiple of 8 inside a larger one (k_decode_shapes_indexed: one
// such grid per section): b is the block's index relative to the grid's first block, so b % 8 is still its XCD.
__device__ __forceinline__ bool header_block_xcd_at(uint32_t b, uint32_t n_hr, uint32_t every, uint32_t npay8,
                                                    uint32_t* hb, uint32_t* pb)
{
    const uint32_t R = b >> 3, x = b & 7u;
    uint32_t pr;
    if (!every) {
        if (R < n_hr) {
            *hb = x * n_hr + R;
            return true;
        }
        pr = R - n_hr;
    } else {
        const uint32_t per = R / (every + 1);
        if (per < n_hr && R == per * (every + 1)) {
            *hb = x * n_hr + per;
            return true;
        }
        pr = R - min(per + 1, n_hr);
    }
    *pb = xcd_block(pr * 8u + x, npay8);
    return false;
}

// Header blocks of the fused decodes: every (every + 1)-th block until they
// run out (every == 0: the first n_hdr of the grid), spread over the grid so
// their latency-bound chains overlap the payload stream (cold: k = 32 / 256 B
// 41.6 vs 46.9 us at the head; k = 10 / 1,200 B 139.4-141.1 vs 144.0-144.4
// us).  Returns true with *hb = header block index, else false with *pb =
// payload block index.
__device__ __forceinline__ bool header_block(uint32_t n_hdr, uint32_t every, uint32_t* hb, uint32_t* pb)
{
    const uint32_t b = blockIdx.x;
    if (!every) {
        *hb = b;
        *pb = b - n_hdr;
        return b < n_hdr;
    }
    const uint32_t per = b / (every + 1);
    *hb = per;
    *pb = b - min(per, n_hdr);
    return per < n_hdr && b - per * (every + 1) == every;
}

// Copies n dwords global -> LDS with the whole block (nt lanes), several loads
// in flight per lane: the loads go through a buffer descriptor over exactly
// the n dwords, so a lane past the end reads zeros with no branch around the
// load (hipcc waited on each guarded load before issuing the next).  `lds`
// must be 16-byte aligned; 16-byte loads are used when `src` is too.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const void* p, uint32_t nbytes)
{
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>((uint64_t)hi << 32 | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane((int)nbytes), 0x00020000);
}

__device__ __forceinline__ void stage_dwords(uint32_t* lds, const uint32_t* __restrict__ src, uint32_t n,
                                             uint32_t nt = kBlock)
{
    constexpr int U = 4;
    const __amdgpu_buffer_rsrc_t r = span_rsrc(src, n * 4u);
    const uint32_t nv = ((reinterpret_cast<uintptr_t>(src) & 15) == 0) ? n / 4 : 0;
    v4u* d4 = reinterpret_cast<v4u*>(lds);
    for (uint32_t base = 0; base < nv; base += U * nt) {
        v4u tmp[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            tmp[u] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(
                                                 r, (base + u * nt + threadIdx.x) * 16u, 0, 0));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = base + u * nt + threadIdx.x;
            if (i < nv)
                d4[i] = tmp[u];
        }
    }
    for (uint32_t base = nv * 4; base < n; base += 4 * U * nt) {
        uint32_t tmp[4 * U];
#pragma unroll
        for (int u = 0; u < 4 * U; ++u)
            tmp[u] = __builtin_amdgcn_raw_buffer_load_b32(r, (base + u * nt + threadIdx.x) * 4u, 0, 0);
#pragma unroll
        for (int u = 0; u < 4 * U; ++u) {
            const uint32_t i = base + u * nt + threadIdx.x;
            if (i < n)
                lds[i] = tmp[u];
        }
    }
}

static inline FastDiv make_fastdiv(uint32_t d)
{
    FastDiv f;
    f.d = d;
    f.s = rfec_ceil_log2(d);
    f.m = (uint32_t)(((1ull << 32) * ((1ull << f.s) - d)) / d + 1);
    return f;
}

static inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// The grid of header_block_xcd's decodes: hdr_rounds rounds of 8 header blocks spread over the payload blocks,
// these rounded up to whole rounds.  The row decodes (k_decode_rows*) take the header BLOCKS and derive the rounds
// themselves, the cascade and matrix decodes the header ROUNDS: a call site names the field its kernel wants.
struct Rounds8 {
    uint32_t hdr_blocks, hdr_rounds; // header blocks as given; rounds of 8 that hold them
    uint32_t npay8, every;           // payload blocks in whole rounds of 8; payload rounds per header round
    uint32_t grid;
};

static inline Rounds8 rounds_of_8(uint32_t hdr_blocks, uint32_t pay_blocks)
{
    Rounds8 g;
    g.hdr_blocks = hdr_blocks;
    g.hdr_rounds = (hdr_blocks + 7u) >> 3;
    g.npay8 = (pay_blocks + 7u) & ~7u;
    g.every = g.hdr_rounds ? (g.npay8 >> 3) / g.hdr_rounds : 0u;
    g.grid = 8u * g.hdr_rounds + g.npay8;
    return g;
}

#endif
