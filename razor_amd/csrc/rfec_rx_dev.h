/*
 * rfec_rx_dev.h -- the device side of receiver ingestion (rfec_rx_dev.c), for
 * the receiver sessions (rfec_rx_session.c).
 */
#ifndef RFEC_RX_DEV_H
#define RFEC_RX_DEV_H

#include "rfec_host_internal.h"
#include "rfec_rx_plane.h"

#pragma GCC visibility push(hidden)

/* The device address of host memory the device can read directly (pinned:
 * rfec_pinned_alloc, hipHostMalloc, registered), else NULL (pageable: the
 * caller copies).  A failed query leaves no pending HIP error behind. */
const uint8_t* host_mapped(const void* p);
/* the calling thread's own stream (created on first use) */
int rx_recv_stream(hipStream_t* sm);
/* The device side of one call over the T shards XS (plan: rx_plan; run: the
 * staging, the peel, the delivered rows copied out).  `pool`: fills the
 * tables on the replay threads, or NULL. */
int rx_device(rx_sim* const* XS, uint32_t T, rx_pool* pool, rx_dev* D, const uint8_t* rows, uint32_t stride,
              uint32_t capacity, size_t hoff, int r_stage, rfec_rx_seg* out, uint8_t* out_payload, uint32_t max_out,
              uint32_t* n_out, rfec_rx_report* rep, hipStream_t sm);

#pragma GCC visibility pop

#endif
