/*
 * rfec_wire_census.c -- rfec_wire_window_census (razor_fec.h, wire codec): the
 * shapes of a parsed window and the groups of each, on the device
 * (rfec_census.hip): argument checks, all before any runtime call, then the
 * launches through rfec_launch_wire_census.
 *
 * Not one of build.py's HOST_SRC: the CPU builds of the host layer link
 * against a stub of the HIP runtime, which has no launch shims.
 */
#include "razor_fec.h"
#include "rfec_internal.h"
#include "rfec_host_internal.h"

int rfec_wire_window_census(uint32_t groups, uint16_t fec_id0, uint32_t n, const rfec_wire_rec* recs,
                            uint32_t capacity, rfec_window_census* census, uint32_t* anchor_of, uint32_t* key_of,
                            void* stream)
{
    if (fec_id0 == 0)
        return set_err(RFEC_EINVAL, "fec_id0 must not be 0 (the sender skips it)", 0);
    if (groups > 65535u)
        return set_err(RFEC_EINVAL, "groups must be <= 65535 (the fec_ids of one succession)", 0);
    if (n > 0x7FFFFFFFu)
        return set_err(RFEC_EINVAL, "n must be <= 0x7FFFFFFF", 0);
    if (capacity > 65535u)
        return set_err(RFEC_EINVAL, "capacity must be <= 65535 (data_size is 16 bits)", 0);
    if (groups == 0)
        return RFEC_OK;
    if (n && !recs)
        return set_err(RFEC_EINVAL, "recs is NULL", 0);
    if (!census)
        return set_err(RFEC_EINVAL, "census is NULL", 0);
    if (!anchor_of)
        return set_err(RFEC_EINVAL, "anchor_of is NULL", 0);
    if (!key_of)
        return set_err(RFEC_EINVAL, "key_of is NULL", 0);
    if (misaligned(recs, 16))
        return set_err(RFEC_EINVAL, "recs must be 16-byte aligned", 0);
    if (misaligned(census, 16))
        return set_err(RFEC_EINVAL, "census must be 16-byte aligned", 0);
    if (misaligned(anchor_of, 4))
        return set_err(RFEC_EINVAL, "anchor_of must be 4-byte aligned", 0);
    if (misaligned(key_of, 4))
        return set_err(RFEC_EINVAL, "key_of must be 4-byte aligned", 0);
    const int e = rfec_launch_wire_census(groups, fec_id0, n, recs, capacity, census, anchor_of, key_of, stream);
    return e ? set_err(RFEC_EDEVICE, "wire_window_census launch", e) : RFEC_OK;
}
