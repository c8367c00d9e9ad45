/*
 * rx_replay.c -- a stand-alone driver of the receiver session's host control
 * plane, linked with the C host layer and stub_hip.c into an executable that
 * the sanitizers can check (tests/test_rx_shards.py builds it with
 * -fsanitize=address,undefined and with -fsanitize=thread).
 *
 *   rx_replay RECORDS OUT BATCH THREADS EVICT_EVERY
 *
 * RECORDS: a file of rfec_wire_rec (64 B each), pushed through
 * rfec_rx_session_push in batches of BATCH records over THREADS shards, with
 * rfec_rx_session_evict after every EVICT_EVERY records (0: never; batches
 * end there).  OUT: uint32 n, max_ts, the summed n_fec_dropped, then the n
 * delivered rfec_rx_seg in delivery order.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "razor_fec.h"

#define CAP 16u /* payload capacity = row stride: the control plane reads sizes only */

static int fail(const char* what)
{
    fprintf(stderr, "rx_replay: %s: %s\n", what, rfec_last_error());
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 6) {
        fprintf(stderr, "usage: rx_replay RECORDS OUT BATCH THREADS EVICT_EVERY\n");
        return 2;
    }
    const uint32_t batch = (uint32_t)atol(argv[3]), threads = (uint32_t)atol(argv[4]);
    const uint32_t evict = (uint32_t)atol(argv[5]);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fseek(f, 0, SEEK_END))
        return fail("records file");
    const long bytes = ftell(f);
    rewind(f);
    const uint32_t n = (uint32_t)(bytes / (long)sizeof(rfec_wire_rec));
    rfec_wire_rec* recs = (rfec_wire_rec*)malloc((size_t)n * sizeof(rfec_wire_rec) + 1);
    const uint32_t max_out = 4 * (batch > evict ? batch : evict) + 64;
    uint8_t* pay = (uint8_t*)calloc((size_t)n + 1, CAP);
    rfec_rx_seg* out = (rfec_rx_seg*)malloc((size_t)max_out * sizeof(rfec_rx_seg));
    uint8_t* outp = (uint8_t*)malloc((size_t)max_out * CAP);
    rfec_rx_seg* got = (rfec_rx_seg*)malloc(((size_t)n + 1) * sizeof(rfec_rx_seg));
    if (!recs || !pay || !out || !outp || !got || batch == 0 || fread(recs, sizeof(rfec_wire_rec), n, f) != n)
        return fail("records file / memory");
    fclose(f);
    rfec_rx_session* s = rfec_rx_session_create(CAP, CAP);
    if (!s || rfec_rx_session_set_threads(s, threads))
        return fail("session");
    uint32_t ngot = 0, dropped = 0, nout = 0;
    rfec_rx_report rep;
    for (uint32_t a = 0; a < n;) {
        uint32_t b = n - a < batch ? n : a + batch;
        if (evict && b > (a / evict + 1) * evict)
            b = (a / evict + 1) * evict;
        if (rfec_rx_session_push(s, b - a, recs + a, pay + (size_t)a * CAP, out, outp, max_out, &nout, &rep, NULL))
            return fail("push");
        if (rep.n_unmodelled || ngot + nout > n)
            return fail("unmodelled deliveries");
        memcpy(got + ngot, out, (size_t)nout * sizeof(rfec_rx_seg));
        ngot += nout;
        dropped += rep.n_fec_dropped;
        if (evict && b % evict == 0 && rfec_rx_session_evict(s, NULL))
            return fail("evict");
        a = b;
    }
    rfec_rx_session_info info;
    if (rfec_rx_session_get_info(s, &info))
        return fail("info");
    rfec_rx_session_destroy(s);
    const uint32_t head[3] = {ngot, info.max_ts, dropped};
    f = fopen(argv[2], "wb");
    if (!f || fwrite(head, sizeof(head), 1, f) != 1 || fwrite(got, sizeof(rfec_rx_seg), ngot, f) != ngot || fclose(f))
        return fail("output file");
    free(recs);
    free(pay);
    free(out);
    free(outp);
    free(got);
    return 0;
}
