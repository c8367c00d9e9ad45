"""Wire-codec checks shared by the oracle tests (CPU) and the HIP tests (GPU).

An *engine* exposes (numpy in, numpy out, layouts of include/razor_fec.h):
    frame_fec(parity[N][stride], meta[N], fsize[N], status|None, stamps[N], capacity, dstride) -> (dgram, dlen)
    frame_seg(shards[N][stride], hdr[N], stamps[N], capacity, dstride) -> (dgram, dlen)
    parse(dgram[N][dstride], dlen[N], stride, capacity) -> (recs[N], payload[N][stride])
(both framing calls take order=[N] u32: datagram i goes to slot order[i]).  WireEngine below implements it over
guarded arenas: OracleWire on the CPU, gpu_engine.GpuWire on the GPU.

Expected values: tests/golden/wire_*.bin, written by oracle/gen_wire.c from the
reference's sim_encode_msg / sim_decode_header / sim_decode_msg.
"""
from __future__ import annotations

import numpy as np

import guarded_arena as ga
import pyoracle as po

CAP = 1000  # SIM_VIDEO_SIZE of the reference build that wrote the fixtures
STRIDE = 1008

# pre-fills of the outputs (the call must overwrite every byte of them), all different from the arena's canary
DGRAM_FILL, DLEN_FILL, REC_FILL, SPLIT_FILL = 0xEE, 0x77, 0xEE, 0xAB
assert ga.CANARY not in (DGRAM_FILL, DLEN_FILL, REC_FILL, SPLIT_FILL)
SPLIT_DTYPE = np.dtype([("shard", "u1"), ("kind", "u1"), ("reserved", "<u2"), ("value", "<u4")])  # rfec_rx_split

# minimum alignment of each pointer of rfec_wire_frame_fec / _seg, rfec_wire_parse (razor_fec.h, "Alignment") and of
# rfec_launch_wire_parse_split's split entries: the kernels' 16-byte chunk accesses (slots, payloads, records), uint2
# split entries, dword field loads, u16 lengths and sizes, status bytes
WIRE_ALIGN = {"shards": 16, "parity": 16, "dgram": 16, "payload": 16, "recs": 16, "split": 8, "hdr": 4, "meta": 4,
              "stamps": 4, "order": 4, "dlen": 2, "fec_size": 2, "status": 1}


class WireEngine:
    """The engine over guarded arenas (guarded_arena.py): every buffer of a call in one allocation, each at
    exactly WIRE_ALIGN's alignment and between canary guards; after the call every guard byte and every input
    buffer are checked where the memory is.  A subclass supplies the memory (self.be) and the raw calls on an
    arena's addresses (_frame_fec, _frame_seg, _parse).  mutate (tests): called with (arena, call name) after the
    call and before the checks.  last_path: rfec_wire_last_path's tag after the call (0 where there is none);
    last_arena: the call's arena."""

    be = None
    mutate = None
    last_path = 0
    last_arena = None

    def _buf(self, name, nbytes, init, role):
        return ga.Buf(name, nbytes, init, role, WIRE_ALIGN[name])

    def _finish(self, A, what):
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A, what)
        A.check(what)
        self.last_arena = A

    def _frame_out(self, A, N, dstride):
        return A.get("dgram", np.uint8, (N, dstride)), A.get("dlen", np.uint16, (N,))

    def frame_fec(self, parity, meta, fsize, status, stamps, capacity, dstride, order=None):
        stride = parity.shape[-1]
        N = parity.size // stride
        bufs = [self._buf("parity", N * stride, parity, "in"), self._buf("meta", N * 20, meta, "in"),
                self._buf("fec_size", N * 2, np.ascontiguousarray(fsize, np.uint16), "in"),
                self._buf("stamps", N * 24, stamps, "in")]
        if status is not None:
            bufs.append(self._buf("status", N, np.ascontiguousarray(status, np.int8), "in"))
        if order is not None:
            bufs.append(self._buf("order", N * 4, np.ascontiguousarray(order, np.uint32), "in"))
        bufs += [self._buf("dgram", N * dstride, DGRAM_FILL, "out"), self._buf("dlen", N * 2, DLEN_FILL, "out")]
        A = ga.Arena(self.be, bufs)
        self._frame_fec(A, N, stride, capacity, dstride)
        self._finish(A, "wire_frame_fec")
        return self._frame_out(A, N, dstride)

    def frame_seg(self, shards, hdr, stamps, capacity, dstride, order=None):
        stride = shards.shape[-1]
        N = shards.size // stride
        bufs = [self._buf("shards", N * stride, shards, "in"), self._buf("hdr", N * 20, hdr, "in"),
                self._buf("stamps", N * 12, stamps, "in")]
        if order is not None:
            bufs.append(self._buf("order", N * 4, np.ascontiguousarray(order, np.uint32), "in"))
        bufs += [self._buf("dgram", N * dstride, DGRAM_FILL, "out"), self._buf("dlen", N * 2, DLEN_FILL, "out")]
        A = ga.Arena(self.be, bufs)
        self._frame_seg(A, N, stride, capacity, dstride)
        self._finish(A, "wire_frame_seg")
        return self._frame_out(A, N, dstride)

    def _parse_arena(self, dgram, dlen, stride, split_entries):
        N, dstride = dgram.shape
        bufs = [self._buf("dgram", N * dstride, dgram, "in"),
                self._buf("dlen", N * 2, np.ascontiguousarray(dlen, np.uint16), "in"),
                self._buf("recs", N * 64, REC_FILL, "out"), self._buf("payload", N * stride, REC_FILL, "out")]
        if split_entries:
            bufs.append(self._buf("split", split_entries * 8, SPLIT_FILL, "out"))
        return ga.Arena(self.be, bufs)

    def parse(self, dgram, dlen, stride, capacity):
        N, dstride = dgram.shape
        A = self._parse_arena(dgram, dlen, stride, 0)
        self._parse(A, N, dstride, stride, capacity, None, 0, None)
        self._finish(A, "wire_parse")
        return A.get("recs", po.WIRE_REC, (N,)), A.get("payload", np.uint8, (N, stride))

    def parse_split(self, dgram, dlen, stride, capacity, max_len, T, tuning=None, tail=0):
        """The parse with the receiver session's split entries beside the records (rfec_launch_wire_parse_split):
        (recs, payload, split [N + tail]); the `tail` further entries of the split buffer keep their pre-fill
        (SPLIT_FILL).  tuning: for this call instead of the engine's own."""
        N, dstride = dgram.shape
        A = self._parse_arena(dgram, dlen, stride, N + tail)
        self._parse(A, N, dstride, stride, capacity, T, max_len, tuning)
        self._finish(A, "wire_parse_split")
        return (A.get("recs", po.WIRE_REC, (N,)), A.get("payload", np.uint8, (N, stride)),
                A.get("split", SPLIT_DTYPE, (N + tail,)))


def permuted(dgram, dlen, order):
    """Datagram i in slot order[i]."""
    if order is None:
        return dgram, dlen
    d, l = np.empty_like(dgram), np.empty_like(dlen)
    d[order], l[order] = dgram, dlen
    return d, l


class OracleWire(WireEngine):
    """The CPU oracle (oracle/rfec_oracle.c) behind the same arenas: reads its inputs from the arena, writes whole
    output buffers into it; the split entries by the rule of rfec_internal.h on its own records
    (aux_kernel_cases.ref_rx_split)."""

    def __init__(self, o):
        self.o, self.be = o, ga.NumpyBackend()

    def _order(self, A, N):
        return A.get("order", np.uint32, (N,)) if "order" in A.bufs else None

    def _put_frames(self, A, N, d, l):
        d, l = permuted(d, l, self._order(A, N))
        A.view("dgram")[...] = d.reshape(-1)
        A.view("dlen")[...] = l.view(np.uint8).reshape(-1)

    def _frame_fec(self, A, N, stride, capacity, dstride):
        status = A.get("status", np.int8, (N,)) if "status" in A.bufs else None
        d, l = self.o.frame_fec_batch(A.get("parity", np.uint8, (N, stride)), A.get("meta", po.HDR_DTYPE, (N,)),
                                      A.get("fec_size", np.uint16, (N,)), status,
                                      A.get("stamps", po.FEC_STAMP, (N,)), capacity, dstride)
        self._put_frames(A, N, d, l)

    def _frame_seg(self, A, N, stride, capacity, dstride):
        d, l = self.o.frame_seg_batch(A.get("shards", np.uint8, (N, stride)), A.get("hdr", po.HDR_DTYPE, (N,)),
                                      A.get("stamps", po.SEG_STAMP, (N,)), capacity, dstride)
        self._put_frames(A, N, d, l)

    def _parse(self, A, N, dstride, stride, capacity, T, max_len, tuning):
        recs, pay = self.o.parse_batch(A.get("dgram", np.uint8, (N, dstride)), A.get("dlen", np.uint16, (N,)),
                                       stride, capacity)
        A.view("recs")[...] = recs.view(np.uint8).reshape(-1)
        A.view("payload")[...] = pay.reshape(-1)
        if T is not None:
            import aux_kernel_cases as ac
            A.view("split")[:N * 8] = ac.ref_rx_split(recs, T).view(np.uint8).reshape(-1)


def _r16(n):
    return (n + 15) // 16 * 16


def fec_fixture():
    cases = po.load_wire_fec()
    N = len(cases)
    parity = np.zeros((N, STRIDE), np.uint8)
    meta = np.zeros(N, po.HDR_DTYPE)
    fsize = np.zeros(N, np.uint16)
    stamps = np.zeros(N, po.FEC_STAMP)
    exp = []
    for i, (r, f) in enumerate(cases):
        L = int(r["fec_data_size"])
        parity[i, :L] = f["payload"]
        meta[i] = r["meta"]
        fsize[i] = L
        for k in ("uid", "base_id", "send_ts", "fec_id", "count", "transport_seq", "row", "col", "index"):
            stamps[i][k] = r[k]
        exp.append(f["dgram"])
    return parity, meta, fsize, stamps, exp


def seg_fixture():
    cases = po.load_wire_seg()
    N = len(cases)
    shards = np.zeros((N, STRIDE), np.uint8)
    hdr = np.zeros(N, po.HDR_DTYPE)
    stamps = np.zeros(N, po.SEG_STAMP)
    exp = []
    for i, (r, f) in enumerate(cases):
        L = int(r["data_size"])
        shards[i, :L] = f["payload"]
        for a, b in (("seq", "packet_id"), ("fid", "fid"), ("ts", "timestamp"), ("index", "index"),
                     ("total", "total"), ("ftype", "ftype"), ("payload_type", "payload_type"), ("size", "data_size")):
            hdr[i][a] = r[b]
        for k in ("uid", "fec_id", "send_ts", "transport_seq", "remb"):
            stamps[i][k] = r[k]
        exp.append(f["dgram"])
    return shards, hdr, stamps, exp


def check_frames(dgram, dlen, exp):
    assert dgram.shape[0] == len(exp)
    for i, e in enumerate(exp):
        n = len(e)
        assert int(dlen[i]) == n, f"datagram {i}: length {int(dlen[i])} != reference {n}"
        assert np.array_equal(dgram[i, :n], e), f"datagram {i}: bytes differ from the reference"
        assert not dgram[i, n:].any(), f"datagram {i}: slot not zero past the datagram"


def check_frame_fec(engine):
    parity, meta, fsize, stamps, exp = fec_fixture()
    dstride = _r16(CAP + 49)
    dgram, dlen = engine.frame_fec(parity, meta, fsize, None, stamps, CAP, dstride)
    check_frames(dgram, dlen, exp)
    # status -1 / oversize lines are not emitted
    status = np.zeros(len(exp), np.int8)
    status[::7] = -1
    dgram, dlen = engine.frame_fec(parity, meta, fsize, status, stamps, CAP, dstride)
    for i, e in enumerate(exp):
        if status[i] < 0:
            assert dlen[i] == 0 and not dgram[i].any()
        else:
            assert int(dlen[i]) == len(e) and np.array_equal(dgram[i, :len(e)], e)


def check_frame_seg(engine):
    shards, hdr, stamps, exp = seg_fixture()
    dgram, dlen = engine.frame_seg(shards, hdr, stamps, CAP, _r16(CAP + 36))
    check_frames(dgram, dlen, exp)


def parse_fixture():
    cases = po.load_wire_parse()
    N = len(cases)
    dstride = _r16(max(int(r["len"]) for r, _ in cases))
    dgram = np.zeros((N, dstride), np.uint8)
    dlen = np.zeros(N, np.uint16)
    recs = np.zeros(N, po.WIRE_REC)
    pays = []
    kinds = np.zeros(N, np.uint8)
    for i, (r, f) in enumerate(cases):
        n = int(r["len"])
        dgram[i, :n] = f["dgram"]
        # garbage past the datagram end must not matter
        dgram[i, n:] = (np.arange(dstride - n) * 37 + i) & 0xFF
        dlen[i] = n
        recs[i] = r["rec"]
        kinds[i] = r["kind"]
        pays.append(f["payload"])
    return dgram, dlen, recs, pays, kinds


REC_FIELDS = ("status", "ver", "mid", "remb", "uid", "base_id", "send_ts", "fec_id", "count", "transport_seq",
              "data_size", "row", "col", "index")


def check_recs(got, exp_recs, i, kind=None):
    for k in REC_FIELDS:
        assert got[k] == exp_recs[i][k], f"datagram {i} (kind {kind}): {k} {got[k]} != reference {exp_recs[i][k]}"
    assert got["hdr"].tobytes() == exp_recs[i]["hdr"].tobytes(), f"datagram {i} (kind {kind}): header fields differ"


def check_parse(engine):
    dgram, dlen, exp, pays, kinds = parse_fixture()
    recs, payload = engine.parse(dgram, dlen, STRIDE, CAP)
    seen = set()
    for i in range(len(exp)):
        check_recs(recs[i], exp, i, int(kinds[i]))
        n = int(exp[i]["data_size"])
        assert np.array_equal(payload[i, :n], pays[i]), f"datagram {i}: payload differs"
        assert not payload[i, n:].any(), f"datagram {i}: payload slot not zero past data_size"
        seen.add((int(exp[i]["status"]), int(exp[i]["mid"]) if exp[i]["status"] >= 0 else -1))
    # every outcome the reference produced on the fixtures is exercised
    assert {s for s, _ in seen} >= {0, 1, -1, -2, -3}


def random_batch(rng, N, stride, capacity, seg=False):
    """Random framing inputs, sizes biased to the edges."""
    sizes = rng.integers(0, capacity + 1, N)
    sizes[: min(N, 64)] = np.arange(min(N, 64)) % (capacity + 1)
    sizes[rng.random(N) < 0.1] = capacity
    data = rng.integers(0, 256, (N, stride), dtype=np.uint8)
    data[np.arange(stride)[None, :] >= sizes[:, None]] = 0
    hdr = np.zeros(N, po.HDR_DTYPE)
    for k in ("seq", "fid", "ts"):
        hdr[k] = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    small = rng.random(N) < 0.5
    hdr["seq"][small] %= 65536
    hdr["fid"][rng.random(N) < 0.5] %= 65536
    hdr["index"] = rng.integers(0, 2**16, N)
    hdr["total"] = rng.integers(0, 2**16, N)
    hdr["total"][rng.random(N) < 0.5] %= 256
    hdr["ftype"] = rng.integers(0, 256, N)
    hdr["payload_type"] = rng.integers(0, 256, N)
    hdr["size"] = sizes
    if seg:
        stamps = np.zeros(N, po.SEG_STAMP)
        stamps["remb"] = rng.integers(0, 3, N)
    else:
        stamps = np.zeros(N, po.FEC_STAMP)
        for k in ("base_id", "send_ts"):
            stamps[k] = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
        for k in ("row", "col", "index"):
            stamps[k] = rng.integers(0, 256, N)
        stamps["count"] = rng.integers(0, 2**16, N)
    stamps["uid"] = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    stamps["fec_id"] = rng.integers(0, 2**16, N)
    stamps["send_ts"] = rng.integers(0, 2**16, N) if seg else stamps["send_ts"]
    stamps["transport_seq"] = rng.integers(0, 2**16, N)
    return data, hdr, sizes.astype(np.uint16), stamps


def mixed_corrupt_batch(oracle, capacity, stride, dstride, N, zero_ids=0.0, seed=0, bad_len=0.0):
    """N datagram slots mixing SIM_SEG (every header width) and SIM_FEC in
    random order, with flipped bytes (CRC mismatches), lengths cut short or
    past the slot, data sizes that overrun the datagram, control messages and
    bad message ids.  zero_ids: the fraction of datagrams framed with fec_id 0
    (segments outside FEC) and, independently, of SIM_SEG with packet id 0 --
    random_batch draws both from their whole range, so without it next to none
    is 0 (drawn from a generator of its own: the batch is otherwise the same).
    seed: another batch of the same shape (0: the batch the shape has always had).
    bad_len: the fraction of the otherwise untouched datagrams whose data length field is made invalid under a
    recomputed CRC (without it no SIM_FEC of the batch reads RFEC_WIRE_EBODY).
    Returns (dgram [N][dstride], dlen [N])."""
    rng = np.random.default_rng(capacity + stride * 3 + dstride * 7 + N + (seed << 20))
    rng_ids = np.random.default_rng(N + 1)
    frames, lens = [], []
    for seg in (True, False):
        data, hdr, sizes, stamps = random_batch(rng, N, stride, capacity, seg=seg)
        if zero_ids:
            stamps["fec_id"][rng_ids.random(N) < zero_ids] = 0
            if seg:
                hdr["seq"][rng_ids.random(N) < zero_ids] = 0
        over = 36 if seg else 49
        ds = max(dstride, (capacity + over + 15) // 16 * 16)
        if seg:
            g, gl = oracle.frame_seg_batch(data, hdr, stamps, capacity, ds)
        else:
            g, gl = oracle.frame_fec_batch(data, hdr, sizes, None, stamps, capacity, ds)
        frames.append(g[:, :dstride] if ds > dstride else np.pad(g, ((0, 0), (0, dstride - ds))))
        lens.append(np.minimum(gl, dstride).astype(np.uint16))
    dgram = np.concatenate(frames)
    dlen = np.concatenate(lens)
    pick = rng.permutation(len(dgram))[:N]
    dgram, dlen = dgram[pick].copy(), dlen[pick].copy()
    n = len(dgram)
    flip = rng.random(n) < 0.08  # a flipped byte inside the message
    for i in np.nonzero(flip & (dlen > 8))[0]:
        dgram[i, rng.integers(0, int(dlen[i]))] ^= 1 << int(rng.integers(8))
    cut = rng.random(n) < 0.04  # cut short (the trailer then sits elsewhere: a CRC mismatch)
    dlen[cut] = rng.integers(0, 60, int(cut.sum()))
    over = rng.random(n) < 0.02  # longer than the slot
    dlen[over] = dstride + 1 + rng.integers(0, 100, int(over.sum()))
    mid = rng.random(n) < 0.03  # another message id, CRC recomputed (a control message or a bad id)
    for i in np.nonzero(mid & (dlen >= 10) & (dlen <= dstride))[0]:
        L = int(dlen[i])
        dgram[i, 1] = rng.choice([0x10, 0x12, 0x1D, 0x05, 0x40])
        crc = oracle.crc32(dgram[i, :L - 4].tobytes())
        dgram[i, L - 4:L] = np.frombuffer(crc.to_bytes(4, "big"), np.uint8)
    if bad_len:
        # a data length that overruns the datagram or the capacity under a good CRC, in datagrams nothing above
        # touched: a SIM_FEC then reads EBODY, a SIM_SEG decodes with data_size 0 (drawn from a generator of its own)
        rng_len = np.random.default_rng(N + 2 + (seed << 20))
        pick_len = (rng_len.random(n) < bad_len) & ~(flip | cut | over | mid) & (dlen >= 36)
        for i in np.nonzero(pick_len)[0]:
            L = int(dlen[i])
            fec = dgram[i, 1] == 0x1C
            at = 43 if fec else 24 + 2 * sum((int(dgram[i, 6]) >> b) & 1 for b in (5, 6, 7))
            have = L - 4 - (at + 2)  # the data bytes the datagram holds
            bad = int(rng_len.choice([have + 1, capacity + 1, 0xFFFF]))
            dgram[i, at], dgram[i, at + 1] = bad >> 8, bad & 0xFF
            crc = oracle.crc32(dgram[i, :L - 4].tobytes())
            dgram[i, L - 4:L] = np.frombuffer(crc.to_bytes(4, "big"), np.uint8)
    return dgram, dlen
