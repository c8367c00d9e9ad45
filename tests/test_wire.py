"""Wire codec (SIM_FEC / SIM_SEG datagrams + CRC32, sim_proto.c / sim_proto.inl):
the oracle against the reference's own encoder/decoder outputs
(tests/golden/wire_*.bin from oracle/gen_wire.c), then the HIP kernels against
the same fixtures and against the oracle on large random batches."""
from __future__ import annotations

import zlib

import numpy as np
import pytest
import torch

import pyoracle as po
import wire_cases as wc


OracleWire = wc.OracleWire  # the oracle behind the guarded arenas the GPU engine uses (wire_cases.WireEngine)


# -- CPU: oracle pinned to the reference ---------------------------------------
def test_wire_crc_is_zlib_crc32_with_seed(oracle1000):
    """cf_crc32.c:56-68 == zlib crc32 continued from 0x0e3dfc0a; every fixture
    datagram ends in it, big-endian (sim_proto.c:92-94)."""
    for r, f in po.load_wire_fec() + po.load_wire_seg():
        d = f["dgram"].tobytes()
        c = zlib.crc32(d[:-4], po.CRC_SEED)
        assert int.from_bytes(d[-4:], "big") == c == oracle1000.crc32(d[:-4])
    for n in range(0, 9):
        d = bytes(range(n))
        assert oracle1000.crc32(d) == zlib.crc32(d, po.CRC_SEED)


def test_wire_frame_fec_oracle(oracle1000):
    wc.check_frame_fec(OracleWire(oracle1000))


def test_wire_frame_seg_oracle(oracle1000):
    wc.check_frame_seg(OracleWire(oracle1000))


def test_wire_parse_oracle(oracle1000):
    wc.check_parse(OracleWire(oracle1000))


def test_wire_fixture_coverage():
    m = po.wire_manifest()
    assert m["sim_video_size"] == wc.CAP and m["crc_seed"] == po.CRC_SEED
    kinds = np.array([int(r["kind"]) for r, _ in po.load_wire_parse()])
    assert set(kinds.tolist()) == set(range(7))
    segs = po.load_wire_seg()
    masks = {(r["packet_id"] > 65535, r["fid"] > 65535, r["total"] > 255, r["remb"] == 0) for r, _ in segs}
    assert len(masks) == 16  # every header-width / remb combination (sim_proto.inl:85-98)


def test_wire_short_datagram_oracle(oracle1000):
    """Shorter than the CRC trailer: rejected (the reference would read before its buffer)."""
    dgram = np.zeros((4, 64), np.uint8)
    recs, _ = oracle1000.parse_batch(dgram, np.array([0, 1, 2, 3], np.uint16), wc.STRIDE, wc.CAP)
    assert (recs["status"] == -1).all()


# -- CPU: the guarded engine's checks can each fail ------------------------------
def test_wire_engine_checks_can_fail(oracle1000):
    """On the oracle's run of the engine: one changed guard byte after each output, one changed input byte, and --
    in the comparisons the loop cases use -- one changed datagram byte, length and record byte are each reported."""
    import wire_loop_cases as wl
    rng = np.random.default_rng(7)
    N, capacity, stride, dstride = 9, 230, 240, 288
    data, hdr, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=True)
    eng = OracleWire(oracle1000)
    g, gl = eng.frame_seg(data, hdr, stamps, capacity, dstride, order=np.arange(N, dtype=np.uint32))
    o, ol = oracle1000.frame_seg_batch(data, hdr, stamps, capacity, dstride)
    wl.same_frames(g, gl, o, ol, "oracle run")
    recs, pay, split = eng.parse_split(g, gl, stride, capacity, 0, 3)
    orecs, opay = oracle1000.parse_batch(g, gl, stride, capacity)
    wl.same_parse(recs, pay, orecs, opay, "oracle run")
    wl.same_split(split, orecs, 3, "oracle run")
    assert (recs["status"] == 0).all() and np.array_equal(pay, np.where(np.arange(stride) < sizes[:, None], data, 0))

    g2 = g.copy()
    g2[N - 1, int(gl[N - 1]) + 1] ^= 1  # a byte past the datagram's length: whole slots are compared
    with pytest.raises(AssertionError, match="slots differ"):
        wl.same_frames(g2, gl, o, ol, "changed datagram byte")
    gl2 = gl.copy()
    gl2[3] += 1
    with pytest.raises(AssertionError, match="lengths differ"):
        wl.same_frames(g, gl2, o, ol, "changed length")
    r2 = recs.copy()
    r2.view(np.uint8).reshape(N, 64)[5, 63] ^= 1  # a reserved byte: all 64 are compared
    with pytest.raises(AssertionError, match="records differ"):
        wl.same_parse(r2, pay, orecs, opay, "changed record byte")
    p2 = pay.copy()
    p2[0, stride - 1] ^= 1
    with pytest.raises(AssertionError, match="payload slots differ"):
        wl.same_parse(recs, p2, orecs, opay, "changed payload byte")
    s2 = split.copy()
    s2["reserved"][N - 1] = 1
    with pytest.raises(AssertionError, match="split entries differ"):
        wl.same_split(s2, orecs, 3, "changed split byte")

    def after(name):
        def mutate(A, what):
            A.mem[A.bufs[name].off + A.bufs[name].nbytes] ^= 1  # the first byte past the buffer
        return mutate

    def inside(name, at):
        def mutate(A, what):
            A.view(name)[at] ^= 1
        return mutate

    calls = {
        "frame_seg": lambda: eng.frame_seg(data, hdr, stamps, capacity, dstride, order=np.arange(N, dtype=np.uint32)),
        "frame_fec": lambda: eng.frame_fec(data, hdr, sizes, np.zeros(N, np.int8), stamps_fec, capacity, dstride),
        "parse": lambda: eng.parse(g, gl, stride, capacity),
        "parse_split": lambda: eng.parse_split(g, gl, stride, capacity, 0, 3),
    }
    _, _, _, stamps_fec = wc.random_batch(rng, N, stride, capacity, seg=False)
    for call, mutate, msg in (
            ("frame_seg", after("dgram"), "guard after dgram"), ("frame_seg", after("dlen"), "guard after dlen"),
            ("frame_fec", after("dgram"), "guard after dgram"), ("frame_fec", after("dlen"), "guard after dlen"),
            ("parse", after("recs"), "guard after recs"), ("parse", after("payload"), "guard after payload"),
            ("parse_split", after("split"), "guard after split"),
            ("frame_seg", inside("shards", 17), "input shards was written"),
            ("frame_seg", inside("order", 4), "input order was written"),
            ("frame_fec", inside("status", N - 1), "input status was written"),
            ("frame_fec", inside("fec_size", 2), "input fec_size was written"),
            ("parse", inside("dgram", 100), "input dgram was written"),
            ("parse_split", inside("dlen", 1), "input dlen was written")):
        eng.mutate = mutate
        with pytest.raises(AssertionError, match=msg):
            calls[call]()
    eng.mutate = None
    # every pointer of a call at exactly its documented alignment and nothing larger
    eng.parse_split(g, gl, stride, capacity, 0, 3)
    A = eng.last_arena
    for name, b in A.bufs.items():
        assert b.align == wc.WIRE_ALIGN[name] and A.ptr(name) % b.align == 0 and A.ptr(name) % (2 * b.align) != 0, name


# -- CPU: the three entries' argument checks, through the host stub (no device) ---------------------------------------
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    import ctypes as C

    from host_stub_build import build_stub_library, have_hip_headers
    from razor_amd import fec
    if not have_hip_headers():
        pytest.skip("HIP headers not available")
    lib = C.CDLL(str(build_stub_library(tmp_path_factory.mktemp("wirestub") / "librazor_fec_wirestub.so")))
    for fn in ("rfec_wire_frame_fec", "rfec_wire_frame_seg", "rfec_wire_parse", "rfec_last_error"):
        f = getattr(lib, fn)
        f.restype, f.argtypes = fec._SIGS[fn]
    return lib


# addresses that are never dereferenced: the stub's launches do nothing, the checks come before them
P16, P4, P2, P1 = 0x10000, 0x20004, 0x30002, 0x40001
WIRE_ARGS = {
    "rfec_wire_frame_fec": (("count", 8), ("stride", 1216), ("capacity", 1200), ("parity", P16), ("meta", P4),
                            ("fec_size", P2), ("status", P1), ("stamps", P4 + 0x100), ("order", P4 + 0x200),
                            ("dstride", 1264), ("dgram", P16 + 0x1000), ("dlen", P2 + 0x100)),
    "rfec_wire_frame_seg": (("count", 8), ("stride", 1216), ("capacity", 1200), ("shards", P16), ("hdr", P4),
                            ("stamps", P4 + 0x100), ("order", P4 + 0x200), ("dstride", 1264), ("dgram", P16 + 0x1000),
                            ("dlen", P2 + 0x100)),
    "rfec_wire_parse": (("n", 8), ("dstride", 1264), ("dgram", P16), ("dlen", P2), ("stride", 1216),
                        ("capacity", 1200), ("recs", P16 + 0x1000), ("payload", P16 + 0x2000)),
}
WIRE_MISALIGNED = {
    "rfec_wire_frame_fec": {"parity": (8, "parity and dgram must be 16-byte aligned"),
                            "dgram": (8, "parity and dgram must be 16-byte aligned"),
                            "meta": (2, "meta, stamps and order must be 4-byte aligned"),
                            "stamps": (2, "meta, stamps and order must be 4-byte aligned"),
                            "order": (2, "meta, stamps and order must be 4-byte aligned"),
                            "fec_size": (1, "fec_size and dlen must be 2-byte aligned"),
                            "dlen": (1, "fec_size and dlen must be 2-byte aligned")},
    "rfec_wire_frame_seg": {"shards": (8, "shards and dgram must be 16-byte aligned"),
                            "dgram": (8, "shards and dgram must be 16-byte aligned"),
                            "hdr": (2, "hdr, stamps and order must be 4-byte aligned"),
                            "stamps": (2, "hdr, stamps and order must be 4-byte aligned"),
                            "order": (2, "hdr, stamps and order must be 4-byte aligned"),
                            "dlen": (1, "dlen must be 2-byte aligned")},
    "rfec_wire_parse": {"dgram": (8, "dgram, recs and payload must be 16-byte aligned"),
                        "recs": (8, "dgram, recs and payload must be 16-byte aligned"),
                        "payload": (8, "dgram, recs and payload must be 16-byte aligned"),
                        "dlen": (1, "dlen must be 2-byte aligned")},
}


def _wire_call(stub, fn, **kw):
    args = [kw.get(name, v) for name, v in WIRE_ARGS[fn]]
    rc = getattr(stub, fn)(*args, None)
    return rc, stub.rfec_last_error().decode()


@pytest.mark.parametrize("fn", sorted(WIRE_ARGS))
def test_wire_alignment_checks(stub, fn):
    """Each pointer one step below its documented alignment is RFEC_EINVAL with a message that names it; the
    checks come after the geometry and NULL checks, widest alignment first, are skipped for count == 0 and pass a
    NULL status / order and a status at any address."""
    base = dict(WIRE_ARGS[fn])
    rc, err = _wire_call(stub, fn)
    assert rc == 0, err
    optional = [a for a in ("status", "order") if a in base]
    rc, err = _wire_call(stub, fn, **{a: None for a in optional})
    assert rc == 0, err
    for arg, (off, msg) in WIRE_MISALIGNED[fn].items():
        rc, err = _wire_call(stub, fn, **{arg: base[arg] + off})
        assert rc == -1 and msg in err and arg in msg, (arg, rc, err)
        # at the documented alignment and nothing larger: accepted
        align = 2 * off
        rc, err = _wire_call(stub, fn, **{arg: (base[arg] & ~0xFF) + align})
        assert rc == 0, (arg, err)
    # order: geometry, then NULL, then 16, 4, 2 bytes
    first16 = next(a for a, (off, _) in WIRE_MISALIGNED[fn].items() if off == 8)
    first2 = next(a for a, (off, _) in WIRE_MISALIGNED[fn].items() if off == 1)
    bad16, bad2 = {first16: base[first16] + 8}, {first2: base[first2] + 1}
    rc, err = _wire_call(stub, fn, dstride=1265, **bad16)
    assert rc == -1 and "dstride must be a multiple of 16" in err, err
    rc, err = _wire_call(stub, fn, dlen=None, **bad16)
    assert rc == -1 and "NULL buffer" in err, err
    rc, err = _wire_call(stub, fn, **bad16, **({} if first2 in bad16 else bad2))
    assert rc == -1 and "16-byte" in err, err
    first4 = [a for a, (off, _) in WIRE_MISALIGNED[fn].items() if off == 2]
    if first4:
        rc, err = _wire_call(stub, fn, **{first4[0]: base[first4[0]] + 2}, **bad2)
        assert rc == -1 and "4-byte" in err, err
    # nothing to do: nothing is looked at
    count = WIRE_ARGS[fn][0][0]
    rc, err = _wire_call(stub, fn, **{count: 0}, **bad16, **bad2)
    assert rc == 0, err


# -- GPU -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def gwire():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuWire
    return GpuWire()


RFEC_TUNE_WAVE_PARSE = 1 << 3


@pytest.fixture(params=["quarter", "wave"])
def pwire(request):
    """The parse both ways: the quarter-wave kernel (default) and the
    wave-per-datagram one (RFEC_TUNE_WAVE_PARSE), the cross-check."""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuWire
    return GpuWire(tuning=0 if request.param == "quarter" else RFEC_TUNE_WAVE_PARSE)


@pytest.mark.gpu
def test_wire_frame_fec_gpu(gwire):
    wc.check_frame_fec(gwire)


@pytest.mark.gpu
def test_wire_frame_seg_gpu(gwire):
    wc.check_frame_seg(gwire)


@pytest.mark.gpu
def test_wire_parse_gpu(pwire):
    wc.check_parse(pwire)


@pytest.mark.gpu
def test_wire_short_datagram_gpu(pwire):
    gwire = pwire
    dgram = np.full((5, 64), 0xAB, np.uint8)
    recs, pay = gwire.parse(dgram, np.array([0, 1, 2, 3, 4], np.uint16), wc.STRIDE, wc.CAP)
    assert (recs["status"][:4] == -1).all() and not pay.any()
    # 4 bytes: an empty message whose trailer must equal crc32(seed, "") = seed
    d = np.zeros((1, 64), np.uint8)
    d[0, :4] = np.frombuffer(po.CRC_SEED.to_bytes(4, "big"), np.uint8)
    recs, _ = gwire.parse(d, np.array([4], np.uint16), wc.STRIDE, wc.CAP)
    # CRC accepted; ver/mid then read the trailer bytes themselves (0x0e, 0x3d): mid out of range
    assert recs["status"][0] == -2 and recs["ver"][0] == 0x0E and recs["mid"][0] == 0x3D


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,stride,dstride,N", [(1200, 1200, 1248, 4097), (1200, 1216, 1264, 4099),
                                                       (1000, 1008, 1056, 3001), (230, 240, 288, 2051),
                                                       (1200, 1280, 1280, 2050), (1200, 1200, 1504, 2049),
                                                       (1300, 1312, 1360, 1025)])
def test_wire_parse_mixed_gpu(pwire, oracle1000, capacity, stride, dstride, N):
    """The parse against the oracle on batches that mix SIM_SEG (every header
    width: data at bytes 26-32) and SIM_FEC (data at 45) datagrams in random
    order -- a quarter-wave quad holds datagrams with different data offsets
    -- with flipped bytes (CRC mismatches: record EBADCRC, slot zero), lengths
    cut short or past the slot, data sizes that overrun the datagram, control
    messages and bad message ids; slots of 1,248-1,504 bytes (wider than 1,280:
    the datagrams still fit, the quarter-wave parse reads the first 1,280),
    payload slots up to 1,280 bytes, N not a multiple of 4."""
    dgram, dlen = wc.mixed_corrupt_batch(oracle1000, capacity, stride, dstride, N)
    n = len(dgram)
    recs, pay = pwire.parse(dgram, dlen, stride, capacity)
    orecs, opay = oracle1000.parse_batch(dgram, dlen, stride, capacity)
    bad = np.nonzero((recs.view(np.uint8).reshape(n, 64) != orecs.view(np.uint8).reshape(n, 64)).any(1))[0]
    assert len(bad) == 0, (bad[:8], recs[bad[:2]], orecs[bad[:2]])
    bad = np.nonzero((pay != opay).any(1))[0]
    assert len(bad) == 0, (bad[:8], recs[bad[:4]]["status"], recs[bad[:4]]["data_size"])
    st = set(int(x) for x in recs["status"])
    assert {0, -1} <= st and (recs["status"] == 0).sum() > n // 2


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,stride", [(1000, 1008), (1200, 1200), (256, 256), (1984, 1984), (1999, 2000)])
def test_wire_random_roundtrip_gpu(gwire, oracle1000, capacity, stride):
    """Large random batches: HIP framing == oracle framing byte for byte, and
    HIP parse(HIP frame(x)) returns x (fields, payload, zero tails)."""
    rng = np.random.default_rng(capacity)
    N = 20000
    for seg in (False, True):
        data, hdr, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=seg)
        over = 36 if seg else 49
        dstride = min(2048, (capacity + over + 15) // 16 * 16)
        if seg:
            g, gl = gwire.frame_seg(data, hdr, stamps, capacity, dstride)
            o, ol = oracle1000.frame_seg_batch(data, hdr, stamps, capacity, dstride)
        else:
            g, gl = gwire.frame_fec(data, hdr, sizes, None, stamps, capacity, dstride)
            o, ol = oracle1000.frame_fec_batch(data, hdr, sizes, None, stamps, capacity, dstride)
        assert np.array_equal(gl, ol)
        assert np.array_equal(g, o)
        recs, pay = gwire.parse(g, gl, stride, capacity)
        orecs, opay = oracle1000.parse_batch(g, gl, stride, capacity)
        assert np.array_equal(recs.view(np.uint8), orecs.view(np.uint8))
        assert np.array_equal(pay, opay)
        assert (recs["status"] == 0).all()
        assert np.array_equal(recs["data_size"], sizes)
        assert np.array_equal(pay, data)
        assert np.array_equal(recs["uid"], stamps["uid"])
        assert np.array_equal(recs["transport_seq"], stamps["transport_seq"])
        if seg:
            assert np.array_equal(recs["hdr"]["seq"], hdr["seq"]) and np.array_equal(recs["hdr"]["fid"], hdr["fid"])
            assert np.array_equal(recs["hdr"]["ftype"], hdr["ftype"] & 1)
            assert np.array_equal(recs["remb"], np.where(stamps["remb"] == 0, 0, 0xFF))
        else:
            assert recs["hdr"].tobytes() == hdr.tobytes()
            assert np.array_equal(recs["base_id"], stamps["base_id"])


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,stride,dstride", [(1200, 1200, 1248), (1200, 1216, 1264), (1000, 1008, 1280),
                                                     (1201, 1216, 1248), (1240, 1248, 1280), (230, 240, 272),
                                                     (1300, 1312, 1344)])
def test_wire_frame_seg_edges_gpu(gwire, oracle1000, capacity, stride, dstride):
    """SIM_SEG framing against the oracle where the quarter-wave kernel must
    mask and place bytes itself: garbage past each segment's data (other
    bytes of its slot), sizes above capacity (zero datagram, length 0),
    every header width, an output permutation (`order`), and slot widths
    on both sides of the quarter-wave path's condition (datagram slots up
    to 1,280 B; wider ones take the 32-byte lanes)."""
    rng = np.random.default_rng(capacity * 7 + stride + dstride)
    N = 4099  # not a multiple of 4: the last quad is partial
    data, hdr, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=True)
    garbage = rng.integers(0, 256, data.shape, dtype=np.uint8)
    tail = np.arange(stride)[None, :] >= sizes[:, None]
    data = np.where(tail, garbage, data)
    big = rng.random(N) < 0.02
    hdr["size"][big] = capacity + 1 + rng.integers(0, 50, int(big.sum()))
    o, ol = oracle1000.frame_seg_batch(data, hdr, stamps, capacity, dstride)
    assert (ol[big] == 0).all() and not o[big].any()
    g, gl = gwire.frame_seg(data, hdr, stamps, capacity, dstride)
    assert np.array_equal(gl, ol)
    assert np.array_equal(g, o)
    perm = rng.permutation(N).astype(np.uint32)
    g2, gl2 = gwire.frame_seg(data, hdr, stamps, capacity, dstride, order=perm)
    assert np.array_equal(gl2[perm], ol)
    assert np.array_equal(g2[perm], o)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,stride,dstride", [(1200, 1200, 1264), (1200, 1216, 1280), (1000, 1008, 1056),
                                                     (230, 240, 288), (1300, 1312, 1360)])
def test_wire_frame_fec_edges_gpu(gwire, oracle1000, capacity, stride, dstride):
    """SIM_FEC framing against the oracle with garbage past each line's
    fec_data_size, status -1 and oversize lines (zero datagram, length 0),
    random stamps and meta, a partial last quad and an output permutation,
    on both sides of the quarter-wave path's slot limit (1,280 B)."""
    rng = np.random.default_rng(capacity * 5 + stride + dstride)
    N = 4097
    data, meta, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=False)
    garbage = rng.integers(0, 256, data.shape, dtype=np.uint8)
    data = np.where(np.arange(stride)[None, :] >= sizes[:, None], garbage, data)
    sizes = sizes.astype(np.uint16)
    big = rng.random(N) < 0.02
    sizes[big] = capacity + 1 + rng.integers(0, 40, int(big.sum()))
    status = np.where(rng.random(N) < 0.05, -1, 0).astype(np.int8)
    o, ol = oracle1000.frame_fec_batch(data, meta, sizes, status, stamps, capacity, dstride)
    assert (ol[big | (status < 0)] == 0).all()
    g, gl = gwire.frame_fec(data, meta, sizes, status, stamps, capacity, dstride)
    assert np.array_equal(gl, ol)
    assert np.array_equal(g, o)
