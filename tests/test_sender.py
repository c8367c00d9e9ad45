"""Sender staging end to end on the GPU: frames in host memory ->
rfec_host_send_frames -> SIM_SEG / SIM_FEC datagrams in host memory, checked
against what the reference flex sender emitted for the same frames
(tests/golden/stage.json, oracle/gen_stage.c) and against the oracle's wire
parser."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pyoracle as po
import stage_cases as sc

UID = 0x1234ABCD
DSTRIDE = 1056  # >= 1000 + 49


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from razor_amd.fec import native
    return native(1000)


def _fnv(b: bytes) -> int:
    h = 0xCBF29CE484222325
    for x in b:
        h ^= x
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _check_scenario(lib, oracle, scn, splits, zero_copy=False):
    frames, blob = po.stage_frames(scn)
    keep = []
    if zero_copy:  # frames and datagram outputs in rfec_pinned_alloc blocks: the device reads / writes them
        pb, k = lib.pinned_array(blob.shape, np.uint8)
        pb[...] = blob
        frames["data"] = frames["data"] - np.uint64(blob.ctypes.data) + np.uint64(pb.ctypes.data)
        blob = pb
        keep.append(k)
    st = lib.sender_init()
    segs, groups, sdg, sdl, fdg, fdl = [], [], [], [], [], []
    seg_base = 0
    for lo, hi in zip(splits[:-1], splits[1:]):
        bufs, kw = None, {}
        if zero_copy:
            ms = 64 * (hi - lo) + 256
            mp = 2 * ms
            out = [lib.pinned_array(shape, dt) for shape, dt in (((ms, DSTRIDE), np.uint8), ((ms,), np.uint16),
                                                                 ((mp, DSTRIDE), np.uint8), ((mp,), np.uint16))]
            keep += [o[1] for o in out]
            bufs = tuple(o[0] for o in out)
            kw = dict(max_segs=ms, max_parities=mp, bufs=bufs)
        s, g, a, al, b, bl, rep = lib.send_frames(st, frames[lo:hi], UID, DSTRIDE, **kw)
        if zero_copy:
            assert rep.zero_copy == 3 or (rep.n_segs == 0 and rep.zero_copy & 2), rep.zero_copy
            a, al, b, bl = a.copy(), al.copy(), b.copy(), bl.copy()
        s = s.copy()
        s["frame"] += lo
        g = g.copy()
        g["first_seg"] += seg_base
        seg_base += len(s)
        for lst, v in ((segs, s), (groups, g), (sdg, a), (sdl, al), (fdg, b), (fdl, bl)):
            lst.append(v)
    segs, groups = np.concatenate(segs), np.concatenate(groups)
    sdg, sdl, fdg, fdl = np.concatenate(sdg), np.concatenate(sdl), np.concatenate(fdg), np.concatenate(fdl)
    exp = np.array(scn["segments"], np.int64)
    for j, k in enumerate(sc.SEG_FIELDS[:-1]):
        assert np.array_equal(segs[k].astype(np.int64), exp[:, j]), (scn["name"], k)
    # SIM_SEG datagrams: header fields and payload = the frame bytes
    recs, pay = oracle.parse_batch(sdg, sdl, 1008, 1000)
    assert (recs["status"] == 0).all() and (recs["mid"] == 0x17).all() and (recs["uid"] == UID).all()
    assert np.array_equal(recs["hdr"]["seq"], segs["packet_id"]) and np.array_equal(recs["fec_id"], segs["fec_id"])
    assert np.array_equal(recs["data_size"], segs["data_size"]) and (recs["remb"] == 0xFF).all()  # remb 1 on the wire
    base = blob.ctypes.data
    for i in range(len(segs)):
        off = int(frames["data"][segs["frame"][i]] - base) + int(segs["offset"][i])
        n = int(segs["data_size"][i])
        assert np.array_equal(pay[i, :n], blob[off:off + n]), (scn["name"], i)
    # SIM_FEC datagrams, group by group: what the reference sender emitted
    frecs, fpay = oracle.parse_batch(fdg, fdl, 1008, 1000)
    assert (frecs["status"] == 0).all() and (frecs["mid"] == 0x1C).all()
    p = 0
    assert len(groups) == len(scn["groups"])
    for g, eg in zip(groups, scn["groups"]):
        for par in eg["parities"]:
            r = frecs[p]
            got = [int(r["index"]), int(r["row"]), int(r["col"]), int(r["count"]), int(r["hdr"]["seq"]),
                   int(r["hdr"]["fid"]), int(r["hdr"]["ts"]), int(r["hdr"]["index"]), int(r["hdr"]["total"]),
                   int(r["hdr"]["ftype"]), int(r["hdr"]["payload_type"]), int(r["hdr"]["size"]),
                   int(r["data_size"])]
            assert got == par[:13], (scn["name"], p)
            assert int(r["fec_id"]) == eg["fec_id"] and int(r["base_id"]) == eg["base_id"]
            assert f"{_fnv(fpay[p, :int(r['data_size'])].tobytes()):016x}" == par[13], (scn["name"], p)
            p += 1
    assert p == len(frecs)
    # transport_seq: creation order, each group's parities right after its last segment
    order = []
    gi = 0
    for i in range(len(segs)):
        order.append(("s", i))
        while gi < len(groups) and groups["first_seg"][gi] + groups["count"][gi] - 1 == i:
            order.extend(("f", q) for q in range(int(groups["n_lines"][gi])))
            gi += 1
    ts = np.zeros(len(order), np.int64)
    fcur = 0
    for t, (kind, i) in enumerate(order):
        if kind == "s":
            ts[t] = recs["transport_seq"][i]
        else:
            ts[t] = frecs["transport_seq"][fcur]
            fcur += 1
    assert np.array_equal(ts, np.arange(len(order)) & 0xFFFF)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_copy", [False, True])
@pytest.mark.parametrize("name", ["steady_k10_pf80", "mixed", "fractions"])
def test_send_frames_gpu(lib, oracle1000, name, zero_copy):
    """zero_copy: the frames and the datagram outputs in pinned blocks (the
    device gathers the segments out of the frames at their byte offsets and
    frames straight into the outputs)."""
    scn = {s["name"]: s for s in po.stage_fixture()["scenarios"]}[name]
    _check_scenario(lib, oracle1000, scn, [0, len(scn["frames"])], zero_copy)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_copy", [False, True])
@pytest.mark.parametrize("name", ["mixed", "fractions"])
def test_send_frames_split_calls_gpu(lib, oracle1000, name, zero_copy):
    """The same frames over several calls: open groups are carried across
    (zero copy: the carried segments from the pinned staging, the rows of
    their datagrams past the caller's output not written)."""
    scn = {s["name"]: s for s in po.stage_fixture()["scenarios"]}[name]
    n = len(scn["frames"])
    _check_scenario(lib, oracle1000, scn, [0, 1, 2, 5, n // 2, n // 2 + 1, n], zero_copy)


def _scenario(name):
    return {s["name"]: s for s in po.stage_fixture()["scenarios"]}[name]


@pytest.mark.gpu
@pytest.mark.parametrize("chunks,zero_copy,split", [(2, False, False), (2, True, False), (5, False, False),
                                                     (5, True, False), (16, False, False), (16, True, False),
                                                     (5, True, True)])
def test_send_frames_chunked_gpu(lib, oracle1000, monkeypatch, chunks, zero_copy, split):
    """The chunked path (RFEC_SEND_CHUNKS, read on every call): the slots of
    'mixed' (1,013 segments) arrive in 2, 5 and 16 chunks on the second stream
    (k_send_gather per chunk, or an H2D per chunk), each framed as it lands,
    and the datagrams are still the reference sender's.  split: over several
    calls at 5 chunks, the carried rows crossing chunk edges."""
    monkeypatch.setenv("RFEC_SEND_CHUNKS", str(chunks))
    scn = _scenario("mixed")
    n = len(scn["frames"])
    _check_scenario(lib, oracle1000, scn, [0, 1, 2, 5, n // 2, n // 2 + 1, n] if split else [0, n], zero_copy)


@pytest.mark.gpu
def test_send_frames_default_chunking_gpu(lib, oracle1000, monkeypatch):
    """One zero-copy call of more than 8,192 slots takes the chunked path by
    itself (n_slots / 2,048 >= 4 chunks): 950 generated frames of 8.5-11 kB,
    mixed ftype and protection, in one pinned block.  SIM_SEG / SIM_FEC
    datagrams and lengths == the same call from a fresh sender state in one
    chunk (RFEC_SEND_CHUNKS=1, the path the fixtures pin to the reference),
    and the SIM_SEG payloads the oracle parses out == the frame bytes."""
    rng = np.random.default_rng(8192)
    nf = 950
    sizes = rng.integers(8500, 11001, nf)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    blob, keep = lib.pinned_array((int(sizes.sum()) + 64,), np.uint8)
    blob[...] = rng.integers(0, 256, len(blob), dtype=np.uint8)
    frames = np.zeros(nf, po.FRAME)
    frames["data"] = np.uint64(blob.ctypes.data) + offs.astype(np.uint64)
    frames["size"] = sizes
    frames["ftype"] = rng.integers(0, 2, nf)
    frames["payload_type"] = 96
    frames["protect_fraction"] = rng.choice([30, 80, 120], nf)
    frames["now_ms"] = 1_700_000_000_000 + 33 * np.arange(nf)
    ms = mp = 11 * nf + 256
    out = [lib.pinned_array(sh, dt) for sh, dt in (((ms, DSTRIDE), np.uint8), ((ms,), np.uint16),
                                                    ((mp, DSTRIDE), np.uint8), ((mp,), np.uint16))]
    runs = {}
    for chunks in (None, 1):
        if chunks is None:
            monkeypatch.delenv("RFEC_SEND_CHUNKS", raising=False)
        else:
            monkeypatch.setenv("RFEC_SEND_CHUNKS", str(chunks))
        for o in out:
            o[0][...] = 0xEE
        got = lib.send_frames(lib.sender_init(), frames, UID, DSTRIDE, max_segs=ms, max_parities=mp,
                              bufs=tuple(o[0] for o in out))
        assert got[6].zero_copy == 3 and got[6].n_segs >= 8192  # zero copy, so chunked by default at this size
        runs[chunks] = [a.copy() for a in got[:6]]
    for a, b in zip(runs[None], runs[1]):
        assert np.array_equal(a, b)
    segs, _, sdg, sdl, fdg, fdl = runs[None]
    assert len(fdg) > 0 and (fdl > 0).all()
    recs, pay = oracle1000.parse_batch(sdg, sdl, 1008, 1000)
    assert (recs["status"] == 0).all() and (recs["mid"] == 0x17).all()
    assert np.array_equal(recs["data_size"], segs["data_size"])
    at = offs[segs["frame"]] + segs["offset"]
    col = np.arange(1008)[None, :]
    want = np.where(col < segs["data_size"][:, None], blob[np.minimum(at[:, None] + col, len(blob) - 1)], 0)
    assert np.array_equal(pay, want.astype(np.uint8))
    del keep, out
