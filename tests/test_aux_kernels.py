"""The helper kernels around the codec, on their own (aux_kernel_cases.py):
k_rx_split, k_gather_rows, k_rx_stage, k_line_jobs (rfec_helpers.hip),
k_send_gather (rfec_hostio.hip) and the split entries the parse writes beside
its records (k_parse_q's split_entry + the CRC rewrite, or k_rx_split after a
wave parse; rfec_wire.hip), bit-exact against numpy restatements.

CPU: the same checks against tests/host_stub/stub_hip.c, whose host versions of
these launches carry every CPU test of the receiver's plane -- the model and the
kernels are held to one set of rules.  (The stub's line jobs do no XOR
arithmetic: that check is GPU only.)"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import aux_kernel_cases as ac
import pyoracle as po
import wire_cases as wc
from host_stub_build import build_stub_library, have_hip_headers

RFEC_TUNE_WAVE_PARSE = 1 << 3


# -- CPU: the host stub ------------------------------------------------------------------------------------------
class StubAux:
    """The stub-linked host library's launches on host pointers."""

    def __init__(self, cdll):
        self.c = ac.bind_launches(cdll)

    @staticmethod
    def _canary(shape):
        return np.full(shape, ac.CANARY, np.uint8)

    def rx_split(self, recs, T):
        recs = np.ascontiguousarray(recs)
        out = self._canary((len(recs) + ac.GUARD) * 8)
        assert self.c.rfec_launch_rx_split(recs.ctypes.data, len(recs), T, out.ctypes.data, None) == 0
        return out.view(ac.SPLIT_DTYPE)

    def gather_rows(self, src, map_, stride):
        src, map_ = np.ascontiguousarray(src), np.ascontiguousarray(map_, np.int32)
        dst = self._canary((len(map_) + ac.GUARD, stride))
        assert self.c.rfec_launch_gather_rows(dst.ctypes.data, src.ctypes.data, map_.ctypes.data, len(map_), stride,
                                              None) == 0
        return dst

    def rx_stage(self, src, map_, stride, tables):
        src, map_ = np.ascontiguousarray(src), np.ascontiguousarray(map_, np.int32)
        tables = np.ascontiguousarray(tables)
        dst = self._canary((len(map_) + ac.GUARD, stride))
        tdst = self._canary(len(tables) + ac.GUARD * 16)
        assert self.c.rfec_launch_rx_stage(dst.ctypes.data, src.ctypes.data, map_.ctypes.data, len(map_), stride,
                                           tdst.ctypes.data, tables.ctypes.data, len(tables), None) == 0
        return dst, tdst

    def send_gather(self, blob, offsets, sizes, stride):
        room = np.zeros(len(blob) + 16, np.uint8)  # the blob at a 16-byte boundary: offsets[s] & 3 is the misalignment
        at = -room.ctypes.data % 16
        room[at:at + len(blob)] = blob
        base = room.ctypes.data + at
        src = np.where(offsets >= 0, base + offsets, 0).astype(np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint16)
        dst = self._canary((len(offsets) + ac.GUARD, stride))
        assert self.c.rfec_launch_send_gather(src.ctypes.data, sizes.ctypes.data, len(offsets), stride,
                                              dst.ctypes.data, None) == 0
        return dst


@pytest.fixture(scope="module")
def stub_aux(tmp_path_factory):
    if not have_hip_headers():
        pytest.skip("HIP headers not available")
    return StubAux(C.CDLL(str(build_stub_library(tmp_path_factory.mktemp("auxstub") / "librazor_fec_auxstub.so"))))


def test_rx_split_stub(stub_aux):
    ac.check_rx_split(stub_aux)


def test_gather_rows_stub(stub_aux):
    ac.check_gather_rows(stub_aux)


def test_rx_stage_stub(stub_aux):
    ac.check_rx_stage(stub_aux)


def test_send_gather_stub(stub_aux):
    ac.check_send_gather(stub_aux)


def test_line_jobs_reference_levels():
    """The numpy restatement on a case small enough to work out by hand: a
    level-2 job reads a level-1 output through a negative code; unwritten
    output rows keep their bytes."""
    rows = np.array([[1] * 16, [2] * 16, [4] * 16], np.uint8)
    out = np.full((3, 16), ac.CANARY, np.uint8)
    j1 = np.array([(1, 0, 0, 1)], ac.JOB_DTYPE)  # out 1 = rows[0] ^ rows[1] = 3
    out = ac.ref_line_jobs(j1, np.array([1], np.int32), rows, out)
    j2 = np.array([(0, 2, 1, 2)], ac.JOB_DTYPE)  # out 0 = rows[2] ^ out[1] ^ rows[0] = 4 ^ 3 ^ 1 = 6
    out = ac.ref_line_jobs(j2, np.array([9, -2, 0], np.int32), rows, out)
    assert (out[0] == 6).all() and (out[1] == 3).all() and (out[2] == ac.CANARY).all()


# -- the split beside the parse: its inputs (CPU: the oracle alone) and the kernels (GPU) -----------------------
#               capacity, stride, dstride, N
SPLIT_SHAPES = [(1200, 1216, 1264, 4099), (1000, 1008, 1056, 3001), (1200, 1200, 1504, 2049)]
SPLIT_T = (1, 3, 8, 64)
QWINDOW = 1280  # the quarter-wave parse's reach into a slot


@functools.lru_cache(maxsize=None)
def split_batch(shape):
    """test_wire_parse_mixed_gpu's batch of the shape with a fifth of the
    fec_ids and of the packet ids 0, the oracle's parse of it, and the
    conditions the split checks need of it.  The 1,504-byte slots
    also hold datagrams longer than 1,280 bytes: a control message with a good
    CRC, a SIM_SEG header under a good CRC, and random bytes."""
    capacity, stride, dstride, N = shape
    o = po.Oracle(1000)
    dgram, dlen = wc.mixed_corrupt_batch(o, capacity, stride, dstride, N, zero_ids=0.2)
    if dstride > QWINDOW:
        rng = np.random.default_rng(N)
        for i, (L, mid) in {7: (1400, 0x10), 1000: (1300, 0x17), 2048: (1500, None)}.items():
            dgram[i, :L] = rng.integers(0, 256, L, dtype=np.uint8)
            dlen[i] = L
            if mid is not None:
                dgram[i, 0], dgram[i, 1] = 0x01, mid
                dgram[i, L - 4:L] = np.frombuffer(o.crc32(dgram[i, :L - 4].tobytes()).to_bytes(4, "big"), np.uint8)
        assert (dlen[[7, 1000, 2048]] > QWINDOW).all()
    recs, pay = o.parse_batch(dgram, dlen, stride, capacity)
    n = len(recs)
    kinds = ac.split_kind_counts(ac.ref_rx_split(recs, 8))
    cond = dict(n=n, ok=int((recs["status"] == 0).sum()), badcrc=int((recs["status"] == -1).sum()),
                control=int((recs["status"] == 1).sum()), kinds=kinds)
    print("split batch", shape, cond)
    assert cond["ok"] >= n // 2 and cond["badcrc"] * 100 >= n and cond["control"] >= 1 and min(kinds[1:]) >= 1, cond
    return dgram, dlen, recs, pay


@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_parse_split_batches_meet_their_conditions(shape):
    """At least n/2 OK records, 1 % CRC mismatches, an OK control message and
    every split kind in each batch the GPU test parses (asserted in split_batch)."""
    split_batch(shape)


# -- GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_aux():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuAux
    return GpuAux()


@pytest.mark.gpu
def test_rx_split_gpu(gpu_aux):
    ac.check_rx_split(gpu_aux)


@pytest.mark.gpu
def test_gather_rows_gpu(gpu_aux):
    ac.check_gather_rows(gpu_aux)


@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["pinned", "device"])
def test_rx_stage_gpu(memory):
    """pinned: the map and the table source in rfec_pinned_alloc memory (what
    rfec_rx_dev.c passes: the lanes read them over PCIe); device: in HBM."""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuAux
    ac.check_rx_stage(GpuAux(pinned=memory == "pinned"))


@pytest.mark.gpu
def test_line_jobs_gpu(gpu_aux):
    ac.check_line_jobs(gpu_aux)


@pytest.mark.gpu
def test_send_gather_gpu(gpu_aux):
    ac.check_send_gather(gpu_aux)


@pytest.mark.gpu
@pytest.mark.parametrize("parse", ["quarter", "wave"])
@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_parse_split_gpu(gpu_aux, shape, parse):
    """rfec_launch_wire_parse_split on the mixed corrupt batches: records and
    payloads == the oracle's, and the split entries == the numpy rule applied to
    the oracle's records, all 8 bytes of every datagram -- with tuning 0
    (k_parse_q where the slots allow it: split_entry in the header pass, the
    entry rewritten when the CRC fails) and with RFEC_TUNE_WAVE_PARSE (a wave
    parse, then k_rx_split).  Slots of 1,504 bytes: max_len given and 0."""
    capacity, stride, dstride, N = shape
    dgram, dlen, orecs, opay = split_batch(shape)
    tuning = 0 if parse == "quarter" else RFEC_TUNE_WAVE_PARSE
    for max_len in ([int(dlen.max()), 0] if dstride > QWINDOW else [int(dlen.max())]):
        for T in SPLIT_T:
            what = f"parse_split {shape} {parse} max_len={max_len} T={T}"
            recs, pay, split = gpu_aux.parse_split(dgram, dlen, stride, capacity, max_len, T, tuning)
            assert np.array_equal(recs.view(np.uint8), orecs.view(np.uint8)), what
            assert np.array_equal(pay, opay), what
            got = split[:N]
            assert (split[N:].view(np.uint8) == 0xAB).all(), what + ": written past the last entry"
            ac.same_split(got, ac.ref_rx_split(orecs, T), what)
