"""rfec_wire_encode_send: a batch's SIM_SEG and SIM_FEC datagrams in one kernel
against the oracle composed and against the product's own rfec_wire_frame_seg +
rfec_wire_encode_fec; the entry point's argument checks without a device
(wire_send_cases.py)."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wire_send_cases as wsc

ROOT = Path(__file__).resolve().parent.parent


# -- CPU: the cases keep their point ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's inputs and expected output, computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = wsc.make_inputs(oracle1000, c)
        return cache[c]

    return get


def test_wire_send_cases_cover_their_conditions(inputs):
    """Over the case set, from the oracle's outputs: all four SIM_SEG header sizes and a line whose members differ
    in it; fid wide and narrow; total 255 / 256 in one quad of groups; remb 0 and set; data_size 0, 1, capacity and
    capacity + 1 (SEG length 0); a refused line; ragged sizes in a line; a SEG and a FEC trailer across a 16-byte
    chunk and across a 64-lane row (256 bytes); a member on no line, on two lines, on a one-member line; a plan
    without lines; ns and nf = 0-3 (mod 4) independently; one group; every combination of the orders."""
    seen = {}
    for c in wsc.CASES:
        for k, v in wsc.conditions(inputs(c)).items():
            seen[k] = (seen.get(k, set()) | v) if isinstance(v, set) else (seen.get(k, False) or v)
    assert seen.pop("hs") == {26, 28, 30, 32}
    assert all(seen.values()) and len(seen) == 20, seen
    xs = [inputs(c) for c in wsc.CASES]
    assert {x.ns % 4 for x in xs} == {0, 1, 2, 3} and {x.nf % 4 for x in xs if x.nf} == {0, 1, 2, 3}
    assert any(x.G == 1 for x in xs)
    assert {c[0] for c in wsc.CASES} == set(wsc.PLANS) and {c[1] for c in wsc.CASES} | {"c64"} == set(wsc.GEOMS)
    small = [(c[3], c[4]) for c in wsc.CASES if c[:3] == ("full3x4k10", "c1000", 3)]
    assert sorted(small) == [(False, False), (False, True), (True, False), (True, True)]
    # the plans are what their names say
    o = wsc.owners(inputs(("rows9x4", "c1200w", 3, False, False)).plan)
    assert o[8] == [] and all(len(m) == 1 for m in o[:8])
    o = wsc.owners(inputs(("full3x4k9", "c1000p", 5, False, False)).plan)
    assert len(o[8]) == 1 and all(len(m) == 2 for m in o[:8])
    p = inputs(wsc.CASES[0]).plan
    assert [p.line[i].count for i in range(p.n_lines)] == [4, 4, 2]
    # the poisoned cases hold the poison where no call may read it, and nowhere else
    for c in wsc.CASES:
        if c[1].endswith("p"):
            x = inputs(c)
            cd16 = 16 * ((x.capacity + 15) // 16)
            assert (x.shards[:, :, cd16:] == wsc.POISON).all() and cd16 + 16 <= x.stride


def test_wire_send_checks_can_fail(oracle1000, inputs):
    """The comparison and the arena's checks report one changed byte and one changed length in each output, one
    changed guard byte and one changed input byte (on the oracle's run of a case)."""
    x = inputs(wsc.CASES[0])
    eng = wsc.OracleSend(oracle1000)
    got = eng.send(x)
    wsc.compare_all(got, x.exp, "oracle run")
    for i, what in ((0, "SIM_SEG"), (2, "SIM_FEC")):
        live = int(np.nonzero(x.exp[i + 1])[0][-1])
        bad = [a.copy() for a in got]
        bad[i][live, int(x.exp[i + 1][live]) + 1] ^= 1  # a byte past the datagram's length: whole slots are compared
        with pytest.raises(AssertionError, match=f"{what}: 1 slots differ"):
            wsc.compare_all(bad, x.exp, "changed byte")
        bad = [a.copy() for a in got]
        bad[i + 1][live] += 1
        with pytest.raises(AssertionError, match=f"{what}: 1 lengths differ"):
            wsc.compare_all(bad, x.exp, "changed length")

    def guard(name):
        def f(A):
            A.mem[A.bufs[name].off + A.bufs[name].nbytes] ^= 1  # the first byte past the buffer
        return f

    def inp(A):
        A.view("seg_stamps")[5] ^= 1

    for mutate, msg in ((guard("seg_dgram"), "guard after seg_dgram"), (guard("fec_dlen"), "guard after fec_dlen"),
                        (inp, "input seg_stamps was written")):
        eng.mutate = mutate
        with pytest.raises(AssertionError, match=msg):
            eng.send(x)


# -- CPU: argument checks (no device) ----------------------------------------------------------------------------------
def test_wire_send_is_declared_and_bound():
    from razor_amd import fec
    assert "rfec_wire_encode_send" in fec.header_functions() and "rfec_wire_encode_send" in fec._SIGS
    assert hasattr(fec.native(1000), "wire_encode_send")


P_SH, P_HD, P_SS, P_SO, P_SD, P_SL = 0x10000, 0x20004, 0x30004, 0x40004, 0x50000, 0x60002
P_FS, P_FO, P_FD, P_FL = 0x70004, 0x80004, 0x90000, 0xA0002


def _call(product, plan, groups=4, stride=1216, capacity=1200, shards=P_SH, hdr=P_HD, seg_stamps=P_SS, seg_order=P_SO,
          seg_dgram=P_SD, seg_dlen=P_SL, fec_stamps=P_FS, fec_order=P_FO, fec_dgram=P_FD, fec_dlen=P_FL,
          dstride=1280):
    from razor_amd.fec import as_plan
    rc = product.lib.rfec_wire_encode_send(C.byref(as_plan(plan)), groups, stride, capacity, shards, hdr, seg_stamps,
                                           seg_order, seg_dgram, seg_dlen, fec_stamps, fec_order, fec_dgram, fec_dlen,
                                           dstride, None)
    return rc, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "dstride-1296": (dict(dstride=1296), "rfec_wire_frame_seg + rfec_wire_encode_fec"),
    "dstride-small": (dict(capacity=1200, dstride=1248), "dstride too small"),
    "dstride-seg-only": (dict(capacity=1204, dstride=1248), "dstride too small"),  # 1204 + 36 fits, + 49 does not
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "null-shards": (dict(shards=None), "NULL"), "null-hdr": (dict(hdr=None), "NULL"),
    "null-seg-stamps": (dict(seg_stamps=None), "NULL"), "null-seg-dgram": (dict(seg_dgram=None), "NULL"),
    "null-seg-dlen": (dict(seg_dlen=None), "NULL"),
    "null-fec-stamps": (dict(fec_stamps=None), "NULL"), "null-fec-dgram": (dict(fec_dgram=None), "NULL"),
    "null-fec-dlen": (dict(fec_dlen=None), "NULL"),
    "shards-8": (dict(shards=P_SH + 8), "16-byte"), "seg-dgram-8": (dict(seg_dgram=P_SD + 8), "16-byte"),
    "fec-dgram-8": (dict(fec_dgram=P_FD + 8), "16-byte"),
    "hdr-2": (dict(hdr=P_HD + 2), "4-byte"), "seg-stamps-2": (dict(seg_stamps=P_SS + 2), "4-byte"),
    "fec-stamps-2": (dict(fec_stamps=P_FS + 2), "4-byte"), "seg-order-2": (dict(seg_order=P_SO + 2), "4-byte"),
    "fec-order-2": (dict(fec_order=P_FO + 2), "4-byte"),
    "seg-dlen-1": (dict(seg_dlen=P_SL + 1), "2-byte"), "fec-dlen-1": (dict(fec_dlen=P_FL + 1), "2-byte"),
    # with an order its output must stay below 4 GiB: 2^22 groups of 10 x 1,280-byte slots, of 3 x 1,280
    "seg-order-4g": (dict(groups=1 << 19), "seg_order"),
    "fec-order-4g": (dict(groups=1 << 21, seg_order=None), "fec_order"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_wire_send_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    rc, err = _call(product, wsc.PLANS["rows10x4"](oracle1000), **kw)
    assert rc == -1 and msg in err, (rc, err)


def test_wire_send_rejects_plan_line_past_k(product, oracle1000):
    plan = wsc.PLANS["rows10x4"](oracle1000)
    plan.line[2].first, plan.line[2].count = 8, 4  # members 8..11 of k = 10
    rc, err = _call(product, plan)
    assert rc == -1 and "beyond k" in err, (rc, err)
    rc = product.lib.rfec_wire_encode_send(None, 4, 1216, 1200, P_SH, P_HD, P_SS, None, P_SD, P_SL, P_FS, None, P_FD,
                                           P_FL, 1280, None)
    assert rc == -1 and "plan is NULL" in product.lib.rfec_last_error().decode()


def test_wire_send_zero_groups_is_ok(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL."""
    rc, _ = _call(product, wsc.PLANS["rows10x4"](oracle1000), groups=0, shards=None, hdr=None, seg_stamps=None,
                  seg_order=None, seg_dgram=None, seg_dlen=None, fec_stamps=None, fec_order=None, fec_dgram=None,
                  fec_dlen=None)
    assert rc == 0


def test_wire_send_no_lines_takes_null_fec_pointers(product, oracle1000):
    """A plan without lines: the SIM_FEC pointers pass the argument checks as NULL (and misaligned: they are not
    looked at), the SIM_SEG ones are still checked.  The launch itself needs a device: its error is RFEC_EDEVICE
    (-2), past every argument check."""
    plan = wsc.PLANS["k1"](oracle1000)
    null_fec = dict(fec_stamps=None, fec_order=None, fec_dgram=None, fec_dlen=None)
    rc, err = _call(product, plan, seg_dlen=P_SL + 1, **null_fec)
    assert rc == -1 and "2-byte" in err, (rc, err)
    rc, err = _call(product, plan, seg_dgram=None, **null_fec)
    assert rc == -1 and "NULL" in err, (rc, err)
    if not torch.cuda.is_available():
        rc, err = _call(product, plan, **null_fec)
        assert rc == -2 and "launch" in err, (rc, err)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gsend(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return wsc.GpuSend(product)


def _check_case(gsend, x):
    got = gsend.send(x)
    two = gsend.two_calls(x)
    wsc.compare_all(two, x.exp, "rfec_wire_frame_seg + rfec_wire_encode_fec vs the oracle composed")
    wsc.compare_all(got, x.exp, "rfec_wire_encode_send vs the oracle composed")
    wsc.compare_all(got, two, "rfec_wire_encode_send vs rfec_wire_frame_seg + rfec_wire_encode_fec")


@pytest.mark.gpu
@pytest.mark.parametrize("c", wsc.CASES, ids=wsc.case_id)
def test_wire_send_gpu(gsend, inputs, c):
    """The fused call == the oracle composed == the product's two calls, whole slots and lengths; the guards
    around the four outputs and every input buffer as uploaded."""
    _check_case(gsend, inputs(c))


@pytest.mark.gpu
def test_wire_send_persistent_loop_gpu(gsend, inputs):
    """The kernel's unit of work is four groups per wave, and its LDS (the CRC tables and the waves' header
    batches, 109,056 bytes of a CU's 160 KiB) admits one block of 16 waves per CU: with more units than that, some
    wave must loop."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = inputs(wsc.LOOP_CASE)
    assert cus * 16 < (x.G + 3) // 4, (cus, x.G)
    _check_case(gsend, x)


@pytest.mark.gpu
def test_wire_send_chunked_gpu(gsend, inputs):
    """RFEC_WIRE_ENCODE_CHUNK_GROUPS=7 on 50 groups (8 launches, with and without the orders) writes what the
    single launch writes; the variable is read per call, so the chunked run is a child process."""
    env = dict(os.environ, RFEC_WIRE_ENCODE_CHUNK_GROUPS="7",
               PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, str(ROOT / "tests" / "wire_send_cases.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("chunk ")]
    assert [ln[1] for ln in lines] == ["0", "1"], r.stdout
    for ln, with_order in zip(lines, (False, True)):
        x = inputs(wsc.CHUNK_CASE[:3] + (with_order, with_order))
        gsend.lib.timing_events(None, None)
        got = gsend.send(x)
        assert gsend.lib.timing_launches() == 1 and int(ln[2]) == (x.G + 6) // 7 == 8, ln
        wsc.compare_all(got, x.exp, "single launch vs the oracle composed")
        assert ln[3] == hashlib.sha256(b"".join(a.tobytes() for a in got)).hexdigest()
