"""rfec_wire_encode_fec: a batch of groups straight into SIM_FEC datagrams (the
encode and the framing in one kernel) against the oracle composed and against
the product's own rfec_encode_batch + rfec_wire_frame_fec; the entry point's
argument checks without a device (wire_encode_cases.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wire_encode_cases as wec

ROOT = Path(__file__).resolve().parent.parent


# -- CPU: the cases keep their point ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's inputs and expected output, computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = wec.make_inputs(oracle1000, c)
        return cache[c]

    return get


def test_wire_encode_cases_cover_their_conditions(inputs):
    """Over the case set: a refused line, a line as long as the capacity, an empty line, a CRC trailer across a
    16-byte chunk, a quad whose lines differ in member count; datagram counts 0-3 (mod 4) and 1."""
    seen = {}
    counts = set()
    for c in wec.CASES:
        x = inputs(c)
        counts.add(1 if x.count == 1 else -(x.count % 4))
        for k, v in wec.conditions(x).items():
            seen[k] = seen.get(k, False) or v
    assert all(seen.values()) and len(seen) == 5, seen
    assert counts >= {1, 0, -1, -2, -3}, counts
    assert {c[0] for c in wec.CASES} == set(wec.PLANS) and {c[1] for c in wec.CASES} | {"c48"} == set(wec.GEOMS)
    p = inputs(wec.CASES[0]).plan
    assert [p.line[i].count for i in range(p.n_lines)] == [4, 4, 2]
    # the poisoned cases hold the poison where no call may read it, and nowhere else
    for c in wec.CASES:
        if c[1].endswith("p"):
            x = inputs(c)
            cd16 = 16 * ((x.capacity + 15) // 16)
            assert (x.shards[:, :, cd16:] == wec.POISON).all() and cd16 + 16 <= x.stride


def test_wire_encode_checks_can_fail(oracle1000, inputs):
    """The comparison and the arena's checks report one changed datagram byte, one changed length and one
    changed guard byte (on the oracle's run of a case)."""
    x = inputs(wec.CASES[0])
    eng = wec.OracleFused(oracle1000)
    d, l = eng.fused(x)
    wec.compare(d, l, x.exp_dgram, x.exp_dlen, "oracle run")
    live = int(np.nonzero(x.exp_dlen)[0][-1])
    d2 = d.copy()
    d2[live, int(x.exp_dlen[live]) + 1] ^= 1  # a byte past the datagram's length: whole slots are compared
    with pytest.raises(AssertionError, match="slots differ"):
        wec.compare(d2, l, x.exp_dgram, x.exp_dlen, "changed byte")
    l2 = l.copy()
    l2[live] += 1
    with pytest.raises(AssertionError, match="lengths differ"):
        wec.compare(d, l2, x.exp_dgram, x.exp_dlen, "changed length")

    def guard(A):
        A.mem[A.bufs["dgram"].off + A.bufs["dgram"].nbytes] ^= 1  # the first byte past dgram

    def inp(A):
        A.view("stamps")[5] ^= 1

    for mutate, msg in ((guard, "guard after dgram"), (inp, "input stamps was written")):
        eng.mutate = mutate
        with pytest.raises(AssertionError, match=msg):
            eng.fused(x)


# -- CPU: argument checks (no device) ----------------------------------------------------------------------------------
def test_wire_encode_is_declared_and_bound():
    from razor_amd import fec
    assert "rfec_wire_encode_fec" in fec.header_functions() and "rfec_wire_encode_fec" in fec._SIGS


P_SH, P_HD, P_ST, P_OR, P_DG, P_DL = 0x10000, 0x20004, 0x30004, 0x40004, 0x50000, 0x60002


def _call(product, plan, groups=4, stride=1216, capacity=1200, shards=P_SH, hdr=P_HD, stamps=P_ST, order=P_OR,
          dstride=1280, dgram=P_DG, dlen=P_DL):
    from razor_amd.fec import as_plan
    rc = product.lib.rfec_wire_encode_fec(C.byref(as_plan(plan)), groups, stride, capacity, shards, hdr, stamps, order,
                                          dstride, dgram, dlen, None)
    return rc, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "dstride-1296": (dict(dstride=1296), "rfec_encode_batch + rfec_wire_frame_fec"),
    "dstride-small": (dict(capacity=1200, dstride=1248), "dstride too small"),
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "null-shards": (dict(shards=None), "NULL"), "null-hdr": (dict(hdr=None), "NULL"),
    "null-stamps": (dict(stamps=None), "NULL"), "null-dgram": (dict(dgram=None), "NULL"),
    "null-dlen": (dict(dlen=None), "NULL"),
    "shards-8": (dict(shards=P_SH + 8), "16-byte"), "dgram-8": (dict(dgram=P_DG + 8), "16-byte"),
    "hdr-2": (dict(hdr=P_HD + 2), "4-byte"), "stamps-2": (dict(stamps=P_ST + 2), "4-byte"),
    "order-2": (dict(order=P_OR + 2), "4-byte"), "dlen-1": (dict(dlen=P_DL + 1), "2-byte"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_wire_encode_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    rc, err = _call(product, wec.PLANS["rows10x4"](oracle1000), **kw)
    assert rc == -1 and msg in err, (rc, err)


def test_wire_encode_rejects_plan_line_past_k(product, oracle1000):
    plan = wec.PLANS["rows10x4"](oracle1000)
    plan.line[2].first, plan.line[2].count = 8, 4  # members 8..11 of k = 10
    rc, err = _call(product, plan)
    assert rc == -1 and "beyond k" in err, (rc, err)
    rc = product.lib.rfec_wire_encode_fec(None, 4, 1216, 1200, P_SH, P_HD, P_ST, None, 1280, P_DG, P_DL, None)
    assert rc == -1 and "plan is NULL" in product.lib.rfec_last_error().decode()


def test_wire_encode_zero_groups_is_ok(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL."""
    rc, _ = _call(product, wec.PLANS["rows10x4"](oracle1000), groups=0, shards=None, hdr=None, stamps=None, order=None,
                  dgram=None, dlen=None)
    assert rc == 0


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gfused(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return wec.GpuFused(product)


def _check_case(gfused, x):
    d, l = gfused.fused(x)
    d2, l2 = gfused.two_calls(x)
    wec.compare(d2, l2, x.exp_dgram, x.exp_dlen, "rfec_encode_batch + rfec_wire_frame_fec vs the oracle composed")
    wec.compare(d, l, x.exp_dgram, x.exp_dlen, "rfec_wire_encode_fec vs the oracle composed")
    wec.compare(d, l, d2, l2, "rfec_wire_encode_fec vs rfec_encode_batch + rfec_wire_frame_fec")


@pytest.mark.gpu
@pytest.mark.parametrize("c", wec.CASES, ids=wec.case_id)
def test_wire_encode_gpu(gfused, inputs, c):
    """The fused call == the oracle composed == the product's two calls, whole slots and lengths; the guards
    around dgram and dlen and every input buffer as uploaded."""
    _check_case(gfused, inputs(c))


@pytest.mark.gpu
def test_wire_encode_persistent_loop_gpu(gfused, inputs):
    """More datagrams than the waves resident at once frame in their first quads: some wave must loop."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = inputs(wec.LOOP_CASE)
    assert cus * 2 * 16 * 4 < x.count, (cus, x.count)  # at most two blocks of 16 waves per CU, 4 datagrams per quad
    _check_case(gfused, x)


@pytest.mark.gpu
def test_wire_encode_chunked_gpu(gfused, inputs):
    """RFEC_WIRE_ENCODE_CHUNK_GROUPS=7 on 50 groups (8 launches, with and without `order`) writes what the
    single launch writes; the variable is read per call, so the chunked run is a child process."""
    import hashlib
    env = dict(os.environ, RFEC_WIRE_ENCODE_CHUNK_GROUPS="7",
               PYTHONPATH=os.pathsep.join([str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, str(ROOT / "tests" / "wire_encode_cases.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("chunk ")]
    assert [ln[1] for ln in lines] == ["0", "1"], r.stdout
    for ln, with_order in zip(lines, (False, True)):
        x = inputs(wec.CHUNK_CASE[:3] + (with_order,))
        gfused.lib.timing_events(None, None)
        d, l = gfused.fused(x)
        assert gfused.lib.timing_launches() == 1 and int(ln[2]) == (x.G + 6) // 7 == 8, ln
        wec.compare(d, l, x.exp_dgram, x.exp_dlen, "single launch vs the oracle composed")
        assert ln[3] == hashlib.sha256(d.tobytes() + l.tobytes()).hexdigest()
