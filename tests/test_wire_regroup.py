"""rfec_wire_regroup: parsed datagrams into recover's batch layout.  The rule
(regroup_cases.regroup_ref) against the reference's receiver and against its own
bent forms on the CPU, the entry point's argument checks without a device, and
the product against the rule on the GPU (regroup_cases.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import regroup_cases as rc


@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's records and the rule's outputs for them, computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            x = rc.make_inputs(oracle1000, c)
            cache[c] = (x, rc.ref_outputs(x))
        return cache[c]

    return get


# -- CPU: declared, bound, argument checks -----------------------------------------------------------------------------
def test_wire_regroup_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert "rfec_wire_regroup" in fec.header_functions() and "rfec_wire_regroup" in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, "rfec_wire_regroup") and hasattr(lib, "wire_regroup")
    text = fec.HEADER.read_text()
    for name, val in (("NONE", "0xFFFFFFFFu"), ("ENOTFEC", "(-1)"), ("EWINDOW", "(-2)"), ("ESHAPE", "(-3)"),
                      ("ENOPARITY", "(-4)"), ("EBASE", "(-5)"), ("EDUP", "(-6)")):
        assert any(ln.split() == ["#define", f"RFEC_REGROUP_{name}", val] for ln in text.splitlines()), name


P = dict(recs=0x10000, payload=0x20000, shards=0x30000, hdr=0x40004, present=0x50008, parity=0x60000, meta=0x70004,
         fec_size=0x80002, parity_present=0x90008, base_id=0xA0004, src_of=0xB0004, slot_of=0xC0004)
ORDER = ("shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")


def _call(product, plan, groups=4, fec_id0=7, n=100, stride=1216, capacity=1200, **ptrs):
    from razor_amd.fec import as_plan
    p = dict(P, **ptrs)
    rc_ = product.lib.rfec_wire_regroup(None if plan is None else C.byref(as_plan(plan)), groups, fec_id0, n,
                                        p["recs"], p["payload"], stride, capacity, *(p[name] for name in ORDER), None)
    return rc_, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "stride-0": (dict(stride=0, capacity=0), "multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity"),
    "fec-id0-0": (dict(fec_id0=0), "fec_id0"),
    "groups-65536": (dict(groups=65536), "groups"),
    "n-2g": (dict(n=0x80000000), "n must be"),
    **{f"null-{name}": ({name: None}, "NULL") for name in P},
    **{f"{name}-8": ({name: P[name] + 8}, "16-byte") for name in ("recs", "payload", "shards", "parity")},
    **{f"{name}-4": ({name: P[name] + 4}, "8-byte") for name in ("present", "parity_present")},
    **{f"{name}-2": ({name: P[name] + 2}, "4-byte") for name in ("hdr", "meta", "base_id", "src_of", "slot_of")},
    "fec_size-1": (dict(fec_size=P["fec_size"] + 1), "2-byte"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_wire_regroup_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    rc_, err = _call(product, rc.PLANS["rows10x4"](oracle1000), **kw)
    assert rc_ == -1 and msg in err, (rc_, err)


def test_wire_regroup_rejects_plan(product, oracle1000):
    rc_, err = _call(product, None)
    assert rc_ == -1 and "plan is NULL" in err, (rc_, err)
    rc_, err = _call(product, rc._hand_plan(129, 1, 129, []))  # above RFEC_MAX_K
    assert rc_ == -1 and "out of range" in err, (rc_, err)
    plan = rc.PLANS["rows10x4"](oracle1000)
    plan.line[2].first, plan.line[2].count = 8, 4  # members 8..11 of k = 10
    rc_, err = _call(product, plan)
    assert rc_ == -1 and "beyond k" in err, (rc_, err)


def test_wire_regroup_zero_groups_is_ok(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL."""
    rc_, _ = _call(product, rc.PLANS["rows10x4"](oracle1000), groups=0, **{name: None for name in P})
    assert rc_ == 0


def test_wire_regroup_optional_pointers(product, oracle1000):
    """n == 0 has no record, row or slot_of element, a plan without lines no parity, meta or fec_size element:
    those pointers pass the argument checks as NULL, the others are still checked.  The launch itself needs a
    device: its error is RFEC_EDEVICE (-2), past every argument check."""
    rows, k1 = rc.PLANS["rows10x4"](oracle1000), rc.PLANS["k1"](oracle1000)
    no_recs, no_lines = dict(recs=None, payload=None, slot_of=None), dict(parity=None, meta=None, fec_size=None)
    for plan, kw in ((rows, dict(n=0, **no_recs)), (k1, no_lines), (k1, dict(n=0, **no_recs, **no_lines))):
        rc_, err = _call(product, plan, **kw, src_of=None)
        assert rc_ == -1 and "NULL" in err, (rc_, err)
        rc_, err = _call(product, plan, **kw, present=P["present"] + 4)
        assert rc_ == -1 and "8-byte" in err, (rc_, err)
        if not torch.cuda.is_available():
            rc_, err = _call(product, plan, **kw)
            assert rc_ == -2 and "launch" in err, (rc_, err)
    rc_, err = _call(product, rows, **no_lines)
    assert rc_ == -1 and "NULL" in err, (rc_, err)


# -- CPU: the rule against the reference's receiver --------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["rows10x4", "full3x4k10"])
def test_regroup_rule_delivers_what_the_receiver_delivers(oracle1000, pname):
    """Uniform-shape streams of the oracle's sender path with lost and duplicated datagrams, no reordering (every
    parity after its group's segments) and all timestamps within 1 s: regroup_ref, then oracle.recover_batch_out,
    delivers exactly the segments the reference's receiver (oracle.rx_recover, event by event) delivers -- packet
    ids, header records, payload bytes.  Reordered streams are outside this comparison on purpose: the receiver
    delivers a segment recovered before its own late arrival, a closed window sees that segment as present."""
    o = oracle1000
    plan = rc.PLANS[pname](o)
    k = plan.k
    total = 0
    for seed, (G, fec_id0, capacity, stride) in enumerate(((40, 65520, 1000, 1008), (25, 1, 100, 112))):
        x = rc.inorder_stream(o, plan, G, fec_id0, capacity, stride, seed)
        out = rc.regroup_ref(plan, G, fec_id0, x.recs, x.payload, capacity, rc.new_outputs(plan, G, x.n, stride, 0))
        assert (out["slot_of"] == rc.EDUP).any() and (out["src_of"] == rc.NONE).any()
        o_sh, o_hd, o_ix, _ = o.recover_batch_out(plan, out["shards"], out["hdr"], out["present"], out["parity"],
                                                  out["meta"], out["fec_size"], out["parity_present"], capacity, k)
        ok = o_ix != 0xFF
        got_hdr, got_pay = o_hd[ok], o_sh[ok][:, :capacity]
        order = np.argsort(got_hdr["seq"], kind="stable")
        rx, rxp, _, dropped = o.rx_recover(x.recs, x.payload, capacity)
        assert dropped == 0
        assert len(rx) == len(got_hdr) > 0, (len(rx), len(got_hdr))
        by_id = np.argsort(rx["hdr"]["seq"], kind="stable")
        rx, rxp = rx[by_id], rxp[by_id]
        assert np.array_equal(rx["hdr"], got_hdr[order])
        assert np.array_equal(rxp[:, :capacity], got_pay[order])
        fid = np.array([rc.fec_id_of(fec_id0, g) for g in np.nonzero(ok)[0]], np.uint16)
        assert np.array_equal(rx["fec_id"], fid[order])
        total += len(rx)
    assert total > 20


# -- CPU: the checks can fail ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", rc.WRONG)
def test_regroup_cases_catch_each_wrong_rule(inputs, wrong):
    """Each bent rule of regroup_ref differs from the rule on at least one case."""
    caught = []
    for c in rc.CASES:
        x, ref = inputs(c)
        try:
            rc.compare(rc.ref_outputs(x, (wrong,)), ref, wrong)
        except AssertionError:
            caught.append(rc.case_id(c))
    assert caught, wrong


def test_regroup_cases_cover_their_conditions(inputs):
    """Over the case set: every refusal code, placed records and empty slots; every parse status; fec_id 0; a
    placed parity with data_size == capacity and a patched one above it; member ids that wrap 32 bits; a beaten
    duplicate with other bytes a block of records or more behind the winner; n = 0, 1, 63, 64, 65 and several
    blocks; every plan and geometry; a window that crosses 65535 -> 1, fec_id0 = 1, one group."""
    seen = {}
    for c in rc.CASES:
        for k, v in rc.conditions(*inputs(c)).items():
            seen[k] = (seen.get(k, set()) | v) if isinstance(v, set) else (seen.get(k, False) or v)
    assert seen.pop("status") >= {0, 1, -1, -2, -3}
    assert all(seen.values()) and len(seen) == 13, seen
    ns = {inputs(c)[0].n for c in rc.CASES}
    assert {0, 1, 63, 64, 65} <= ns and max(ns) > 3 * 256
    assert {c[0] for c in rc.CASES} == set(rc.PLANS) and {c[1] for c in rc.CASES} | {"c32"} == set(rc.GEOMS)
    assert any(c[2] == 1 for c in rc.CASES) and any(c[3] == 1 for c in rc.CASES)
    assert any(c[3] + c[2] > 65536 for c in rc.CASES)
    x, ref = inputs(("rows10x4", "c15", 7, 100, 1))
    assert ref["slot_of"][0] >= 0  # n = 1: the record is placed
    x, ref = inputs(("hand6", "c20", 7, 300, None))
    assert sorted(x.plan.line[l].index for l in range(4)) != [0, 1, 2, 3]


def test_regroup_arena_checks_can_fail(inputs):
    """The arena reports one changed guard byte after an output and one changed input byte; the comparison one
    changed byte in each output (on the rule's run of a case)."""
    x, ref = inputs(rc.CASES[0])
    eng = rc.RefRegroup()
    got = eng.run(x)
    rc.compare(got, ref, "the rule in an arena")
    for name in rc.OUTPUTS:
        bad = {k: v.copy() for k, v in got.items()}
        bad[name].view(np.uint8).reshape(-1)[-1] ^= 1
        with pytest.raises(AssertionError, match=f"{name}: 1 bytes differ"):
            rc.compare(bad, ref, "changed byte")

    def guard(name):
        def f(A):
            A.mem[A.bufs[name].off + A.bufs[name].nbytes] ^= 1
        return f

    def inp(A):
        A.view("payload")[5] ^= 1

    for mutate, msg in ((guard("shards"), "guard after shards"), (guard("slot_of"), "guard after slot_of"),
                        (inp, "input payload was written")):
        eng.mutate = mutate
        with pytest.raises(AssertionError, match=msg):
            eng.run(x)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return rc.GpuRegroup(product)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.CASES, ids=rc.case_id)
def test_wire_regroup_gpu(gpu, inputs, c):
    """The product == regroup_ref, all ten outputs byte for byte over their pre-fill (empty slots and bytes
    [16 CD, stride) keep it); the guards around the outputs and both inputs as uploaded."""
    x, ref = inputs(c)
    rc.compare(gpu.run(x), ref, f"rfec_wire_regroup {rc.case_id(c)}")


@pytest.mark.gpu
def test_wire_regroup_loop_gpu(gpu, inputs):
    """About 70,000 records over 3,000 groups, every datagram about twice: hundreds of blocks whose lanes
    contend for the same slots' words across blocks."""
    x, ref = inputs(rc.LOOP_CASE)
    assert 60000 < x.n < 80000 and (ref["slot_of"] == rc.EDUP).sum() > 20000
    gpu.lib.timing_events(None, None)
    got = gpu.run(x)
    assert gpu.lib.timing_launches() == 4
    rc.compare(got, ref, "rfec_wire_regroup, the looped case")


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["rows10x4", "full3x4k10"])
def test_wire_regroup_composed_gpu(gpu, oracle1200, product1200, pname):
    """rfec_wire_encode_send -> permute and lose with torch -> rfec_wire_parse -> rfec_wire_regroup ->
    rfec_recover_batch_out on device buffers == oracle.recover_batch_out on the sender's batch with the same
    losses (regroup_cases.composed)."""
    assert rc.composed(product1200, oracle1200, pname, "c1200", 50) >= 50
