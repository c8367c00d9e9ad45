"""rfec_wire_encode_send_shapes: a send window of several shapes into its SIM_SEG
and SIM_FEC datagrams in one launch, against the oracle composed per shape and
against the product's own rfec_wire_encode_send called per shape; the entry
point's argument checks without a device (wire_send_shapes_cases.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import wire_send_shapes_cases as wss

DFILL = wss.DLEN_FILL * 0x0101


@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's inputs and expected output, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = wss.make_inputs(oracle1000, name, wss.LOOP_CASE if name == "loop" else None)
        return cache[name]

    return get


# -- CPU: the cases keep their point ---------------------------------------------------------------------------------
def test_wire_send_shapes_cases_cover_their_conditions(inputs):
    """Over the case set, from the oracle's outputs and the descriptors: all four SIM_SEG header sizes; a member on
    no line, on two lines, on a one-member line; a refused line; an oversize segment; a SEG and a FEC trailer across
    a 16-byte chunk and across a 256-byte row; every composition of a wave's four descriptors (4, 2 + 2, 3 + 1,
    2 + 1 + 1, 1 + 1 + 1 + 1, trailing waves of 1, 2 and 3, a wave with nothing live); every skip reason; rows and
    lines that no group covers; 32 plans with 512 lines, each used."""
    seen = {}
    for name in wss.CASES:
        for k, v in wss.conditions(inputs(name)).items():
            seen[k] = (seen.get(k, set()) | v) if isinstance(v, set) else (seen.get(k, False) or v)
    assert seen.pop("hs") == {26, 28, 30, 32}
    assert seen.pop("skips") == set(wss.SKIPS)
    quads = seen.pop("quads")
    assert {(4, (4,)), (4, (2, 2)), (4, (3, 1)), (4, (2, 1, 1)), (4, (1, 1, 1, 1)), (1, (1,)), (2, (1, 1)),
            (3, (1, 1, 1)), (2, ())} <= quads, quads
    assert any(n == 4 and len(c) and sum(c) < 4 for n, c in quads)  # a skipped group among live ones
    assert all(seen.values()) and len(seen) == 11, seen
    assert inputs("one-group").G == 1
    x = inputs("shapes32")
    assert len(x.plans) == wss.MAX_SHAPES and sum(p.n_lines for p in x.plans) == wss.MAX_LINES
    assert set(x.desc["shape"].tolist()) == set(range(wss.MAX_SHAPES))
    assert {wss.CASES[n][1] for n in wss.CASES} >= {"c1200w", "c463", "c464", "c15", "c1000p"}
    assert sorted((wss.CASES[n][5], wss.CASES[n][6]) for n in wss.CASES if n.startswith("orders-")) == \
        [(False, False), (False, True), (True, False), (True, True)]
    # the layouts are what their names say
    x = inputs("rows-perm")
    assert (np.diff(x.desc["row0"].astype(np.int64)) < 0).any() and x.covered_r.all()
    x = inputs("desc-byshape")
    assert (np.diff(x.desc["shape"].astype(np.int64)) >= 0).all() and (np.diff(x.desc["row0"].astype(np.int64)) < 0).any()
    x = inputs("c1000p")
    cd16 = 16 * ((x.capacity + 15) // 16)
    assert (x.shards[:, cd16:] == wss.POISON).all() and cd16 + 16 <= x.stride
    # a skipped group's rows and lines expect the fill
    x = inputs("skips")
    for d, why in zip(x.desc, x.skip):
        if why in ("shape", "lines"):
            assert (x.exp[1][d["row0"]:d["row0"] + 7] == DFILL).all(), why
        if why in ("shape", "rows"):
            assert (x.exp[3][d["line0"]:d["line0"] + 3] == DFILL).all(), why


def test_wire_send_shapes_checks_can_fail(oracle1000, inputs):
    """The comparison and the arena's checks report one changed byte and one changed length in each output, one
    changed guard byte, one changed input byte and one byte written into a slot that no group covers (on the
    oracle's run of a case)."""
    x = inputs("gaps")
    eng = wss.OracleShapes(oracle1000)
    got = eng.send(x)
    wss.compare_all(got, x.exp, "oracle run")
    for i, what in ((0, "SIM_SEG"), (2, "SIM_FEC")):
        live = int(np.nonzero((x.exp[i + 1] != DFILL) & (x.exp[i + 1] > 0))[0][-1])
        bad = [a.copy() for a in got]
        bad[i][live, int(x.exp[i + 1][live]) + 1] ^= 1  # a byte past the datagram's length: whole slots are compared
        with pytest.raises(AssertionError, match=f"{what}: 1 slots differ"):
            wss.compare_all(bad, x.exp, "changed byte")
        bad = [a.copy() for a in got]
        bad[i + 1][live] += 1
        with pytest.raises(AssertionError, match=f"{what}: 1 lengths differ"):
            wss.compare_all(bad, x.exp, "changed length")
        gap = int(np.nonzero(~(x.covered_r, None, x.covered_l)[i])[0][0])
        bad = [a.copy() for a in got]
        bad[i][gap, 17] ^= 1
        with pytest.raises(AssertionError, match=f"{what}: 1 slots differ, the first slot {gap} at byte 17"):
            wss.compare_all(bad, x.exp, "a byte in a gap slot")

    def guard(name):
        def f(A):
            A.mem[A.bufs[name].off + A.bufs[name].nbytes] ^= 1  # the first byte past the buffer
        return f

    def inp(A):
        A.view("group")[5] ^= 1

    for mutate, msg in ((guard("seg_dgram"), "guard after seg_dgram"), (guard("fec_dlen"), "guard after fec_dlen"),
                        (inp, "input group was written")):
        eng.mutate = mutate
        with pytest.raises(AssertionError, match=msg):
            eng.send(x)


# -- CPU: argument checks (no device) ----------------------------------------------------------------------------------
def test_wire_send_shapes_is_declared_and_bound():
    from razor_amd import fec
    assert "rfec_wire_encode_send_shapes" in fec.header_functions() and "rfec_wire_encode_send_shapes" in fec._SIGS
    lib = fec.native(1000)
    assert hasattr(lib, "wire_encode_send_shapes") and hasattr(lib.lib, "rfec_wire_encode_send_shapes")
    assert C.sizeof(fec.rfec_send_group) == 16 == fec.SEND_GROUP_DTYPE.itemsize == wss.SEND_GROUP.itemsize
    assert [f for f, _ in fec.rfec_send_group._fields_] == list(fec.SEND_GROUP_DTYPE.names) == list(wss.SEND_GROUP.names)
    assert (fec.RFEC_SEND_MAX_SHAPES, fec.RFEC_SEND_MAX_LINES) == (32, 512)
    assert lib.lib.rfec_abi_version() == 7


P_GR, P_SH, P_HD, P_SS, P_SO, P_SD, P_SL = 0x8004, 0x10000, 0x20004, 0x30004, 0x40004, 0x50000, 0x60002
P_FS, P_FO, P_FD, P_FL = 0x70004, 0x80004, 0x90000, 0xA0002
NO_PLANS = object()


def _call(product, plans, n_plans=None, groups=4, group=P_GR, n_rows=40, n_fec=12, stride=1216, capacity=1200,
          shards=P_SH, hdr=P_HD, seg_stamps=P_SS, seg_order=P_SO, seg_dgram=P_SD, seg_dlen=P_SL, fec_stamps=P_FS,
          fec_order=P_FO, fec_dgram=P_FD, fec_dlen=P_FL, dstride=1280):
    from razor_amd.fec import as_plan, rfec_plan
    if plans is NO_PLANS:
        pa, n = None, 1
    else:
        pa, n = (rfec_plan * max(len(plans), 1))(*(as_plan(p) for p in plans)), len(plans)
    rc = product.lib.rfec_wire_encode_send_shapes(pa, n if n_plans is None else n_plans, groups, group, n_rows, n_fec,
                                                  stride, capacity, shards, hdr, seg_stamps, seg_order, seg_dgram,
                                                  seg_dlen, fec_stamps, fec_order, fec_dgram, fec_dlen, dstride, None)
    return rc, product.lib.rfec_last_error().decode()


SMALL = dict(stride=16, capacity=15, dstride=64)
BAD_ARGS = {
    "n-plans-0": (dict(n_plans=0), "n_plans"), "n-plans-33": (dict(n_plans=33), "n_plans"),
    "dstride-1296": (dict(dstride=1296), "dstride <= 1280"),
    "dstride-small": (dict(capacity=1200, dstride=1248), "dstride too small"),
    "dstride-seg-only": (dict(capacity=1204, dstride=1248), "dstride too small"),  # 1204 + 36 fits, + 49 does not
    "dstride-not-16": (dict(dstride=1272), "multiple of 16"),
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "capacity-above-stride": (dict(stride=1008, capacity=1200), "capacity"),
    "null-group": (dict(group=None), "group is NULL"),
    "null-shards": (dict(shards=None), "NULL"), "null-hdr": (dict(hdr=None), "NULL"),
    "null-seg-stamps": (dict(seg_stamps=None), "NULL"), "null-seg-dgram": (dict(seg_dgram=None), "NULL"),
    "null-seg-dlen": (dict(seg_dlen=None), "NULL"),
    "null-fec-stamps": (dict(fec_stamps=None), "NULL"), "null-fec-dgram": (dict(fec_dgram=None), "NULL"),
    "null-fec-dlen": (dict(fec_dlen=None), "NULL"),
    "group-2": (dict(group=P_GR + 2), "4-byte"),
    "shards-8": (dict(shards=P_SH + 8), "16-byte"), "seg-dgram-8": (dict(seg_dgram=P_SD + 8), "16-byte"),
    "fec-dgram-8": (dict(fec_dgram=P_FD + 8), "16-byte"),
    "hdr-2": (dict(hdr=P_HD + 2), "4-byte"), "seg-stamps-2": (dict(seg_stamps=P_SS + 2), "4-byte"),
    "fec-stamps-2": (dict(fec_stamps=P_FS + 2), "4-byte"), "seg-order-2": (dict(seg_order=P_SO + 2), "4-byte"),
    "fec-order-2": (dict(fec_order=P_FO + 2), "4-byte"),
    "seg-dlen-1": (dict(seg_dlen=P_SL + 1), "2-byte"), "fec-dlen-1": (dict(fec_dlen=P_FL + 1), "2-byte"),
    # the 32-bit buffer offsets of the one launch, each the first to fail
    "bound-shards": (dict(n_rows=1 << 21, stride=2048, capacity=15, dstride=64), "(n_rows + 4) * stride + 1280"),
    "bound-hdr": (dict(n_rows=215_000_000, **SMALL), "n_rows * 20"),
    "bound-seg-dgram": (dict(n_rows=1 << 22, stride=16, capacity=15, dstride=1280), "n_rows * dstride"),
    "bound-fec-stamps": (dict(n_fec=180_000_000, **SMALL), "n_fec * 24"),
    "bound-fec-dgram": (dict(n_fec=1 << 22, stride=16, capacity=15, dstride=1280), "n_fec * dstride"),
    "bound-group": (dict(groups=1 << 28, **SMALL), "groups * 16"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_wire_send_shapes_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    plans = [wss.PLANS[s](oracle1000) for s in ("rows10x4", "hand7")]
    rc, err = _call(product, plans, **kw)
    assert rc == -1 and msg in err, (rc, err)
    if name.startswith("bound-"):
        assert "split the window" in err, err


def test_wire_send_shapes_rejects_plans(product, oracle1000):
    """plans NULL; a plan line beyond k, in the second plan; k above RFEC_MAX_K_ENCODE; 513 lines over the plans
    (512 pass the checks)."""
    rc, err = _call(product, NO_PLANS)
    assert rc == -1 and "plans is NULL" in err, (rc, err)
    good, bad = wss.PLANS["hand7"](oracle1000), wss.PLANS["rows10x4"](oracle1000)
    bad.line[2].first, bad.line[2].count = 8, 4  # members 8..11 of k = 10
    rc, err = _call(product, [good, bad])
    assert rc == -1 and "beyond k" in err, (rc, err)
    bad = wss.PLANS["k2"](oracle1000)
    bad.k = 256
    rc, err = _call(product, [good, bad])
    assert rc == -1 and "out of range" in err, (rc, err)
    full = [wss.PLANS[f"wide{i}"](oracle1000) for i in range(wss.MAX_SHAPES)]
    assert sum(p.n_lines for p in full) == 512
    rc, err = _call(product, full[:-1] + [wss.wec._hand_plan(26, [(l, 1, 2) for l in range(9)])])
    assert rc == -1 and "sum of n_lines" in err, (rc, err)
    if not torch.cuda.is_available():
        rc, err = _call(product, full)
        assert rc == -2 and "launch" in err, (rc, err)


def test_wire_send_shapes_zero_groups_is_ok(product, oracle1000):
    """groups == 0 touches nothing: every pointer but plans may be NULL."""
    rc, _ = _call(product, [wss.PLANS["rows10x4"](oracle1000)], groups=0, group=None, shards=None, hdr=None,
                  seg_stamps=None, seg_order=None, seg_dgram=None, seg_dlen=None, fec_stamps=None, fec_order=None,
                  fec_dgram=None, fec_dlen=None)
    assert rc == 0


def test_wire_send_shapes_no_fec_takes_null_fec_pointers(product, oracle1000):
    """n_fec == 0: the SIM_FEC pointers pass the argument checks as NULL, the SIM_SEG ones are still checked.  The
    launch itself needs a device: without one a call that passes every check returns RFEC_EDEVICE (-2)."""
    plans = [wss.PLANS[s](oracle1000) for s in ("k1", "rows10x4")]
    null_fec = dict(n_fec=0, fec_stamps=None, fec_order=None, fec_dgram=None, fec_dlen=None)
    rc, err = _call(product, plans, seg_dlen=P_SL + 1, **null_fec)
    assert rc == -1 and "2-byte" in err, (rc, err)
    rc, err = _call(product, plans, seg_dgram=None, **null_fec)
    assert rc == -1 and "NULL" in err, (rc, err)
    if not torch.cuda.is_available():
        rc, err = _call(product, plans, **null_fec)
        assert rc == -2 and "launch" in err, (rc, err)
        rc, err = _call(product, plans, seg_order=None, fec_order=None)
        assert rc == -2 and "launch" in err, (rc, err)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gshapes(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return wss.GpuShapes(product)


def _check_case(gshapes, x):
    got = gshapes.send(x)  # (the guards and the inputs are checked in there)
    assert gshapes.launches == 1, gshapes.launches
    own = gshapes.per_shape(x)
    wss.compare_all(own, x.exp, "rfec_wire_encode_send per shape vs the oracle composed")
    wss.compare_all(got, x.exp, "rfec_wire_encode_send_shapes vs the oracle composed")
    wss.compare_all(got, own, "rfec_wire_encode_send_shapes vs rfec_wire_encode_send per shape")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(wss.CASES))
def test_wire_send_shapes_gpu(gshapes, inputs, name):
    """The call == the oracle composed per shape == the product's rfec_wire_encode_send per shape, whole slots and
    lengths, uncovered slots at their fill; one launch; the guards around the four outputs and every input buffer
    as uploaded.  A one-shape window in window order: also what rfec_wire_encode_send writes from the same
    buffers."""
    x = inputs(name)
    got = _check_case(gshapes, x)
    if name.startswith("one-shape"):
        assert len(x.plans) == 1 and x.covered_r.all() and (np.diff(x.desc["row0"].astype(np.int64)) > 0).all()
        wss.compare_all(got, gshapes.same_buffers(x), "rfec_wire_encode_send_shapes vs rfec_wire_encode_send in place")


@pytest.mark.gpu
def test_wire_send_shapes_persistent_loop_gpu(gshapes, inputs):
    """A wave takes four descriptors and the kernel's LDS admits one block of 16 waves per CU: with more units than
    that, some wave must loop.  Shapes drawn at random per group: mixed waves throughout."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = inputs("loop")
    assert cus * 16 < (x.G + 3) // 4, (cus, x.G)
    _check_case(gshapes, x)
