"""rfec_recover_deliver: what rfec_recover_indexed_shapes_out wrote -- dense over
the sections, per_group out slots a row, holes where out_index is 0xFF, section
order -- as a dense list of rfec_rx_seg records and payload rows in window
order, on the device.  On the CPU: the declaration and binding, every argument
check with its message and in its order, the accepted NULLs, the empty window,
the workspace size, the rule against the reference's receiver on a mixed-shape
in-order stream, each bent rule caught, and the case set's census.  On the GPU:
every case against deliver_ref over all six outputs with the tag and the launch
count, the composed chain behind one rfec_wire_regroup_shapes and one
rfec_recover_indexed_shapes_out with no synchronisation in between, and the
self-test that the comparison can fail (deliver_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import deliver_cases as dc
import regroup_cases as rc
import shapes_cases as sc

NAME, METHOD = "rfec_recover_deliver", "recover_deliver"
WS_NAME = "rfec_recover_deliver_workspace_size"


@pytest.fixture(scope="module")
def cases():
    """Every case's inputs and the rule's outputs, computed once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            x = dc.make(name)
            cache[name] = (x, dc.RefDeliver().run(x))
        return cache[name]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_deliver_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    for name in (NAME, WS_NAME):
        assert name in fec.header_functions() and name in fec._SIGS
        for lib in (product, product1200):
            assert hasattr(lib.lib, name)
    for lib in (product, product1200):
        assert hasattr(lib, METHOD) and hasattr(lib, "recover_deliver_workspace_size")
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7 and product1200.lib.rfec_abi_version() == 7


def test_deliver_workspace_size(product):
    sizes = [product.recover_deliver_workspace_size(G) for G in range(0, 2000)] + \
        [product.recover_deliver_workspace_size(G) for G in (65534, 65535)]
    assert all(s % 16 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] >= 16 and sizes[-1] >= 4 * 65535 + 4 * 256


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(shape_of=0x10001, rank_of=0x20004, out_shards=0x30010, out_hdr=0x40004, out_index=0x50001, seg=0x60004,
         seg_payload=0x70010, first_of=0x80004, n_out=0x90004, workspace=0xA0010)
GROUP_OF = 0xB0004


def _call(product, n=2, groups=(4, 4), caps=None, group_of=None, G=8, fec_id0=7, stride=1216, capacity=1200, per_group=2,
          max_out=16, n_plans=None, null_plans=False, null_sections=False, plans=None, **ptrs):
    """One raw call on made-up addresses: groups a tuple or None (NULL), caps the sections' cap (default: groups, or
    4), group_of per section an address or None."""
    from razor_amd.fec import as_plan, rfec_plan, rfec_regroup_section
    plans = plans or [dc.hand_plan() for _ in range(n)]
    n = len(plans)
    caps = list(caps) if caps is not None else (list(groups) if groups is not None else [4] * n)
    group_of = list(group_of) if group_of is not None else [GROUP_OF + 0x1000 * p for p in range(n)]
    pa = (rfec_plan * max(n, 1))(*(as_plan(p) for p in plans))
    sa = (rfec_regroup_section * max(n, 1))(*(rfec_regroup_section(cap=caps[p], group_of=group_of[p])
                                             for p in range(n)))
    ga_ = None if groups is None else (C.c_uint32 * max(n, 1))(*groups)
    p = dict(P, **ptrs)
    r = getattr(product.lib, NAME)(None if null_plans else pa, n if n_plans is None else n_plans,
                                   None if null_sections else sa, ga_, G, fec_id0, p["shape_of"], p["rank_of"], stride,
                                   capacity, per_group, p["out_shards"], p["out_hdr"], p["out_index"], max_out,
                                   p["seg"], p["seg_payload"], p["first_of"], p["n_out"], p["workspace"], None)
    return r, product.lib.rfec_last_error().decode()


def _bad_plan():
    p = rc._hand_plan(10, 3, 4, [(0, 1, 4, 0), (4, 1, 4, 1), (8, 1, 4, 2)])  # members 8..11 of k = 10
    return [dc.hand_plan(), p]


# name -> (keyword arguments, the message)
BAD_ARGS = {
    "null-plans": (dict(null_plans=True), "plans is NULL"),
    "no-plans": (dict(n_plans=0), "n_plans"),
    "33-plans": (dict(n_plans=33), "n_plans"),
    "null-sections": (dict(null_sections=True), "sections is NULL"),
    "bad-plan": (dict(plans="bad"), "beyond k"),
    "window-65536": (dict(G=65536), "window_groups"),
    "fec-id-0": (dict(fec_id0=0), "fec_id0"),
    "stride-0": (dict(stride=0), "stride"),
    "stride-1208": (dict(stride=1208), "stride"),
    "capacity-above-stride": (dict(capacity=1217), "capacity"),
    "per-group-0": (dict(per_group=0), "per_group"),
    "groups-above-cap": (dict(groups=(4, 5), caps=(4, 4)), "groups[1] must be <= sections[p].cap"),
    "lanes": (dict(groups=(4, 1 << 22), stride=1024, capacity=1024, per_group=8), "window too large"),
    "rows-2^32": (dict(groups=(1 << 31, 1 << 31), stride=16, capacity=16, per_group=1), "window too large"),
    "null-shape-of": (dict(shape_of=None), "NULL buffer"),
    "null-rank-of": (dict(rank_of=None), "NULL buffer"),
    "null-first-of": (dict(first_of=None), "NULL buffer"),
    "null-n-out": (dict(n_out=None), "NULL buffer"),
    "null-workspace": (dict(workspace=None), "NULL buffer"),
    "null-seg": (dict(seg=None), "NULL buffer (seg, seg_payload)"),
    "null-seg-payload": (dict(seg_payload=None), "NULL buffer (seg, seg_payload)"),
    "null-out-shards": (dict(out_shards=None), "NULL buffer (out_shards, out_hdr, out_index)"),
    "null-out-hdr": (dict(out_hdr=None), "NULL buffer (out_shards, out_hdr, out_index)"),
    "null-out-index": (dict(out_index=None), "NULL buffer (out_shards, out_hdr, out_index)"),
    "null-group-of": (dict(group_of=(GROUP_OF, None)), "sections[1].group_of is NULL"),
    "out-shards-8": (dict(out_shards=0x30008), "16-byte aligned"),
    "seg-payload-8": (dict(seg_payload=0x70008), "16-byte aligned"),
    "workspace-8": (dict(workspace=0xA0008), "16-byte aligned"),
    "out-hdr-2": (dict(out_hdr=0x40002), "4-byte aligned"),
    "seg-2": (dict(seg=0x60002), "4-byte aligned"),
    "rank-of-2": (dict(rank_of=0x20002), "4-byte aligned"),
    "first-of-2": (dict(first_of=0x80002), "4-byte aligned"),
    "n-out-2": (dict(n_out=0x90002), "4-byte aligned"),
    "group-of-2": (dict(group_of=(GROUP_OF + 2, GROUP_OF)), "sections[0].group_of must be 4-byte aligned"),
}


def _kw(kw):
    kw = dict(kw)
    if kw.get("plans") == "bad":
        kw["plans"] = _bad_plan()
    return kw


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_deliver_rejects(product, name):
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, **_kw(kw))
    assert r == -1 and msg in err, (r, err)


def test_deliver_checks_in_order(product):
    """Each check comes before the next: a call that breaks two is refused for the earlier one.  The order is plans,
    n_plans, sections, each plan, window_groups, fec_id0, stride, capacity, per_group, groups <= cap, the lanes, the
    NULL pointers, the alignments."""
    steps = [
        (dict(null_plans=True), "plans is NULL"),
        (dict(n_plans=33), "n_plans"),
        (dict(null_sections=True), "sections is NULL"),
        (dict(plans="bad"), "beyond k"),
        (dict(G=65536), "window_groups"),
        (dict(fec_id0=0), "fec_id0"),
        (dict(stride=1208), "stride"),
        (dict(capacity=1300), "capacity"),
        (dict(per_group=0), "per_group"),
        (dict(groups=(4, 5), caps=(4, 4)), "sections[p].cap"),
        (dict(groups=(4, 1 << 27), stride=1024, capacity=1024), "window too large"),
        (dict(seg=None), "NULL"),
        (dict(out_index=None), "NULL buffer (out_shards"),
        (dict(group_of=(None, GROUP_OF)), "group_of is NULL"),
        (dict(workspace=0xA0008), "16-byte aligned"),
        (dict(n_out=0x90002), "4-byte aligned"),
        (dict(group_of=(GROUP_OF, GROUP_OF + 2)), "group_of must be 4-byte aligned"),
    ]
    for i, (kw, msg) in enumerate(steps):
        for later, _ in steps[i + 1:]:
            both = _kw(later)
            both.update(_kw(kw))
            r, err = _call(product, **both)
            assert r == -1 and msg in err, (kw, later, r, err)


def test_deliver_lane_bounds(product):
    """One lane below the bound passes the value checks (then a NULL pointer is what is refused); the bound counts the
    chunks of work, not the stride."""
    r, err = _call(product, groups=((1 << 22) - 1, 0), per_group=8, stride=1024, capacity=1024, seg=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, groups=(1 << 22, 0), per_group=8, stride=1024, capacity=1009, seg=None)
    assert r == -1 and "window too large" in err, (r, err)
    r, err = _call(product, groups=(1 << 22, 0), per_group=8, stride=1024, capacity=1008, seg=None)
    assert r == -1 and "NULL" in err, (r, err)


def test_deliver_accepted_nulls_empty_window_and_device(product):
    """window_groups == 0 touches nothing: every pointer but plans may be NULL, and the value checks still come
    first.  seg and seg_payload may be NULL with max_out == 0, the decode's outputs with no rows, a section's group_of
    with groups[p] == 0; groups NULL means cap.  Without a device a valid call fails past every check, at the
    launch."""
    nothing = {n: None for n in P}
    r, err = _call(product, G=0, null_sections=True, groups=None, **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, G=0, group_of=(None, None), **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, G=0, per_group=0, **nothing)
    assert r == -1 and "per_group" in err, (r, err)
    r, err = _call(product, G=0, groups=(4, 5), caps=(4, 4), **nothing)
    assert r == -1 and "groups[1]" in err, (r, err)
    ok = [dict(max_out=0, seg=None, seg_payload=None),
          dict(groups=(0, 0), caps=(4, 4), group_of=(None, None), out_shards=None, out_hdr=None, out_index=None),
          dict(groups=None, caps=(0, 0), group_of=(None, None), out_shards=None, out_hdr=None, out_index=None),
          dict(groups=(0, 4), group_of=(None, GROUP_OF)), dict(groups=None, caps=(3, 5)), {}]
    for kw in ok:
        r, err = _call(product, **kw, workspace=0xA0008)  # past the NULL checks, at the alignment
        assert r == -1 and "aligned" in err, (kw, r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, **kw)
            assert r == -2 and "launch" in err, (kw, r, err)
    r, err = _call(product, groups=None, caps=(4, 4), group_of=(None, GROUP_OF))  # cap rows: the pointer is wanted
    assert r == -1 and "sections[0].group_of is NULL" in err, (r, err)


# -- CPU: the rule against the reference's receiver --------------------------------------------------------------------
RX_SEED = 3


def test_deliver_rule_delivers_what_the_receiver_delivers(oracle1000):
    """A mixed-shape in-order stream (deliver_cases.inorder_window: three plans interleaved over 40 groups from fec_id
    65520, base ids ascending with the window index, every parity after its group's segments, all timestamps within
    1 s, lost and duplicated datagrams): regroup_shapes_ref, then oracle.recover_batch_out per section, then
    deliver_ref delivers, entry for entry and in order, what the reference's receiver (oracle.rx_recover, event by
    event) delivers sorted by packet id -- header records, fec_ids, payload bytes."""
    o = oracle1000
    G, fec_id0, E = 40, 65520, 10
    plans, shape, recs, pay, capacity, stride = dc.inorder_window(o, RX_SEED, G, fec_id0)
    P = len(plans)
    assert fec_id0 + G > 65536 and E <= min(p.k for p in plans)
    caps = [G] * P
    reg = sc.regroup_shapes_ref(plans, caps, G, fec_id0, recs, capacity, sc.new_outputs(plans, caps, G, len(recs), 0))
    assert np.array_equal(reg["shape_of"], shape)  # every group kept a parity
    assert (reg["slot_of"] == sc.EDUP).any()
    rows = [int(c) for c in reg["counts"]]
    osh, ohd, oix = dc.decode_sections(o, plans, caps, rows, reg["sec"], pay, capacity, stride, E)
    x = dc.from_tables("inorder", plans, caps, rows, G, fec_id0, reg["shape_of"], reg["rank_of"],
                       [s["group_of"] for s in reg["sec"]], capacity, stride, E, osh, ohd, oix, None)
    out = dc.RefDeliver().run(x)
    T = int(out["n_out"][0])
    rx, rxp, _, dropped = o.rx_recover(recs, pay, capacity)
    # conditions the reference alone meets for this seed
    assert dropped == 0 and len(rx) >= 20
    rx_shape = reg["shape_of"][[(int(f) - fec_id0) % 65535 for f in rx["fec_id"]]]
    assert set(rx_shape.tolist()) == set(range(P))
    by_id = np.argsort(rx["hdr"]["seq"], kind="stable")
    rx, rxp = rx[by_id], rxp[by_id]
    assert T == len(rx), (T, len(rx))
    seg, segp = out["seg"][:T], out["seg_payload"][:T]
    assert np.array_equal(seg["hdr"], rx["hdr"])
    assert np.array_equal(seg["fec_id"], rx["fec_id"]) and not seg["reserved"].any()
    assert np.array_equal(segp[:, :capacity], rxp[:, :capacity])
    assert (seg["fec_id"] < 100).any() and (seg["fec_id"] > 65000).any()  # both sides of 65535 -> 1


# -- CPU: the checks can fail, the case set ----------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", dc.WRONG)
def test_deliver_cases_catch_each_wrong_rule(cases, wrong):
    """Each bent rule of deliver_ref differs from the rule on at least one case."""
    caught = []
    for name in dc.CASES:
        x, ref = cases(name)
        try:
            dc.compare(dc.RefDeliver((wrong,)).run(x), ref, wrong)
        except AssertionError:
            caught.append(name)
    assert caught, wrong


def test_deliver_cases_cover_their_conditions(cases):
    """The case set holds every condition the GPU tests are there for."""
    c = {name: dc.conditions(*cases(name)) for name in dc.CASES}
    x = {name: cases(name)[0] for name in dc.CASES}
    # the window's size, every group decoded at the workgroup scan's edge; several blocks
    assert x["G1"].G == 1 and x["G1"].T >= 1
    for G in (255, 256, 257):
        assert x[f"G{G}"].G == G and c[f"G{G}"]["decoded"] == G
    assert x["G600"].G == 600 and dc.launches(600) == 3 and dc.launches(256) == 2 and dc.launches(257) == 3
    # the 65,535-group window
    b = x["big"]
    assert b.G == 65535 and b.fec_id0 == 65530 and 200 <= c["big"]["decoded"] <= 400 and c["big"]["wrap"]
    assert all(b.shape_of[g] != dc.NOSHAPE for g in dc.BIG_POSITIONS) and c["big"]["no_shape_group"]
    # out-slot patterns
    assert [x[f"E{E}"].E for E in (1, 2, 4, 6)] == [1, 2, 4, 6]
    for E in (2, 4, 6):
        for key in ("row_all_holes", "row_all_delivered", "hole_before", "hole_after"):
            assert c[f"E{E}"][key], (E, key)
    assert c["E1"]["row_all_holes"] and c["E1"]["row_all_delivered"]
    assert c["E4"]["hole_between"] and c["E6"]["hole_between"] and c["unsorted"]["unsorted_index"]
    # payload lanes
    for name, cd in (("cd1", 1), ("cd2", 2), ("cd75", 75)):
        assert rc.cd16(x[name].capacity) // 16 == cd and 30 <= x[name].G <= 50 and c[name]["last_entry_mid_wave"]
    assert x["cd75"].capacity == 1200 and x["cd75"].stride == 1216
    # overflow
    T = x["max-T"].T
    assert x["max-T"].max_out == T and x["max-T-1"].max_out == x["max-T-1"].T - 1
    assert x["max-1"].max_out == 1 and x["max-0"].max_out == 0 and x["max-1"].T > 1 and x["max-0"].T > 0
    # section variants
    assert c["null-groups"]["trailing_none_rows"] and x["null-groups"].groups is None
    assert c["below-counts"]["rank_past_groups"]
    assert [c[f"zero-{w}"]["zero_sections"] for w in ("first", "middle", "last")] == [[0], [1], [2]]
    for w in ("first", "middle", "last"):
        assert sum(g is None for g in x[f"zero-{w}"].group_of) == 1 and x[f"zero-{w}"].T > 0
    assert x["thirty-two"].P == 32 and x["one-section"].P == 1
    assert x["no-rows"].R == 0 and x["no-rows"].G > 0 and x["no-rows"].T == 0
    s = x["swap"]
    assert s.P == 2 and s.rows[0] == s.rows[1] and s.T > 0
    # every default case crosses 65535 -> 1
    assert all(c[name]["wrap"] for name in dc.CASES if x[name].fec_id0 == 65530 and x[name].G > 6)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _check_call(eng, G):
    assert eng.last_path == (dc.DELIVER | dc.launches(G) << 8), hex(eng.last_path)
    assert eng.last_launches == dc.launches(G), eng.last_launches


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.CASES))
def test_deliver_gpu(gpu_lib, cases, name):
    """The product == deliver_ref over all six outputs; the guards, every input, the delivered rows' tails and the
    entries at and past min(T, max_out) as before the call (the engine's checks); the tag and the launch count."""
    x, ref = cases(name)
    eng = dc.GpuDeliver(gpu_lib)
    out = eng.run(x)
    _check_call(eng, x.G)
    dc.compare(out, ref, f"{NAME} {name}")


@pytest.mark.gpu
def test_deliver_gpu_checks_can_fail(gpu_lib, cases):
    """Two sections' group_of pointers swapped in the call: the comparison fails (the tables have as many words, and
    every entry stays a group of the window)."""
    x, ref = cases("swap")
    out = dc.GpuDeliver(gpu_lib).run(x, swap=(0, 1))
    with pytest.raises(AssertionError):
        dc.compare(out, ref, "swapped group_of pointers")


@pytest.mark.gpu
def test_deliver_chain_composed_gpu(gpu_lib, oracle1000):
    """24 groups of three plans at c20 from fec_id 65520 (the window crosses 65535 -> 1), two segments lost per group,
    the arrival order shuffled: rfec_wire_regroup_shapes, rfec_recover_indexed_shapes_out and rfec_recover_deliver on
    one stream with no synchronisation in between, with groups NULL and with groups = min(counts, cap) == deliver_ref
    over oracle.recover_batch_out on each plan's sender batch with the same losses.  T == 48."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0 = 24, 2, 65520
    capacity, stride = sc.GEOMS["c20"]
    plans = [sc.PLANS[name](oracle) for name in sc.PLANSETS["decode3"]]
    P = len(plans)
    rng = np.random.default_rng(zlib.crc32(b"recover-deliver-composed"))
    shape = rng.permutation(np.arange(G) % P)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    recs_l, pay_l, exp = [], [], []
    for p, plan in enumerate(plans):
        gs = np.nonzero(shape == p)[0]
        k, n = plan.k, plan.n_lines
        b = rc.sender_batch(oracle, plan, len(gs), 1, capacity, stride, rng,
                            (5000 + gs.astype(np.uint64) * 140).astype(np.uint32))
        assert n and not b.status.any()
        b.recs["fec_id"] = [rc.fec_id_of(fec_id0, int(g)) for g in np.concatenate([np.repeat(gs, k), np.repeat(gs, n)])]
        lost = np.zeros(len(b.recs), bool)
        lost[(np.arange(len(gs))[:, None] * k + np.stack([rng.choice(k, 2, replace=False) for _ in gs])).reshape(-1)] = True
        present = np.zeros((len(gs), 2), np.uint64)
        for j, i in zip(*np.nonzero(~lost[:len(gs) * k].reshape(len(gs), k))):
            present[j, i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        pp = np.full(len(gs), (1 << n) - 1, np.uint64)
        exp.append(oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp, capacity, E))
        recs_l.append(b.recs[~lost])
        pay_l.append(b.pay[~lost])
    order = rng.permutation(sum(len(r) for r in recs_l))
    recs, pay = np.concatenate(recs_l)[order], np.concatenate(pay_l)[order]
    N = len(recs)
    # the tables the regroup must write: every group keeps its parities, so its shape is the sender's
    rank = np.zeros(G, np.uint32)
    for p in range(P):
        rank[shape == p] = np.arange((shape == p).sum())
    counts = [int((shape == p).sum()) for p in range(P)]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    def down(t, dtype, shp):
        nb = int(np.prod(shp)) * np.dtype(dtype).itemsize
        return t[:nb].cpu().numpy().view(dtype).reshape(shp)

    d_recs, d_rows = up(recs), up(pay)
    w, secs = sc.shapes_of(plans, [G] * P, G, N)
    win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
    tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
           for s in secs]
    sections = [dict(cap=G, **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(P)]
    max_out = 64
    for groups in (None, [min(c, G) for c in counts]):
        rows_of = [G] * P if groups is None else groups
        total = int(sum(rows_of))
        rec_, osh, ohd, oix = zeros(total * 16, 0xEE), zeros(total * E * stride, 0x3C), zeros(total * E * 20, 0x3C), \
            zeros(total * E, 0x3C)
        seg, segp = zeros(max_out * 24, dc.FILL), zeros(max_out * stride, dc.FILL)
        first_of, n_out = zeros((G + 1) * 4, dc.FILL), zeros(4, dc.FILL)
        ws = zeros(lib.recover_deliver_workspace_size(G), 0x11)
        # three calls, one stream, no synchronisation
        lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, d_recs.data_ptr(), capacity,
                                *(win[name].data_ptr() for name in sc.WINDOW), st)
        lib.recover_indexed_shapes_out(plans, sections, groups, stride, capacity, d_rows.data_ptr(), N,
                                       rec_.data_ptr(), E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), st)
        lib.lib.rfec_timing_events(None, None)
        lib.recover_deliver(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                            stride, capacity, E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), max_out,
                            seg.data_ptr(), segp.data_ptr(), first_of.data_ptr(), n_out.data_ptr(), ws.data_ptr(), st)
        assert int(lib.lib.rfec_timing_launches()) == dc.launches(G)
        assert int(lib.lib.rfec_indexed_last_path()) == (dc.DELIVER | dc.launches(G) << 8)
        torch.cuda.synchronize(dev)
        assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), shape)
        assert np.array_equal(down(win["rank_of"], np.uint32, (G,)), rank)
        # the rule over the oracle's decode of each plan's batch, its rows those of the section (rank order is the
        # batch's order: both are window order)
        e_sh = np.zeros((total, E, stride), np.uint8)
        e_hd = np.zeros((total, E), rc.po.HDR_DTYPE)
        e_ix = np.full((total, E), 0xFF, np.uint8)
        first = np.concatenate([[0], np.cumsum(rows_of)]).astype(int)
        group_of = []
        for p in range(P):
            c = counts[p]
            e_sh[first[p]:first[p] + c], e_hd[first[p]:first[p] + c], e_ix[first[p]:first[p] + c] = exp[p][:3]
            go = np.full(G, sc.NONE, np.uint32)
            go[:c] = np.nonzero(shape == p)[0]
            group_of.append(go)
            assert np.array_equal(down(tab[p]["group_of"], np.uint32, (G,)), go)
        x = dc.from_tables("composed", plans, [G] * P, groups, G, fec_id0, shape, rank, group_of, capacity, stride, E,
                           e_sh, e_hd, e_ix, max_out)
        ref = dc.deliver_ref(x, dc.new_outputs(x))
        assert x.T == 48
        got = {"seg": down(seg, rc.po.RX_SEG, (max_out,)), "seg_payload": down(segp, np.uint8, (max_out, stride)),
               "first_of": down(first_of, np.uint32, (G + 1,)), "n_out": down(n_out, np.uint32, (1,))}
        dc.compare(got, ref, f"{NAME} composed, groups {groups}")
        dc.check_untouched(x, got, "composed")
