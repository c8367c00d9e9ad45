"""rfec_wire_regroup_shapes (one regroup pass over a window whose groups have
different shapes: a dense section of rfec_recover_indexed_out's tables per
shape).  On the CPU: the declarations, the argument checks without a device,
the rule (shapes_cases.regroup_shapes_ref) against one regroup_cases.regroup_ref
per plan and against its bent forms, and what the case set reaches.  On the GPU:
the call against the rule byte for byte, against the product's own
rfec_wire_regroup_index, and composed with rfec_recover_indexed_out against the
oracle's recovery."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import indexed_cases as ic
import regroup_cases as rc
import shapes_cases as sc

ALL_CASES = sc.CASES + [sc.LOOP_CASE]


@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's records, room and the rule's outputs, computed once and left unchanged."""
    cache = {}

    def get(c):
        if c not in cache:
            x = sc.make_inputs(oracle1000, c)
            cache[c] = (x, sc.ref_outputs(x))
        return cache[c]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_shapes_call_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    name = "rfec_wire_regroup_shapes"
    assert name in fec.header_functions() and name in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, name) and hasattr(lib, "wire_regroup_shapes")
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7
    assert fec.RFEC_REGROUP_MAX_SHAPES == sc.MAX_SHAPES and fec.RFEC_REGROUP_EFULL == sc.EFULL
    header = fec.HEADER.read_text()
    assert "#define RFEC_REGROUP_MAX_SHAPES 32" in header and "#define RFEC_REGROUP_EFULL (-7)" in header
    assert C.sizeof(fec.rfec_regroup_section) == 8 + 8 * 8


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
W = dict(recs=0x10000, shape_of=0x20001, rank_of=0x30004, anchor_of=0x40004, counts=0x50004, slot_of=0x60004)
S = dict(hdr=0x100004, present=0x110008, meta=0x120004, fec_size=0x130002, parity_present=0x140008,
         base_id=0x150004, src_of=0x160004, group_of=0x170004)


def _call(product, plans, n_plans=None, groups=4, fec_id0=7, n=100, capacity=1200, caps=None, sec=None,
          no_sections=False, **ptrs):
    """sec: {(p, name): pointer} overrides of the sections' fields; ptrs: overrides of the window pointers."""
    from razor_amd import fec
    w = dict(W, **ptrs)
    P = len(plans) if plans is not None else 0
    pa = (fec.rfec_plan * max(P, 1))(*(fec.as_plan(p) for p in plans or ()))
    sa = (fec.rfec_regroup_section * max(P, 1))()
    for p in range(P):
        sa[p].cap = groups if caps is None else caps[p]
        for name in S:
            setattr(sa[p], name, (sec or {}).get((p, name), S[name] + 0x1000000 * p))
    r = product.lib.rfec_wire_regroup_shapes(None if plans is None else pa, P if n_plans is None else n_plans,
                                             None if no_sections else sa, groups, fec_id0, n, w["recs"], capacity,
                                             *(w[name] for name in sc.WINDOW), None)
    return r, product.lib.rfec_last_error().decode()


def _two(oracle):
    return [rc.PLANS["rows10x4"](oracle), rc.PLANS["k2"](oracle)]


BAD = {
    "plans-null": (dict(plans=None), "plans"),
    "n-plans-0": (dict(n_plans=0), "n_plans"),
    "n-plans-33": (dict(n_plans=33), "n_plans"),
    "fec-id0-0": (dict(fec_id0=0), "fec_id0"),
    "groups-65536": (dict(groups=65536), "groups"),
    "n-2g": (dict(n=0x80000000), "n must be"),
    "cap-above-groups": (dict(caps=[4, 5]), "sections[1].cap"),
    "sections-null": (dict(no_sections=True), "sections"),
    **{f"null-{name}": ({name: None}, name) for name in W},
    **{f"null-section-{name}": (dict(sec={(1, name): None}), "sections[1]") for name in S},
    "recs-8": (dict(recs=W["recs"] + 8), "recs"),
    **{f"{name}-2": ({name: W[name] + 2}, name) for name in ("rank_of", "anchor_of", "counts", "slot_of")},
    **{f"section-{name}-4": (dict(sec={(0, name): S[name] + 4}), name) for name in ("present", "parity_present")},
    **{f"section-{name}-2": (dict(sec={(1, name): S[name] + 2}), name)
       for name in ("hdr", "meta", "base_id", "src_of", "group_of")},
    "section-fec_size-1": (dict(sec={(0, "fec_size"): S["fec_size"] + 1}), "fec_size"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_shapes_rejects(product, oracle1000, name):
    kw, msg = BAD[name]
    kw = dict(kw)
    plans = kw.pop("plans", _two(oracle1000))
    r, err = _call(product, plans, **kw)
    assert r == -1 and msg in err, (r, err)


def test_shapes_rejects_plans(product, oracle1000):
    rows, k2 = _two(oracle1000)
    r, err = _call(product, [rows, rc._hand_plan(129, 1, 129, [])])  # above RFEC_MAX_K
    assert r == -1 and "plan" in err and "out of range" in err, (r, err)
    bad = rc.PLANS["rows10x4"](oracle1000)
    bad.line[2].first, bad.line[2].count = 8, 4  # members 8..11 of k = 10
    r, err = _call(product, [k2, bad])
    assert r == -1 and "plan" in err and "beyond k" in err, (r, err)
    # the same (k, row, col) twice, whatever the lines: rows10x4 and full3x4k10 are both (10, 3, 4)
    r, err = _call(product, [rows, k2, rc.PLANS["full3x4k10"](oracle1000)])
    assert r == -1 and "plans[2]" in err and "(k, row, col)" in err, (r, err)
    # 32 plans pass the count check: 32 strips of different k (then a NULL pointer is what is refused)
    many = [rc._hand_plan(k, 1, k, [(0, 1, k, 0)]) for k in range(1, 33)]
    r, err = _call(product, many, shape_of=None)
    assert r == -1 and "shape_of" in err, (r, err)
    r, err = _call(product, many + [rc._hand_plan(33, 1, 33, [(0, 1, 33, 0)])], shape_of=None)
    assert r == -1 and "n_plans" in err, (r, err)


def test_shapes_zero_groups_optional_pointers_and_device(product, oracle1000):
    """groups == 0 touches nothing: every pointer but plans may be NULL.  A section with cap == 0 may hold NULLs, a
    plan without lines needs no meta / fec_size, n == 0 no recs / slot_of.  Without a device a valid call fails
    past every check, at the launch (RFEC_EDEVICE)."""
    plans = _two(oracle1000)
    nothing = {name: None for name in W}
    r, _ = _call(product, plans, groups=0, no_sections=True, **nothing)
    assert r == 0
    r, _ = _call(product, plans, groups=0, sec={(p, name): None for p in range(2) for name in S}, **nothing)
    assert r == 0
    r, err = _call(product, plans, groups=0, fec_id0=0, **nothing)
    assert r == -1 and "fec_id0" in err  # the value checks come first
    r, err = _call(product, plans, groups=0, caps=[0, 1], **nothing)
    assert r == -1 and "sections[1].cap" in err
    k1 = rc.PLANS["k1"](oracle1000)
    legal = (
        (plans, dict(caps=[4, 0], sec={(1, name): None for name in S})),
        ([plans[0], k1], dict(sec={(1, "meta"): None, (1, "fec_size"): None})),
        (plans, dict(n=0, recs=None, slot_of=None)),
        (plans, {}),
    )
    for pl, kw in legal:
        r, err = _call(product, pl, **dict(kw, counts=None))
        assert r == -1 and "counts" in err, (r, err)  # past the optional pointers
        if not torch.cuda.is_available():
            r, err = _call(product, pl, **kw)
            assert r == -2 and "launch" in err, (r, err)
    r, err = _call(product, plans, sec={(1, "meta"): None})  # k2 has a line
    assert r == -1 and "sections[1]" in err, (r, err)


# -- CPU: the rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_CASES, ids=sc.case_id)
def test_shapes_rule_equals_the_per_plan_rule(inputs, c):
    """The header's "Equivalence", rule against rule: for every g with shape_of[g] == p and rank_of[g] < cap, row
    rank_of[g] of section p == row g of regroup_cases.regroup_ref for plans[p] on the same records, and the
    records of such groups have the same slot_of, rebased."""
    x, ref = inputs(c)
    per_plan = [rc.regroup_ref(plan, x.G, x.fec_id0, x.recs, x.payload, x.capacity,
                               rc.new_outputs(plan, x.G, x.n, x.stride)) for plan in x.plans]
    rows = sc.check_equivalence(x, ref, per_plan, sc.case_id(c))
    if c[4] == "fit":
        assert rows == int(ref["counts"].sum()) == int((ref["shape_of"] != sc.NOSHAPE).sum())
    # rule 4 as the header states it, from the outputs alone
    shape, rank = ref["shape_of"], ref["rank_of"]
    for p in range(x.P):
        gs = np.nonzero(shape == p)[0]
        assert np.array_equal(rank[gs], np.arange(len(gs))) and ref["counts"][p] == len(gs)
    assert (rank[shape == sc.NOSHAPE] == sc.NONE).all() and (ref["anchor_of"][shape == sc.NOSHAPE] == sc.NONE).all()
    # rows past counts are empty
    for p, s in enumerate(ref["sec"]):
        lo = min(int(ref["counts"][p]), x.caps[p])
        assert (s["group_of"][lo:] == sc.NONE).all() and not s["present"][lo:].any() and not s["base_id"][lo:].any()
        assert not s["parity_present"][lo:].any() and (s["src_of"][lo * (x.plans[p].k + x.plans[p].n_lines):] == sc.NONE).all()


def test_shapes_cases_cover_their_conditions(inputs):
    """From the rule alone: every code, EFULL included; both shape conflicts; a window across 65535 -> 1 and G = 1;
    a group with no shape; counts above cap and a section with cap == 0; the second mask word; the rank pass's
    edges in a window of 65,535 groups with a few thousand records; the loop case's size."""
    seen = {}
    for c in sc.CASES:
        x, ref = inputs(c)
        for k, v in sc.conditions(x, ref).items():
            seen[k] = max(seen.get(k, 0), int(v))
    assert all(seen.values()), seen
    assert seen["shapes"] == 3 and seen["conflict_later"] >= 2 and seen["conflict_refused"] >= 1
    assert {c[2] for c in sc.CASES} == {1, 12, 65535} and {c[1] for c in sc.CASES} == {"c15", "c20"}
    x, ref = inputs(sc.CASES[-1])
    assert x.G == 65535 and 2000 <= x.n <= 8000 and x.caps == [64] * 3
    assert set(sc.EDGE_POSITIONS) >= {0, 63, 64, 1023, 1024, 65534}
    edge_ranks = ref["rank_of"][list(sc.EDGE_POSITIONS)]
    assert edge_ranks[0] == 0 and (np.diff(edge_ranks.astype(np.int64)) > 0).all()
    assert ref["rank_of"][65534] == ref["counts"][0] - 1 >= 64  # the window's last group, past the section's room
    x, ref = inputs(sc.LOOP_CASE)
    assert x.G == 3000 and x.P == 3 and 60000 <= x.n <= 80000
    filled = np.concatenate([s["src_of"][:int(ref["counts"][p]) * (x.plans[p].k + x.plans[p].n_lines)]
                             for p, s in enumerate(ref["sec"])]) != sc.NONE  # the slots of the rows in use
    # 15 % of the datagrams are lost, and with its one parity a k2 group: the other slots all have contenders
    assert filled.mean() > 0.75 and (ref["slot_of"] == sc.EDUP).sum() > filled.sum()


@pytest.mark.parametrize("wrong", sc.WRONG)
def test_shapes_cases_catch_each_bent_rule(inputs, wrong):
    caught = []
    for c in sc.CASES:
        x, ref = inputs(c)
        try:
            sc.compare(sc.ref_outputs(x, (wrong,)), ref, wrong)
        except AssertionError:
            caught.append(sc.case_id(c))
    assert caught, wrong
    if wrong in ("counts_clamped", "full_wraps"):
        assert all("tight" in c or "c64" in c for c in caught), caught


def test_shapes_arena_checks_can_fail(inputs):
    """The rule behind the arena equals the rule; with two group_of entries swapped after the call the
    comparison fails."""
    x, ref = inputs(sc.CASES[0])
    eng = sc.RefShapes()
    sc.compare(eng.run(x), ref, "the rule in an arena")
    eng.mutate = sc.swap_two_group_of(x, ref)
    with pytest.raises(AssertionError, match="group_of"):
        sc.compare(eng.run(x), ref, "swapped group_of entries")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL_CASES, ids=sc.case_id)
def test_wire_regroup_shapes_gpu(gpu_lib, inputs, c):
    """The five window outputs and every section's eight tables == regroup_shapes_ref's, byte for byte over the
    pre-fill; the guards whole and recs unchanged; six launches."""
    x, ref = inputs(c)
    gpu_lib.timing_events(None, None)
    got = sc.GpuShapes(gpu_lib).run(x)
    assert gpu_lib.timing_launches() == 6
    sc.compare(got, ref, f"rfec_wire_regroup_shapes {sc.case_id(c)}")


def _without_records(x):
    y = sc.Inputs()
    y.__dict__.update(x.__dict__)
    y.recs, y.payload, y.n = x.recs[:0], x.payload[:0], 0
    return y


def test_shapes_rule_without_records(inputs):
    """n == 0: no group has a shape, every section row is empty."""
    x = _without_records(inputs(sc.CASES[1])[0])
    ref = sc.ref_outputs(x)
    assert (ref["shape_of"] == sc.NOSHAPE).all() and (ref["rank_of"] == sc.NONE).all() and not ref["counts"].any()
    assert all((s["group_of"] == sc.NONE).all() and (s["src_of"] == sc.NONE).all() and not s["present"].any()
               for s, cap in zip(ref["sec"], x.caps) if cap)
    assert (ref["sec"][0]["hdr"].view(np.uint8) == sc.FILL).all()


@pytest.mark.gpu
def test_wire_regroup_shapes_without_records_gpu(gpu_lib, inputs):
    """n == 0 (recs and slot_of of no bytes): the record passes are not launched, the rest equals the rule."""
    x = _without_records(inputs(sc.CASES[1])[0])
    gpu_lib.timing_events(None, None)
    got = sc.GpuShapes(gpu_lib).run(x)
    assert gpu_lib.timing_launches() == 4
    sc.compare(got, sc.ref_outputs(x), "rfec_wire_regroup_shapes, n == 0")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [sc.CASES[1], sc.CASES[3]], ids=sc.case_id)
def test_wire_regroup_shapes_equals_regroup_index_gpu(gpu_lib, inputs, c):
    """Product against product: every section row equals the row of the product's own rfec_wire_regroup_index for
    that plan on the same records."""
    x, _ = inputs(c)
    got = sc.GpuShapes(gpu_lib).run(x)
    per_plan = []
    for name, plan in zip(sc.PLANSETS[c[0]], x.plans):
        y = sc.Inputs()
        y.case, y.plan, y.G, y.n, y.recs = (name, c[1], x.G, x.fec_id0, None), plan, x.G, x.n, x.recs
        y.fec_id0, y.capacity, y.stride = x.fec_id0, x.capacity, x.stride
        per_plan.append(ic.regroup_index_gpu(gpu_lib, y))
    assert sc.check_equivalence(x, got, per_plan, sc.case_id(c)) >= 4


@pytest.mark.gpu
def test_wire_regroup_shapes_gpu_checks_can_fail(gpu_lib, inputs):
    x, ref = inputs(sc.CASES[0])
    eng = sc.GpuShapes(gpu_lib)
    eng.mutate = sc.swap_two_group_of(x, ref)
    with pytest.raises(AssertionError, match="group_of"):
        sc.compare(eng.run(x), ref, "swapped group_of entries")


@pytest.mark.gpu
def test_shapes_chain_composed_gpu(gpu_lib, oracle1000):
    """24 groups of three plans at c20, two segments lost per group: the parse's records and rows uploaded, one
    rfec_wire_regroup_shapes, counts read back, one rfec_recover_indexed_out per section over counts[p] groups ==
    oracle.recover_batch_out on each plan's sender batch with the same losses, mapped through group_of; and the
    same with groups = cap, whose trailing rows decode to nothing."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0 = 24, 2, 65520
    capacity, stride = sc.GEOMS["c20"]
    plans = [sc.PLANS[name](oracle) for name in sc.PLANSETS["decode3"]]
    P = len(plans)
    rng = np.random.default_rng(zlib.crc32(b"shapes-composed"))
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
        exp.append((gs, oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp,
                                                 capacity, E)))
        recs_l.append(b.recs[~lost])
        pay_l.append(b.pay[~lost])
    order = rng.permutation(sum(len(r) for r in recs_l))
    recs, pay = np.concatenate(recs_l)[order], np.concatenate(pay_l)[order]
    N = len(recs)

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
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, d_recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    torch.cuda.synchronize(dev)
    counts = down(win["counts"], np.uint32, (P,))
    assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), shape)
    assert counts.tolist() == [int((shape == p).sum()) for p in range(P)]
    cw = rc.cd16(capacity)
    recovered = 0
    for p, plan in enumerate(plans):
        gs, (e_sh, e_hd, e_ix, e_rec) = exp[p]
        group_of = down(tab[p]["group_of"], np.uint32, (G,))
        j_of = np.searchsorted(gs, group_of[:counts[p]])
        assert np.array_equal(gs[j_of], group_of[:counts[p]]) and (group_of[counts[p]:] == sc.NONE).all()
        for groups in (int(counts[p]), G):
            rec_, osh, ohd, oix = zeros(groups * 16, 0xEE), zeros(groups * E * stride, 0x3C), \
                zeros(groups * E * 20, 0x3C), zeros(groups * E, 0x3C)
            ws = zeros(lib.workspace_size(plan, groups), 0x11)
            lib.recover_indexed_out(plan, groups, stride, capacity, d_rows.data_ptr(), N,
                                    *(tab[p][name].data_ptr() for name in ("src_of", "hdr", "present", "meta", "fec_size",
                                                                           "parity_present")),
                                    rec_.data_ptr(), E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), ws.data_ptr(), st)
            torch.cuda.synchronize(dev)
            g_ix, g_rec = down(oix, np.uint8, (groups, E)), down(rec_, np.uint64, (groups, 2))
            g_hd, g_sh = down(ohd, rc.po.HDR_DTYPE, (groups, E)), down(osh, np.uint8, (groups, E, stride))
            c = int(counts[p])
            assert np.array_equal(g_ix[:c], e_ix[j_of]) and np.array_equal(g_rec[:c], e_rec[j_of]), (p, groups)
            ok = e_ix[j_of] != 0xFF
            assert np.array_equal(g_hd[:c][ok], e_hd[j_of][ok]), (p, groups)
            assert np.array_equal(g_sh[:c][ok][:, :cw], e_sh[j_of][ok][:, :cw]), (p, groups)
            assert (g_ix[c:] == 0xFF).all() and not g_rec[c:].any(), (p, groups)  # the trailing rows: nothing
            recovered += int(ok.sum())
    assert recovered >= G  # of the 2 G segments lost, in each of the two runs
