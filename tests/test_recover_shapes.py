"""rfec_recover_indexed_shapes_out: the sections of a window of several shapes
(rfec_wire_regroup_shapes' tables) decoded in one launch of
k_decode_shapes_indexed -- a full row + column plan of k = 6..16 as
rfec_recover_indexed_matrix_out decodes it, a row layout of rows of <= 4 segments
with k <= 64 as rfec_recover_indexed_out does.  On the CPU: the declaration and
binding, every argument check in its order, the plan refusals and acceptances
without a device, and the window set's census against the reference.  On the
GPU: every window against the reference and, byte for byte, against the
single-shape call of each section on the same arena; the erasure-pattern sweeps
of k = 6..16 as the sections of one call; the composed chain behind one
rfec_wire_regroup_shapes; the empty pool; and the self-test that the comparison
can fail (recover_shapes_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import indexed_cases as ic
import indexed_matrix_cases as imc
import pattern_cases as pc
import recover_shapes_cases as rsc
import regroup_cases as rc
import shapes_cases as sc

NAME, METHOD = "rfec_recover_indexed_shapes_out", "recover_indexed_shapes_out"


@pytest.fixture(scope="module")
def windows(oracle1000):
    """Every window's inputs and reference outputs, computed once and left unchanged; windows that hold the same
    section share it."""
    sections, cache = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = rsc.make_window(oracle1000, rsc.WINDOW[name], sections)
        return cache[name]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_shapes_decode_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert NAME in fec.header_functions() and NAME in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, NAME) and hasattr(lib, METHOD)
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(rows=0x10000, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001)
T = dict(src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002, parity_present=0x70008)


def _call(product, plans, groups=(4,), caps=None, tables=None, stride=1216, capacity=1200, n_rows=100, per_group=2,
          n_plans=None, null_plans=False, null_sections=False, **ptrs):
    """One raw call on made-up addresses: plans a list, groups a tuple or None (NULL), caps the sections' cap
    (default: groups, or 4), tables per section a dict over T (None: a NULL pointer)."""
    from razor_amd.fec import as_plan, rfec_plan, rfec_regroup_section
    n = len(plans)
    caps = list(caps) if caps is not None else (list(groups) if groups is not None else [4] * n)
    tables = tables or [{}] * n
    pa = (rfec_plan * max(n, 1))(*(as_plan(p) for p in plans))
    sa = (rfec_regroup_section * max(n, 1))(*(rfec_regroup_section(cap=caps[p], **dict(T, **tables[p]))
                                             for p in range(n)))
    ga_ = None if groups is None else (C.c_uint32 * max(n, 1))(*groups)
    p = dict(P, **ptrs)
    r = getattr(product.lib, NAME)(None if null_plans else pa, n if n_plans is None else n_plans,
                                   None if null_sections else sa, ga_, stride, capacity, p["rows"], n_rows,
                                   p["recovered"], per_group, p["out_shards"], p["out_hdr"], p["out_index"], None)
    return r, product.lib.rfec_last_error().decode()


def _two(oracle):
    return [ic.PLANS["full3x4k10"](oracle), ic.PLANS["rows12x3"](oracle)]


NULL_T = {name: None for name in T}

# name -> (keyword arguments over a matrix and a row-layout section of 4 groups each, the message)
BAD_ARGS = {
    "null-plans": (dict(null_plans=True), "plans is NULL"),
    "no-plans": (dict(n_plans=0), "n_plans"),
    "33-plans": (dict(n_plans=33), "n_plans"),
    "null-sections": (dict(null_sections=True), "sections is NULL"),
    "stride-0": (dict(stride=0), "stride"),
    "stride-1208": (dict(stride=1208), "stride"),
    "capacity-above-stride": (dict(capacity=1217), "capacity"),
    "per-group-0": (dict(per_group=0), "per_group"),
    "per-group-above-min-k": (dict(per_group=11), "per_group"),  # the matrix has k = 10, the rows k = 12
    "groups-above-cap": (dict(groups=(4, 5), caps=(4, 4)), "groups[1] must be <= sections[p].cap"),
    "lanes": (dict(groups=(4, 1 << 22), stride=1024, capacity=1024, per_group=8), "groups[1]: section too large"),
    "null-rows": (dict(rows=None), "NULL buffer"),
    "null-recovered": (dict(recovered=None), "NULL buffer"),
    "null-out-shards": (dict(out_shards=None), "NULL buffer"),
    "null-out-hdr": (dict(out_hdr=None), "NULL buffer"),
    "null-out-index": (dict(out_index=None), "NULL buffer"),
    **{f"null-{name}": (dict(tables=[{}, {name: None}]), "sections[1]: NULL buffer") for name in T},
    "rows-8": (dict(rows=0x10008), "rows and out_shards must be 16-byte aligned"),
    "out-shards-8": (dict(out_shards=0x90008), "rows and out_shards must be 16-byte aligned"),
    "recovered-4": (dict(recovered=0x80004), "recovered must be 8-byte aligned"),
    "out-hdr-2": (dict(out_hdr=0xA0002), "out_hdr must be 4-byte aligned"),
    "present-4": (dict(tables=[{"present": 0x40004}, {}]), "sections[0]: present and parity_present"),
    "parity-present-4": (dict(tables=[{}, {"parity_present": 0x70004}]), "sections[1]: present and parity_present"),
    "src-of-2": (dict(tables=[{"src_of": 0x20002}, {}]), "sections[0]: src_of, hdr and meta"),
    "hdr-2": (dict(tables=[{}, {"hdr": 0x30002}]), "sections[1]: src_of, hdr and meta"),
    "meta-2": (dict(tables=[{}, {"meta": 0x50002}]), "sections[1]: src_of, hdr and meta"),
    "fec-size-1": (dict(tables=[{"fec_size": 0x60001}, {}]), "sections[0]: fec_size"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_shapes_decode_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    kw = dict(dict(groups=(4, 4)), **kw)
    r, err = _call(product, _two(oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_shapes_decode_checks_in_order(product, oracle1000):
    """Each check comes before the next: a call that breaks two is refused for the earlier one.  The order is the
    plans and n_plans, stride, capacity, per_group, groups <= cap, the lanes of a section, the launch's blocks, the
    NULL pointers, the alignments."""
    two = _two(oracle1000)
    bad = ic.PLANS["full3x4k10"](oracle1000)
    bad.line[2].first, bad.line[2].count = 8, 4  # members 8..11 of k = 10
    steps = [
        (dict(plans=[two[0], bad]), "beyond k"),
        (dict(plans=[two[0], ic.PLANS["strip65"](oracle1000)]), "plans[1]"),
        (dict(stride=1208), "stride"),
        (dict(capacity=1300), "capacity"),
        (dict(per_group=11), "per_group"),
        (dict(groups=(4, 5), caps=(4, 4)), "sections[p].cap"),
        (dict(groups=(4, 1 << 30), caps=(4, 1 << 30), stride=16, capacity=16, per_group=1), "header lanes"),
        (dict(rows=None), "NULL"),
        (dict(rows=0x10008), "aligned"),
    ]
    for i, (kw, msg) in enumerate(steps):
        for later, _ in steps[i + 1:]:
            both = dict(dict(groups=(4, 4)), **later)
            both.update(kw)
            plans = both.pop("plans", two)
            r, err = _call(product, plans, **both)
            assert r == -1 and msg in err, (kw, later, r, err)


def test_shapes_decode_lane_and_block_bounds(product, oracle1000):
    """One lane below a section's bound passes the value checks (then a NULL pointer is what is refused); the
    checker's and the header lanes' bounds; and the launch's blocks: sections that pass alone, too many together."""
    m, r12 = _two(oracle1000)
    r, err = _call(product, [m], groups=((1 << 22) - 1,), per_group=8, stride=1024, capacity=1024, rows=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, [m], groups=(1 << 22,), per_group=8, stride=1024, capacity=1009, rows=None)
    assert r == -1 and "groups[0]: section too large" in err and "chunks" in err, (r, err)
    r, err = _call(product, [m], groups=(1 << 30,), per_group=1, stride=16, capacity=16)
    assert r == -1 and "header lanes" in err, (r, err)
    r, err = _call(product, [r12], groups=(1 << 30,), per_group=1, stride=16, capacity=16)  # 4 lines: 4 lanes
    assert r == -1 and "header lanes" in err, (r, err)
    r, err = _call(product, [m], groups=((1 << 30) - 1,), per_group=1, stride=16, capacity=16, rows=None)
    assert r == -1 and "NULL" in err, (r, err)
    # 2^22 - 1 groups x 8 slots x 64 chunks: 2^23 blocks a section, 256 sections' worth make 2^31 -- 32 cannot;
    # the output rows can: 32 sections of 2^27 groups at one lane each are 2^32 rows
    r, err = _call(product, [m] * 32, groups=((1 << 27),) * 32, per_group=1, stride=16, capacity=16, rows=None)
    assert r == -1 and "window too large" in err, (r, err)
    r, err = _call(product, [m] * 31, groups=((1 << 27),) * 31, per_group=1, stride=16, capacity=16, rows=None)
    assert r == -1 and "NULL" in err, (r, err)


REFUSED = {
    "strip65": lambda o: ic.PLANS["strip65"](o),
    "hand6": lambda o: ic.PLANS["hand6"](o),
    "k1": lambda o: ic.PLANS["k1"](o),
    "rows10x5": lambda o: o.plan_matrix(10, 2, 5, rc.ROWS),  # a row layout of 5 columns
}
ACCEPTED_ROWS = ("rows32x4", "rows12x3", "rows10x4", "k2")


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_shapes_decode_refuses_other_plans_with_groups_only(product, oracle1000, name):
    """A plan that is neither a full matrix of k = 6..16 nor a row layout of rows of <= 4 with k <= 64 is RFEC_EINVAL
    where its section has groups -- the error names the plan's index and the call that takes it -- and passes where
    it has none: that is how a caller leaves such a section to rfec_recover_indexed_out."""
    plan = REFUSED[name](oracle1000)
    assert product.packed_matrix_stride(plan, 1) == 0
    plans = [ic.PLANS["full3x4k10"](oracle1000), plan]
    r, err = _call(product, plans, groups=(4, 4), per_group=1)
    assert r == -1 and "plans[1]" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plans, groups=None, caps=(4, 4), per_group=1)  # NULL: cap
    assert r == -1 and "plans[1]" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plans, groups=(4, 0), per_group=1, tables=[{}, NULL_T], rows=None)
    assert r == -1 and "NULL buffer" in err and "sections" not in err, (r, err)  # past the plans, at rows
    r, err = _call(product, plans, groups=(0, 0), per_group=1, tables=[NULL_T, NULL_T], **{n: None for n in P})
    assert r == 0, (r, err)


@pytest.mark.parametrize("k", pc.KS)
def test_shapes_decode_accepts_every_sender_plan(product, oracle1000, k):
    plan = pc.full_plan(oracle1000, k)
    assert product.packed_matrix_stride(plan, 1) != 0
    r, err = _call(product, [plan], per_group=6, tables=[{"src_of": None}])
    assert r == -1 and "sections[0]: NULL buffer" in err, (r, err)


@pytest.mark.parametrize("name", ACCEPTED_ROWS)
def test_shapes_decode_accepts_row_layouts(product, oracle1000, name):
    plan = ic.PLANS[name](oracle1000)
    assert product.packed_matrix_stride(plan, 1) == 0
    r, err = _call(product, [plan], per_group=2, tables=[{"src_of": None}])
    assert r == -1 and "sections[0]: NULL buffer" in err, (r, err)


def test_shapes_decode_zero_groups_and_device(product, oracle1000):
    """All groups[p] == 0 touches nothing: every pointer but plans and sections may be NULL, and the value checks
    still come first.  groups NULL means cap.  An empty pool needs no rows.  Without a device a valid call fails past
    every check, at the launch."""
    two = _two(oracle1000)
    nothing = dict(tables=[NULL_T, NULL_T], **{n: None for n in P})
    r, err = _call(product, two, groups=(0, 0), caps=(4, 4), **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, two, groups=None, caps=(0, 0), **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, two, groups=(0, 0), caps=(4, 4), per_group=0, **nothing)
    assert r == -1 and "per_group" in err, (r, err)
    r, err = _call(product, two, groups=(0, 0), caps=(4, 4), per_group=200, **nothing)
    assert r == 0, (r, err)  # no section with groups: no k bounds per_group
    r, err = _call(product, two, groups=None, caps=(4, 4), **nothing)
    assert r == -1 and "NULL buffer" in err, (r, err)  # cap groups each: the pointers are wanted
    for kw in (dict(n_rows=0, rows=None), {}):
        r, err = _call(product, two, groups=(4, 4), **kw, recovered=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, two, groups=(4, 4), **kw)
            assert r == -2 and "launch" in err, (r, err)
            r, err = _call(product, two, groups=None, caps=(4, 4), **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: the window set -----------------------------------------------------------------------------------------------
def _prefilled(out, x):
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


def test_shapes_decode_windows_cover_their_conditions(oracle1000, windows):
    """With the oracle behind indexed_cases' arena (RefIndexed) every launched section of every window passes the
    comparison, and from the reference's own outputs the set as a whole holds: a recovered segment in every launched
    section; a cascade, a line refused by the header checks and an out slot left at 0xFF; a winning row above
    65,535; an empty section between two filled ones, an empty first and an empty last section; 32 sections; and
    n_plans = 1 for either kind of section.  The edge windows hold sections of 1, 255, 256 and 257 payload lanes and
    one with more checker than payload blocks, and every window has a twin in another order."""
    seen = {}
    eng = ic.RefIndexed(oracle1000)
    done = set()
    for w in rsc.WINDOWS:
        W = windows(w[0])
        assert len(W.plans) <= 32 and rsc.launched(W)
        for p in rsc.launched(W):
            x, ref = W.x[p], W.ref[p]
            assert min(x.k for x in W.x if x is not None) >= W.E
            if x.case not in done:
                done.add(x.case)
                ic.compare(eng.run(x), _prefilled(ref, x), x, f"{w[0]} section {p}")
            cond = imc.conditions(x, ref) if rsc.is_matrix(W.names[p]) else ic.conditions(x, ref)
            assert cond["recovered"], (w[0], p)
            for key, v in cond.items():
                seen[key] = seen.get(key, False) or v
            so = W.src_of[p]
            seen["joined_row_above_65535"] = seen.get("joined_row_above_65535", False) or bool((so[so != rsc.NONE] > 65535).any())
    for key in ("recovered", "cascade", "refused_line", "unrecovered_slot", "row_above_65535", "joined_row_above_65535"):
        assert seen[key], (key, seen)
    g = windows("empties").groups
    assert g[0] == 0 and g[-1] == 0 and any(g[i] == 0 and any(g[:i]) and any(g[i + 1:]) for i in range(len(g)))
    assert len(windows("thirty-two").plans) == 32 and 0 in windows("thirty-two").groups
    assert [len(windows(n).plans) for n in ("one-matrix", "one-rows")] == [1, 1]
    assert rsc.is_matrix(windows("one-matrix").names[0]) and not rsc.is_matrix(windows("one-rows").names[0])
    # the edge windows: plans, geometries, lane counts
    for geom in ("c15", "c20", "c1200"):
        a, b = windows(f"edges-{geom}"), windows(f"edges-{geom}-reordered")
        assert set(a.names) == set(rsc.EDGE_PLANS) and a.names != b.names
        assert sorted(zip(a.names, a.groups)) == sorted(zip(b.names, b.groups))
    W = windows("edges-c15")
    cd = rc.cd16(W.capacity) // 16
    lanes = {g * W.E * cd for g in W.groups}
    assert cd == 1 and {1, 255, 256, 257} <= lanes
    blocks = lambda n: (n + 255) // 256  # noqa: E731
    assert any(rsc.is_matrix(n) and blocks(4 * g) > blocks(g * W.E * cd) for n, g in zip(W.names, W.groups))
    assert any((g * W.E * cd) % 64 for g in W.groups)
    W = windows("swap")
    assert len(W.src_of[0]) == len(W.src_of[1])


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _check_window(eng, W, out, what):
    """Every launched section: the tag, the reference, and the single-shape call byte for byte."""
    live = rsc.launched(W)
    assert eng.last_path == (rsc.SHAPES | len(live) << 8), f"{what}: path {eng.last_path:#x}"
    for p in live:
        x = W.x[p]
        got, single = out[p]
        assert eng.single_paths[p] == rsc.single_tag(x), f"{what} section {p}: path {eng.single_paths[p]:#x}"
        ic.compare(got, W.ref[p], x, f"{NAME} {what} section {p} ({W.names[p]} x {W.groups[p]})")
        ic.compare(got, single, x, f"{NAME} {what} section {p} against its single-shape call")


@pytest.mark.gpu
@pytest.mark.parametrize("w", rsc.WINDOWS, ids=rsc.window_id)
def test_shapes_decode_gpu(gpu_lib, windows, w):
    """The product == the reference in every launched section: recovered, out_index, out_hdr, out_shards over
    [0, 16 CD) of the recovered slots; the out slots' tails, the guards and every input as before the call; the
    same four outputs byte for byte against the section's single-shape call on the same arena; one launch."""
    W = windows(w[0])
    eng = rsc.GpuShapesDecode(gpu_lib)
    gpu_lib.lib.rfec_timing_events(None, None)
    out = eng.run(W, singles=False)
    assert gpu_lib.lib.rfec_timing_launches() == 1
    out = eng.run(W)
    _check_window(eng, W, out, w[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges-c20", "empties", "one-rows"])
def test_shapes_decode_null_groups_gpu(gpu_lib, windows, name):
    """groups NULL: every section's cap, here its groups -- the same outputs."""
    W = windows(name)
    eng = rsc.GpuShapesDecode(gpu_lib)
    _check_window(eng, W, eng.run(W, pass_groups=False), f"{name} groups NULL")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_shapes_decode_erasure_patterns_gpu(gpu_lib, oracle1000, variant):
    """Every erasure pattern of the eleven matrix sweeps of k = 6..16, the sweeps the sections of one call, at
    per_group 1, 4 and 6: masks, out_index, header records and slots of every section equal the expected ones
    (clean: the model's mask and the original group; tampered: the oracle's), the tails hold the pre-fill."""
    ks = list(pc.KS)
    sweeps = [pc.sweep(oracle1000, k, "s16", variant) for k in ks]
    for E in (1, 4, 6):
        W = rsc.pattern_window(sweeps, E)
        eng = rsc.GpuShapesDecode(gpu_lib)
        out = eng.run(W, singles=False)
        assert eng.last_path == (rsc.SHAPES | len(ks) << 8), hex(eng.last_path)
        for p, sw in enumerate(sweeps):
            pc.check_dense(sw, out[p][0], E, f"{sw.name()} section {p} of {NAME}", fill=ic.FILL)


@pytest.mark.gpu
def test_shapes_decode_empty_pool_gpu(gpu_lib, oracle1000):
    """n_rows == 0 with rows NULL and all-absent tables, a matrix and a row-layout section: recovered is 0, every
    out_index 0xFF, no out slot byte is written and the guards are intact (the arena's check)."""
    W = rsc.empty_pool_window(oracle1000)
    eng = rsc.GpuShapesDecode(gpu_lib)
    out = eng.run(W, singles=False)
    assert eng.last_path == (rsc.SHAPES | 2 << 8)
    for p in (0, 1):
        sh, hd, ix, rec = out[p][0]
        assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all(), p


@pytest.mark.gpu
def test_shapes_decode_gpu_checks_can_fail(gpu_lib, windows):
    """Two sections' src_of pointers swapped in the window call: the comparison fails (the maps have as many words,
    and every entry stays a valid row)."""
    W = windows("swap")
    eng = rsc.GpuShapesDecode(gpu_lib)
    out = eng.run(W, swap=(0, 1), singles=False)
    for p in (0, 1):
        with pytest.raises(AssertionError):
            ic.compare(out[p][0], W.ref[p], W.x[p], "swapped src_of pointers")


@pytest.mark.gpu
def test_shapes_decode_chain_composed_gpu(gpu_lib, oracle1000):
    """24 groups of three plans at c20 from fec_id 65520 (the window crosses 65535 -> 1), two segments lost per
    group, the arrival order shuffled: one rfec_wire_regroup_shapes, then one rfec_recover_indexed_shapes_out with
    groups NULL (every section's cap: the trailing rows decode to nothing) and one with groups = min(counts, cap) ==
    oracle.recover_batch_out on each plan's sender batch with the same losses, mapped through group_of."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0 = 24, 2, 65520
    capacity, stride = sc.GEOMS["c20"]
    plans = [sc.PLANS[name](oracle) for name in sc.PLANSETS["decode3"]]
    P = len(plans)
    rng = np.random.default_rng(zlib.crc32(b"recover-shapes-composed"))
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
    assert int(fec_id0) + G > 65535  # the window crosses 65535 -> 1
    cw = rc.cd16(capacity)
    for groups in (None, [min(int(c), G) for c in counts]):
        rows_of = [G] * P if groups is None else groups
        first = np.concatenate([[0], np.cumsum(rows_of)]).astype(int)
        total = int(first[-1])
        rec_, osh, ohd, oix = zeros(total * 16, 0xEE), zeros(total * E * stride, 0x3C), zeros(total * E * 20, 0x3C), \
            zeros(total * E, 0x3C)
        lib.recover_indexed_shapes_out(plans, sections, groups, stride, capacity, d_rows.data_ptr(), N,
                                       rec_.data_ptr(), E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), st)
        assert int(lib.lib.rfec_indexed_last_path()) == (rsc.SHAPES | P << 8)
        torch.cuda.synchronize(dev)
        a_ix, a_rec = down(oix, np.uint8, (total, E)), down(rec_, np.uint64, (total, 2))
        a_hd, a_sh = down(ohd, rc.po.HDR_DTYPE, (total, E)), down(osh, np.uint8, (total, E, stride))
        assert (a_sh[:, :, cw:] == 0x3C).all()
        recovered = 0
        for p in range(P):
            gs, (e_sh, e_hd, e_ix, e_rec) = exp[p]
            c = int(counts[p])
            group_of = down(tab[p]["group_of"], np.uint32, (G,))
            j_of = np.searchsorted(gs, group_of[:c])
            assert np.array_equal(gs[j_of], group_of[:c]) and (group_of[c:] == sc.NONE).all()
            a, b = int(first[p]), int(first[p + 1])
            g_ix, g_rec, g_hd, g_sh = a_ix[a:b], a_rec[a:b], a_hd[a:b], a_sh[a:b]
            assert np.array_equal(g_ix[:c], e_ix[j_of]) and np.array_equal(g_rec[:c], e_rec[j_of]), (p, groups)
            ok = e_ix[j_of] != 0xFF
            assert np.array_equal(g_hd[:c][ok], e_hd[j_of][ok]), (p, groups)
            assert np.array_equal(g_sh[:c][ok][:, :cw], e_sh[j_of][ok][:, :cw]), (p, groups)
            assert (g_ix[c:] == 0xFF).all() and not g_rec[c:].any(), (p, groups)  # the trailing rows: nothing
            recovered += int(ok.sum())
        assert recovered >= G // 2, recovered
