"""rfec_wire_window_census (the shapes of a parsed window, in window order, and
the groups of each, on the device) and rfec_plan_from_key (the plan a receiver
takes for a SIM_FEC's key).  On the CPU: the declarations, the argument checks
without a device, the helper against the planner, the kernels' line rule
against the helper's plans, the rule (census_cases.census_ref) against
shapes_cases.regroup_shapes_ref through the header's "Equivalence", and its
bent forms.  On the GPU: the call against the rule byte for byte in guarded
arenas, the equivalence against the product's own rfec_wire_regroup_shapes, and
the receive chain run from the census alone."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import census_cases as cc
import deliver_cases as dc
import regroup_cases as rc
import shapes_cases as sc
import window_each_cases as we

CASES = cc.make_cases()
BY_NAME = {x.name: x for x in CASES}
assert len(BY_NAME) == len(CASES)


@pytest.fixture(scope="module")
def refs(oracle1000):
    """Every case's census by the rule, computed once and left unchanged."""
    return {x.name: cc.census_ref(oracle1000, x.G, x.fec_id0, x.recs, x.capacity) for x in CASES}


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_census_calls_are_declared_and_bound(product, product1200):
    from razor_amd import fec
    for name in ("rfec_wire_window_census", "rfec_plan_from_key"):
        assert name in fec.header_functions() and name in fec._SIGS
        for lib in (product, product1200):
            assert hasattr(lib.lib, name)
    for lib in (product, product1200):
        assert all(hasattr(lib, m) for m in ("wire_window_census", "plan_from_key", "plans_from_census",
                                             "census_lines_of_key", "census_last_path"))
        assert lib.lib.rfec_abi_version() == 7
        assert lib.census_tile() == fec.CENSUS_TILE == cc.TILE
    assert fec.RFEC_ABI_VERSION == 7 and fec.RFEC_CENSUS_MAX_SHAPES == cc.MAX_SHAPES
    for internal in ("rfec_census_lines_of_key", "rfec_census_last_path", "rfec_census_tile"):
        assert internal not in fec.header_functions() and hasattr(product.lib, internal)
    header = fec.HEADER.read_text()
    assert "#define RFEC_CENSUS_MAX_SHAPES 32" in header and "#define RFEC_ABI_VERSION 7" in header
    assert C.sizeof(fec.rfec_window_census) == 576 == cc.CENSUS.itemsize == fec.WINDOW_CENSUS_DTYPE.itemsize
    assert [(n, fec.WINDOW_CENSUS_DTYPE.fields[n][1]) for n in fec.WINDOW_CENSUS_DTYPE.names] == \
        [(n, cc.CENSUS.fields[n][1]) for n in cc.CENSUS.names]
    assert fec.rfec_window_census.shape.offset == 64 and fec.rfec_census_shape.first_g.offset == 8


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
PTRS = dict(recs=0x10010, census=0x20010, anchor_of=0x30004, key_of=0x40004)


def _call(product, groups=4, fec_id0=7, n=100, capacity=1200, **ptrs):
    w = dict(PTRS, **ptrs)
    r = product.lib.rfec_wire_window_census(groups, fec_id0, n, w["recs"], capacity, w["census"], w["anchor_of"],
                                            w["key_of"], None)
    return r, product.lib.rfec_last_error().decode()


# every check in the call's order: (arguments, what the message names)
CHECKS = [
    (dict(fec_id0=0), "fec_id0"),
    (dict(groups=65536), "groups"),
    (dict(n=0x80000000), "n must be"),
    (dict(capacity=65536), "capacity"),
    (dict(recs=None), "recs is NULL"),
    (dict(census=None), "census is NULL"),
    (dict(anchor_of=None), "anchor_of is NULL"),
    (dict(key_of=None), "key_of is NULL"),
    (dict(recs=PTRS["recs"] + 8), "recs must be 16"),
    (dict(census=PTRS["census"] + 8), "census must be 16"),
    (dict(anchor_of=PTRS["anchor_of"] + 2), "anchor_of must be 4"),
    (dict(key_of=PTRS["key_of"] + 1), "key_of must be 4"),
]


@pytest.mark.parametrize("i", range(len(CHECKS)), ids=[m.split()[0] + f"-{i}" for i, (_, m) in enumerate(CHECKS)])
def test_census_rejects_in_order(product, i):
    """Each check alone, and with every later check failing as well: the earliest one is reported."""
    kw, msg = CHECKS[i]
    r, err = _call(product, **kw)
    assert r == -1 and msg in err, (r, err)
    later = {}
    for k2, _ in CHECKS[i + 1:]:
        for name, v in k2.items():
            later.setdefault(name, v)
    r, err = _call(product, **dict(later, **kw))
    assert r == -1 and msg in err, (r, err)


def test_census_zero_groups_optional_pointers_and_device(product):
    """groups == 0 touches nothing: every pointer may be NULL; the value checks still come first.  n == 0 needs no
    recs.  Without a device a valid call fails past every check, at the launch (RFEC_EDEVICE)."""
    nothing = {name: None for name in PTRS}
    assert _call(product, groups=0, **nothing)[0] == 0
    assert _call(product, groups=0, n=0, **nothing)[0] == 0
    r, err = _call(product, groups=0, fec_id0=0, **nothing)
    assert r == -1 and "fec_id0" in err
    r, err = _call(product, groups=0, capacity=65536, **nothing)
    assert r == -1 and "capacity" in err
    for kw in (dict(n=0, recs=None), dict(groups=65535, capacity=65535, n=0x7FFFFFFF), {}):
        r, err = _call(product, **dict(kw, key_of=None))
        assert r == -1 and "key_of" in err, (r, err)  # past the value checks and the optional pointer
    if not torch.cuda.is_available():
        for kw in (dict(n=0, recs=None), {}):
            r, err = _call(product, **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: rfec_plan_from_key against the planner -------------------------------------------------------------------------------
def _family(product):
    f = product.lib.rfec_recover_window_family
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    return lambda plan: f(C.addressof(plan))


def test_plan_from_key_against_the_planner(product):
    """For every k = 1..128 and pf = 1..255 whose planner plan has lines: the helper's plan for that plan's (k, row,
    col) holds every planner line at the same index, equals the planner's lines unless the key is the matrix key, and
    is one of the window decode's families."""
    family = _family(product)
    seen, with_lines, matrix_keys = {}, 0, 0
    for k in range(1, 129):
        _, mrow, mcol = product.num_packets(k, 255)
        for pf in range(1, 256):
            rcm, row, col = product.num_packets(k, pf)
            if (k, row, col, rcm) in seen:
                continue
            seen[(k, row, col, rcm)] = pf
            P = product.plan_from_fraction(k, pf)
            if not P.n_lines:
                continue
            with_lines += 1
            H = product.plan_from_key(P.k, P.row, P.col)
            assert (H.k, H.row, H.col) == (P.k, P.row, P.col)
            assert H.lines()[:P.n_lines] == P.lines(), (k, pf)
            is_matrix = k >= 6 and (row, col) == (mrow, mcol)
            matrix_keys += is_matrix
            if not is_matrix:
                assert H.lines() == P.lines() and H.n_row_lines == P.n_row_lines, (k, pf)
            else:
                assert H.lines() == product.plan_from_fraction(k, 255).lines(), (k, pf)
            assert family(H) != 0, (k, pf, H)
    assert with_lines > 300 and matrix_keys >= 123


@pytest.mark.parametrize("key", [(0, 1, 2), (129, 1, 129), (5, 0, 5), (5, 5, 0), (5, 5, 1), (13, 3, 4), (13, 4, 3)],
                         ids=str)
def test_plan_from_key_rejects(product, key):
    from razor_amd import fec
    p = fec.rfec_plan()
    assert key[1] * key[2] < key[0] or key[0] in (0, 129) or key[2] < 2
    assert product.lib.rfec_plan_from_key(*key, C.byref(p)) == -1
    assert "plannable" in product.lib.rfec_last_error().decode()
    with pytest.raises(fec.RfecError):
        product.plan_from_key(*key)


def test_plan_from_key_edges(product):
    from razor_amd import fec
    assert product.lib.rfec_plan_from_key(5, 1, 5, None) == -1 and "NULL" in product.lib.rfec_last_error().decode()
    p = product.plan_from_key(1, 1, 2)  # plannable, and no line: RFEC_OK with n_lines == 0
    assert (p.k, p.row, p.col, p.n_lines) == (1, 1, 2, 0)
    p = product.plan_from_key(12, 3, 4)  # row * col == count, the matrix key of 12
    assert p.n_lines == 7 and p.n_row_lines == 3
    p = product.plan_from_key(12, 4, 3)  # the same count, another key: rows only
    assert p.n_lines == p.n_row_lines == 4
    p = product.plan_from_key(128, 255, 2)  # the rows that reach below k: 64 lines
    assert p.n_lines == 64 == fec.RFEC_MAX_LINES and p.line[63].first == 126


# -- CPU: the kernels' line rule against the helper's plans -------------------------------------------------------------
ROWS_SWEPT = list(range(45)) + [63, 64, 65, 127, 128, 255]
COLS_SWEPT = list(range(22)) + [63, 64, 65, 127, 128, 129, 255]


def test_census_lines_of_key_against_the_plans(product):
    """rfec_census_lines_of_key (rfec_census_rules.h as the kernels apply it) == the first line with each index in
    rfec_plan_from_key's plan, for all 256 indices of every swept key; an unplannable key has no lines."""
    from razor_amd import fec
    lines_of = product.lib.rfec_census_lines_of_key
    lines_of.restype, lines_of.argtypes = None, [C.c_uint16, C.c_uint8, C.c_uint8, C.c_void_p]
    from_key = product.lib.rfec_plan_from_key
    got = np.empty(256, np.uint8)
    plan = fec.rfec_plan()
    raw = np.frombuffer(plan, np.uint8)  # the struct's bytes: line l's index at 8 + 4 l + 3
    none = np.full(256, 0xFF, np.uint8)
    plannable = with_cols = 0
    for count in range(131):
        for row in ROWS_SWEPT:
            for col in COLS_SWEPT:
                lines_of(count, row, col, got.ctypes.data)
                ok = cc.plannable(count, row, col)
                rcode = from_key(count, row, col, C.byref(plan))
                assert rcode == (0 if ok else -1), (count, row, col)
                if not ok:
                    assert np.array_equal(got, none), (count, row, col)
                    continue
                plannable += 1
                n = int(raw[5])
                exp = none.copy()
                exp[raw[11:11 + 4 * n:4][::-1]] = np.arange(n - 1, -1, -1, dtype=np.uint8)  # the first line stays
                assert np.array_equal(got, exp), (count, row, col)
                with_cols += n > int(raw[6])
    assert plannable > 50000 and with_cols >= 100


# -- CPU: the rule ------------------------------------------------------------------------------------------------------
def _regroup_rule(G, fec_id0, recs, capacity):
    def run(plans, caps):
        return sc.regroup_shapes_ref(plans, caps, G, fec_id0, recs, capacity,
                                     sc.new_outputs(plans, caps, G, len(recs)))
    return run


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_census_rule_equivalence(oracle1000, refs, name):
    """The header's "Equivalence", rule against rule, on every window of the case set with other_groups == 0, the
    plans in window order and reversed."""
    x, ref = BY_NAME[name], refs[name]
    c = ref["census"][0]
    assert c["anchored"] == (ref["anchor_of"] != cc.NONE).sum() == sum(s[3] for s in cc.shapes_of_census(ref["census"])) \
        + c["other_groups"]
    if c["other_groups"]:
        assert c["n_shapes"] == 32 and name in ("shapes-33", "shapes-34")
        return
    run = _regroup_rule(x.G, x.fec_id0, x.recs, x.capacity)
    cc.check_equivalence(oracle1000, x, ref, run, name)
    n = int(c["n_shapes"])
    if 2 <= n and x.G <= 4096:
        cc.check_equivalence(oracle1000, x, ref, run, name + " reversed", order=list(range(n))[::-1])


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_census_rule_equivalence_on_shapes_cases(oracle1000, c):
    """The same on the windows rfec_wire_regroup_shapes is tested with (their records; the plans are the census's)."""
    x = sc.make_inputs(oracle1000, c)
    y = cc.Inputs()
    y.name, y.G, y.fec_id0, y.capacity, y.recs, y.n = sc.case_id(c), x.G, x.fec_id0, x.capacity, x.recs, x.n
    ref = cc.census_ref(oracle1000, y.G, y.fec_id0, y.recs, y.capacity)
    assert ref["census"][0]["other_groups"] == 0
    cc.check_equivalence(oracle1000, y, ref, _regroup_rule(y.G, y.fec_id0, y.recs, y.capacity), y.name)


def test_census_rule_on_the_capability_window(oracle1000, product):
    """window_each_cases' capability window (the only window of that module made of records; its others are tables
    behind the regroup): the census lists its two shapes in window order with the stream's group
    counts, the plans from it are the sender's, and the equivalence holds."""
    cap = we.capability_stream(oracle1000)
    ref = cc.census_ref(oracle1000, cap.G, cap.fec_id0, cap.recs, cap.capacity)
    c = ref["census"][0]
    counts = [int((cap.shape == p).sum()) for p in range(2)]
    assert cc.shapes_of_census(ref["census"]) == [(3, 1, 3, counts[0], 0), (100, 10, 10, counts[1], 1)]
    assert (c["g_first"], c["g_end"], c["n_refused"], c["n_notfec"], c["n_window"]) == (0, cap.G, 0, 0, 0)
    assert c["n_seg"] + c["n_fec"] == len(cap.recs)
    plans, groups = product.plans_from_census(ref["census"].tobytes())
    assert groups == counts and [p.lines() for p in plans] == [p.lines() for p in cap.plans]
    y = cc.Inputs()
    y.name, y.G, y.fec_id0, y.capacity, y.recs, y.n = "capability", cap.G, cap.fec_id0, cap.capacity, cap.recs, len(cap.recs)
    cc.check_equivalence(oracle1000, y, ref, _regroup_rule(cap.G, cap.fec_id0, cap.recs, cap.capacity), "capability")


def test_census_cases_cover_their_conditions(refs):
    seen = {}
    for x in CASES:
        for k, v in cc.conditions(x, refs[x.name]).items():
            seen[k] = max(seen.get(k, 0), v)
    assert all(seen.values()), seen
    T = cc.TILE
    assert {x.G for x in CASES} >= {1, T - 1, T, T + 1, 2 * T + 1, 65535}
    assert [int(refs[f"shapes-{S}"]["census"][0]["n_shapes"]) for S in (31, 32, 33, 34)] == [31, 32, 32, 32]
    assert [int(refs[f"shapes-{S}"]["census"][0]["other_groups"]) for S in (31, 32, 33, 34)] == [0, 0, 4, 5]
    full = refs["size-G65535"]
    assert 100 <= BY_NAME["size-G65535"].n <= 400 and full["census"][0]["n_shapes"] == 6
    assert [s[4] for s in cc.shapes_of_census(full["census"])][-2:] == [63 * T + 1, 65534]
    two = cc.shapes_of_census(refs["two-new-keys"]["census"])
    assert [s[:3] for s in two] == [cc.M10, cc.strip(6), cc.strip(4), cc.strip(8)]  # B before A: window order
    a_of = refs["two-new-keys"]["anchor_of"]
    assert a_of[T + 69] < a_of[T + 10]                                             # A's parity arrived first
    assert cc.shapes_of_census(refs["second-tile"]["census"])[1] == (7, 1, 7, 3, T + 5)
    r = refs["rules"]
    assert r["key_of"][0] == (3 | 1 << 8 | 3 << 16) and r["anchor_of"][0] == 1     # the refused parity came first
    assert (r["anchor_of"][[2, 3, 4, 6]] == cc.NONE).all() and r["anchor_of"][5] != cc.NONE
    assert r["census"][0]["g_first"] == 0 and r["census"][0]["g_end"] == 12
    assert refs["segments-only"]["census"][0]["n_shapes"] == 0 and refs["segments-only"]["census"][0]["g_first"] == 2
    e = refs["no-records"]["census"][0]
    assert e["g_first"] == cc.NONE and not e["g_end"] and (refs["no-records"]["key_of"] == cc.NONE).all()


@pytest.mark.parametrize("wrong", cc.WRONG)
def test_census_cases_catch_each_bent_rule(oracle1000, refs, wrong):
    caught = []
    for x in CASES:
        try:
            cc.compare(cc.census_ref(oracle1000, x.G, x.fec_id0, x.recs, x.capacity, (wrong,)), refs[x.name], wrong)
        except AssertionError:
            caught.append(x.name)
    assert caught, wrong


def test_census_arena_checks_can_fail(oracle1000, refs):
    """The rule behind the arena equals the rule; with two shape[] entries swapped after the call the comparison
    fails."""
    x = BY_NAME["two-new-keys"]
    eng = cc.RefCensus(oracle1000)
    cc.compare(eng.run(x), refs[x.name], "the rule in an arena")
    eng.mutate = cc.swap_two_shapes
    with pytest.raises(AssertionError, match="census"):
        cc.compare(eng.run(x), refs[x.name], "swapped shape entries")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _tag(x):
    return (4 if x.n else 3) | -(-x.G // cc.TILE) << 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_wire_window_census_gpu(gpu_lib, refs, name):
    """The census's 576 bytes, anchor_of and key_of == census_ref's, byte for byte over the pre-fill; the guards whole
    and recs unchanged; four launches (three with n == 0) and the tag."""
    x = BY_NAME[name]
    gpu_lib.timing_events(None, None)
    eng = cc.GpuCensus(gpu_lib)
    got = eng.run(x)
    assert gpu_lib.timing_launches() == (4 if x.n else 3)
    assert eng.last_path == _tag(x), hex(eng.last_path)
    cc.compare(got, refs[name], f"rfec_wire_window_census {name}")


@pytest.mark.gpu
def test_wire_window_census_zero_groups_gpu(gpu_lib):
    """groups == 0: no launch, and no byte of the three outputs is written."""
    x = BY_NAME["rules"]
    gpu_lib.timing_events(None, None)
    got = cc.GpuCensus(gpu_lib).run(x, groups=0)
    assert gpu_lib.timing_launches() == 0
    assert all((got[name].view(np.uint8) == cc.FILL).all() for name in ("census", "anchor_of", "key_of"))


@pytest.mark.gpu
def test_wire_window_census_gpu_checks_can_fail(gpu_lib, refs):
    x = BY_NAME["two-new-keys"]
    eng = cc.GpuCensus(gpu_lib)
    eng.mutate = cc.swap_two_shapes
    with pytest.raises(AssertionError, match="census"):
        cc.compare(eng.run(x), refs[x.name], "swapped shape entries")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rules", "shapes-32", "size-G2049", "size-G65535", "second-tile"])
def test_wire_window_census_equivalence_gpu(gpu_lib, oracle1000, name):
    """Product against product: the census, plans_from_census of its bytes, then rfec_wire_regroup_shapes with
    cap = shape[p].groups on the same records -- counts equals the census's, anchor_of is byte for byte equal,
    shape_of is the index map of key_of and no record gets EFULL."""
    x = BY_NAME[name]
    cen = cc.GpuCensus(gpu_lib).run(x)
    plans, groups = gpu_lib.plans_from_census(cen["census"].tobytes())
    assert groups == [s[3] for s in cc.shapes_of_census(cen["census"])] and len(plans) >= 2

    def regroup(ref_plans, caps):
        assert caps == groups and [p.lines() for p in ref_plans] == [p.lines() for p in plans]
        y = sc.Inputs()
        y.case = ("census", name, x.G, x.fec_id0, "exact", "census")
        y.plans, y.P, y.caps, y.G, y.n, y.recs = plans, len(plans), caps, x.G, x.n, x.recs
        y.fec_id0, y.capacity = x.fec_id0, x.capacity
        return sc.GpuShapes(gpu_lib).run(y)

    cc.check_equivalence(oracle1000, x, cen, regroup, f"{name} on the device")


@pytest.fixture(scope="module")
def capability(oracle1000):
    return we.capability_stream(oracle1000)


@pytest.mark.gpu
def test_census_chain_composed_gpu(gpu_lib, capability):
    """window_each_cases' capability window as datagrams: rfec_wire_parse, rfec_wire_window_census, ONE copy of the
    576-byte struct to the host, the plans and the sections (cap = groups = the census's counts) from it alone,
    rfec_wire_regroup_shapes, ONE rfec_recover_indexed_window_each_out and rfec_recover_deliver_each.  The list is
    entry for entry what the chain of test_window_each_chain_composed_gpu gives with the sender's plans known ahead,
    sections of cap = G and the stream's counts."""
    lib, cap = gpu_lib, capability
    G, fec_id0, capacity, stride = cap.G, cap.fec_id0, cap.capacity, cap.stride
    N, ds, max_out = len(cap.dgram), cap.dgram.shape[1], 64
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    def down(t, dtype, shp):
        nb = int(np.prod(shp)) * np.dtype(dtype).itemsize
        return t[:nb].cpu().numpy().view(dtype).reshape(shp)

    d_dg, d_dl = up(cap.dgram), up(cap.dlen)
    recs, rows = zeros(N * 64, sc.FILL), zeros(N * stride, sc.FILL)
    lib.wire_parse(N, ds, d_dg.data_ptr(), d_dl.data_ptr(), stride, capacity, recs.data_ptr(), rows.data_ptr(), st)

    def rest_of_chain(plans, caps, groups, Es):
        NP = len(plans)
        w, secs = sc.shapes_of(plans, caps, G, N)
        win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
        tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
               for s in secs]
        sections = [dict(cap=caps[p], **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(NP)]
        first, slot_first = we.first_slots(groups, Es)
        R, S = int(first[-1]), int(slot_first[-1])
        o = dict(rec=zeros(R * 16, 0xEE), osh=zeros(S * stride, 0x3C), ohd=zeros(S * 20, 0x3C), oix=zeros(S, 0x3C),
                 seg=zeros(max_out * 24, dc.FILL), segp=zeros(max_out * stride, dc.FILL),
                 first_of=zeros((G + 1) * 4, dc.FILL), n_out=zeros(4, dc.FILL),
                 ws=zeros(lib.recover_deliver_workspace_size(G), 0x11))
        lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, recs.data_ptr(), capacity,
                                *(win[name].data_ptr() for name in sc.WINDOW), st)
        lib.recover_indexed_window_each_out(plans, sections, groups, stride, capacity, rows.data_ptr(), N,
                                            o["rec"].data_ptr(), Es, o["osh"].data_ptr(), o["ohd"].data_ptr(),
                                            o["oix"].data_ptr(), st)
        assert int(lib.lib.rfec_indexed_last_path()) == (we.WINDOW_EACH_TAG | NP << 8)
        lib.recover_deliver_each(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(),
                                 win["rank_of"].data_ptr(), stride, capacity, Es, o["osh"].data_ptr(),
                                 o["ohd"].data_ptr(), o["oix"].data_ptr(), max_out, o["seg"].data_ptr(),
                                 o["segp"].data_ptr(), o["first_of"].data_ptr(), o["n_out"].data_ptr(),
                                 o["ws"].data_ptr(), st)
        torch.cuda.synchronize(dev)
        assert not (down(win["slot_of"], np.int32, (N,)) == sc.EFULL).any()
        return {"seg": down(o["seg"], rc.po.RX_SEG, (max_out,)), "seg_payload": down(o["segp"], np.uint8, (max_out, stride)),
                "first_of": down(o["first_of"], np.uint32, (G + 1,)), "n_out": down(o["n_out"], np.uint32, (1,)),
                "counts": down(win["counts"], np.uint32, (NP,))}

    # the census, and the one read-back
    d_cen, d_anchor, d_key = zeros(576, sc.FILL), zeros(G * 4, sc.FILL), zeros(G * 4, sc.FILL)
    lib.wire_window_census(G, fec_id0, N, recs.data_ptr(), capacity, d_cen.data_ptr(), d_anchor.data_ptr(),
                           d_key.data_ptr(), st)
    assert lib.census_last_path() == (4 | 1 << 8)
    census_bytes = d_cen[:576].cpu().numpy().tobytes()  # synchronises the stream
    plans, groups = lib.plans_from_census(census_bytes)
    cen = np.frombuffer(census_bytes, cc.CENSUS)[0]
    assert cen["other_groups"] == 0 and cen["n_shapes"] == 2 and cen["anchored"] == G == sum(groups)
    assert (cen["g_first"], cen["g_end"], cen["n_seg"] + cen["n_fec"]) == (0, G, N)
    per_group = {3: 3, 100: 10}  # the out slots per row a caller grants a shape (the capability window's)
    got = rest_of_chain(plans, groups, groups, [per_group[p.k] for p in plans])
    assert got["counts"].tolist() == groups
    # the parent's chain: the sender's plans known ahead, sections of cap = G, the stream's counts
    counts = [int((cap.shape == p).sum()) for p in range(len(cap.plans))]
    exp = rest_of_chain(cap.plans, [G] * len(cap.plans), counts, cap.Es)
    T = int(exp["n_out"][0])
    assert 0 < T <= max_out
    for name in ("n_out", "first_of", "seg", "seg_payload"):
        assert got[name].tobytes() == exp[name].tobytes(), name
    assert T == counts[0] + 5 * counts[1]  # one member back per k = 3 group, five per k = 100 group
