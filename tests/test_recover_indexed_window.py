"""rfec_recover_indexed_window_out: the sections of a window of ANY of the
planner's shapes (rfec_wire_regroup_shapes' tables) decoded in one launch of
k_decode_window_indexed -- a full matrix of k = 6..16 as
rfec_recover_indexed_matrix_out decodes it, rows of <= 4 with k <= 64 as
rfec_recover_indexed_out does, a full matrix of k = 17..128 as
rfec_recover_indexed_matrix_wide_out does, any other row layout as
rfec_recover_indexed_rows_wide_out does.  On the CPU: the declaration and
binding, every argument check in its order, the family rule against its
statement in Python over the planner's plans, the refusals, the existing
entries' answers, the launch without a device, the window set's census against
the reference, and the self-tests that the comparison can fail.  On the GPU:
every window against the reference and, byte for byte, against the single-shape
call of each section on the same arena; the windows of
rfec_recover_indexed_shapes_out against that call; the staircases in a middle
section; the empty pool; groups NULL over caps above the rows in use; and the
composed chain from datagrams to rfec_recover_deliver's list in four calls
(window_cases.py)."""
from __future__ import annotations

import copy
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import deliver_cases as dc
import indexed_cases as ic
import matrix_wide_cases as mw
import recover_shapes_cases as rsc
import regroup_cases as rc
import rows_wide_cases as rw
import shapes_cases as sc
import test_recover_indexed_rows_wide as trw
import window_cases as wc

NAME, METHOD = "rfec_recover_indexed_window_out", "recover_indexed_window_out"
PFS = (1, 5, 9, 10, 80, 255)


@pytest.fixture(scope="module")
def windows(oracle1000):
    """Every window's inputs and reference outputs, computed once and left unchanged; windows that hold the same
    section share it."""
    sections, cache = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = wc.make_window(oracle1000, wc.WINDOW[name], sections)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def shapes_windows(oracle1000):
    sections, cache = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = wc.from_shapes_window(oracle1000, rsc.make_window(oracle1000, rsc.WINDOW[name], sections))
        return cache[name]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_window_decode_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert NAME in fec.header_functions() and NAME in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, NAME) and hasattr(lib, METHOD)
        assert hasattr(lib.lib, "rfec_recover_window_family") and hasattr(lib.lib, "rfec_recover_window_blocks")
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(rows=0x10000, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001)
T = dict(src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002, parity_present=0x70008)
NULL_T = {name: None for name in T}


def _call(product, plans, groups=(4,), caps=None, tables=None, stride=1216, capacity=1200, n_rows=100, per_group=2,
          n_plans=None, null_plans=False, null_sections=False, name=NAME, **ptrs):
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
    r = getattr(product.lib, name)(None if null_plans else pa, n if n_plans is None else n_plans,
                                   None if null_sections else sa, ga_, stride, capacity, p["rows"], n_rows,
                                   p["recovered"], per_group, p["out_shards"], p["out_hdr"], p["out_index"], None)
    return r, product.lib.rfec_last_error().decode()


def _four(o):
    """One plan of each family: k = 10, 12, 17 and 30."""
    return [ic.PLANS["full3x4k10"](o), ic.PLANS["rows12x3"](o), mw.wide_plan(o, 17), rw.rows_plan(o, 30, 30)]


def _family(product, plan):
    from razor_amd.fec import as_plan
    f = product.lib.rfec_recover_window_family
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    return int(f(C.byref(as_plan(plan))))


def _blocks(product, plan, groups, per_group, cd, n_rows):
    from razor_amd.fec import as_plan
    f = product.lib.rfec_recover_window_blocks
    f.restype, f.argtypes = C.c_uint32, [C.c_void_p] + [C.c_uint32] * 4
    return int(f(C.byref(as_plan(plan)), groups, per_group, cd, n_rows))


G4 = (4, 4, 4, 4)
# name -> (keyword arguments over one section of each family of 4 groups each, the message)
BAD_ARGS = {
    "null-plans": (dict(null_plans=True), "plans is NULL"),
    "no-plans": (dict(n_plans=0), "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]"),
    "33-plans": (dict(n_plans=33), "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]"),
    "null-sections": (dict(null_sections=True), "sections is NULL"),
    "stride-0": (dict(stride=0), "stride must be a positive multiple of 16"),
    "stride-1208": (dict(stride=1208), "stride must be a positive multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity must be <= stride"),
    "per-group-0": (dict(per_group=0), "per_group must be in [1, min k of the sections with groups]"),
    "per-group-above-min-k": (dict(per_group=11), "per_group must be in [1, min k of the sections with groups]"),
    "groups-above-cap": (dict(groups=(4, 4, 5, 4), caps=G4), "groups[2] must be <= sections[p].cap"),
    "lanes": (dict(groups=(4, 4, 1 << 22, 4), stride=1024, capacity=1024, per_group=8),
              "groups[2]: section too large for one launch (groups x per_group x chunks)"),
    "null-rows": (dict(rows=None), "NULL buffer"),
    "null-recovered": (dict(recovered=None), "NULL buffer"),
    "null-out-shards": (dict(out_shards=None), "NULL buffer"),
    "null-out-hdr": (dict(out_hdr=None), "NULL buffer"),
    "null-out-index": (dict(out_index=None), "NULL buffer"),
    **{f"null-{name}-{p}": (dict(tables=[{}] * p + [{name: None}] + [{}] * (3 - p)), f"sections[{p}]: NULL buffer")
       for name in T for p in (2, 3)},
    "rows-8": (dict(rows=0x10008), "rows and out_shards must be 16-byte aligned"),
    "out-shards-8": (dict(out_shards=0x90008), "rows and out_shards must be 16-byte aligned"),
    "recovered-4": (dict(recovered=0x80004), "recovered must be 8-byte aligned"),
    "out-hdr-2": (dict(out_hdr=0xA0002), "out_hdr must be 4-byte aligned"),
    "present-4": (dict(tables=[{}, {}, {"present": 0x40004}, {}]),
                  "sections[2]: present and parity_present must be 8-byte aligned"),
    "parity-present-4": (dict(tables=[{}, {}, {}, {"parity_present": 0x70004}]),
                         "sections[3]: present and parity_present must be 8-byte aligned"),
    "src-of-2": (dict(tables=[{}, {}, {"src_of": 0x20002}, {}]), "sections[2]: src_of, hdr and meta must be 4-byte"),
    "hdr-2": (dict(tables=[{}, {}, {}, {"hdr": 0x30002}]), "sections[3]: src_of, hdr and meta must be 4-byte"),
    "meta-2": (dict(tables=[{}, {"meta": 0x50002}, {}, {}]), "sections[1]: src_of, hdr and meta must be 4-byte"),
    "fec-size-1": (dict(tables=[{}, {}, {"fec_size": 0x60001}, {}]), "sections[2]: fec_size must be 2-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_window_decode_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    kw = dict(dict(groups=G4), **kw)
    r, err = _call(product, _four(oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_window_decode_checks_in_order(product, oracle1000):
    """Each check comes before the next: a call that breaks two is refused for the earlier one.  The order is the
    plans and n_plans, each plan and its family, stride, capacity, per_group, groups <= cap, the lanes of a section,
    the header lanes, the launch's blocks and rows, the NULL pointers, the alignments."""
    four = _four(oracle1000)
    bad = ic.PLANS["full3x4k10"](oracle1000)
    bad.line[2].first, bad.line[2].count = 8, 4  # members 8..11 of k = 10
    big = dict(stride=16, capacity=16, per_group=1)
    steps = [
        (dict(null_plans=True), "plans is NULL"),
        (dict(n_plans=33), "n_plans"),
        (dict(null_sections=True), "sections is NULL"),
        (dict(plans=[four[0], four[1], bad, four[3]]), "beyond k"),
        (dict(plans=[four[0], four[1], ic.PLANS["hand6"](oracle1000), four[3]]), "plans[2]"),
        (dict(stride=1208), "stride"),
        (dict(capacity=1300), "capacity"),
        (dict(per_group=11), "per_group"),
        (dict(groups=(4, 4, 4, 5), caps=G4), "groups[3] must be <= sections[p].cap"),
        (dict(groups=(4, 4, 4, 1 << 31), caps=(4, 4, 4, 1 << 31), **big), "groups x per_group x chunks"),
        (dict(groups=(4, 1 << 30, 4, 4), caps=(4, 1 << 30, 4, 4), **big), "header lanes"),
        (dict(rows=None), "NULL buffer"),
        (dict(tables=[{}, {}, {}, {"meta": None}]), "sections[3]: NULL buffer"),
        (dict(rows=0x10008), "rows and out_shards"),
        (dict(tables=[{}, {}, {}, {"present": 0x40004}]), "sections[3]: present"),
    ]
    for i, (kw, msg) in enumerate(steps):
        for later, _ in steps[i + 1:]:
            both = dict(dict(groups=G4), **later)
            both.update(kw)
            plans = both.pop("plans", four)
            r, err = _call(product, plans, **both)
            assert r == -1 and msg in err, (kw, later, r, err)


def test_window_decode_lane_and_block_bounds(product, oracle1000):
    """One lane below a section's bound passes the value checks (then a NULL pointer is what is refused); the header
    lanes' bound of each family -- 4 per group, 2^lg per group, and none beyond the groups' own for family 3 -- and
    the launch's blocks and rows: sections that pass alone, too many together.  rfec_recover_window_blocks is a
    multiple of 8, the grid the section's own call takes."""
    m, r12, w17, s30 = _four(oracle1000)
    one = dict(per_group=1, stride=16, capacity=16)
    for plan, lanes in ((m, 4), (r12, 4), (s30, 2), (rw.rows_plan(oracle1000, 128, 2), 64)):
        g = (1 << 32) // lanes
        if g < 1 << 31:
            r, err = _call(product, [plan], groups=(g,), **one)
            assert r == -1 and "groups[0]: section too large for one launch (groups x header lanes)" in err, (r, err)
            r, err = _call(product, [plan], groups=(g - 1,), **one, rows=None)
            assert r == -1 and "NULL buffer" in err, (plan.k, r, err)
    # family 3, one checker lane per group: 2^31 - 1 groups pass the lanes' bounds; the blocks' bound is next
    r, err = _call(product, [w17], groups=((1 << 31) - 1,), **one, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    r, err = _call(product, [w17], groups=(1 << 31,), **one)
    assert r == -1 and "groups x per_group x chunks" in err, (r, err)
    r, err = _call(product, [w17] * 32, groups=((1 << 27),) * 32, **one, rows=None)
    assert r == -1 and "window too large" in err, (r, err)
    r, err = _call(product, [w17] * 31, groups=((1 << 27),) * 31, **one, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    # blocks: rounds of 8 over the header (or checker) blocks and the payload blocks
    up8 = lambda n: -(-n // 8) * 8  # noqa: E731
    blk = lambda n: -(-n // 256)  # noqa: E731
    for plan, lanes in ((m, 4), (r12, 4), (w17, 1), (s30, 2), (rw.rows_plan(oracle1000, 128, 2), 64)):
        for g, E, cd, n_rows in ((1, 1, 1, 5), (257, 2, 1, 5), (300, 2, 75, 5), (300, 2, 75, 0), (2049, 1, 2, 9)):
            want = up8(blk(g * lanes)) + (up8(blk(g * E * cd)) if n_rows else 0)
            assert _blocks(product, plan, g, E, cd, n_rows) == want, (plan.k, g, E, cd, n_rows)
    assert _blocks(product, ic.PLANS["hand6"](oracle1000), 4, 1, 1, 5) == 0


# -- CPU: the family rule ----------------------------------------------------------------------------------------------
def test_window_family_rule_over_the_planner(product, oracle1000):
    """rfec_recover_window_family == the rule's statement in Python (window_cases.family_of) on every
    rfec_plan_from_fraction(k, pf), k = 1..128 at pf 1, 5, 9, 10, 80 and 255: every plan with lines is accepted with
    groups; k = 6..16 at pf >= 10 are family 1; a plan without lines is refused with groups and accepted with none."""
    seen = set()
    for k in range(1, 129):
        for pf in PFS:
            plan = product.plan_from_fraction(k, pf, rc.ROWS | rc.COLS)
            f = _family(product, plan)
            assert f == wc.family_of(oracle1000, plan), (k, pf, f)
            seen.add(f)
            if plan.n_lines:
                assert f in (1, 2, 3, 4), (k, pf)
                r, err = _call(product, [plan], per_group=1, tables=[{"src_of": None}])
                assert r == -1 and "sections[0]: NULL buffer" in err, (k, pf, r, err)
            else:
                assert f == 0
                r, err = _call(product, [plan], per_group=1)
                assert r == -1 and "plans[0]" in err and "rfec_recover_indexed_out" in err, (k, pf, r, err)
                r, err = _call(product, [plan], groups=(0,), per_group=1, tables=[NULL_T], **{n: None for n in P})
                assert r == 0, (k, pf, r, err)
            if 6 <= k <= 16 and pf >= 10:
                assert f == 1, (k, pf)
            if k >= 17 and pf >= 10:
                assert f == 3, (k, pf)
    assert seen == {0, 1, 2, 3, 4}
    # the GPU cases' shapes, and the compiled families first where two predicates hold
    for k, col in rw.SHAPES:
        plan = rw.rows_plan(oracle1000, k, col)
        want = 2 if col <= 4 and k <= 64 and rw.n_lines(k, col) == -(-k // col) else 4
        assert _family(product, plan) == wc.family_of(oracle1000, plan) == want, (k, col)
    for k in mw.SHAPES:
        assert _family(product, mw.wide_plan(oracle1000, k)) == 3, k


# the refused sets of the two wide entries and this module's bent row layouts, one namespace
CANDIDATES = {**mw.REFUSED, **trw.REFUSED, **wc.REFUSED}
MUST_REFUSE = ("hand6", "k10col3", "k40col6", "cols_only40", "k5", "k1", "k5pf255", "gap", "widths_5_4_5",
               "strip65_first1", "rows_of_1", "stride2", "last_row_missing", "rows_gap", "rows_unequal", "strip_from_1")


@pytest.mark.parametrize("name", sorted(CANDIDATES))
def test_window_decode_refuses_other_plans_with_groups_only(product, oracle1000, name):
    """The plans the wide entries refuse (matrix_wide_cases.REFUSED, test_recover_indexed_rows_wide.REFUSED) and
    this module's bent row layouts.  What no family takes -- hand-made plans, a full matrix in another col, columns
    only, k = 5 as a matrix, no lines, rows with a gap, unequal rows, a stride, a strip from segment 1 -- is
    RFEC_EINVAL where its section has groups (the error names the section and the call that takes the plan) and
    passes where it has none; what one entry refused because it is the other's (a row layout, a full matrix) is a
    section of this call."""
    plan = CANDIDATES[name](oracle1000)
    family = wc.family_of(oracle1000, plan)
    assert _family(product, plan) == family and (family == 0) == (name in MUST_REFUSE), (name, family)
    plans = [ic.PLANS["full3x4k10"](oracle1000), mw.wide_plan(oracle1000, 17), plan]
    if family:
        r, err = _call(product, plans, groups=(4, 4, 4), per_group=1, tables=[{}, {}, {"src_of": None}])
        assert r == -1 and "sections[2]: NULL buffer" in err, (r, err)
        return
    r, err = _call(product, plans, groups=(4, 4, 4), per_group=1)
    assert r == -1 and "plans[2]" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plans, groups=None, caps=(4, 4, 4), per_group=1)  # NULL: cap
    assert r == -1 and "plans[2]" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plans, groups=(4, 4, 0), per_group=1, tables=[{}, {}, NULL_T], rows=None)
    assert r == -1 and "NULL buffer" in err and "sections" not in err, (r, err)  # past the plans, at rows
    r, err = _call(product, plans, groups=(0, 0, 0), per_group=1, tables=[NULL_T] * 3, **{n: None for n in P})
    assert r == 0, (r, err)


def test_window_decode_takes_what_the_wide_entries_take(product, oracle1000):
    """The row layouts among matrix_wide_cases.REFUSED (rows10x4, strip65, the rows-only layer at k = 40) are
    sections of this call: families 2, 4 and 4."""
    for name, want in (("rows10x4", 2), ("strip65", 4), ("rows_only40", 4)):
        plan = mw.REFUSED[name](oracle1000)
        assert _family(product, plan) == want
        r, err = _call(product, [plan], per_group=1, tables=[{"src_of": None}])
        assert r == -1 and "sections[0]: NULL buffer" in err, (name, r, err)


def test_window_decode_existing_entries_keep_their_answers(product, oracle1000):
    """rfec_recover_indexed_shapes_out still refuses a strip plan and a k = 17 matrix with groups, with its old
    message."""
    old = "is neither the sender's full row + column plan of k = 6..16 nor a row layout of rows of <= 4 segments"
    for plan in (ic.PLANS["strip65"](oracle1000), mw.wide_plan(oracle1000, 17), rw.rows_plan(oracle1000, 5, 5)):
        r, err = _call(product, [plan], per_group=1, name="rfec_recover_indexed_shapes_out")
        assert r == -1 and "plans[0]" in err and old in err and "rfec_recover_indexed_out" in err, (r, err)


def test_window_decode_zero_groups_and_device(product, oracle1000):
    """All groups[p] == 0 touches nothing: every pointer but plans and sections may be NULL, and the value checks
    still come first.  groups NULL means cap.  An empty pool needs no rows.  Without a device a valid call fails past
    every check, at the launch."""
    four = _four(oracle1000)
    nothing = dict(tables=[NULL_T] * 4, **{n: None for n in P})
    r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, four, groups=None, caps=(0, 0, 0, 0), **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, per_group=0, **nothing)
    assert r == -1 and "per_group" in err, (r, err)
    r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, per_group=200, **nothing)
    assert r == 0, (r, err)  # no section with groups: no k bounds per_group
    r, err = _call(product, four, groups=None, caps=G4, **nothing)
    assert r == -1 and "NULL buffer" in err, (r, err)  # cap groups each: the pointers are wanted
    for kw in (dict(n_rows=0, rows=None), {}):
        r, err = _call(product, four, groups=G4, **kw, recovered=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, four, groups=G4, **kw)
            assert r == -2 and "launch" in err, (r, err)
            r, err = _call(product, four, groups=None, caps=G4, **kw)
            assert r == -2 and "launch" in err, (r, err)
            r, err = _call(product, four[2:], groups=(4, 4), per_group=17, **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: the window set -----------------------------------------------------------------------------------------------
def _prefilled(out, x):
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


def test_window_decode_windows_cover_their_conditions(oracle1000, windows):
    """From the reference alone (the exact peel held to its recovered masks on every group): every launched section
    recovers a segment (or, tampered with one group, refuses its one line); each wide matrix section holds a group whose target needs a cascade (neither its row nor
    its column fires at once) and, tampered, a group with a banned line; every family has a section at
    first[p] > 0; every tampered window has a rejected line in each family it holds; a wide section straddles mask
    bits 63 / 64; the mixed windows hold all four families in two orders with sections of 1, 255, 256 and 257
    groups at CD = 1, CD = 2 with a tail and CD = 75, per_group the least k; and with the oracle behind the arena
    (RefIndexed) a section of each family passes the comparison."""
    later, straddle, done = set(), 0, {}
    for w in wc.WINDOWS:
        W = windows(w[0])
        variant = w[3]
        assert len(W.plans) <= 32 and wc.launched(W)
        assert W.E <= min(W.x[p].k for p in wc.launched(W))
        refused = {}
        for p in wc.launched(W):
            x, ref = W.x[p], W.ref[p]
            key = id(x)
            if key not in done:
                done[key] = wc.census(x, ref)
            c = done[key]
            # (a tampered section of one group: its one firing line is the banned one)
            assert c["recovered"] or (variant == "tampered" and x.G == 1 and c["refused"]), (w[0], p)
            if x.family == 3:
                assert c["cascade"], (w[0], p, c)
                if variant == "tampered":
                    assert c["refused"], (w[0], p, c)
            if x.family in (3, 4) and x.k > 64:
                straddle += c["straddle"]
            refused[x.family] = refused.get(x.family, 0) + c["refused"]
            if W.first[p] > 0:
                later.add(x.family)
        if variant == "tampered":
            assert all(refused.values()), (w[0], refused)
    assert later == {1, 2, 3, 4} and straddle
    for geom in ("c15", "c20", "c1200"):
        for variant in ("clean", "tampered"):
            a, b = windows(f"mixed-{geom}-{variant}"), windows(f"mixed-{geom}-reordered-{variant}")
            assert sorted(x.family for x in a.x) == [1, 1, 2, 2, 3, 3, 4, 4, 4, 4] and a.E == 2
            assert a.names != b.names and sorted(zip(a.names, a.groups)) == sorted(zip(b.names, b.groups))
            assert {x.k for x in a.x} >= {2, 6, 10, 12, 17, 65, 5, 11, 128}
            # (in the reordered twin every family has a section past the first, and another family is first)
            assert a.x[0].family != b.x[0].family
    W = windows("mixed-c15-clean")
    assert rc.cd16(W.capacity) == 16 and {1, 255, 256, 257} == set(W.groups)
    assert rc.cd16(windows("mixed-c20-clean").capacity) == 32 < windows("mixed-c20-clean").stride
    assert rc.cd16(windows("mixed-c1200-clean").capacity) == 75 * 16
    W = windows("wide-only")
    assert W.E == 17 == min(x.k for x in W.x)
    W = windows("staircase")
    assert W.x[1].k == 100 and W.first[1] > 0 and W.groups[2] > 0 and wc.census(W.x[1], W.ref[1])["cascade"] >= 20
    g = windows("empties").groups
    assert g[0] == 0 and g[-1] == 0 and any(g[i] == 0 and any(g[:i]) and any(g[i + 1:]) for i in range(len(g)))
    assert all(wc.family_of(oracle1000, p) == 0 for p, n in zip(windows("empties").plans, g) if not n)
    W = windows("thirty-two")
    assert len(W.plans) == 32 and 0 in W.groups and {x.family for x in W.x if x is not None} == {1, 2, 3, 4}
    assert [windows(n).x[0].family for n in ("one-matrix", "one-rows", "one-wide-matrix", "one-wide-rows")] == [1, 2, 3, 4]
    W = windows("sparse")
    for p in (1, 2, 3):
        so = W.src_of[p]
        assert (so[so != wc.NONE] > 65535).all()
    W = windows("swap")
    assert len(W.src_of[0]) == len(W.src_of[1]) and [x.family for x in W.x] == [3, 4]
    eng = ic.RefIndexed(oracle1000)
    W = windows("mixed-c20-tampered")
    for p in (0, 1, 2, 3):
        ic.compare(eng.run(W.x[p]), _prefilled(W.ref[p], W.x[p]), W.x[p], f"section {p}")


def test_window_decode_comparison_catches_each_bent_result(oracle1000, windows):
    """Results bent on purpose fail the comparison: a section written one output row too far; two sections' src_of
    swapped; a wide section decoded at the narrow pitch (ceil(k / col) in place of NL)."""
    W = windows("swap")
    refs = [_prefilled(W.ref[p], W.x[p]) for p in (0, 1)]
    for p in (0, 1):
        ic.compare(refs[p], W.ref[p], W.x[p], "the reference itself")
    # the window's outputs, the second section written from row first[1] + 1 on
    joined = [np.concatenate([refs[0][i], refs[1][i], refs[1][i][:1]]) for i in range(4)]
    a = int(W.first[1])
    shifted = tuple(v[a + 1:a + 1 + W.groups[1]] for v in joined)
    with pytest.raises(AssertionError):
        ic.compare(shifted, W.ref[1], W.x[1], "first row + 1")
    # the maps swapped: each section decoded through the other's words, over the joined pool
    for p in (0, 1):
        y = copy.copy(W.x[p])
        y.src_of, y.rows, y.n_rows = W.src_of[1 - p], W.rows, W.n_rows
        with pytest.raises(AssertionError):
            ic.compare(_prefilled(ic.reference(oracle1000, y), y), W.ref[p], W.x[p], "swapped src_of")
    # the narrow pitch on (11, 5): rows of 5, 5 and 1, NL = 2 where ceil(k / col) = 3
    x = W.x[1]
    assert (x.k, x.col, x.nl) == (11, 5, 2)
    ic.compare(rw.model(x), refs[1], x, "the model unbent")
    with pytest.raises(AssertionError):
        ic.compare(rw.model(x, ("pitch_rows",)), refs[1], x, "the narrow pitch")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _check_window(eng, W, out, what, ref=True, tags=True):
    """Every launched section: the tag, the reference, and the single-shape call byte for byte."""
    live = wc.launched(W)
    assert eng.last_path == (wc.WINDOW_TAG | len(live) << 8), f"{what}: path {eng.last_path:#x}"
    for p in live:
        x = W.x[p]
        got, single, _ = out[p]
        if tags:
            assert eng.single_paths[p] == wc.single_tag(x), f"{what} section {p}: path {eng.single_paths[p]:#x}"
        if ref and W.ref[p] is not None:
            ic.compare(got, W.ref[p], x, f"{NAME} {what} section {p} ({W.names[p]} x {W.groups[p]})")
        ic.compare(got, single, x, f"{NAME} {what} section {p} (family {x.family}) against its single-shape call")


@pytest.mark.gpu
@pytest.mark.parametrize("w", wc.WINDOWS, ids=wc.window_id)
def test_window_decode_gpu(gpu_lib, windows, w):
    """The product == the reference in every launched section: recovered, out_index, out_hdr, out_shards over
    [0, 16 CD) of the recovered slots; the out slots' tails, the guards and every input as before the call; the
    same four outputs byte for byte against the section's single-shape call on the same arena; one launch."""
    W = windows(w[0])
    eng = wc.GpuWindowDecode(gpu_lib)
    gpu_lib.lib.rfec_timing_events(None, None)
    eng.run(W, singles=False)
    assert gpu_lib.lib.rfec_timing_launches() == 1
    out = eng.run(W)
    _check_window(eng, W, out, w[0])


@pytest.mark.gpu
@pytest.mark.parametrize("w", rsc.WINDOWS, ids=rsc.window_id)
def test_window_decode_equals_shapes_decode_gpu(gpu_lib, shapes_windows, w):
    """Every window of rfec_recover_indexed_shapes_out through the new call: byte for byte that call's outputs on
    the same arena (families 1 and 2 are unchanged), the reference, and the single-shape calls."""
    W = shapes_windows(w[0])
    eng = wc.GpuWindowDecode(gpu_lib)
    out = eng.run(W, shapes=True)
    _check_window(eng, W, out, w[0])
    assert eng.shapes_path == (rsc.SHAPES | len(wc.launched(W)) << 8)
    for p in wc.launched(W):
        got, _, theirs = out[p]
        ic.compare(got, theirs, W.x[p], f"{NAME} {w[0]} section {p} against rfec_recover_indexed_shapes_out")
        assert np.array_equal(got[3], theirs[3]) and np.array_equal(got[2], theirs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed-c20-tampered", "empties", "one-wide-rows"])
def test_window_decode_null_groups_gpu(gpu_lib, windows, name):
    """groups NULL: every section's cap, here its groups -- the same outputs."""
    W = windows(name)
    eng = wc.GpuWindowDecode(gpu_lib)
    _check_window(eng, W, eng.run(W, pass_groups=False), f"{name} groups NULL")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed-c20-reordered-tampered", "mixed-c1200-clean"])
def test_window_decode_cap_above_the_rows_in_use_gpu(gpu_lib, windows, name):
    """groups NULL with every cap three rows above the rows in use, those rows as the regroup leaves them (no
    member, no parity): the rows in use decode as before, the trailing rows to nothing -- recovered 0, every
    out_index 0xFF, no out slot byte written."""
    V = windows(name)
    W = wc.padded(V, 3)
    eng = wc.GpuWindowDecode(gpu_lib)
    out = eng.run(W, pass_groups=False)
    _check_window(eng, W, out, f"{name} padded")
    for p in wc.launched(W):
        sh, hd, ix, rec = out[p][0]
        g = V.groups[p]
        assert not rec[g:].any() and (ix[g:] == 0xFF).all() and (sh[g:] == ic.FILL).all(), p


@pytest.mark.gpu
def test_window_decode_empty_pool_and_zero_groups_gpu(gpu_lib, oracle1000):
    """n_rows == 0 with rows NULL and all-absent tables, a section of each family: recovered is 0, every out_index
    0xFF, no out slot byte is written and the guards are intact (the arena's check); the single-shape calls agree.
    All groups 0 with NULL pointers returns at once."""
    W = wc.empty_pool_window(oracle1000)
    eng = wc.GpuWindowDecode(gpu_lib)
    out = eng.run(W)
    # (rfec_recover_indexed_out picks its own kernels for an empty pool: the single calls' tags are not this test's)
    _check_window(eng, W, out, "empty pool", tags=False)
    assert [eng.single_paths[p] & 0xFF for p in (0, 2, 3)] == [3, mw.WIDE, rw.ROWS_WIDE]
    for p in range(4):
        sh, hd, ix, rec = out[p][0]
        assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all(), p
    gpu_lib.recover_indexed_window_out(W.plans, [dict(cap=0)] * 4, [0] * 4, W.stride, W.capacity, None, 0, None, 3,
                                       None, None, None, None)
    gpu_lib.recover_indexed_window_out(W.plans, [dict(cap=9)] * 4, [0] * 4, W.stride, W.capacity, None, 0, None, 3,
                                       None, None, None, None)


@pytest.mark.gpu
def test_window_decode_gpu_checks_can_fail(gpu_lib, windows):
    """Two sections' src_of pointers swapped in the window call: the comparison fails (the maps have as many words,
    and every entry stays a valid row)."""
    W = windows("swap")
    eng = wc.GpuWindowDecode(gpu_lib)
    out = eng.run(W, swap=(0, 1), singles=False)
    for p in (0, 1):
        with pytest.raises(AssertionError):
            ic.compare(out[p][0], W.ref[p], W.x[p], "swapped src_of pointers")


@pytest.mark.gpu
@pytest.mark.parametrize("null_groups", (False, True), ids=("counts", "cap"))
def test_window_decode_chain_composed_gpu(gpu_lib, oracle1000, null_groups):
    """The window of test_rows_wide_window_chain_gpu -- 60 groups from fec_id 65520 (it crosses the wrap) in runs of
    five of k = 3 in one row, k = 30 in one row and k = 40 as a 6 x 7 matrix, one segment lost in every row group and
    two in every matrix group, a parity in every third group, the datagrams shuffled -- as rfec_wire_parse, one
    rfec_wire_regroup_shapes, ONE rfec_recover_indexed_window_out and rfec_recover_deliver: four calls on one stream
    with no synchronisation in between, with groups = min(counts, cap) and with groups NULL.  All six deliver
    outputs equal deliver_ref over the oracle's decode of each run's batch with the same losses."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0, run, NP = 60, 3, 65520, 5, 3  # (per_group <= k of every section)
    capacity, stride = sc.GEOMS["c20"]
    plans = [oracle.plan_matrix(3, 1, 3, rc.ROWS), oracle.plan_matrix(30, 1, 30, rc.ROWS), mw.wide_plan(oracle, 40)]
    assert [wc.family_of(oracle, p) for p in plans] == [2, 4, 3]
    rng = np.random.default_rng(zlib.crc32(b"rows-wide-window"))
    shape = (np.arange(G) // run) % NP
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    dg_l, dl_l, exp = [], [], [[] for _ in range(NP)]
    anchored = np.zeros(G, bool)
    for g0 in range(0, G, run):
        p = int(shape[g0])
        plan = plans[p]
        k, n = plan.k, plan.n_lines
        b = rc.sender_batch(oracle, plan, run, rc.fec_id_of(fec_id0, g0), capacity, stride, rng,
                            (5000 + (g0 + np.arange(run, dtype=np.uint64)) * 140).astype(np.uint32))
        assert n and not b.status.any()
        nlost = 2 if p == 2 else 1
        lost = np.zeros(run * (k + n), bool)
        lost[(np.arange(run)[:, None] * k +
              np.stack([rng.choice(k, nlost, replace=False) for _ in range(run)])).reshape(-1)] = True
        for j in range(run):
            if (g0 + j) % 3 == 0:
                lost[run * k + j * n + int(rng.integers(0, n))] = True
        present = np.zeros((run, 2), np.uint64)
        for j, i in zip(*np.nonzero(~lost[:run * k].reshape(run, k))):
            present[j, i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        pp = np.zeros(run, np.uint64)
        for j, l in zip(*np.nonzero(~lost[run * k:].reshape(run, n))):
            pp[j] |= np.uint64(1) << np.uint64(l)
        # (a group none of whose parities arrived has no anchor: the regroup gives it no shape and no row)
        anchored[g0:g0 + run] = pp != 0
        out = oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp, capacity, E)
        exp[p].append(tuple(a[pp != 0] for a in out))
        dg_l.append(b.dgram[~lost])
        dl_l.append(b.dlen[~lost])
    ds = dg_l[0].shape[1]
    order = rng.permutation(sum(len(d) for d in dg_l))
    dgram, dlen = np.concatenate(dg_l)[order], np.concatenate(dl_l)[order].astype(np.uint16)
    N = len(dgram)
    shape = np.where(anchored, shape, sc.NOSHAPE)
    counts = [int((shape == p).sum()) for p in range(NP)]
    rank = np.full(G, sc.NONE, np.uint32)
    for p in range(NP):
        rank[shape == p] = np.arange(counts[p])

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    def down(t, dtype, shp):
        nb = int(np.prod(shp)) * np.dtype(dtype).itemsize
        return t[:nb].cpu().numpy().view(dtype).reshape(shp)

    d_dg, d_dl = up(dgram), up(dlen)
    recs, rows = zeros(N * 64, sc.FILL), zeros(N * stride, sc.FILL)
    w, secs = sc.shapes_of(plans, [G] * NP, G, N)
    win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
    tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
           for s in secs]
    sections = [dict(cap=G, **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(NP)]
    decoded = [G] * NP if null_groups else [min(c, G) for c in counts]  # rows per section
    groups = None if null_groups else decoded
    first = np.concatenate([[0], np.cumsum(decoded)]).astype(int)
    total, max_out = int(first[NP]), 256
    rec_, osh, ohd, oix = zeros(total * 16, 0xEE), zeros(total * E * stride, 0x3C), zeros(total * E * 20, 0x3C), \
        zeros(total * E, 0x3C)
    seg, segp = zeros(max_out * 24, dc.FILL), zeros(max_out * stride, dc.FILL)
    first_of, n_out = zeros((G + 1) * 4, dc.FILL), zeros(4, dc.FILL)
    ws = zeros(lib.recover_deliver_workspace_size(G), 0x11)
    # four calls, one stream, no synchronisation
    lib.wire_parse(N, ds, d_dg.data_ptr(), d_dl.data_ptr(), stride, capacity, recs.data_ptr(), rows.data_ptr(), st)
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    lib.recover_indexed_window_out(plans, sections, groups, stride, capacity, rows.data_ptr(), N, rec_.data_ptr(), E,
                                   osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), st)
    assert int(lib.lib.rfec_indexed_last_path()) == (wc.WINDOW_TAG | NP << 8)
    lib.recover_deliver(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                        stride, capacity, E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), max_out,
                        seg.data_ptr(), segp.data_ptr(), first_of.data_ptr(), n_out.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), shape)
    assert np.array_equal(down(win["rank_of"], np.uint32, (G,)), rank)
    assert np.array_equal(down(win["counts"], np.uint32, (NP,)), counts)
    # the expected dense outputs: per section the decoded rows in use, then (groups NULL) rows that decode to nothing
    e_sh, e_hd, e_ix, e_rec = [], [], [], []
    for p in range(NP):
        parts = [np.concatenate([e[i] for e in exp[p]]) for i in range(4)]
        pad = decoded[p] - counts[p]
        e_sh.append(np.concatenate([parts[0], np.full((pad, E, stride), 0x3C, np.uint8)]))
        e_hd.append(np.concatenate([parts[1], np.zeros((pad, E), rc.po.HDR_DTYPE)]))
        e_ix.append(np.concatenate([parts[2], np.full((pad, E), 0xFF, np.uint8)]))
        e_rec.append(np.concatenate([parts[3], np.zeros((pad, 2), np.uint64)]))
    e_sh, e_hd, e_ix, e_rec = (np.concatenate(v) for v in (e_sh, e_hd, e_ix, e_rec))
    assert np.array_equal(down(rec_, np.uint64, (total, 2)), e_rec)
    assert np.array_equal(down(oix, np.uint8, (total, E)), e_ix)
    group_of = []
    for p in range(NP):
        go = np.full(G, sc.NONE, np.uint32)
        go[:counts[p]] = np.nonzero(shape == p)[0]
        group_of.append(go)
    x = dc.from_tables("window-chain", plans, [G] * NP, decoded, G, fec_id0, shape, rank, group_of, capacity, stride,
                       E, e_sh, e_hd, e_ix, max_out)
    ref = dc.deliver_ref(x, dc.new_outputs(x))
    got = {"seg": down(seg, rc.po.RX_SEG, (max_out,)), "seg_payload": down(segp, np.uint8, (max_out, stride)),
           "first_of": down(first_of, np.uint32, (G + 1,)), "n_out": down(n_out, np.uint32, (1,))}
    dc.compare(got, ref, f"{NAME} window chain")
    dc.check_untouched(x, got, "window chain")
    fo = got["first_of"]
    n30 = sum(int(fo[g + 1] - fo[g]) for g in range(G) if shape[g] == 1)
    assert n30 == counts[1] and 10 <= n30 < 20 and x.T == int(got["n_out"][0])
