"""rfec_recover_indexed_rows_wide_out: the one-launch indexed decode of a row
layout of any width (k_decode_rows_wide: the shape taken at run time, masks of
two words, lines of up to 128 members) -- every strip-mode plan of the sender --
an entry point beside rfec_recover_indexed_out, rfec_recover_indexed_shapes_out
and the matrix entries, whose answers it leaves alone.  On the CPU: the
declaration and binding, the argument checks and the plan refusals without a
device, the planner's strip-mode census, the case set's census against the
reference with the two-word model of the row rule held to it on every group,
and the self-tests that the comparison catches each bent result.  On the GPU:
the shapes clean and tampered at four per_group values, the geometry cases, the
empty pool, and a mixed window from datagrams to rfec_recover_deliver's list
(rows_wide_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import deliver_cases as dc
import indexed_cases as ic
import matrix_wide_cases as mw
import regroup_cases as rc
import rows_wide_cases as rw
import shapes_cases as sc

NAME, METHOD = "rfec_recover_indexed_rows_wide_out", "recover_indexed_rows_wide_out"
CASES = [(k, col, v) for k, col in rw.SHAPES for v in rw.VARIANTS]


@pytest.fixture(scope="module")
def shape_inputs(oracle1000):
    """Every shape case's pool, map, tables and reference outputs, computed once and left unchanged."""
    cache = {}

    def get(k, col, variant, E):
        key = (k, col, variant, E)
        if key not in cache:
            x = rw.shape_case(oracle1000, k, col, variant, E)
            cache[key] = (x, ic.reference(oracle1000, x))
        return cache[key]

    return get


@pytest.fixture(scope="module")
def geometry_inputs(oracle1000):
    cache = {}

    def get(c):
        if c not in cache:
            x = rw.geometry_case(oracle1000, c)
            cache[c] = (x, ic.reference(oracle1000, x))
        return cache[c]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_rows_wide_call_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert NAME in fec.header_functions() and NAME in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, NAME) and hasattr(lib, METHOD)
    assert fec._SIGS[NAME] == fec._SIGS["rfec_recover_indexed_matrix_out"]  # the same signature
    assert fec._SIGS[NAME] == fec._SIGS["rfec_recover_indexed_matrix_wide_out"]
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(rows=0x10000, src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002,
         parity_present=0x70008, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001)
IN_ORDER = ("hdr", "present", "meta", "fec_size", "parity_present", "recovered")


def _call(product, plan, groups=4, stride=1216, capacity=1200, n_rows=100, per_group=3, name=NAME, **ptrs):
    from razor_amd.fec import as_plan
    p = dict(P, **ptrs)
    r = getattr(product.lib, name)(None if plan is None else C.byref(as_plan(plan)), groups, stride, capacity,
                                   p["rows"], n_rows, p["src_of"], *(p[n] for n in IN_ORDER), per_group,
                                   p["out_shards"], p["out_hdr"], p["out_index"], None)
    return r, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "stride-not-16": (dict(stride=1208), "stride must be a positive multiple of 16"),
    "stride-0": (dict(stride=0, capacity=0), "stride must be a positive multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity must be <= stride"),
    "per-group-0": (dict(per_group=0), "per_group must be in [1, k]"),
    "per-group-k1": (dict(per_group=101), "per_group must be in [1, k]"),
    # groups * per_group * CD = 2^31 exactly (CD = 64 at capacity 1024)
    "lanes-2g": (dict(groups=1 << 22, per_group=8, stride=1024, capacity=1024),
                 "batch too large for one launch (groups x per_group x chunks)"),
    **{f"null-{name}": ({name: None}, "NULL buffer") for name in P},
    **{f"{name}-8": ({name: P[name] + 8}, "rows and out_shards must be 16-byte aligned")
       for name in ("rows", "out_shards")},
    **{f"{name}-4": ({name: P[name] + 4}, "present, parity_present and recovered must be 8-byte aligned")
       for name in ("present", "parity_present", "recovered")},
    **{f"{name}-2": ({name: P[name] + 2}, "src_of, hdr, meta and out_hdr must be 4-byte aligned")
       for name in ("src_of", "hdr", "meta", "out_hdr")},
    "fec_size-1": (dict(fec_size=P["fec_size"] + 1), "fec_size must be 2-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_rows_wide_rejects(product, oracle1000, name):
    """Every check with rfec_recover_indexed.c's message."""
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, rw.rows_plan(oracle1000, 100, 25), **kw)
    assert r == -1 and msg in err, (r, err)


def test_rows_wide_rejects_header_lanes(product, oracle1000):
    """The "groups x lines" bound is the last check: 2^26 groups of 64 lines are 2^32 header lanes, while the payload
    lanes (2^26 x 1 x 1) pass theirs; with a misaligned fec_size as well, the error speaks of that."""
    plan = rw.rows_plan(oracle1000, 128, 2)
    kw = dict(groups=1 << 26, per_group=1, stride=16, capacity=16)
    r, err = _call(product, plan, **kw)
    assert r == -1 and "batch too large for one launch (groups x lines)" in err, (r, err)
    r, err = _call(product, plan, **kw, fec_size=P["fec_size"] + 1)
    assert r == -1 and "2-byte" in err, (r, err)
    r, err = _call(product, plan, **dict(kw, groups=(1 << 26) - 1), src_of=None)
    assert r == -1 and "NULL" in err, (r, err)


def test_rows_wide_checks_in_order(product, oracle1000):
    """rfec_recover_indexed.c's order: plan, shape, stride, capacity, per_group, the lane bound, the groups == 0
    return, NULLs, alignments (16, 8, 4, 2 bytes) -- each call breaks the named argument and every one after it, and
    the named one is what the error speaks of."""
    plan = rw.rows_plan(oracle1000, 100, 25)
    refused = oracle1000.plan_from_fraction(40, 80, 3)
    later = dict(stride=8, capacity=9999, per_group=0, groups=1 << 31, src_of=None, rows=P["rows"] + 8,
                 present=P["present"] + 4, hdr=P["hdr"] + 2, fec_size=P["fec_size"] + 1)
    order = [("plan", "plan"), ("stride", "multiple of 16"), ("capacity", "capacity must"), ("per_group", "per_group"),
             ("groups", "too large"), ("src_of", "NULL"), ("rows", "16-byte"), ("present", "8-byte"),
             ("hdr", "4-byte"), ("fec_size", "2-byte")]
    for i, (arg, msg) in enumerate(order):
        kw = {name: later[name] for name, _ in order[max(i, 1):]}
        if arg == "capacity":
            kw["stride"] = 1216
        r, err = _call(product, refused if arg == "plan" else plan, **kw)
        assert r == -1 and msg in err, (arg, r, err)
    # one lane below the bound passes the value checks; CD rounds up
    r, err = _call(product, plan, groups=(1 << 22) - 1, per_group=8, stride=1024, capacity=1024, rows=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, plan, groups=1 << 22, per_group=8, stride=1024, capacity=1009, rows=None)
    assert r == -1 and "too large" in err, (r, err)


def test_rows_wide_rejects_plan(product, oracle1000):
    r, err = _call(product, None)
    assert r == -1 and "plan is NULL" in err, (r, err)
    r, err = _call(product, rc._hand_plan(129, 1, 129, []), per_group=1)
    assert r == -1 and "out of range" in err, (r, err)
    plan = rw.rows_plan(oracle1000, 100, 25)
    plan.line[3].count = 26  # members 75..100 of k = 100
    r, err = _call(product, plan)
    assert r == -1 and "beyond k" in err, (r, err)


def _strip65_shifted(o, count):
    p = ic.PLANS["strip65"](o)
    p.line[0].first, p.line[0].count = 1, count
    return p


REFUSED = {
    "full10": lambda o: o.plan_from_fraction(10, 80, 3),
    "full40": lambda o: o.plan_from_fraction(40, 80, 3),
    "cols_only40": lambda o: o.plan_from_fraction(40, 80, rc.COLS),
    "k1": lambda o: ic.PLANS["k1"](o),
    "k5pf255": lambda o: o.plan_from_fraction(5, 255, rc.ROWS),
    "hand6": lambda o: ic.PLANS["hand6"](o),
    "gap": lambda o: rc._hand_plan(12, 2, 5, [(0, 1, 5, 0), (6, 1, 5, 1)]),
    "widths_5_4_5": lambda o: rc._hand_plan(14, 3, 5, [(0, 1, 5, 0), (5, 1, 4, 1), (9, 1, 5, 2)]),
    "strip65_first1": lambda o: _strip65_shifted(o, 64),
    "rows_of_1": lambda o: rc._hand_plan(3, 3, 1, [(0, 1, 1, 0), (1, 1, 1, 1), (2, 1, 1, 2)]),
    "stride2": lambda o: rc._hand_plan(6, 1, 3, [(0, 2, 3, 0)]),
    "last_row_missing": lambda o: rc._hand_plan(12, 3, 5, [(0, 1, 5, 0), (5, 1, 5, 1)]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_rows_wide_refuses_other_plans(product, oracle1000, name):
    """A full matrix, columns alone, a plan without lines, rows with a gap, rows of unequal width, a hand-made
    plan, a strip that starts at segment 1: RFEC_EINVAL, the error says it is the plan and names the call that takes
    it; the refusal is a value check, so it comes before groups == 0."""
    plan = REFUSED[name](oracle1000)
    if name in ("k1", "k5pf255"):
        assert plan.n_lines == 0
    r, err = _call(product, plan, per_group=1)
    assert r == -1 and "plan is not a row layout" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plan, per_group=1, groups=0, **{n: None for n in P})
    assert r == -1 and "plan" in err, (r, err)


def test_rows_wide_refuses_strip65_from_1(product, oracle1000):
    """strip65 with its line's first = 1 and all 65 members: the plan check itself refuses it (a member beyond k)."""
    r, err = _call(product, _strip65_shifted(oracle1000, 65), per_group=1)
    assert r == -1 and "plan" in err, (r, err)


def test_rows_wide_accepts_every_strip_plan(product, oracle1000):
    """Every strip-mode plan of rfec_plan_from_fraction(k, pf, ROWS), k = 1..128 and pf = 1..255, that has a line:
    304 distinct (k, col) shapes, (3, 2) and (5, 2) the two whose last row of one segment has no line; each passes
    the plan and the value checks (a NULL pointer is what is refused)."""
    shapes = {}
    for k in range(1, 129):
        for pf in range(1, 256):
            mode, row, col = oracle1000.num_packets(k, pf)
            if mode != 0:
                continue  # matrix mode
            plan = oracle1000.plan_from_fraction(k, pf, rc.ROWS)
            if not plan.n_lines:
                continue
            assert plan.line[0].count == col and (k < 6 or pf < 10), (k, pf)
            shapes.setdefault((k, col), (plan, pf))
    assert len(shapes) == 304
    short = sorted(s for s, (p, _) in shapes.items() if p.n_lines != -(-s[0] // s[1]))
    assert short == [(3, 2), (5, 2)]
    for (k, col), (plan, pf) in shapes.items():
        assert plan.n_lines == rw.n_lines(k, col)
        ours = product.plan_from_fraction(k, pf, rc.ROWS)
        assert ours.n_lines == plan.n_lines and ours.line[0].count == col
        r, err = _call(product, plan, per_group=1, src_of=None)
        assert r == -1 and "NULL" in err, (k, col, r, err)
    # the shapes rfec_recover_indexed_out itself decodes in one launch (rows of <= 4, k <= 64, every row with a line)
    assert sorted(s for s in shapes if (rw.old_tag(*s) & 0xFF) == ic.ROWS_FUSED) == [(2, 2), (3, 3), (4, 2), (4, 4),
                                                                                     (5, 3)]


def test_rows_wide_accepts_other_row_layouts(product, oracle1000):
    """rfec_plan_matrix(k, row, col, ROWS) for (128, 64, 2) and (12, 3, 5), the rows layer of the full matrix at
    k = 100, and every shape of the GPU cases."""
    plans = [oracle1000.plan_matrix(128, 64, 2, rc.ROWS), oracle1000.plan_matrix(12, 3, 5, rc.ROWS),
             oracle1000.plan_from_fraction(100, 80, rc.ROWS)]
    assert [(p.k, p.n_lines, p.line[0].count) for p in plans] == [(128, 64, 2), (12, 3, 5), (100, 10, 10)]
    plans += [rw.rows_plan(oracle1000, k, col) for k, col in rw.SHAPES]
    for p in plans:
        r, err = _call(product, p, per_group=1, src_of=None)
        assert r == -1 and "NULL" in err, (p.k, r, err)


def test_rows_wide_existing_entries_keep_their_answers(product, oracle1000):
    """rfec_recover_indexed_shapes_out still refuses a strip65 section with groups > 0; both matrix entries still
    refuse a row layout."""
    plan = ic.PLANS["strip65"](oracle1000)
    sec = dict(cap=4, **{name: P.get(name, 0x20004) for name in sc.SECTION})
    with pytest.raises(Exception) as e:
        product.recover_indexed_shapes_out([plan], [sec], [4], 1216, 1200, P["rows"], 100, P["recovered"], 1,
                                           P["out_shards"], P["out_hdr"], P["out_index"], None)
    assert "rfec_recover_indexed_out" in str(e.value)
    for name in ("rfec_recover_indexed_matrix_out", "rfec_recover_indexed_matrix_wide_out"):
        for p in (plan, rw.rows_plan(oracle1000, 100, 25), rw.rows_plan(oracle1000, 10, 4)):
            r, err = _call(product, p, per_group=1, name=name)
            assert r == -1 and "plan" in err and "rfec_recover_indexed_out" in err, (name, r, err)


def test_rows_wide_zero_groups_and_device(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL.  An empty pool needs no rows; meta and fec_size are
    never optional.  Without a device a valid call fails past every check, at the launch."""
    plan = rw.rows_plan(oracle1000, 100, 100)
    r, _ = _call(product, plan, groups=0, **{name: None for name in P})
    assert r == 0
    r, err = _call(product, plan, groups=0, per_group=101, **{name: None for name in P})
    assert r == -1 and "per_group" in err  # the value checks come first
    for kw in (dict(n_rows=0, rows=None), {}):
        for name in ("src_of", "meta", "fec_size"):
            r, err = _call(product, plan, **kw, **{name: None})
            assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, plan, **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: the case set -------------------------------------------------------------------------------------------------
def _prefilled(out, x):
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


def test_rows_wide_model_and_census(oracle1000, shape_inputs, geometry_inputs):
    """The numpy model of the row rule over two-word masks equals the oracle's recover_batch_out on every group of
    every shape case (per_group 1 and k) and of the geometry cases; and from the reference alone each shape holds
    lines that fire, lines with two or more members lost, lines whose parity is lost, lines the header checks refuse
    (tampered), erased segments of rank >= per_group left out, targets at the first and at the last position of a
    row, and for k > 64 targets in both mask words and a target in a row across bits 63 / 64."""
    for k, col in rw.SHAPES:
        seen = {}
        for variant in rw.VARIANTS:
            for E in (1, k):
                x, ref = shape_inputs(k, col, variant, E)
                ic.compare(rw.model(x), _prefilled(ref, x), x, f"the model, {x.case[0]} E={E}")
                c = rw.census(x, ref)
                if E == k:
                    assert c["fire_left_out"] == 0 and c["rank_left_out"] == 0
                    if variant == "clean":
                        assert c["refused"] == 0, (k, col, c)
                for key, v in c.items():
                    seen[(key, variant, E)] = v
        nl = rw.n_lines(k, col)
        for key in ("fires", "two_lost", "parity_lost", "recovered"):
            assert seen[(key, "clean", k)] and seen[(key, "tampered", k)], (k, col, key, seen)
        for key in ("first_of_row", "last_of_row"):  # (groups 0..2 of the clean variant, set by hand)
            assert seen[(key, "clean", k)], (k, col, key, seen)
        assert seen[("refused", "tampered", k)], (k, col, seen)
        assert seen[("rank_left_out", "clean", 1)], (k, col, seen)
        assert bool(seen[("fire_left_out", "clean", 1)]) == (nl >= 2), (k, col, seen)
        if k > 64:
            assert seen[("word1", "clean", k)] and seen[("word2", "clean", k)], (k, col, seen)
        straddles = any(l * col < 64 <= min(k, (l + 1) * col) - 1 for l in range(nl))
        assert bool(seen[("straddle", "clean", k)]) == straddles, (k, col, seen)
    for c in rw.GEOMETRY:
        x, ref = geometry_inputs(c)
        ic.compare(rw.model(x), _prefilled(ref, x), x, f"the model, {x.case[0]}")
        assert rw.census(x, ref)["fires"], c
    # the geometry set: CD = 1, 2 and 75, both sides of the header and payload blocks' edges, a sparse pool
    assert {rc.cd16(rw.GEOMS[c[2]][0]) // 16 for c in rw.GEOMETRY} == {1, 2, 75}
    assert {c[3] for c in rw.GEOMETRY} >= {127, 128, 129, 257}
    assert {c[:2] for c in rw.GEOMETRY} == {(65, 65), (11, 5)} and any(c[5] for c in rw.GEOMETRY)
    x, _ = geometry_inputs(next(c for c in rw.GEOMETRY if c[5]))
    assert (x.src_of[x.src_of != ic.NONE] > 65535).any()


def test_rows_wide_reference_passes_behind_the_arena(oracle1000, shape_inputs, geometry_inputs):
    """With the oracle behind the same arena (RefIndexed) a case of each kind passes the comparison."""
    eng = ic.RefIndexed(oracle1000)
    for x, ref in (shape_inputs(66, 33, "tampered", 66), shape_inputs(11, 5, "clean", 1),
                   geometry_inputs(rw.GEOMETRY[1])):
        ic.compare(eng.run(x), _prefilled(ref, x), x, x.case[0])


BENT = {"pitch_rows": (11, 5), "second_word_dropped": (66, 33), "last_round_skipped": (100, 25),
        "target_row_xored": (100, 25), "wrong_index": (100, 25)}


@pytest.mark.parametrize("wrong", rw.WRONG)
def test_rows_wide_comparison_catches_each_bent_result(shape_inputs, wrong):
    """Each bent result (rows_wide_cases.model's switches: the pitch ceil(k / col) instead of k + NL, the second
    mask word dropped, the last round of a line skipped, the target's own row XORed in, a wrong out_index) fails the
    comparison, on the smallest shape that can show it."""
    k, col = BENT[wrong]
    x, ref = shape_inputs(k, col, "clean", k)
    ref = _prefilled(ref, x)
    with pytest.raises(AssertionError):
        ic.compare(rw.model(x, (wrong,)), ref, x, wrong)
    ic.compare(rw.model(x), ref, x, "the model unbent")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _run_both(gpu_lib, x, ref, what):
    """The new entry == the reference and == rfec_recover_indexed_out on the same arena inputs; both tags; the arena
    checks its guards and every input after each call."""
    eng = rw.GpuIndexedRowsWide(gpu_lib)
    got = eng.run(x)
    assert eng.last_path == (rw.ROWS_WIDE | x.k << 8 | x.col << 16), f"{what}: path {eng.last_path:#x}"
    if ref is not None:
        ic.compare(got, ref, x, f"{NAME} {what}")
    old = ic.GpuIndexed(gpu_lib)
    theirs = old.run(x)
    assert old.last_path == rw.old_tag(x.k, x.col), f"{what}: the other call's path {old.last_path:#x}"
    ic.compare(got, theirs, x, f"{NAME} against rfec_recover_indexed_out {what}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k,col,variant", CASES, ids=[f"k{k}-col{c}-{v}" for k, c, v in CASES])
def test_rows_wide_shapes_gpu(gpu_lib, shape_inputs, k, col, variant):
    """200 groups of one shape, 0, 1, 1, 1 or 2 members lost per row and a parity now and then, clean or with one
    tampered header per group, at per_group 1, 2, col and k."""
    for E in rw.per_groups(k, col):
        x, ref = shape_inputs(k, col, variant, E)
        _run_both(gpu_lib, x, ref, f"k={k} col={col} {variant} E={E}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", rw.GEOMETRY,
                         ids=lambda c: f"k{c[0]}-col{c[1]}-{c[2]}-G{c[3]}-E{c[4]}{'-sparse' if c[5] else ''}")
def test_rows_wide_geometry_gpu(gpu_lib, geometry_inputs, c):
    """CD = 1, 2 (a tail) and 75, both sides of the header blocks' and the payload blocks' edges, more header than
    payload blocks, a sparse pool with row indices above 65,535; the out slots' tails, the guards and every input as
    before the call."""
    x, ref = geometry_inputs(c)
    _run_both(gpu_lib, x, ref, str(c))


@pytest.mark.gpu
@pytest.mark.parametrize("k,col", ((65, 65), (11, 5)))
def test_rows_wide_empty_pool_and_zero_groups_gpu(gpu_lib, oracle1000, k, col):
    """n_rows == 0 with rows NULL and all-absent tables over 600 groups (header blocks, no payload block): recovered
    is 0, every out_index 0xFF, no out slot byte is written and the guards are intact (the arena's check).
    groups == 0 with NULL pointers returns at once."""
    x = rw.empty_pool_inputs(oracle1000, k, col)
    eng = rw.GpuIndexedRowsWide(gpu_lib)
    sh, hd, ix, rec = eng.run(x)
    assert eng.last_path == (rw.ROWS_WIDE | k << 8 | col << 16)
    assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all()
    gpu_lib.recover_indexed_rows_wide_out(x.plan, 0, x.stride, x.capacity, None, 0, *([None] * 7), 3, None, None, None,
                                          None)


@pytest.mark.gpu
def test_rows_wide_gpu_checks_can_fail(gpu_lib, oracle1000, geometry_inputs):
    """Two present members' map words swapped in the arena before the call: the comparison fails (both entries stay
    valid rows).  At (11, 5): two members of one row would change nothing, so a one-row shape cannot show it."""
    x, ref = geometry_inputs(next(c for c in rw.GEOMETRY if c[:2] == (11, 5)))
    eng = rw.GpuIndexedRowsWide(gpu_lib)
    eng.mutate, _ = ic.swap_two_members(oracle1000, x, ref)
    got = eng.run(x)
    with pytest.raises(AssertionError):
        ic.compare(got, ref, x, "swapped map words")


@pytest.mark.gpu
def test_rows_wide_window_chain_gpu(gpu_lib, oracle1000):
    """A mixed window of 60 groups from fec_id 65520 (it crosses the wrap) in three sections -- runs of five groups of
    k = 3 in one row of 3, of k = 30 in one row of 30 and of k = 40 as a 6 x 7 full matrix, in turn; one segment lost
    in every row group and two in every matrix group, a parity in every third group (a row group's only one: it
    then has no anchor, so no shape, no row and nothing to deliver), the datagrams shuffled: rfec_wire_parse, one rfec_wire_regroup_shapes, rfec_recover_indexed_shapes_out for the k = 3 section (groups 0 for
    the others), the new entry for the k = 30 section and rfec_recover_indexed_matrix_wide_out for the k = 40 one, each
    with its outputs at first[p] of the same dense arrays, and rfec_recover_deliver with groups[p] =
    min(counts[p], cap) -- six calls on one stream with no synchronisation in between.  All six outputs equal
    deliver_ref over the oracle's decode of each run's batch with the same losses; the k = 30 groups deliver their
    recovered segments."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0, run, NP = 60, 3, 65520, 5, 3  # (per_group <= k of every section)
    capacity, stride = sc.GEOMS["c20"]
    plans = [oracle.plan_matrix(3, 1, 3, rc.ROWS), oracle.plan_matrix(30, 1, 30, rc.ROWS), mw.wide_plan(oracle, 40)]
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
    assert all(d.shape[1] == ds for d in dg_l)
    order = rng.permutation(sum(len(d) for d in dg_l))
    dgram, dlen = np.concatenate(dg_l)[order], np.concatenate(dl_l)[order].astype(np.uint16)
    N = len(dgram)
    shape = np.where(anchored, shape, sc.NOSHAPE)
    assert (shape == sc.NOSHAPE).sum() == 16  # the row groups with g % 3 == 0: their one parity is lost
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
    groups = [min(c, G) for c in counts]
    first = [0, groups[0], groups[0] + groups[1], sum(groups)]
    total, max_out = first[NP], 256
    rec_, osh, ohd, oix = zeros(total * 16, 0xEE), zeros(total * E * stride, 0x3C), zeros(total * E * 20, 0x3C), \
        zeros(total * E, 0x3C)
    seg, segp = zeros(max_out * 24, dc.FILL), zeros(max_out * stride, dc.FILL)
    first_of, n_out = zeros((G + 1) * 4, dc.FILL), zeros(4, dc.FILL)
    ws = zeros(lib.recover_deliver_workspace_size(G), 0x11)
    # six calls, one stream, no synchronisation
    lib.wire_parse(N, ds, d_dg.data_ptr(), d_dl.data_ptr(), stride, capacity, recs.data_ptr(), rows.data_ptr(), st)
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    lib.recover_indexed_shapes_out(plans, sections, [groups[0], 0, 0], stride, capacity, rows.data_ptr(), N,
                                   rec_.data_ptr(), E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), st)
    for p, call, tag in ((1, lib.recover_indexed_rows_wide_out, rw.ROWS_WIDE | 30 << 8 | 30 << 16),
                         (2, lib.recover_indexed_matrix_wide_out, mw.WIDE | 40 << 8)):
        f, t = first[p], tab[p]
        call(plans[p], groups[p], stride, capacity, rows.data_ptr(), N,
             *(t[name].data_ptr() for name in ("src_of", "hdr", "present", "meta", "fec_size", "parity_present")),
             rec_.data_ptr() + 16 * f, E, osh.data_ptr() + f * E * stride, ohd.data_ptr() + f * E * 20,
             oix.data_ptr() + f * E, st)
        assert int(lib.lib.rfec_indexed_last_path()) == tag
    lib.recover_deliver(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                        stride, capacity, E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), max_out,
                        seg.data_ptr(), segp.data_ptr(), first_of.data_ptr(), n_out.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), shape)
    assert np.array_equal(down(win["rank_of"], np.uint32, (G,)), rank)
    e_sh, e_hd, e_ix, e_rec = (np.concatenate([np.concatenate([e[i] for e in exp[p]]) for p in range(NP)])
                               for i in range(4))
    assert np.array_equal(down(rec_, np.uint64, (total, 2)), e_rec)
    assert np.array_equal(down(oix, np.uint8, (total, E)), e_ix)
    group_of = []
    for p in range(NP):
        go = np.full(G, sc.NONE, np.uint32)
        go[:counts[p]] = np.nonzero(shape == p)[0]
        group_of.append(go)
    x = dc.from_tables("rows-wide-window", plans, [G] * NP, groups, G, fec_id0, shape, rank, group_of, capacity, stride,
                       E, e_sh, e_hd, e_ix, max_out)
    ref = dc.deliver_ref(x, dc.new_outputs(x))
    got = {"seg": down(seg, rc.po.RX_SEG, (max_out,)), "seg_payload": down(segp, np.uint8, (max_out, stride)),
           "first_of": down(first_of, np.uint32, (G + 1,)), "n_out": down(n_out, np.uint32, (1,))}
    dc.compare(got, ref, f"{NAME} window chain")
    dc.check_untouched(x, got, "window chain")
    # the k = 30 groups deliver: one lost segment in each group whose parity arrived, every one recovered
    fo = got["first_of"]
    n30 = sum(int(fo[g + 1] - fo[g]) for g in range(G) if shape[g] == 1)
    assert n30 == int((e_ix[first[1]:first[2]] != 0xFF).sum()) == counts[1] and 10 <= n30 < 20
    assert x.T == int(got["n_out"][0])
