"""rfec_recover_indexed_window_each_out: rfec_recover_indexed_window_out with an
out-slot count per section (per_group a host array), the sections' slots packed
end to end -- the ragged numbering of include/razor_fec.h -- and
rfec_recover_window_slots.  On the CPU: the declarations and bindings, every
argument check in its order, the upper bound per section, zero groups and the
launch without a device, the ragged reference against the existing window
reference at a uniform E, the bent readings, the window set's conditions, and the
capability window (1 x 3 groups beside a k = 100 frame) against the reference's
receiver.  On the GPU: every window against the oracle and, byte for byte,
against each section's single-shape call with that section's own per_group on
the same arena; every window of window_cases at its uniform E byte for byte
against rfec_recover_indexed_window_out; groups NULL, caps above the rows in use,
the empty pool; and the composed chain from datagrams to
rfec_recover_deliver_each's list (window_each_cases.py)."""
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
import window_cases as wc
import window_each_cases as we

NAME, METHOD = "rfec_recover_indexed_window_each_out", "recover_indexed_window_each_out"
NEW = {NAME: METHOD, "rfec_recover_window_slots": "recover_window_slots",
       "rfec_recover_deliver_each": "recover_deliver_each"}


@pytest.fixture(scope="module")
def windows(oracle1000):
    """Every window's inputs and reference outputs, computed once and left unchanged."""
    sections, cache = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = we.make_window(oracle1000, we.WINDOW[name], sections)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def uniform_windows(oracle1000):
    sections, cache = {}, {}

    def get(name):
        if name not in cache:
            cache[name] = wc.make_window(oracle1000, wc.WINDOW[name], sections)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def capability(oracle1000):
    return we.capability_stream(oracle1000)


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_each_entries_are_declared_bound_and_exported(product, product1200):
    from razor_amd import fec
    for name, method in NEW.items():
        assert name in fec.header_functions() and name in fec._SIGS, name
        for lib in (product, product1200):
            assert hasattr(lib.lib, name) and hasattr(lib, method), name
    assert hasattr(fec, "window_first_slots")
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7 and product1200.lib.rfec_abi_version() == 7


def test_window_slots_and_first_slots(product):
    """rfec_recover_window_slots is the sum of groups[p] * per_group[p] (cap when groups is NULL; per_group of a
    section without groups is not read), and razor_amd.fec.window_first_slots states the ragged numbering."""
    from razor_amd import fec
    secs = [dict(cap=c) for c in (1, 7, 0, 5)]
    E = [3, 6, 99, 17]
    assert product.recover_window_slots(secs, None, E) == 3 + 42 + 85
    assert product.recover_window_slots(secs, [1, 0, 0, 2], E) == 3 + 34
    assert product.recover_window_slots(None, [1, 0, 0, 2], E) == 3 + 34
    assert product.recover_window_slots(secs, [1 << 31] * 4, [128] * 4) == 4 * 128 << 31
    f = product.lib.rfec_recover_window_slots
    assert f(None, 4, None, (C.c_uint32 * 4)(*E)) == 0 and f(None, 4, (C.c_uint32 * 4)(1, 1, 1, 1), None) == 0
    first, slot_first = fec.window_first_slots([1, 0, 0, 2], E)
    assert first == [0, 1, 1, 1, 3] and slot_first == [0, 3, 3, 3, 37]
    a, b = we.first_slots([1, 0, 0, 2], E)
    assert a.tolist() == first and b.tolist() == slot_first


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(rows=0x10000, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001)
T = dict(src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002, parity_present=0x70008)
NULL_T = {name: None for name in T}
G4 = (4, 4, 4, 4)
E4 = (2, 3, 17, 1)


def _call(product, plans, groups=(4,), caps=None, tables=None, stride=1216, capacity=1200, n_rows=100, per_group=E4,
          n_plans=None, null_plans=False, null_sections=False, **ptrs):
    """One raw call on made-up addresses: per_group a tuple (cut or repeated to the plans) or None (NULL)."""
    from razor_amd.fec import as_plan, rfec_plan, rfec_regroup_section
    n = len(plans)
    caps = list(caps) if caps is not None else (list(groups) if groups is not None else [4] * n)
    tables = tables or [{}] * n
    pa = (rfec_plan * max(n, 1))(*(as_plan(p) for p in plans))
    sa = (rfec_regroup_section * max(n, 1))(*(rfec_regroup_section(cap=caps[p], **dict(T, **tables[p]))
                                             for p in range(n)))
    ga_ = None if groups is None else (C.c_uint32 * max(n, 1))(*groups)
    ea = None if per_group is None else (C.c_uint32 * max(n, 1))(*[per_group[p % len(per_group)] for p in range(n)])
    p = dict(P, **ptrs)
    r = getattr(product.lib, NAME)(None if null_plans else pa, n if n_plans is None else n_plans,
                                   None if null_sections else sa, ga_, stride, capacity, p["rows"], n_rows,
                                   p["recovered"], ea, p["out_shards"], p["out_hdr"], p["out_index"], None)
    return r, product.lib.rfec_last_error().decode()


def _four(o):
    """One plan of each family: k = 10, 12, 17 and 30."""
    return [ic.PLANS["full3x4k10"](o), ic.PLANS["rows12x3"](o), mw.wide_plan(o, 17), rw.rows_plan(o, 30, 30)]


BAD_ARGS = {
    "null-plans": (dict(null_plans=True), "plans is NULL"),
    "no-plans": (dict(n_plans=0), "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]"),
    "33-plans": (dict(n_plans=33), "n_plans must be in [1, RFEC_RECOVER_MAX_SHAPES]"),
    "null-sections": (dict(null_sections=True), "sections is NULL"),
    "stride-0": (dict(stride=0), "stride must be a positive multiple of 16"),
    "stride-1208": (dict(stride=1208), "stride must be a positive multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity must be <= stride"),
    "null-per-group": (dict(per_group=None), "per_group is NULL"),
    "per-group-0": (dict(per_group=(2, 0, 17, 1)), "per_group[1] must be in [1, plans[p].k]"),
    "per-group-k+1-matrix": (dict(per_group=(11, 3, 17, 1)), "per_group[0] must be in [1, plans[p].k]"),
    "per-group-k+1-rows": (dict(per_group=(10, 13, 17, 1)), "per_group[1] must be in [1, plans[p].k]"),
    "per-group-k+1-wide": (dict(per_group=(10, 12, 18, 1)), "per_group[2] must be in [1, plans[p].k]"),
    "per-group-k+1-wide-rows": (dict(per_group=(10, 12, 17, 31)), "per_group[3] must be in [1, plans[p].k]"),
    "groups-above-cap": (dict(groups=(4, 4, 5, 4), caps=G4), "groups[2] must be <= sections[p].cap"),
    "lanes": (dict(groups=(4, 4, 1 << 22, 4), stride=1024, capacity=1024, per_group=(2, 3, 8, 1)),
              "groups[2]: section too large for one launch (groups x per_group x chunks)"),
    "slots": (dict(groups=(4, 4, 1 << 30, 1 << 30), stride=16, capacity=16, per_group=(1,)), "window too large"),
    "null-rows": (dict(rows=None), "NULL buffer"),
    "null-recovered": (dict(recovered=None), "NULL buffer"),
    "null-out-shards": (dict(out_shards=None), "NULL buffer"),
    "null-out-hdr": (dict(out_hdr=None), "NULL buffer"),
    "null-out-index": (dict(out_index=None), "NULL buffer"),
    **{f"null-{name}-{p}": (dict(tables=[{}] * p + [{name: None}] + [{}] * (3 - p)), f"sections[{p}]: NULL buffer")
       for name in T for p in (0, 3)},
    "rows-8": (dict(rows=0x10008), "rows and out_shards must be 16-byte aligned"),
    "out-shards-8": (dict(out_shards=0x90008), "rows and out_shards must be 16-byte aligned"),
    "recovered-4": (dict(recovered=0x80004), "recovered must be 8-byte aligned"),
    "out-hdr-2": (dict(out_hdr=0xA0002), "out_hdr must be 4-byte aligned"),
    "present-4": (dict(tables=[{}, {}, {"present": 0x40004}, {}]),
                  "sections[2]: present and parity_present must be 8-byte aligned"),
    "src-of-2": (dict(tables=[{}, {}, {"src_of": 0x20002}, {}]), "sections[2]: src_of, hdr and meta must be 4-byte"),
    "fec-size-1": (dict(tables=[{}, {}, {"fec_size": 0x60001}, {}]), "sections[2]: fec_size must be 2-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_window_each_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    kw = dict(dict(groups=G4), **kw)
    r, err = _call(product, _four(oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_window_each_accepts_each_sections_own_k(product, oracle1000):
    """per_group[p] = plans[p].k in every section passes the value checks (a NULL pointer is what is refused) where
    the uniform call is bounded by the least k, 10; one above any of them is refused with its index."""
    four = _four(oracle1000)
    ks = tuple(p.k for p in four)
    assert ks == (10, 12, 17, 30)
    r, err = _call(product, four, groups=G4, per_group=ks, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    for p in range(4):
        r, err = _call(product, four, groups=G4, per_group=tuple(k + (q == p) for q, k in enumerate(ks)), rows=None)
        assert r == -1 and f"per_group[{p}] must be in [1, plans[p].k]" in err, (p, r, err)
    # a section without groups carries any per_group: 0, and far above its k
    for bad in (0, 31, 0xFFFFFFFF):
        r, err = _call(product, four, groups=(4, 0, 4, 4), per_group=(10, bad, 17, 30), tables=[{}, NULL_T, {}, {}],
                       rows=None)
        assert r == -1 and "NULL buffer" in err and "sections" not in err, (bad, r, err)
    r, err = _call(product, four, groups=None, caps=(4, 0, 4, 4), per_group=(10, 0, 17, 30),
                   tables=[{}, NULL_T, {}, {}], rows=None)
    assert r == -1 and "NULL buffer" in err and "sections" not in err, (r, err)


def test_window_each_checks_in_order(product, oracle1000):
    """Each check comes before the next: a call that breaks two is refused for the earlier one.  The order is the
    plans and n_plans, each plan and its family, stride, capacity, per_group (NULL, then each section's range),
    groups <= cap, the lanes of a section, the header lanes, the launch's blocks, rows and slots, the NULL pointers,
    the alignments."""
    four = _four(oracle1000)
    bad = ic.PLANS["full3x4k10"](oracle1000)
    bad.line[2].first, bad.line[2].count = 8, 4  # members 8..11 of k = 10
    big = dict(stride=16, capacity=16, per_group=(1,))
    steps = [
        (dict(null_plans=True), "plans is NULL"),
        (dict(n_plans=33), "n_plans"),
        (dict(null_sections=True), "sections is NULL"),
        (dict(plans=[four[0], four[1], bad, four[3]]), "beyond k"),
        (dict(plans=[four[0], four[1], ic.PLANS["hand6"](oracle1000), four[3]]), "plans[2]"),
        (dict(stride=1208), "stride"),
        (dict(capacity=1300), "capacity"),
        (dict(per_group=None), "per_group is NULL"),
        (dict(per_group=(2, 3, 17, 31)), "per_group[3] must be in"),
        (dict(groups=(4, 4, 4, 5), caps=G4), "groups[3] must be <= sections[p].cap"),
        (dict(groups=(4, 4, 4, 1 << 31), caps=(4, 4, 4, 1 << 31), **big), "groups x per_group x chunks"),
        (dict(groups=(4, 1 << 30, 4, 4), caps=(4, 1 << 30, 4, 4), **big), "header lanes"),
        (dict(groups=(4, 4, 1 << 30, 1 << 30), caps=(4, 4, 1 << 30, 1 << 30), **big), "window too large"),
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


def test_window_each_lane_and_slot_bounds(product, oracle1000):
    """The per-section bound takes the section's own per_group; the slots' bound is S * CD < 2^31 over the call:
    sections that pass alone, too many slots together."""
    m, r12, w17, s30 = _four(oracle1000)
    geo = dict(stride=16, capacity=16)
    # 2^26 groups: x 17 slots is below 2^31, x 17 at CD = 2 is not; the same groups at E = 1 pass either way
    r, err = _call(product, [w17, s30], groups=(1 << 26, 4), per_group=(17, 1), **geo, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    r, err = _call(product, [w17, s30], groups=(1 << 26, 4), per_group=(17, 1), stride=32, capacity=17, rows=None)
    assert r == -1 and "groups[0]: section too large for one launch (groups x per_group x chunks)" in err, (r, err)
    r, err = _call(product, [s30, w17], groups=(1 << 26, 4), per_group=(1, 17), stride=32, capacity=17, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    # each section below 2^31 lanes, the call's slots not: (2^30 - 1) + 2^30 + 1
    r, err = _call(product, [w17, w17], groups=((1 << 29), (1 << 29) - 1), per_group=(2, 2), **geo, rows=None)
    assert r == -1 and "NULL buffer" in err, (r, err)
    r, err = _call(product, [w17, w17, w17], groups=((1 << 29), (1 << 29) - 1, 1), per_group=(2, 2, 2), **geo,
                   rows=None)
    assert r == -1 and "window too large" in err, (r, err)


def test_window_each_zero_groups_and_device(product, oracle1000):
    """All groups[p] == 0 touches nothing: every pointer but plans, sections and per_group may be NULL and per_group
    may hold anything; the value checks still come first.  Without a device a valid call fails past every check,
    at the launch."""
    four = _four(oracle1000)
    nothing = dict(tables=[NULL_T] * 4, **{n: None for n in P})
    for E in ((0,), (200,), E4):
        r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, per_group=E, **nothing)
        assert r == 0, (r, err)
        r, err = _call(product, four, groups=None, caps=(0, 0, 0, 0), per_group=E, **nothing)
        assert r == 0, (r, err)
    r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, per_group=None, **nothing)
    assert r == -1 and "per_group is NULL" in err, (r, err)
    r, err = _call(product, four, groups=(0, 0, 0, 0), caps=G4, stride=8, **nothing)
    assert r == -1 and "stride" in err, (r, err)
    r, err = _call(product, four, groups=None, caps=G4, **nothing)
    assert r == -1 and "NULL buffer" in err, (r, err)  # cap groups each: the pointers are wanted
    for kw in (dict(n_rows=0, rows=None), {}):
        r, err = _call(product, four, groups=G4, **kw, recovered=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            for E in (E4, (10, 12, 17, 30)):
                r, err = _call(product, four, groups=G4, per_group=E, **kw)
                assert r == -2 and "launch" in err, (r, err)
            r, err = _call(product, four, groups=None, caps=G4, **kw)
            assert r == -2 and "launch" in err, (r, err)
            r, err = _call(product, four, groups=(4, 0, 4, 0), per_group=(10, 0, 17, 999), **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: the ragged reference -------------------------------------------------------------------------------------------
def _prefilled(out, x):
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


@pytest.mark.parametrize("name", ["mixed-c20-tampered", "staircase", "empties", "thirty-two", "swap"])
def test_window_each_ref_reduces_to_the_window_reference(uniform_windows, name):
    """With every per_group[p] = E, window_each_ref is the existing window reference: the sections' references one
    after the other in [R][E] arrays, and section_view gives each section's back."""
    W = uniform_windows(name)
    V = we.from_uniform(W)
    live = wc.launched(W)
    sh, hd, ix, rec = we.window_each_ref(V)
    R, E = int(W.first[-1]), W.E
    assert int(V.slot_first[-1]) == R * E and [int(s) for s in V.slot_first] == [int(f) * E for f in W.first]
    assert np.array_equal(sh.reshape(R, E, W.stride), np.concatenate([W.ref[p][0] for p in live]))
    assert np.array_equal(hd.reshape(R, E), np.concatenate([W.ref[p][1] for p in live]))
    assert np.array_equal(ix.reshape(R, E), np.concatenate([W.ref[p][2] for p in live]))
    assert np.array_equal(rec, np.concatenate([W.ref[p][3] for p in live]))
    arrays = we.window_each_ref(V, prefilled=True)
    for p in live:
        ic.compare(we.section_view(V, arrays, p), W.ref[p], W.x[p], f"{name} section {p}")


def test_window_each_windows_cover_their_conditions(oracle1000, windows):
    """From the reference alone: the mixed windows hold all four families at five different E in two orders, a small
    E before a large one and the reverse; the first section's slot count is odd, so every later section's slot base
    is no multiple of its own E (where E > 1); sections of 1, 255, 256 and 257 groups at CD = 1, a slot tail at
    CD = 2, CD = 75; every launched section recovers a segment or (tampered, one group) refuses its one line; the
    staircases cascade at E = 10 between two E = 3 sections; 32 sections with E cycling through 1, 2, 3 and k; empty
    first, middle and last sections with a per_group out of range."""
    for geom in ("c15", "c20", "c1200"):
        for variant in ("clean", "tampered"):
            a, b = windows(f"each-{geom}-{variant}"), windows(f"each-{geom}-reversed-{variant}")
            for W in (a, b):
                assert sorted(x.family for x in W.x) == [1, 2, 2, 3, 4] and sorted(W.E) == [1, 2, 3, 6, 17]
                assert W.groups[0] == 1 and W.E[0] == 3 and int(W.slot_first[1]) == 3
                assert all(int(W.slot_first[p]) % W.E[p] for p in range(1, 5) if W.E[p] > 1), W.name
                assert all(W.E[p] <= W.x[p].k for p in range(5))
                assert max(W.E) > min(x.k for x in W.x)  # beyond what one per_group for the call allows
                for p in wc.launched(W):
                    c = wc.census(W.x[p], W.ref[p])
                    assert c["recovered"] or (variant == "tampered" and W.x[p].G == 1 and c["refused"]), (W.name, p)
            # (E = 6 and 2 before E = 17 in one order, behind it in the other)
            assert a.E.index(6) < a.E.index(17) and b.E.index(17) < b.E.index(6) and a.E[1:] == b.E[:0:-1]
    W = windows("each-c15-clean")
    assert rc.cd16(W.capacity) == 16 and {1, 255, 256, 257} <= set(W.groups)
    assert rc.cd16(windows("each-c20-clean").capacity) == 32 < windows("each-c20-clean").stride
    assert rc.cd16(windows("each-c1200-clean").capacity) == 75 * 16
    W = windows("staircase")
    assert W.E == [3, 10, 3] and W.x[1].k == 100 and int(W.slot_first[1]) == 9
    assert wc.census(W.x[1], W.ref[1])["cascade"] >= 20
    W = windows("thirty-two")
    assert len(W.plans) == 32 and 0 in W.groups and {x.family for x in W.x if x is not None} == {1, 2, 3, 4}
    live = wc.launched(W)
    assert {W.E[p] for p in live} >= {1, 2, 3, 5, 10, 12, 17} and all(W.E[p] <= W.x[p].k for p in live)
    W = windows("empties")
    assert W.groups[0] == 0 and W.groups[-1] == 0 and W.groups[2] == 0 and W.E[0] == 0 and W.E[2] == 200
    W = windows("sparse")
    for p in (1, 2, 3):
        so = W.src_of[p]
        assert (so[so != wc.NONE] > 65535).all()
    W = windows("swap")
    assert len(W.src_of[0]) == len(W.src_of[1]) and W.E == [3, 2]


@pytest.mark.parametrize("wrong", we.WRONG_VIEW)
def test_window_each_comparison_catches_each_bent_reading(windows, wrong):
    """The ragged reference read back by a bent rule -- o * E with the call's largest E, slot_first taken as
    first * E[p], the row pitch of the neighbouring section -- fails the comparison in some section of the mixed
    window, and the rule itself passes in every section."""
    W = windows("each-c20-clean")
    arrays = we.window_each_ref(W, prefilled=True)
    caught = []
    for p in wc.launched(W):
        ic.compare(we.section_view(W, arrays, p), W.ref[p], W.x[p], "the rule itself")
        try:
            ic.compare(we.section_view(W, arrays, p, (wrong,)), W.ref[p], W.x[p], wrong)
        except AssertionError:
            caught.append(p)
    assert caught, wrong


def test_window_each_comparison_can_fail(oracle1000, windows):
    """Results bent on purpose fail the comparison: a section written one slot too far; two sections' src_of
    swapped."""
    W = windows("swap")
    arrays = we.window_each_ref(W, prefilled=True)
    shifted = tuple(np.roll(a, 1, axis=0) for a in arrays[:3]) + (arrays[3],)
    with pytest.raises(AssertionError):
        ic.compare(we.section_view(W, shifted, 1), W.ref[1], W.x[1], "slot + 1")
    import copy
    for p in (0, 1):
        y = copy.copy(W.x[p])
        y.src_of, y.rows, y.n_rows = W.src_of[1 - p], W.rows, W.n_rows
        with pytest.raises(AssertionError):
            ic.compare(_prefilled(ic.reference(oracle1000, y), y), W.ref[p], W.x[p], "swapped src_of")


# -- CPU: the capability window against the reference's receiver ---------------------------------------------------------
def _capability_tables(o, cap, Es):
    """regroup_shapes_ref over the stream, then oracle.recover_batch_out per section at Es[p], laid out ragged."""
    plans, G = cap.plans, cap.G
    caps = [G] * len(plans)
    reg = sc.regroup_shapes_ref(plans, caps, G, cap.fec_id0, cap.recs, cap.capacity,
                                sc.new_outputs(plans, caps, G, len(cap.recs), 0))
    rows = [int(c) for c in reg["counts"]]
    osh, ohd, oix, rec = [], [], [], []
    for p, plan in enumerate(plans):
        sh, hd, ix = dc.decode_sections(o, [plan], [caps[p]], [rows[p]], [reg["sec"][p]], cap.pay, cap.capacity,
                                        cap.stride, Es[p])
        osh.append(sh.reshape(-1, cap.stride)), ohd.append(hd.reshape(-1)), oix.append(ix.reshape(-1))
    return reg, rows, np.concatenate(osh), np.concatenate(ohd), np.concatenate(oix)


def _receiver_list(o, cap):
    rx, rxp, _, dropped = o.rx_recover(cap.recs, cap.pay, cap.capacity)
    assert dropped == 0
    by_id = np.argsort(rx["hdr"]["seq"], kind="stable")
    return rx[by_id], rxp[by_id]


def test_capability_window_delivers_what_the_receiver_delivers(oracle1000, capability):
    """A window of 1 x 3 row groups (per_group 3) and the planner's k = 100 matrix at protect_fraction 10 (per_group
    10), each k = 100 group losing five members in distinct rows and columns.  The census, from the oracle: the
    reference recovers all five of every k = 100 group -- more than the least k of the window, 3, which bounds the
    uniform call's per_group.  deliver_each_ref over the ragged tables delivers, entry for entry and in order, what
    the reference's receiver (oracle.rx_recover on the in-order stream) delivers sorted by packet id."""
    o, cap = oracle1000, capability
    assert [wc.family_of(o, p) for p in cap.plans] == [2, 3] and cap.plans[1].k == 100 and cap.plans[1].col == 10
    assert len({i // 10 for i in we.CAP_LOST_100}) == 5 and len({i % 10 for i in we.CAP_LOST_100}) == 5
    reg, rows, osh, ohd, oix = _capability_tables(o, cap, cap.Es)
    assert np.array_equal(reg["shape_of"], cap.shape) and rows == [6, 3]
    first, slot_first = we.first_slots(rows, cap.Es)
    # the census: every k = 100 group recovers its five members, in ascending order in its first five out slots
    per100 = oix[slot_first[1]:].reshape(rows[1], 10)
    for row in per100:
        assert row[:5].tolist() == sorted(we.CAP_LOST_100) and (row[5:] == we.HOLE).all()
    min_k = min(p.k for p in cap.plans)
    assert min_k == 3 and int((per100 != we.HOLE).sum(1).max()) == 5 > min_k
    x = we.each_from_tables("capability", cap.plans, [cap.G] * 2, rows, cap.G, cap.fec_id0, reg["shape_of"],
                            reg["rank_of"], [s["group_of"] for s in reg["sec"]], cap.capacity, cap.stride, cap.Es,
                            osh, ohd, oix, None)
    out = we.RefDeliverEach().run(x)
    T = int(out["n_out"][0])
    rx, rxp = _receiver_list(o, cap)
    assert T == len(rx) == 6 * 1 + 3 * 5, (T, len(rx))
    seg, segp = out["seg"][:T], out["seg_payload"][:T]
    assert np.array_equal(seg["hdr"], rx["hdr"])
    assert np.array_equal(seg["fec_id"], rx["fec_id"]) and not seg["reserved"].any()
    assert np.array_equal(segp[:, :cap.capacity], rxp[:, :cap.capacity])
    assert (seg["fec_id"] < 100).any() and (seg["fec_id"] > 65000).any()  # both sides of 65535 -> 1
    # the uniform rule at the window's largest legal per_group delivers fewer
    _, _, ush, uhd, uix = _capability_tables(o, cap, [min_k] * 2)
    u = dc.from_tables("capability-uniform", cap.plans, [cap.G] * 2, rows, cap.G, cap.fec_id0, reg["shape_of"],
                       reg["rank_of"], [s["group_of"] for s in reg["sec"]], cap.capacity, cap.stride, min_k, ush, uhd,
                       uix, None)
    assert u.T == 6 + 3 * 3 < T


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _check_window(eng, W, out, what, ref=True, tags=True):
    """Every launched section: the tag, the reference, and the single-shape call byte for byte."""
    live = wc.launched(W)
    assert eng.last_path == (we.WINDOW_EACH_TAG | len(live) << 8), f"{what}: path {eng.last_path:#x}"
    for p in live:
        x = W.x[p]
        got, single, _ = out[p]
        if tags:
            assert eng.single_paths[p] == wc.single_tag(x), f"{what} section {p}: path {eng.single_paths[p]:#x}"
        if ref and W.ref[p] is not None:
            ic.compare(got, W.ref[p], x, f"{NAME} {what} section {p} ({W.names[p]} x {W.groups[p]} at E {W.E[p]})")
        ic.compare(got, single, x, f"{NAME} {what} section {p} (family {x.family}) against its single-shape call")
        for a, b in zip(got[1:], single[1:]):  # out_hdr, out_index, recovered: every byte
            assert a.tobytes() == b.tobytes(), f"{what} section {p}"


@pytest.mark.gpu
@pytest.mark.parametrize("w", we.WINDOWS, ids=we.window_id)
def test_window_each_gpu(gpu_lib, windows, w):
    """The product == the reference in every launched section at the section's own per_group: recovered, out_index,
    out_hdr, out_shards over [0, 16 CD) of the recovered slots; the out slots' tails, the guards and every input as
    before the call; the same four outputs byte for byte against the section's single-shape call with per_group[p]
    on the same arena; one launch."""
    W = windows(w[0])
    eng = we.GpuWindowEachDecode(gpu_lib)
    gpu_lib.lib.rfec_timing_events(None, None)
    eng.run(W, singles=False)
    assert gpu_lib.lib.rfec_timing_launches() == 1
    out = eng.run(W)
    _check_window(eng, W, out, w[0])


@pytest.mark.gpu
@pytest.mark.parametrize("w", wc.WINDOWS, ids=wc.window_id)
def test_window_each_equals_window_decode_at_uniform_E_gpu(gpu_lib, uniform_windows, w):
    """Every window of window_cases with per_group[p] = its E in every section: byte for byte the four arrays of
    rfec_recover_indexed_window_out on the same arena, and the reference."""
    W = we.from_uniform(uniform_windows(w[0]))
    eng = we.GpuWindowEachDecode(gpu_lib)
    out = eng.run(W, singles=False, uniform=True)
    live = wc.launched(W)
    assert eng.last_path == (we.WINDOW_EACH_TAG | len(live) << 8)
    assert eng.uniform_path == (wc.WINDOW_TAG | len(live) << 8)
    for a, b, name in zip(eng.arrays, eng.uniform_arrays, ("out_shards", "out_hdr", "out_index", "recovered")):
        assert a.tobytes() == b.tobytes(), f"{w[0]}: {name} differs from rfec_recover_indexed_window_out's"
    for p in live:
        ic.compare(out[p][0], W.ref[p], W.x[p], f"{NAME} {w[0]} section {p}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["each-c20-tampered", "empties"])
def test_window_each_null_groups_gpu(gpu_lib, windows, name):
    """groups NULL: every section's cap, here its groups -- the same outputs."""
    W = windows(name)
    eng = we.GpuWindowEachDecode(gpu_lib)
    _check_window(eng, W, eng.run(W, pass_groups=False), f"{name} groups NULL")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["each-c20-reversed-tampered", "each-c1200-clean"])
def test_window_each_cap_above_the_rows_in_use_gpu(gpu_lib, windows, name):
    """groups NULL with every cap three rows above the rows in use, those rows as the regroup leaves them: the rows
    in use decode as before, the trailing rows to nothing -- recovered 0, every out_index 0xFF, no out slot byte
    written."""
    V = windows(name)
    W = we.padded(V, 3)
    eng = we.GpuWindowEachDecode(gpu_lib)
    out = eng.run(W, pass_groups=False)
    _check_window(eng, W, out, f"{name} padded")
    for p in wc.launched(W):
        sh, hd, ix, rec = out[p][0]
        g = V.groups[p]
        assert not rec[g:].any() and (ix[g:] == 0xFF).all() and (sh[g:] == ic.FILL).all(), p


@pytest.mark.gpu
def test_window_each_empty_pool_and_zero_groups_gpu(gpu_lib, oracle1000):
    """n_rows == 0 with rows NULL and all-absent tables, a section of each family at its own E: recovered is 0, every
    out_index 0xFF, no out slot byte is written and the guards are intact; the single-shape calls agree.  All groups
    0 with NULL pointers returns at once."""
    W = we.empty_pool_window(oracle1000)
    eng = we.GpuWindowEachDecode(gpu_lib)
    out = eng.run(W)
    _check_window(eng, W, out, "empty pool", tags=False)
    for p in range(4):
        sh, hd, ix, rec = out[p][0]
        assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all(), p
    for cap in (0, 9):
        gpu_lib.recover_indexed_window_each_out(W.plans, [dict(cap=cap)] * 4, [0] * 4, W.stride, W.capacity, None, 0,
                                                None, [0, 1, 200, 3], None, None, None, None)


@pytest.mark.gpu
def test_window_each_gpu_checks_can_fail(gpu_lib, windows):
    """Two sections' src_of pointers swapped in the call: the comparison fails (the maps have as many words, and
    every entry stays a valid row)."""
    W = windows("swap")
    eng = we.GpuWindowEachDecode(gpu_lib)
    out = eng.run(W, swap=(0, 1), singles=False)
    for p in (0, 1):
        with pytest.raises(AssertionError):
            ic.compare(out[p][0], W.ref[p], W.x[p], "swapped src_of pointers")


@pytest.mark.gpu
def test_window_each_chain_composed_gpu(gpu_lib, oracle1000, capability):
    """The capability window (1 x 3 groups beside k = 100 frames that each lose five members) as datagrams:
    rfec_wire_parse, one rfec_wire_regroup_shapes, ONE rfec_recover_indexed_window_each_out at per_group (3, 10) and
    rfec_recover_deliver_each -- four calls on one stream with no synchronisation in between.  The list equals the
    reference receiver's, and it is strictly longer than the list the uniform calls
    (rfec_recover_indexed_window_out + rfec_recover_deliver) deliver at the window's largest legal per_group, the
    least k = 3; both are computed here."""
    lib, o, cap = gpu_lib, oracle1000, capability
    plans, G, Es, fec_id0, capacity, stride = cap.plans, cap.G, cap.Es, cap.fec_id0, cap.capacity, cap.stride
    NP, N, ds = len(plans), len(cap.dgram), cap.dgram.shape[1]
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
    w, secs = sc.shapes_of(plans, [G] * NP, G, N)
    win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
    tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
           for s in secs]
    sections = [dict(cap=G, **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(NP)]
    counts = [int((cap.shape == p).sum()) for p in range(NP)]
    groups = counts  # (what a caller that read the counts back passes; known here from the stream)
    first, slot_first = we.first_slots(groups, Es)
    R, S, max_out = int(first[-1]), int(slot_first[-1]), 64
    assert lib.recover_window_slots(sections, groups, Es) == S
    E_u = min(p.k for p in plans)

    def outputs(slots):
        return dict(rec=zeros(R * 16, 0xEE), osh=zeros(slots * stride, 0x3C), ohd=zeros(slots * 20, 0x3C),
                    oix=zeros(slots, 0x3C), seg=zeros(max_out * 24, dc.FILL), segp=zeros(max_out * stride, dc.FILL),
                    first_of=zeros((G + 1) * 4, dc.FILL), n_out=zeros(4, dc.FILL),
                    ws=zeros(lib.recover_deliver_workspace_size(G), 0x11))

    a, u = outputs(S), outputs(R * E_u)
    # four calls, one stream, no synchronisation
    lib.wire_parse(N, ds, d_dg.data_ptr(), d_dl.data_ptr(), stride, capacity, recs.data_ptr(), rows.data_ptr(), st)
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    lib.recover_indexed_window_each_out(plans, sections, groups, stride, capacity, rows.data_ptr(), N,
                                        a["rec"].data_ptr(), Es, a["osh"].data_ptr(), a["ohd"].data_ptr(),
                                        a["oix"].data_ptr(), st)
    assert int(lib.lib.rfec_indexed_last_path()) == (we.WINDOW_EACH_TAG | NP << 8)
    lib.recover_deliver_each(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(),
                             win["rank_of"].data_ptr(), stride, capacity, Es, a["osh"].data_ptr(), a["ohd"].data_ptr(),
                             a["oix"].data_ptr(), max_out, a["seg"].data_ptr(), a["segp"].data_ptr(),
                             a["first_of"].data_ptr(), a["n_out"].data_ptr(), a["ws"].data_ptr(), st)
    assert int(lib.lib.rfec_indexed_last_path()) == (we.DELIVER_EACH | dc.launches(G) << 8)
    # what the uniform calls offer for the same window: per_group = the least k
    lib.recover_indexed_window_out(plans, sections, groups, stride, capacity, rows.data_ptr(), N, u["rec"].data_ptr(),
                                   E_u, u["osh"].data_ptr(), u["ohd"].data_ptr(), u["oix"].data_ptr(), st)
    lib.recover_deliver(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                        stride, capacity, E_u, u["osh"].data_ptr(), u["ohd"].data_ptr(), u["oix"].data_ptr(), max_out,
                        u["seg"].data_ptr(), u["segp"].data_ptr(), u["first_of"].data_ptr(), u["n_out"].data_ptr(),
                        u["ws"].data_ptr(), st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), cap.shape)
    assert np.array_equal(down(win["counts"], np.uint32, (NP,)), counts)
    rx, rxp = _receiver_list(o, cap)
    T = int(down(a["n_out"], np.uint32, (1,))[0])
    T_u = int(down(u["n_out"], np.uint32, (1,))[0])
    assert T == len(rx) <= max_out, (T, len(rx))
    seg, segp = down(a["seg"], rc.po.RX_SEG, (max_out,)), down(a["segp"], np.uint8, (max_out, stride))
    assert np.array_equal(seg["hdr"][:T], rx["hdr"])
    assert np.array_equal(seg["fec_id"][:T], rx["fec_id"]) and not seg["reserved"][:T].any()
    assert np.array_equal(segp[:T, :capacity], rxp[:, :capacity])
    assert (seg[T:].view(np.uint8) == dc.FILL).all() and (segp[T:] == dc.FILL).all()
    assert (segp[:T, rc.cd16(capacity):] == dc.FILL).all()
    # all six outputs against the rule over the oracle's ragged tables
    reg, rows_, osh, ohd, oix = _capability_tables(o, cap, Es)
    assert rows_ == counts
    assert np.array_equal(down(a["oix"], np.uint8, (S,)), oix)
    x = we.each_from_tables("capability-chain", plans, [G] * NP, groups, G, fec_id0, reg["shape_of"], reg["rank_of"],
                            [s["group_of"] for s in reg["sec"]], capacity, stride, Es, osh, ohd, oix, max_out)
    got = {"seg": seg, "seg_payload": segp, "first_of": down(a["first_of"], np.uint32, (G + 1,)),
           "n_out": down(a["n_out"], np.uint32, (1,))}
    dc.compare(got, we.deliver_each_ref(x, dc.new_outputs(x)), f"{NAME} capability chain")
    # strictly more than the parent's uniform call can deliver
    assert T_u == 6 + 3 * E_u and T > T_u, (T, T_u)
