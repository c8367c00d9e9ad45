"""rfec_recover_deliver_each: rfec_recover_deliver over the ragged outputs of
rfec_recover_indexed_window_each_out (per_group a host array, section p's rows
per_group[p] out slots each, the sections' slots packed end to end).  On the
CPU: every argument check in its order, the accepted NULLs and the launch
without a device, deliver_each_ref against deliver_cases.deliver_ref at a uniform
E on the existing case set, each bent rule caught by the mixed-E case set, and
the case set's conditions.  On the GPU: the mixed-E cases against
deliver_each_ref over all six outputs, and every case of deliver_cases at its
uniform E byte for byte against rfec_recover_deliver (window_each_cases.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import deliver_cases as dc
import regroup_cases as rc
import window_each_cases as we

NAME = "rfec_recover_deliver_each"


@pytest.fixture(scope="module")
def cases():
    """Every mixed-E case and the rule's outputs for it, computed once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            x = we.make(name)
            cache[name] = (x, we.deliver_each_ref(x, dc.new_outputs(x)))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def uniform_cases():
    cache = {}

    def get(name):
        if name not in cache:
            x = dc.make(name)
            cache[name] = (x, dc.deliver_ref(x, dc.new_outputs(x)))
        return cache[name]

    return get


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(shape_of=0x10001, rank_of=0x20004, out_shards=0x30010, out_hdr=0x40004, out_index=0x50001, seg=0x60004,
         seg_payload=0x70010, first_of=0x80004, n_out=0x90004, workspace=0xA0010)
GROUP_OF = 0xB0004


def _call(product, n=2, groups=(4, 4), caps=None, group_of=None, G=8, fec_id0=7, stride=1216, capacity=1200,
          per_group=(2, 5), max_out=16, n_plans=None, null_plans=False, null_sections=False, plans=None, **ptrs):
    """One raw call on made-up addresses: per_group a tuple (repeated over the plans) or None (NULL)."""
    from razor_amd.fec import as_plan, rfec_plan, rfec_regroup_section
    plans = plans or [dc.hand_plan() for _ in range(n)]
    n = len(plans)
    caps = list(caps) if caps is not None else (list(groups) if groups is not None else [4] * n)
    group_of = list(group_of) if group_of is not None else [GROUP_OF + 0x1000 * p for p in range(n)]
    pa = (rfec_plan * max(n, 1))(*(as_plan(p) for p in plans))
    sa = (rfec_regroup_section * max(n, 1))(*(rfec_regroup_section(cap=caps[p], group_of=group_of[p])
                                             for p in range(n)))
    ga_ = None if groups is None else (C.c_uint32 * max(n, 1))(*groups)
    ea = None if per_group is None else (C.c_uint32 * max(n, 1))(*[per_group[p % len(per_group)] for p in range(n)])
    p = dict(P, **ptrs)
    r = getattr(product.lib, NAME)(None if null_plans else pa, n if n_plans is None else n_plans,
                                   None if null_sections else sa, ga_, G, fec_id0, p["shape_of"], p["rank_of"], stride,
                                   capacity, ea, p["out_shards"], p["out_hdr"], p["out_index"], max_out,
                                   p["seg"], p["seg_payload"], p["first_of"], p["n_out"], p["workspace"], None)
    return r, product.lib.rfec_last_error().decode()


def _bad_plan():
    p = rc._hand_plan(10, 3, 4, [(0, 1, 4, 0), (4, 1, 4, 1), (8, 1, 4, 2)])  # members 8..11 of k = 10
    return [dc.hand_plan(), p]


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
    "null-per-group": (dict(per_group=None), "per_group is NULL"),
    "per-group-0-first": (dict(per_group=(0, 5)), "per_group[0] must be >= 1"),
    "per-group-0-second": (dict(per_group=(2, 0)), "per_group[1] must be >= 1"),
    "groups-above-cap": (dict(groups=(4, 5), caps=(4, 4)), "groups[1] must be <= sections[p].cap"),
    "lanes": (dict(groups=(4, 1 << 22), stride=1024, capacity=1024, per_group=(1, 8)), "window too large"),
    "rows-2^32": (dict(groups=(1 << 31, 1 << 31), stride=16, capacity=16, per_group=(1,)), "window too large"),
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
def test_deliver_each_rejects(product, name):
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, **_kw(kw))
    assert r == -1 and msg in err, (r, err)


def test_deliver_each_checks_in_order(product):
    """Each check comes before the next: plans, n_plans, sections, each plan, window_groups, fec_id0, stride,
    capacity, per_group (NULL, then each section's), groups <= cap, the lanes, the NULL pointers, the alignments."""
    steps = [
        (dict(null_plans=True), "plans is NULL"),
        (dict(n_plans=33), "n_plans"),
        (dict(null_sections=True), "sections is NULL"),
        (dict(plans="bad"), "beyond k"),
        (dict(G=65536), "window_groups"),
        (dict(fec_id0=0), "fec_id0"),
        (dict(stride=1208), "stride"),
        (dict(capacity=1300), "capacity"),
        (dict(per_group=None), "per_group is NULL"),
        (dict(per_group=(2, 0)), "per_group[1] must be >= 1"),
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


def test_deliver_each_lane_bounds(product):
    """S * CD < 2^31 with S the sum of groups[p] * per_group[p]: one lane below the bound passes the value checks
    (then a NULL pointer is what is refused); the bound counts the chunks of work, not the stride; a large section at
    a small per_group passes where the same rows at the other section's per_group would not."""
    r, err = _call(product, groups=((1 << 22) - 1, 0), per_group=(8, 0), stride=1024, capacity=1024, seg=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, groups=(1 << 22, 0), per_group=(8, 0), stride=1024, capacity=1009, seg=None)
    assert r == -1 and "window too large" in err, (r, err)
    r, err = _call(product, groups=(1 << 22, 0), per_group=(8, 0), stride=1024, capacity=1008, seg=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, groups=(1 << 22, 4), per_group=(1, 128), stride=1024, capacity=1024, seg=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, groups=(4, 1 << 22), per_group=(1, 128), stride=1024, capacity=1024, seg=None)
    assert r == -1 and "window too large" in err, (r, err)


def test_deliver_each_accepted_nulls_empty_window_and_device(product):
    """window_groups == 0 touches nothing: every pointer but plans and per_group may be NULL, and the value checks
    still come first.  A section with groups[p] == 0 may carry any per_group[p], 0 included.  Without a device a
    valid call fails past every check, at the launch."""
    nothing = {n: None for n in P}
    r, err = _call(product, G=0, null_sections=True, groups=None, **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, G=0, null_sections=True, groups=None, per_group=(0, 0), **nothing)
    assert r == 0, (r, err)  # (no sections: no per_group is read)
    r, err = _call(product, G=0, group_of=(None, None), **nothing)
    assert r == 0, (r, err)
    r, err = _call(product, G=0, per_group=None, **nothing)
    assert r == -1 and "per_group is NULL" in err, (r, err)
    r, err = _call(product, G=0, per_group=(2, 0), **nothing)
    assert r == -1 and "per_group[1]" in err, (r, err)
    r, err = _call(product, G=0, groups=(4, 5), caps=(4, 4), **nothing)
    assert r == -1 and "groups[1]" in err, (r, err)
    ok = [dict(max_out=0, seg=None, seg_payload=None),
          dict(groups=(0, 0), caps=(4, 4), per_group=(0, 0), group_of=(None, None), out_shards=None, out_hdr=None,
               out_index=None),
          dict(groups=None, caps=(0, 0), per_group=(0, 999), group_of=(None, None), out_shards=None, out_hdr=None,
               out_index=None),
          dict(groups=(0, 4), per_group=(0, 128), group_of=(None, GROUP_OF)), dict(groups=None, caps=(3, 5)), {}]
    for kw in ok:
        r, err = _call(product, **kw, workspace=0xA0008)  # past the NULL checks, at the alignment
        assert r == -1 and "aligned" in err, (kw, r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, **kw)
            assert r == -2 and "launch" in err, (kw, r, err)
    r, err = _call(product, groups=None, caps=(4, 4), group_of=(None, GROUP_OF))  # cap rows: the pointer is wanted
    assert r == -1 and "sections[0].group_of is NULL" in err, (r, err)


# -- CPU: the rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in dc.CASES if n != "big"])
def test_deliver_each_ref_reduces_to_deliver_ref(uniform_cases, name):
    """With every per_group[p] = E, deliver_each_ref is deliver_cases.deliver_ref on the existing case set, all six
    outputs, and each of deliver_cases' bent rules bends it the same way."""
    x, ref = uniform_cases(name)
    y = we.uniform_as_each(x)
    dc.compare(we.deliver_each_ref(y, dc.new_outputs(y)), ref, f"{name} at a uniform E")
    for wrong in dc.WRONG:
        dc.compare(we.deliver_each_ref(y, dc.new_outputs(y), (wrong,)), dc.deliver_ref(x, dc.new_outputs(x), (wrong,)),
                   f"{name} {wrong}")


@pytest.mark.parametrize("wrong", dc.WRONG + we.WRONG_DELIVER)
def test_deliver_each_cases_catch_each_wrong_rule(cases, wrong):
    """Each bent rule -- deliver_cases' five, and o * E with the call's largest E, slot_first taken as first * E[p],
    the neighbouring section's E, the count over the least E -- differs from the rule on at least one case."""
    caught = []
    for name in we.CASES:
        x, ref = cases(name)
        try:
            dc.compare(we.RefDeliverEach((wrong,)).run(x), ref, wrong)
        except AssertionError:
            caught.append(name)
    assert caught, wrong


def test_deliver_each_comparison_can_fail(cases):
    x, ref = cases("G255")
    dc.compare(we.RefDeliverEach().run(x), ref, "the rule itself")
    bent = {k: v.copy() for k, v in ref.items()}
    bent["seg"]["fec_id"][0] ^= 1
    with pytest.raises(AssertionError):
        dc.compare(bent, ref, "one fec_id bent")


def test_deliver_each_cases_cover_their_conditions(cases):
    """The case set holds every condition the GPU tests are there for."""
    x = {name: cases(name)[0] for name in we.CASES}
    for G in (255, 256, 257, 600):
        c = x[f"G{G}"]
        assert c.G == G and c.P == 4 and c.E == [3, 10, 1, 6] and all(c.rows) and c.T > 0
        assert int(c.slot_first[-1]) == sum(r * e for r, e in zip(c.rows, c.E))
        # no later section's slot base is first[p] * E[p]: the bent rules read other slots
        assert all(int(c.slot_first[p]) != int(c.first[p]) * c.E[p] for p in range(1, 4))
    assert x["G1"].G == 1 and x["G1"].T >= 1
    assert dc.launches(256) == 2 and dc.launches(257) == 3
    assert rc.cd16(x["cd1"].capacity) == 16 and rc.cd16(x["cd75"].capacity) == 1200
    T = x["max-T"].T
    assert x["max-T"].max_out == T and x["max-T-1"].max_out == x["max-T-1"].T - 1
    assert x["max-1"].max_out == 1 and x["max-0"].max_out == 0 and x["max-1"].T > 1 and x["max-0"].T > 0
    # holes before, between and after delivered slots in the E = 12 section, among rows that deliver
    c = x["large-E"]
    assert c.E == [2, 12, 3] and c.rows[1] >= 6
    h = c.out_index[int(c.slot_first[1]):int(c.slot_first[2])].reshape(c.rows[1], 12) != we.HOLE
    assert (~h[:, 0] & h.any(1)).any() and (~h[:, -1] & h.any(1)).any()
    assert any(r[0] and r[-1] and not r.all() for r in h) and (~h).all(1).any() and h.all(1).any()
    for w, p in (("first", 0), ("middle", 1), ("last", 3)):
        c = x[f"zero-{w}"]
        assert c.rows[p] == 0 and c.group_of[p] is None and c.counts[p] > 0 and c.T > 0
    assert any(r < n for r, n in zip(x["below-counts"].rows, x["below-counts"].counts))
    assert x["null-groups"].groups is None and x["thirty-two"].P == 32 and len(set(x["thirty-two"].E)) == 5
    s = x["swap"]
    assert s.P == 2 and s.rows[0] == s.rows[1] and s.E == [2, 2] and s.T > 0


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _check_call(eng, G, tag):
    assert eng.last_path == (tag | dc.launches(G) << 8), hex(eng.last_path)
    assert eng.last_launches == dc.launches(G), eng.last_launches


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(we.CASES))
def test_deliver_each_gpu(gpu_lib, cases, name):
    """The product == deliver_each_ref over all six outputs; the guards, every input, the delivered rows' tails and
    the entries at and past min(T, max_out) as before the call (the engine's checks); the tag and the launch count."""
    x, ref = cases(name)
    eng = we.GpuDeliverEach(gpu_lib)
    out = eng.run(x)
    _check_call(eng, x.G, we.DELIVER_EACH)
    dc.compare(out, ref, f"{NAME} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dc.CASES))
def test_deliver_each_equals_deliver_at_uniform_E_gpu(gpu_lib, uniform_cases, name):
    """Every case of deliver_cases with per_group[p] = its E in every section: all six outputs byte for byte those
    of rfec_recover_deliver, and deliver_ref's."""
    x, ref = uniform_cases(name)
    theirs = dc.GpuDeliver(gpu_lib)
    a = theirs.run(x)
    _check_call(theirs, x.G, dc.DELIVER)
    eng = we.GpuDeliverEach(gpu_lib)
    b = eng.run(we.uniform_as_each(x))
    _check_call(eng, x.G, we.DELIVER_EACH)
    dc.compare(b, a, f"{NAME} {name} against rfec_recover_deliver")
    dc.compare(b, ref, f"{NAME} {name}")


@pytest.mark.gpu
def test_deliver_each_gpu_checks_can_fail(gpu_lib, cases):
    """Two sections' group_of pointers swapped in the call: the comparison fails."""
    x, ref = cases("swap")
    out = we.GpuDeliverEach(gpu_lib).run(x, swap=(0, 1))
    with pytest.raises(AssertionError):
        dc.compare(out, ref, "swapped group_of pointers")
