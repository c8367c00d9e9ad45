"""rfec_recover_indexed_matrix_wide_out: the one-launch indexed decode of the
sender's full row + column plan of any k = 6..128 (k_decode_matrix_wide: the
shape taken at run time, masks of two words), an entry point beside
rfec_recover_indexed_out and rfec_recover_indexed_matrix_out, whose answers it
leaves alone.  On the CPU: the declaration and binding, the argument checks and
the plan refusals without a device, the case set's census against the reference
with the exact model held to it on every group, and the self-tests that each
comparison can fail.  On the GPU: the exhaustive erasure-pattern sweeps of
k = 6..16, the wide shapes at two loss rates clean and tampered, the constructed
staircases, the geometry cases, the empty pool, and the mixed window from
datagrams to rfec_recover_deliver's list (matrix_wide_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import deliver_cases as dc
import indexed_cases as ic
import indexed_matrix_cases as imc
import matrix_wide_cases as mw
import pattern_cases as pc
import regroup_cases as rc
import shapes_cases as sc

NAME, METHOD = "rfec_recover_indexed_matrix_wide_out", "recover_indexed_matrix_wide_out"
SWEEPS = [(k, "s16") for k in pc.KS] + [(k, "s48") for k in pc.S48_KS]
WIDE = [(k, v) for k in mw.SHAPES for v in mw.VARIANTS]


@pytest.fixture(scope="module")
def wide_inputs(oracle1000):
    """Every wide case's pool, map, tables and reference outputs, computed once and left unchanged."""
    cache = {}

    def get(k, rate, variant, E):
        key = (k, rate, variant, E)
        if key not in cache:
            x = mw.wide_case(oracle1000, k, rate, variant, E)
            cache[key] = (x, ic.reference(oracle1000, x))
        return cache[key]

    return get


@pytest.fixture(scope="module")
def other_inputs(oracle1000):
    """The staircases' and the geometry cases', likewise."""
    cache = {}

    def get(key):
        if key not in cache:
            x = mw.staircase_case(oracle1000, key[1]) if key[0] == "stairs" else mw.geometry_case(oracle1000, key)
            cache[key] = (x, ic.reference(oracle1000, x))
        return cache[key]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_wide_call_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert NAME in fec.header_functions() and NAME in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, NAME) and hasattr(lib, METHOD)
    assert fec._SIGS[NAME] == fec._SIGS["rfec_recover_indexed_matrix_out"]  # the same signature
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7


# -- CPU: argument checks ----------------------------------------------------------------------------------------------
P = dict(rows=0x10000, src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002,
         parity_present=0x70008, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001)
IN_ORDER = ("hdr", "present", "meta", "fec_size", "parity_present", "recovered")


def _call(product, plan, groups=4, stride=1216, capacity=1200, n_rows=100, per_group=3, **ptrs):
    from razor_amd.fec import as_plan
    p = dict(P, **ptrs)
    r = getattr(product.lib, NAME)(None if plan is None else C.byref(as_plan(plan)), groups, stride, capacity,
                                   p["rows"], n_rows, p["src_of"], *(p[n] for n in IN_ORDER), per_group,
                                   p["out_shards"], p["out_hdr"], p["out_index"], None)
    return r, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "stride-0": (dict(stride=0, capacity=0), "multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity"),
    "per-group-0": (dict(per_group=0), "per_group"),
    "per-group-k1": (dict(per_group=41), "per_group"),
    # groups * per_group * CD = 2^31 exactly (CD = 64 at capacity 1024)
    "lanes-2g": (dict(groups=1 << 22, per_group=8, stride=1024, capacity=1024), "too large"),
    **{f"null-{name}": ({name: None}, "NULL") for name in P},
    **{f"{name}-8": ({name: P[name] + 8}, "16-byte") for name in ("rows", "out_shards")},
    **{f"{name}-4": ({name: P[name] + 4}, "8-byte") for name in ("present", "parity_present", "recovered")},
    **{f"{name}-2": ({name: P[name] + 2}, "4-byte") for name in ("src_of", "hdr", "meta", "out_hdr")},
    "fec_size-1": (dict(fec_size=P["fec_size"] + 1), "2-byte"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_wide_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, mw.wide_plan(oracle1000, 40), **kw)
    assert r == -1 and msg in err, (r, err)


def test_wide_checks_in_order(product, oracle1000):
    """rfec_recover_indexed_matrix.c's order: plan, shape, stride, capacity, per_group, the lane bound, the
    groups == 0 return, NULLs, alignments (16, 8, 4, 2 bytes) -- each call breaks the named argument and every one
    after it, and the named one is what the error speaks of."""
    plan = mw.wide_plan(oracle1000, 40)
    refused = mw.REFUSED["rows_only40"](oracle1000)
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


def test_wide_rejects_plan(product, oracle1000):
    r, err = _call(product, None)
    assert r == -1 and "plan is NULL" in err, (r, err)
    r, err = _call(product, rc._hand_plan(129, 1, 129, []), per_group=1)
    assert r == -1 and "out of range" in err, (r, err)
    plan = mw.wide_plan(oracle1000, 40)
    plan.line[2].first, plan.line[2].count = 36, 7  # members 36..42 of k = 40
    r, err = _call(product, plan)
    assert r == -1 and "beyond k" in err, (r, err)


@pytest.mark.parametrize("name", sorted(mw.REFUSED))
def test_wide_refuses_other_plans(product, oracle1000, name):
    """A row layout, a strip plan, a hand-made plan, a full matrix in rows of another width than the planner's, rows
    only, columns only and k = 5: RFEC_EINVAL, the error says it is the plan and names the call that takes it."""
    plan = mw.REFUSED[name](oracle1000)
    r, err = _call(product, plan, per_group=1)
    assert r == -1 and "plan" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plan, per_group=1, groups=0, **{n: None for n in P})
    assert r == -1 and "plan" in err, (r, err)  # a value check: it comes before groups == 0


@pytest.mark.parametrize("pf", (10, 80, 255))
def test_wide_accepts_every_sender_plan(product, oracle1000, pf):
    """Every k = 6..128 of rfec_plan_from_fraction(k, pf, ROWS | COLS): past the plan and the value checks (a NULL
    pointer is what is refused).  Nothing existing changes its answer: rfec_recover_indexed_matrix_out takes exactly
    k = 6..16 of them."""
    lines = set()
    for k in range(6, 129):
        plan = oracle1000.plan_from_fraction(k, pf, 3)
        ours = product.plan_from_fraction(k, pf, 3)
        assert bytes(plan)[:8] == bytes(ours)[:8] and plan.n_lines == ours.n_lines
        r, err = _call(product, plan, src_of=None)
        assert r == -1 and "NULL" in err, (k, r, err)
        assert (product.packed_matrix_stride(plan, 1) != 0) == (k <= 16)
        lines.add(plan.n_lines)
    assert max(lines) == 23
    for k, (rows, col, n) in mw.SHAPES.items():
        plan = mw.wide_plan(oracle1000, k)
        assert (plan.row, plan.col, plan.n_lines) == (rows, col, n), (k, plan.row, plan.col, plan.n_lines)


def test_wide_existing_entries_keep_their_answers(product, oracle1000):
    """rfec_recover_indexed_matrix_out still refuses k = 17, rfec_recover_indexed_shapes_out a section of it."""
    from razor_amd.fec import as_plan
    plan = mw.wide_plan(oracle1000, 17)
    r = product.lib.rfec_recover_indexed_matrix_out(C.byref(as_plan(plan)), 4, 1216, 1200, P["rows"], 100, P["src_of"],
                                                    *(P[n] for n in IN_ORDER), 3, P["out_shards"], P["out_hdr"],
                                                    P["out_index"], None)
    assert r == -1 and "rfec_recover_indexed_out" in product.lib.rfec_last_error().decode()
    sec = dict(cap=4, **{name: P.get(name, 0x20004) for name in sc.SECTION})
    with pytest.raises(Exception) as e:
        product.recover_indexed_shapes_out([plan], [sec], [4], 1216, 1200, P["rows"], 100, P["recovered"], 3,
                                           P["out_shards"], P["out_hdr"], P["out_index"], None)
    assert "rfec_recover_indexed_out" in str(e.value)


def test_wide_zero_groups_and_device(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL.  An empty pool needs no rows; meta and fec_size are
    never optional (these plans have lines).  Without a device a valid call fails past every check, at the launch."""
    plan = mw.wide_plan(oracle1000, 100)
    r, _ = _call(product, plan, groups=0, **{name: None for name in P})
    assert r == 0
    r, err = _call(product, plan, groups=0, per_group=101, **{name: None for name in P})
    assert r == -1 and "per_group" in err  # the value checks come first
    for kw in (dict(n_rows=0, rows=None), {}):
        r, err = _call(product, plan, **kw, src_of=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, plan, **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: the case set -------------------------------------------------------------------------------------------------
def _prefilled(out, x):
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


def _add(seen, c):
    for key, v in c.items():
        seen[key] = max(seen.get(key, 0), v) if key == "max_steps" else seen.get(key, 0) + v


def test_wide_cases_cover_their_conditions(oracle1000, wide_inputs, other_inputs):
    """From the reference alone (the oracle over the gathered batch), with the exact two-word model held to its
    recovered masks on every group (census): the GPU cases, taken together, hold groups with a row firing at once,
    with a column firing at once and with a cascade, schedules of more than 8 and of more than 16 steps, a refused
    line after which the peel goes on, erased or recovered bits in the second mask word, and an unrecoverable erasure
    between delivered slots; every wide case recovers a segment; the staircases have exactly their lengths."""
    seen, per_shape = {}, {}
    for k in mw.SHAPES:
        for rate in mw.RATES:
            for variant in mw.VARIANTS:
                x, ref = wide_inputs(k, rate, variant, k)
                c = mw.census(x, ref)
                assert c["recovered"], (k, rate, variant)
                _add(seen, c)
                _add(per_shape.setdefault(k, {}), c)
                if variant == "tampered":
                    assert c["refused_reschedules"], (k, rate)
    for k in mw.SHAPES:  # every shape on its own: both kinds of line at once, a cascade, a 0xFF slot between two
        for key in ("row_at_once", "col_at_once", "cascade", "hole_between"):
            assert per_shape[k][key], (k, key, per_shape[k])
        assert bool(per_shape[k]["word2"]) == (k > 64), (k, per_shape[k])
    for k in (100, 128):
        x, ref = other_inputs(("stairs", k))
        c = mw.census(x, ref)
        _add(seen, c)
        lens = [int((row != 0xFF).sum()) for row in ref[2]]
        assert lens == [L for _, L, _ in x.specs], (k, lens)
        assert c["row_at_once"] == c["col_at_once"] == len(x.specs) // 2  # one way and mirrored
        assert c["cascade"] == sum(lens) - len(x.specs) and c["word2"] == (len(x.specs) if k == 128 else 6)
    assert seen["max_steps"] == 19 and seen["steps_gt16"] >= 4 and seen["steps_gt8"] >= 8, seen
    for c in mw.GEOMETRY:
        x, ref = other_inputs(c)
        cc = mw.census(x, ref)
        assert cc["recovered"], c
        _add(seen, cc)
    for key in ("row_at_once", "col_at_once", "cascade", "steps_gt8", "steps_gt16", "refused_reschedules", "word2",
                "hole_between"):
        assert seen[key], (key, seen)
    # the geometry set: CD = 1, 2 and 75, the checker blocks' edges, a sparse pool
    assert {rc.cd16(mw.GEOMS[c[1]][0]) // 16 for c in mw.GEOMETRY} == {1, 2, 75}
    n = mw.CHECK_GROUPS
    assert {c[2] for c in mw.GEOMETRY} >= {n - 1, n, n + 1, 2 * n + 1}
    assert {c[0] for c in mw.GEOMETRY} == {17, 65} and any(c[4] for c in mw.GEOMETRY)
    x, _ = other_inputs(next(c for c in mw.GEOMETRY if c[4]))
    assert (x.src_of[x.src_of != ic.NONE] > 65535).any()


def test_wide_reference_passes_behind_the_arena(oracle1000, wide_inputs, other_inputs):
    """With the oracle behind the same arena (RefIndexed) a case of each kind passes the comparison."""
    eng = ic.RefIndexed(oracle1000)
    for x, ref in (wide_inputs(65, 0.15, "tampered", 65), other_inputs(("stairs", 128)),
                   other_inputs(mw.GEOMETRY[1])):
        ic.compare(eng.run(x), _prefilled(ref, x), x, x.case[0])


@pytest.mark.parametrize("wrong", mw.WRONG)
def test_wide_comparison_catches_each_bent_result(oracle1000, wide_inputs, wrong):
    """Each bent result (matrix_wide_cases.bent: a cascade's intermediate left out, the second mask word dropped,
    the columns tried before the rows, a flipped byte, a wrong out_index) fails the comparison on the tampered
    k = 100 case at the higher loss rate."""
    x, ref = wide_inputs(100, 0.15, "tampered", 100)
    with pytest.raises(AssertionError):
        ic.compare(mw.bent(oracle1000, x, ref, wrong), ref, x, wrong)
    ic.compare(ref, ref, x, "the reference against itself")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


def _run_both(gpu_lib, x, ref, what, old_path=None):
    """The new entry == the reference and == rfec_recover_indexed_out on the same arena inputs; the tag; the arena
    checks its guards and every input after each call."""
    eng = mw.GpuIndexedWide(gpu_lib)
    got = eng.run(x)
    assert eng.last_path == (mw.WIDE | x.k << 8), f"{what}: path {eng.last_path:#x}"
    if ref is not None:
        ic.compare(got, ref, x, f"{NAME} {what}")
    old = ic.GpuIndexed(gpu_lib)
    theirs = old.run(x)
    assert (old.last_path & 0xFF) == ic.PEEL_REPLAY, hex(old.last_path)
    ic.compare(got, theirs, x, f"{NAME} against rfec_recover_indexed_out {what}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("k,geom", SWEEPS, ids=[f"k{k}-{g}" for k, g in SWEEPS])
def test_wide_erasure_patterns_gpu(gpu_lib, oracle1000, k, geom, variant):
    """Every erasure pattern of one sweep (k = 6..16) through the new entry at per_group 1, 3, 4, 5 and k: masks,
    out_index, header records and slots equal the expected ones (clean: the model's mask and the original group;
    tampered: the oracle's), the tails hold the pre-fill, the tag is k_decode_matrix_wide's, and the four outputs
    equal rfec_recover_indexed_matrix_out's byte for byte."""
    sw = pc.sweep(oracle1000, k, geom, variant)
    for E in pc.PER_GROUP(k):
        x = pc.indexed_inputs(sw, E)
        eng = mw.GpuIndexedWide(gpu_lib)
        got = eng.run(x)
        assert eng.last_path == (mw.WIDE | k << 8), f"{sw.name()} E={E}: path {eng.last_path:#x}"
        pc.check_dense(sw, got, E, f"{sw.name()} indexed matrix wide", fill=ic.FILL)
        old = imc.GpuIndexedMatrix(gpu_lib)
        theirs = old.run(x)
        assert old.last_path == (imc.MATRIX | k << 8)
        ic.compare(got, theirs, x, f"{sw.name()} E={E} against rfec_recover_indexed_matrix_out")


@pytest.mark.gpu
@pytest.mark.parametrize("k,variant", WIDE, ids=[f"k{k}-{v}" for k, v in WIDE])
def test_wide_shapes_gpu(gpu_lib, wide_inputs, k, variant):
    """200 groups of one wide shape with independent loss of members and parities at 3 % and at 15 %, clean or with
    one tampered header per group, at per_group 1, 4, 9, 17 and k."""
    for rate in mw.RATES:
        for E in mw.PER_GROUP(k):
            x, ref = wide_inputs(k, rate, variant, E)
            _run_both(gpu_lib, x, ref, f"k={k} rate {rate} {variant} E={E}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", (100, 128))
def test_wide_staircases_gpu(gpu_lib, oracle1000, other_inputs, k):
    """Constructed staircases: every step reads the previous step's result, starting in a column and (mirrored) in a
    row; lengths 2, 8, 9, 16, 17 and 19 at k = 100, and at k = 128 across bits 63 / 64.  At per_group k and at
    per_group 10, which cuts the longer staircases short (only erased segments of rank < per_group are targets)."""
    x, ref = other_inputs(("stairs", k))
    _run_both(gpu_lib, x, ref, f"staircases k={k}")
    y = mw.staircase_case(oracle1000, k, 10)
    _run_both(gpu_lib, y, ic.reference(oracle1000, y), f"staircases k={k} E=10")


@pytest.mark.gpu
@pytest.mark.parametrize("c", mw.GEOMETRY, ids=lambda c: f"k{c[0]}-{c[1]}-G{c[2]}-E{c[3]}{'-sparse' if c[4] else ''}")
def test_wide_geometry_gpu(gpu_lib, other_inputs, c):
    """CD = 1, 2 (a tail) and 75, the checker blocks' and the payload blocks' edges, a sparse pool with row indices
    above 65,535; the out slots' tails, the guards and every input as before the call."""
    x, ref = other_inputs(c)
    _run_both(gpu_lib, x, ref, str(c))


@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 65))
def test_wide_empty_pool_and_zero_groups_gpu(gpu_lib, oracle1000, k):
    """n_rows == 0 with rows NULL and all-absent tables over 600 groups (three checker blocks, no payload block):
    recovered is 0, every out_index 0xFF, no out slot byte is written and the guards are intact (the arena's check).
    groups == 0 with NULL pointers returns at once."""
    x = mw.empty_pool_inputs(oracle1000, k)
    eng = mw.GpuIndexedWide(gpu_lib)
    sh, hd, ix, rec = eng.run(x)
    assert eng.last_path == (mw.WIDE | k << 8)
    assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all()
    gpu_lib.recover_indexed_matrix_wide_out(x.plan, 0, x.stride, x.capacity, *([None] * 1), 0, *([None] * 7), 3,
                                            None, None, None, None)


@pytest.mark.gpu
def test_wide_gpu_checks_can_fail(gpu_lib, oracle1000, other_inputs):
    """Two present members' map words swapped in the arena before the call: the comparison fails (both entries stay
    valid rows)."""
    x, ref = other_inputs(mw.GEOMETRY[0])
    eng = mw.GpuIndexedWide(gpu_lib)
    eng.mutate, _ = ic.swap_two_members(oracle1000, x, ref)
    got = eng.run(x)
    with pytest.raises(AssertionError):
        ic.compare(got, ref, x, "swapped map words")


@pytest.mark.gpu
def test_wide_window_chain_gpu(gpu_lib, oracle1000):
    """A mixed window of 60 groups from fec_id 65520 -- runs of five k = 10 groups (a P-frame's 3 x 4 matrix) and of
    five k = 40 groups (an I-frame's 6 x 7) alternating, two segments lost in every group and a parity in every
    third, the datagrams shuffled: rfec_wire_parse, one rfec_wire_regroup_shapes with the k = 40 plan last,
    rfec_recover_indexed_shapes_out with groups[last] = 0, the new entry for the last section with its outputs at
    first[last], and rfec_recover_deliver with groups[last] = min(counts, cap) -- five calls on one stream with no
    synchronisation in between.  The list equals deliver_ref over the oracle's decode of each run's batch with the
    same losses, all six outputs; the k = 40 groups' entries are the reference's recovered segments."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0, run = 60, 4, 65520, 5
    capacity, stride = sc.GEOMS["c20"]
    plans = [ic.PLANS["full3x4k10"](oracle), mw.wide_plan(oracle, 40)]
    rng = np.random.default_rng(zlib.crc32(b"matrix-wide-window"))
    shape = (np.arange(G) // run) % 2
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    dg_l, dl_l, exp = [], [], [[], []]
    for g0 in range(0, G, run):
        p = int(shape[g0])
        plan = plans[p]
        k, n = plan.k, plan.n_lines
        b = rc.sender_batch(oracle, plan, run, rc.fec_id_of(fec_id0, g0), capacity, stride, rng,
                            (5000 + (g0 + np.arange(run, dtype=np.uint64)) * 140).astype(np.uint32))
        assert n and not b.status.any()
        lost = np.zeros(run * (k + n), bool)
        lost[(np.arange(run)[:, None] * k + np.stack([rng.choice(k, 2, replace=False) for _ in range(run)])).reshape(-1)] = True
        for j in range(run):
            if (g0 + j) % 3 == 0:
                lost[run * k + j * n + int(rng.integers(0, n))] = True
        present = np.zeros((run, 2), np.uint64)
        for j, i in zip(*np.nonzero(~lost[:run * k].reshape(run, k))):
            present[j, i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        pp = np.zeros(run, np.uint64)
        for j, l in zip(*np.nonzero(~lost[run * k:].reshape(run, n))):
            pp[j] |= np.uint64(1) << np.uint64(l)
        exp[p].append(oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp, capacity,
                                               E))
        dg_l.append(b.dgram[~lost])
        dl_l.append(b.dlen[~lost])
    ds = dg_l[0].shape[1]
    assert all(d.shape[1] == ds for d in dg_l)
    order = rng.permutation(sum(len(d) for d in dg_l))
    dgram, dlen = np.concatenate(dg_l)[order], np.concatenate(dl_l)[order].astype(np.uint16)
    N = len(dgram)
    counts = [int((shape == p).sum()) for p in range(2)]
    rank = np.zeros(G, np.uint32)
    for p in range(2):
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
    w, secs = sc.shapes_of(plans, [G] * 2, G, N)
    win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
    tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
           for s in secs]
    sections = [dict(cap=G, **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(2)]
    groups = [min(c, G) for c in counts]
    first = [0, groups[0], groups[0] + groups[1]]
    total, max_out = first[2], 256
    rec_, osh, ohd, oix = zeros(total * 16, 0xEE), zeros(total * E * stride, 0x3C), zeros(total * E * 20, 0x3C), \
        zeros(total * E, 0x3C)
    seg, segp = zeros(max_out * 24, dc.FILL), zeros(max_out * stride, dc.FILL)
    first_of, n_out = zeros((G + 1) * 4, dc.FILL), zeros(4, dc.FILL)
    ws = zeros(lib.recover_deliver_workspace_size(G), 0x11)
    # five calls, one stream, no synchronisation
    lib.wire_parse(N, ds, d_dg.data_ptr(), d_dl.data_ptr(), stride, capacity, recs.data_ptr(), rows.data_ptr(), st)
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    lib.recover_indexed_shapes_out(plans, sections, [groups[0], 0], stride, capacity, rows.data_ptr(), N,
                                   rec_.data_ptr(), E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), st)
    f = first[1]
    t40 = tab[1]
    lib.recover_indexed_matrix_wide_out(plans[1], groups[1], stride, capacity, rows.data_ptr(), N,
                                        *(t40[name].data_ptr() for name in ("src_of", "hdr", "present", "meta",
                                                                            "fec_size", "parity_present")),
                                        rec_.data_ptr() + 16 * f, E, osh.data_ptr() + f * E * stride,
                                        ohd.data_ptr() + f * E * 20, oix.data_ptr() + f * E, st)
    assert int(lib.lib.rfec_indexed_last_path()) == (mw.WIDE | 40 << 8)
    lib.recover_deliver(plans, sections, groups, G, fec_id0, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                        stride, capacity, E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), max_out,
                        seg.data_ptr(), segp.data_ptr(), first_of.data_ptr(), n_out.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(down(win["shape_of"], np.uint8, (G,)), shape)
    assert np.array_equal(down(win["rank_of"], np.uint32, (G,)), rank)
    e_sh = np.concatenate([np.concatenate([e[0] for e in exp[p]]) for p in range(2)])
    e_hd = np.concatenate([np.concatenate([e[1] for e in exp[p]]) for p in range(2)])
    e_ix = np.concatenate([np.concatenate([e[2] for e in exp[p]]) for p in range(2)])
    e_rec = np.concatenate([np.concatenate([e[3] for e in exp[p]]) for p in range(2)])
    assert np.array_equal(down(rec_, np.uint64, (total, 2)), e_rec)
    assert np.array_equal(down(oix, np.uint8, (total, E)), e_ix)
    group_of = []
    for p in range(2):
        go = np.full(G, sc.NONE, np.uint32)
        go[:counts[p]] = np.nonzero(shape == p)[0]
        group_of.append(go)
    x = dc.from_tables("wide-window", plans, [G] * 2, groups, G, fec_id0, shape, rank, group_of, capacity, stride, E,
                       e_sh, e_hd, e_ix, max_out)
    ref = dc.deliver_ref(x, dc.new_outputs(x))
    got = {"seg": down(seg, rc.po.RX_SEG, (max_out,)), "seg_payload": down(segp, np.uint8, (max_out, stride)),
           "first_of": down(first_of, np.uint32, (G + 1,)), "n_out": down(n_out, np.uint32, (1,))}
    dc.compare(got, ref, f"{NAME} window chain")
    dc.check_untouched(x, got, "window chain")
    # the k = 40 groups deliver: two lost segments in each, every one recovered unless its lines' parities are gone
    fo = got["first_of"]
    n40 = sum(int(fo[g + 1] - fo[g]) for g in range(G) if shape[g] == 1)
    assert n40 == int((e_ix[first[1]:] != 0xFF).sum()) and n40 >= 2 * counts[1] - 4 and x.T == int(got["n_out"][0])
