"""rfec_recover_indexed_matrix_out: the one-launch indexed decode of the sender's
full row + column plans of k = 6..16 (k_decode_matrix_indexed), an entry point
beside rfec_recover_indexed_out, whose dispatch it leaves alone.  On the CPU: the
declaration and binding, the argument checks and the plan refusals without a
device, and the case set's census against the reference.  On the GPU: the
exhaustive erasure-pattern sweep and the geometry cases through the new entry,
bit-exact against the reference and against rfec_recover_indexed_out on the same
inputs, the empty pool, the self-test that the comparison can fail, and a mixed
window (indexed_matrix_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import indexed_cases as ic
import indexed_matrix_cases as imc
import pattern_cases as pc
import regroup_cases as rc
import shapes_cases as sc

NAME, METHOD = "rfec_recover_indexed_matrix_out", "recover_indexed_matrix_out"
SWEEPS = [(k, "s16") for k in pc.KS] + [(k, "s48") for k in pc.S48_KS]


@pytest.fixture(scope="module")
def inputs(oracle1000):
    """Every case's pool, map, tables and reference outputs, computed once and left unchanged."""
    cache = {}

    def get(c):
        if c not in cache:
            x = ic.make_inputs(oracle1000, c)
            cache[c] = (x, ic.reference(oracle1000, x))
        return cache[c]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_indexed_matrix_call_is_declared_and_bound(product, product1200):
    from razor_amd import fec
    assert NAME in fec.header_functions() and NAME in fec._SIGS
    for lib in (product, product1200):
        assert hasattr(lib.lib, NAME) and hasattr(lib, METHOD)
        assert hasattr(lib.lib, "rfec_indexed_last_path")
    assert len(fec._SIGS[NAME][1]) == len(fec._SIGS["rfec_recover_indexed_out"][1]) - 1  # no workspace
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


def _bad_args():
    """test_recover_indexed.py's BAD_ARGS but for the workspace, which is not an argument here."""
    import test_recover_indexed as tri
    bad = {name: v for name, v in tri.BAD_ARGS.items() if "workspace" not in name}
    assert len(bad) == len(tri.BAD_ARGS) - 2  # null-workspace and workspace-8
    return bad


BAD_ARGS = _bad_args()


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_indexed_matrix_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, ic.PLANS["full3x4k10"](oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_indexed_matrix_lane_bound_edge(product, oracle1000):
    """One lane below the bound passes the value checks (then a NULL pointer is what is refused); CD rounds up; and
    the checker's lanes: 2^30 groups are 2^32 of them, refused after the pointers, one group fewer passes every
    check."""
    plan = ic.PLANS["full3x4k10"](oracle1000)
    r, err = _call(product, plan, groups=(1 << 22) - 1, per_group=8, stride=1024, capacity=1024, rows=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, plan, groups=1 << 22, per_group=8, stride=1024, capacity=1009, rows=None)
    assert r == -1 and "too large" in err, (r, err)
    r, err = _call(product, plan, groups=1 << 30, per_group=1, stride=16, capacity=16)
    assert r == -1 and "too large" in err and "checker" in err, (r, err)
    r, err = _call(product, plan, groups=1 << 30, per_group=1, stride=16, capacity=16, src_of=None)
    assert r == -1 and "NULL" in err, (r, err)  # the pointers come first
    if not torch.cuda.is_available():
        r, err = _call(product, plan, groups=(1 << 30) - 1, per_group=1, stride=16, capacity=16)
        assert r == -2 and "launch" in err, (r, err)


def test_indexed_matrix_rejects_plan(product, oracle1000):
    r, err = _call(product, None)
    assert r == -1 and "plan is NULL" in err, (r, err)
    r, err = _call(product, rc._hand_plan(129, 1, 129, []), per_group=1)
    assert r == -1 and "out of range" in err, (r, err)
    plan = ic.PLANS["full3x4k10"](oracle1000)
    plan.line[2].first, plan.line[2].count = 8, 4  # members 8..11 of k = 10
    r, err = _call(product, plan)
    assert r == -1 and "beyond k" in err, (r, err)


@pytest.mark.parametrize("name", sorted(imc.REFUSED))
def test_indexed_matrix_refuses_other_plans(product, oracle1000, name):
    """Every plan that is not the sender's full matrix of k = 6..16 is RFEC_EINVAL, the error says it is the plan and
    names the call that takes it; rfec_packed_matrix_stride(plan, 1) is the predicate."""
    plan = imc.REFUSED[name](oracle1000)
    assert product.packed_matrix_stride(plan, 1) == 0
    r, err = _call(product, plan, per_group=1)
    assert r == -1 and "plan" in err and "rfec_recover_indexed_out" in err, (r, err)
    r, err = _call(product, plan, per_group=1, groups=0, **{n: None for n in P})
    assert r == -1 and "plan" in err, (r, err)  # a value check: it comes before groups == 0


@pytest.mark.parametrize("k", pc.KS)
def test_indexed_matrix_accepts_every_sender_plan(product, oracle1000, k):
    plan = pc.full_plan(oracle1000, k)
    assert product.packed_matrix_stride(plan, 1) != 0
    r, err = _call(product, plan, src_of=None)
    assert r == -1 and "NULL" in err, (r, err)


def test_indexed_matrix_zero_groups_and_device(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL.  An empty pool needs no rows; meta and fec_size are
    never optional (these plans have lines).  Without a device a valid call fails past every check, at the launch."""
    plan = ic.PLANS["full3x4k10"](oracle1000)
    r, _ = _call(product, plan, groups=0, **{name: None for name in P})
    assert r == 0
    r, err = _call(product, plan, groups=0, per_group=11, **{name: None for name in P})
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


def test_indexed_matrix_cases_cover_their_conditions(oracle1000, inputs):
    """With the oracle behind the same arena (RefIndexed) every case passes the comparison, and from the
    reference's own outputs the set as a whole holds a recovered segment (every case), a cascade, a line refused by
    the header checks, an out slot left at 0xFF, a group whose winning rows descend, pools with more rows than slots
    and a winning row above 65,535; every plan of the set is one the entry accepts."""
    seen = {}
    eng = ic.RefIndexed(oracle1000)
    for c in imc.CASES:
        x, ref = inputs(c)
        ic.compare(eng.run(x), _prefilled(ref, x), x, ic.case_id(c))
        cond = imc.conditions(x, ref)  # (the refused line as a full matrix shows it: see there)
        assert cond["recovered"], ic.case_id(c)
        for key, v in cond.items():
            seen[key] = seen.get(key, False) or v
    for key in ("recovered", "cascade", "refused_line", "unrecovered_slot", "descending_group", "pool_above_slots",
                "row_above_65535"):
        assert seen[key], (key, seen)
    assert {c[0] for c in imc.CASES} == {"full3x4k10", "full2x3k6", "full4x4k16"}
    assert {c[2] for c in imc.CASES if c[1] == "c15" and c[0] == "full3x4k10"} == {1, 63, 64, 65, 129}
    assert {c[1] for c in imc.CASES} == {"c0", "c15", "c20", "c1000", "c1200"}
    assert any(c[4] for c in imc.CASES)


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("k,geom", SWEEPS, ids=[f"k{k}-{g}" for k, g in SWEEPS])
def test_indexed_matrix_erasure_patterns_gpu(gpu_lib, oracle1000, k, geom, variant):
    """Every erasure pattern of one sweep through the new entry at per_group 1, 3, 4, 5 and k: masks, out_index,
    header records and slots equal the expected ones (clean: the model's mask and the original group; tampered: the
    oracle's), the tails hold the pre-fill, and the tag is that of k_decode_matrix_indexed<k, col>."""
    sw = pc.sweep(oracle1000, k, geom, variant)
    for E in pc.PER_GROUP(k):
        x = pc.indexed_inputs(sw, E)
        eng = imc.GpuIndexedMatrix(gpu_lib)
        got = eng.run(x)
        assert eng.last_path == (imc.MATRIX | k << 8), f"{sw.name()} E={E}: path {eng.last_path:#x}"
        pc.check_dense(sw, got, E, f"{sw.name()} indexed matrix", fill=ic.FILL)


@pytest.mark.gpu
@pytest.mark.parametrize("c", imc.CASES, ids=ic.case_id)
def test_indexed_matrix_gpu(gpu_lib, inputs, c):
    """The product == the reference: recovered, out_index, out_hdr, out_shards over [0, 16 CD) of the recovered
    slots; the out slots' tails, the guards and every input as before the call; and the same four outputs byte for
    byte against rfec_recover_indexed_out on the same arena inputs."""
    x, ref = inputs(c)
    eng = imc.GpuIndexedMatrix(gpu_lib)
    got = eng.run(x)
    assert eng.last_path == (imc.MATRIX | x.k << 8), hex(eng.last_path)
    ic.compare(got, ref, x, f"{NAME} {ic.case_id(c)}")
    old = ic.GpuIndexed(gpu_lib)
    theirs = old.run(x)
    assert old.last_path == (ic.PEEL_REPLAY | 4 << 8), hex(old.last_path)
    ic.compare(got, theirs, x, f"{NAME} against rfec_recover_indexed_out {ic.case_id(c)}")


@pytest.mark.gpu
def test_indexed_matrix_empty_pool_gpu(gpu_lib, oracle1000):
    """n_rows == 0 with rows NULL and all-absent tables: recovered is 0, every out_index 0xFF, no out slot byte is
    written and the guards are intact (the arena's check)."""
    x = imc.empty_pool_inputs(oracle1000)
    eng = imc.GpuIndexedMatrix(gpu_lib)
    sh, hd, ix, rec = eng.run(x)
    assert eng.last_path == (imc.MATRIX | 10 << 8)
    assert not rec.any() and (ix == 0xFF).all() and (sh == ic.FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("c", [imc.CASES[1], imc.CASES[10]], ids=ic.case_id)
def test_indexed_matrix_gpu_checks_can_fail(gpu_lib, oracle1000, inputs, c):
    """Two present members' map words swapped in the arena before the call: the comparison fails (both entries
    stay valid rows)."""
    x, ref = inputs(c)
    eng = imc.GpuIndexedMatrix(gpu_lib)
    eng.mutate, _ = ic.swap_two_members(oracle1000, x, ref)
    got = eng.run(x)
    with pytest.raises(AssertionError):
        ic.compare(got, ref, x, "swapped map words")


@pytest.mark.gpu
def test_indexed_matrix_mixed_window_gpu(gpu_lib, oracle1000):
    """24 groups of three plans (the 3 x 4 matrix among them) at c20, two segments lost per group: one
    rfec_wire_regroup_shapes call; the matrix section decoded by the new entry, the others by
    rfec_recover_indexed_out == every section decoded by rfec_recover_indexed_out."""
    lib, oracle = gpu_lib, oracle1000
    G, E, fec_id0 = 24, 2, 65520
    capacity, stride = sc.GEOMS["c20"]
    names = sc.PLANSETS["decode3"]
    plans = [sc.PLANS[name](oracle) for name in names]
    P = len(plans)
    assert "full3x4k10" in names
    rng = np.random.default_rng(zlib.crc32(b"indexed-matrix-mixed"))
    shape = rng.permutation(np.arange(G) % P)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    recs_l, pay_l = [], []
    for p, plan in enumerate(plans):
        gs = np.nonzero(shape == p)[0]
        k, n = plan.k, plan.n_lines
        b = rc.sender_batch(oracle, plan, len(gs), 1, capacity, stride, rng,
                            (5000 + gs.astype(np.uint64) * 140).astype(np.uint32))
        b.recs["fec_id"] = [rc.fec_id_of(fec_id0, int(g)) for g in np.concatenate([np.repeat(gs, k), np.repeat(gs, n)])]
        lost = np.zeros(len(b.recs), bool)
        lost[(np.arange(len(gs))[:, None] * k + np.stack([rng.choice(k, 2, replace=False) for _ in gs])).reshape(-1)] = True
        recs_l.append(b.recs[~lost])
        pay_l.append(b.pay[~lost])
    order = rng.permutation(sum(len(r) for r in recs_l))
    recs, pay = np.concatenate(recs_l)[order], np.concatenate(pay_l)[order]
    N = len(recs)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    d_recs, d_rows = up(recs), up(pay)
    w, secs = sc.shapes_of(plans, [G] * P, G, N)
    win = {name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in w.items()}
    tab = [{name: zeros(int(np.prod(shp)) * np.dtype(dt).itemsize, sc.FILL) for name, (dt, shp) in s.items()}
           for s in secs]
    sections = [dict(cap=G, **{name: tab[p][name].data_ptr() for name in sc.SECTION}) for p in range(P)]
    lib.wire_regroup_shapes(plans, sections, G, fec_id0, N, d_recs.data_ptr(), capacity,
                            *(win[name].data_ptr() for name in sc.WINDOW), st)
    cw = rc.cd16(capacity)
    recovered = 0
    for p, plan in enumerate(plans):
        outs = []
        for new in (False, True):
            o = (zeros(G * 16, 0xEE), zeros(G * E * stride, 0x3C), zeros(G * E * 20, 0x3C), zeros(G * E, 0x3C))
            args = (plan, G, stride, capacity, d_rows.data_ptr(), N,
                    *(tab[p][name].data_ptr() for name in ("src_of", "hdr", "present", "meta", "fec_size",
                                                           "parity_present")),
                    o[0].data_ptr(), E, o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr())
            if new and names[p] == "full3x4k10":
                lib.recover_indexed_matrix_out(*args, st)
            else:
                ws = zeros(lib.workspace_size(plan, G), 0x11)
                lib.recover_indexed_out(*args, ws.data_ptr(), st)
            torch.cuda.synchronize(dev)
            outs.append(o)
        (rec_a, sh_a, hd_a, ix_a), (rec_b, sh_b, hd_b, ix_b) = outs
        assert torch.equal(rec_a, rec_b) and torch.equal(ix_a, ix_b), names[p]
        ok = ix_a[:G * E] != 0xFF
        assert torch.equal(hd_a[:G * E * 20].view(G * E, 20)[ok], hd_b[:G * E * 20].view(G * E, 20)[ok]), names[p]
        assert torch.equal(sh_a[:G * E * stride].view(G * E, stride)[ok][:, :cw],
                           sh_b[:G * E * stride].view(G * E, stride)[ok][:, :cw]), names[p]
        assert bool((sh_b[:G * E * stride].view(G * E, stride)[:, cw:] == 0x3C).all()), names[p]
        if names[p] == "full3x4k10":
            recovered = int(ok.sum())
    assert recovered >= 8  # the matrix section: 8 groups, two segments lost in each
