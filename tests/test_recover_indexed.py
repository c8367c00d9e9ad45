"""rfec_recover_indexed_out (the dense decode through a slot map over a row pool)
and rfec_wire_regroup_index (rfec_wire_regroup's tables without the row copy).
On the CPU: the declarations, the argument checks of both calls without a
device, and the case set against the reference and its bent forms.  On the GPU:
both calls against the reference (regroup_ref -> gather by src_of in numpy ->
oracle.recover_batch_out), and the device receive chain composed
(indexed_cases.py)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import indexed_cases as ic
import regroup_cases as rc


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


@pytest.fixture(scope="module")
def regroup_inputs(oracle1000):
    cache = {}

    def get(c):
        if c not in cache:
            x = rc.make_inputs(oracle1000, c)
            cache[c] = (x, rc.ref_outputs(x))
        return cache[c]

    return get


# -- CPU: declared, bound ----------------------------------------------------------------------------------------------
def test_indexed_calls_are_declared_and_bound(product, product1200):
    from razor_amd import fec
    for name, method in (("rfec_wire_regroup_index", "wire_regroup_index"),
                         ("rfec_recover_indexed_out", "recover_indexed_out")):
        assert name in fec.header_functions() and name in fec._SIGS, name
        for lib in (product, product1200):
            assert hasattr(lib.lib, name) and hasattr(lib, method), name
    assert fec.RFEC_ABI_VERSION == 7 and product.lib.rfec_abi_version() == 7
    for lib in (product, product1200):  # the dispatch tag's accessor: exported, not in the public header
        assert hasattr(lib.lib, "rfec_indexed_last_path")
    assert "rfec_indexed_last_path" not in fec.header_functions()


# -- CPU: argument checks, rfec_recover_indexed_out --------------------------------------------------------------------
P = dict(rows=0x10000, src_of=0x20004, hdr=0x30004, present=0x40008, meta=0x50004, fec_size=0x60002,
         parity_present=0x70008, recovered=0x80008, out_shards=0x90000, out_hdr=0xA0004, out_index=0xB0001,
         workspace=0xC0000)
IN_ORDER = ("hdr", "present", "meta", "fec_size", "parity_present", "recovered")


def _call(product, plan, groups=4, stride=1216, capacity=1200, n_rows=100, per_group=3, **ptrs):
    from razor_amd.fec import as_plan
    p = dict(P, **ptrs)
    r = product.lib.rfec_recover_indexed_out(None if plan is None else C.byref(as_plan(plan)), groups, stride,
                                             capacity, p["rows"], n_rows, p["src_of"], *(p[n] for n in IN_ORDER),
                                             per_group, p["out_shards"], p["out_hdr"], p["out_index"], p["workspace"],
                                             None)
    return r, product.lib.rfec_last_error().decode()


BAD_ARGS = {
    "stride-not-16": (dict(stride=1208), "multiple of 16"),
    "stride-0": (dict(stride=0, capacity=0), "multiple of 16"),
    "capacity-above-stride": (dict(capacity=1217), "capacity"),
    "per-group-0": (dict(per_group=0), "per_group"),
    "per-group-k1": (dict(per_group=11), "per_group"),
    # groups * per_group * CD = 2^31 exactly (CD = 64 at capacity 1024)
    "lanes-2g": (dict(groups=1 << 22, per_group=8, stride=1024, capacity=1024), "too large"),
    **{f"null-{name}": ({name: None}, "NULL") for name in P},
    **{f"{name}-8": ({name: P[name] + 8}, "16-byte") for name in ("rows", "out_shards", "workspace")},
    **{f"{name}-4": ({name: P[name] + 4}, "8-byte") for name in ("present", "parity_present", "recovered")},
    **{f"{name}-2": ({name: P[name] + 2}, "4-byte") for name in ("src_of", "hdr", "meta", "out_hdr")},
    "fec_size-1": (dict(fec_size=P["fec_size"] + 1), "2-byte"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGS))
def test_recover_indexed_rejects(product, oracle1000, name):
    kw, msg = BAD_ARGS[name]
    r, err = _call(product, ic.PLANS["rows10x4"](oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_recover_indexed_lane_bound_edge(product, oracle1000):
    """One lane below the bound passes the value checks (then a NULL pointer is what is refused)."""
    plan = ic.PLANS["rows10x4"](oracle1000)
    r, err = _call(product, plan, groups=(1 << 22) - 1, per_group=8, stride=1024, capacity=1024, rows=None)
    assert r == -1 and "NULL" in err, (r, err)
    r, err = _call(product, plan, groups=1 << 22, per_group=8, stride=1024, capacity=1009, rows=None)
    assert r == -1 and "too large" in err, (r, err)  # CD rounds up: capacity 1009 is 64 chunks


def test_recover_indexed_rejects_plan(product, oracle1000):
    r, err = _call(product, None)
    assert r == -1 and "plan is NULL" in err, (r, err)
    r, err = _call(product, rc._hand_plan(129, 1, 129, []), per_group=1)  # above RFEC_MAX_K
    assert r == -1 and "out of range" in err, (r, err)
    plan = ic.PLANS["rows10x4"](oracle1000)
    plan.line[2].first, plan.line[2].count = 8, 4  # members 8..11 of k = 10
    r, err = _call(product, plan)
    assert r == -1 and "beyond k" in err, (r, err)


def test_recover_indexed_zero_groups_and_device(product, oracle1000):
    """groups == 0 touches nothing: every pointer may be NULL.  A plan without lines needs no meta / fec_size, an
    empty pool no rows.  Without a device a valid call fails past every check, at the launch (RFEC_EDEVICE)."""
    plan, k1 = ic.PLANS["rows10x4"](oracle1000), ic.PLANS["k1"](oracle1000)
    r, _ = _call(product, plan, groups=0, **{name: None for name in P})
    assert r == 0
    r, err = _call(product, plan, groups=0, per_group=11, **{name: None for name in P})
    assert r == -1 and "per_group" in err  # the value checks come first
    for pl, kw in ((plan, dict(n_rows=0, rows=None)), (k1, dict(meta=None, fec_size=None, per_group=1)), (plan, {})):
        r, err = _call(product, pl, **kw, src_of=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call(product, pl, **kw)
            assert r == -2 and "launch" in err, (r, err)


# -- CPU: argument checks, rfec_wire_regroup_index ---------------------------------------------------------------------
Q = dict(recs=0x10000, hdr=0x40004, present=0x50008, meta=0x70004, fec_size=0x80002, parity_present=0x90008,
         base_id=0xA0004, src_of=0xB0004, slot_of=0xC0004)


def _call_rx(product, plan, groups=4, fec_id0=7, n=100, capacity=1200, **ptrs):
    from razor_amd.fec import as_plan
    p = dict(Q, **ptrs)
    r = product.lib.rfec_wire_regroup_index(None if plan is None else C.byref(as_plan(plan)), groups, fec_id0, n,
                                            p["recs"], capacity, *(p[name] for name in ic.TABLES), None)
    return r, product.lib.rfec_last_error().decode()


BAD_RX = {
    "fec-id0-0": (dict(fec_id0=0), "fec_id0"),
    "groups-65536": (dict(groups=65536), "groups"),
    "n-2g": (dict(n=0x80000000), "n must be"),
    **{f"null-{name}": ({name: None}, "NULL") for name in Q},
    "recs-8": (dict(recs=Q["recs"] + 8), "16-byte"),
    **{f"{name}-4": ({name: Q[name] + 4}, "8-byte") for name in ("present", "parity_present")},
    **{f"{name}-2": ({name: Q[name] + 2}, "4-byte") for name in ("hdr", "meta", "base_id", "src_of", "slot_of")},
    "fec_size-1": (dict(fec_size=Q["fec_size"] + 1), "2-byte"),
}


@pytest.mark.parametrize("name", sorted(BAD_RX))
def test_wire_regroup_index_rejects(product, oracle1000, name):
    kw, msg = BAD_RX[name]
    r, err = _call_rx(product, rc.PLANS["rows10x4"](oracle1000), **kw)
    assert r == -1 and msg in err, (r, err)


def test_wire_regroup_index_plan_zero_groups_and_device(product, oracle1000):
    r, err = _call_rx(product, None)
    assert r == -1 and "plan is NULL" in err, (r, err)
    r, err = _call_rx(product, rc._hand_plan(129, 1, 129, []))
    assert r == -1 and "out of range" in err, (r, err)
    rows, k1 = rc.PLANS["rows10x4"](oracle1000), rc.PLANS["k1"](oracle1000)
    r, _ = _call_rx(product, rows, groups=0, **{name: None for name in Q})
    assert r == 0
    no_recs, no_lines = dict(recs=None, slot_of=None), dict(meta=None, fec_size=None)
    for plan, kw in ((rows, dict(n=0, **no_recs)), (k1, no_lines), (k1, dict(n=0, **no_recs, **no_lines)), (rows, {})):
        r, err = _call_rx(product, plan, **kw, src_of=None)
        assert r == -1 and "NULL" in err, (r, err)
        if not torch.cuda.is_available():
            r, err = _call_rx(product, plan, **kw)
            assert r == -2 and "launch" in err, (r, err)
    r, err = _call_rx(product, rows, **no_lines)
    assert r == -1 and "NULL" in err, (r, err)


# -- CPU: the case set -------------------------------------------------------------------------------------------------
def test_indexed_cases_cover_their_conditions(inputs):
    """From the reference alone: a recovered segment in every case with lines; over the set an erased slot left
    at 0xFF, a line refused by the header checks, a cascade step that reads a segment recovered earlier (the
    3 x 4 plan), a target of index >= 64, a group whose winning rows lie in descending arrival order, pools with
    more rows than slots and a winning row above 65,535; and the issue's plans, geometries, per_group values and
    group counts."""
    seen = {}
    for c in ic.CASES:
        x, ref = inputs(c)
        cond = ic.conditions(x, ref)
        assert cond["recovered"], ic.case_id(c)
        assert cond["pool_above_slots"], ic.case_id(c)
        for k, v in cond.items():
            seen[k] = seen.get(k, False) or v
        if c[0] == "full3x4k10" and c[2] > 3 and c[3] >= 2:
            assert cond["cascade"], ic.case_id(c)
    assert all(seen.values()) and len(seen) == 8, seen
    assert {c[0] for c in ic.CASES} == {"rows10x4", "rows32x4", "rows12x3", "full3x4k10", "strip65", "strip128",
                                        "hand6", "k2"}
    for p in {c[0] for c in ic.CASES}:
        assert {c[1] for c in ic.CASES if c[0] == p} >= {"c20"} and len({c[1] for c in ic.CASES if c[0] == p}) >= 4, p
    assert {c[1] for c in ic.CASES} == {"c0", "c15", "c20", "c1000", "c1200"}
    assert {c[2] for c in ic.CASES if c[1] in ("c0", "c15")} >= {1, 63, 64, 65, 129, 600}
    for c in ic.CASES:
        assert 1 <= c[3] <= inputs(c)[0].k
    assert {c[3] for c in ic.CASES} >= {1, 2, 3} and all(
        any(c[0] == p and c[3] == inputs(c)[0].k for c in ic.CASES) for p in ic.DEFAULT_PATH)


@pytest.mark.parametrize("wrong", ic.WRONG)
def test_indexed_cases_catch_each_wrong_gather(oracle1000, inputs, wrong):
    """Each bent gather (src_of ignored, the parity read from the member table, rows taken as 16 CD apart, the
    index cut to 16 bits) differs from the reference on at least one case."""
    caught = []
    for c in ic.CASES:
        x, ref = inputs(c)
        try:
            ic.compare(_prefilled(ic.reference(oracle1000, x, (wrong,)), x), _prefilled(ref, x), x, wrong)
        except AssertionError:
            caught.append(ic.case_id(c))
    assert caught, wrong
    if wrong == "trunc16":
        assert all("sparse" in c for c in caught)


def _prefilled(out, x):
    """The oracle's whole-slot result as the call leaves it: the tails hold the pre-fill."""
    sh = out[0].copy()
    sh[:, :, rc.cd16(x.capacity):] = ic.FILL
    return (sh,) + tuple(out[1:])


def test_indexed_arena_checks_can_fail(oracle1000, inputs):
    """The reference behind the arena passes; with two present members' map words swapped before the call the
    comparison fails, and so does it on one byte written into an out slot's tail."""
    x, ref = inputs(ic.CASES[0])
    eng = ic.RefIndexed(oracle1000)
    ic.compare(eng.run(x), _prefilled(ref, x), x, "the reference in an arena")
    eng.mutate, _ = ic.swap_two_members(oracle1000, x, ref)
    with pytest.raises(AssertionError, match="out_shards"):
        ic.compare(eng.run(x), _prefilled(ref, x), x, "swapped map words")
    bad = [a.copy() for a in _prefilled(ref, x)]
    bad[0][0, 0, -1] ^= 1
    with pytest.raises(AssertionError, match="tail was written"):
        ic.compare(tuple(bad), _prefilled(ref, x), x, "a tail byte")


# -- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(product):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return product


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.CASES + [rc.LOOP_CASE], ids=rc.case_id)
def test_wire_regroup_index_gpu(gpu_lib, regroup_inputs, c):
    """The eight tables == regroup_ref's, byte for byte over the pre-fill, with no payload, shards or parity buffer
    in the arena; four launches."""
    x, ref = regroup_inputs(c)
    gpu_lib.timing_events(None, None)
    got = ic.regroup_index_gpu(gpu_lib, x)
    assert gpu_lib.timing_launches() == (4 if x.n else 2)
    ic.compare_tables(got, ref, f"rfec_wire_regroup_index {rc.case_id(c)}")


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [0, 1], ids=["default", "generic"])
@pytest.mark.parametrize("c", ic.CASES, ids=ic.case_id)
def test_recover_indexed_gpu(gpu_lib, inputs, c, tuning):
    """The product == the reference: recovered, out_index, out_hdr, out_shards over [0, 16 CD) of the recovered
    slots; the out slots' tails, the guards and every input as before the call; the path the case means."""
    x, ref = inputs(c)
    eng = ic.GpuIndexed(gpu_lib, tuning=tuning)
    got = eng.run(x)
    assert gpu_lib.get_tuning() == 0
    kind, arg = ic.DEFAULT_PATH[c[0]]
    if tuning:
        kind, arg = ic.PEEL_REPLAY, 4 if max(x.plan.line[l].count for l in range(x.nl)) <= 4 else 8
    assert eng.last_path == (kind | arg << 8), hex(eng.last_path)
    ic.compare(got, ref, x, f"rfec_recover_indexed_out {ic.case_id(c)} tuning {tuning}")


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [0, 1], ids=["default", "generic"])
@pytest.mark.parametrize("c", [ic.CASES[0], ic.CASES[18]], ids=ic.case_id)
def test_recover_indexed_gpu_checks_can_fail(gpu_lib, oracle1000, inputs, c, tuning):
    """Two present members' map words swapped in the arena between the map build and the call: the comparison
    fails (both entries stay valid rows)."""
    x, ref = inputs(c)
    eng = ic.GpuIndexed(gpu_lib, tuning=tuning)
    eng.mutate, _ = ic.swap_two_members(oracle1000, x, ref)
    got = eng.run(x)
    with pytest.raises(AssertionError):
        ic.compare(got, ref, x, "swapped map words")


@pytest.mark.gpu
@pytest.mark.parametrize("pname,gname", [("rows10x4", "c1200"), ("full3x4k10", "c1000")])
def test_indexed_chain_composed_gpu(oracle1000, oracle1200, product, product1200, pname, gname):
    """rfec_wire_encode_send -> shuffled and lost with torch -> rfec_wire_parse -> rfec_wire_regroup_index ->
    rfec_recover_indexed_out on device buffers == oracle.recover_batch_out on the sender's batch with the same
    losses, and == the existing chain (rfec_wire_regroup + rfec_recover_batch_out) on the same parse output."""
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    lib, oracle = (product1200, oracle1200) if gname == "c1200" else (product, oracle1000)
    assert composed(lib, oracle, pname, gname, 64) >= 64


def composed(lib, oracle, pname, gname, G, fec_id0=65500, device="cuda:0", per_group=3):
    """See test_indexed_chain_composed_gpu; the window crosses 65535 -> 1.  Returns the recovered segments."""
    capacity, stride = rc.GEOMS[gname]
    plan = rc.PLANS[pname](oracle)
    k, n, E = plan.k, plan.n_lines, per_group
    rng = np.random.default_rng(zlib.crc32(f"indexed-composed-{pname}-{gname}-{G}".encode()))
    b = rc.sender_batch(oracle, plan, G, fec_id0, capacity, stride, rng)
    assert n and not b.status.any() and fec_id0 + G > 65536
    dev = torch.device(device)
    st = torch.cuda.current_stream(dev).cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    ns, N, ds = G * k, G * (k + n), 1280
    d_sh, d_hd, d_ss, d_fs = up(b.shards), up(b.hdr), up(b.sstamps), up(b.fstamps)
    dgram, dlen = zeros(N * ds, 0xEE), zeros(N * 2, 0x77)
    lib.wire_encode_send(plan, G, stride, capacity, d_sh.data_ptr(), d_hd.data_ptr(), d_ss.data_ptr(),
                         dgram.data_ptr(), dlen.data_ptr(), d_fs.data_ptr(), dgram.data_ptr() + ns * ds,
                         dlen.data_ptr() + ns * 2, ds, st)
    lost_seg = np.stack([rng.choice(k, 2, replace=False) for _ in range(G)])
    lost = np.zeros(N, bool)
    lost[(np.arange(G)[:, None] * k + lost_seg).reshape(-1)] = True
    lost[ns + np.arange(0, G, 2) * n + rng.integers(0, n, (G + 1) // 2)] = True
    perm = rng.permutation(N)
    t_perm = torch.from_numpy(perm).to(dev)
    dgram = dgram[:N * ds].view(N, ds)[t_perm].contiguous()
    dlen16 = dlen[:N * 2].view(torch.int16).clone()
    dlen16[torch.from_numpy(lost).to(dev)] = 0
    dlen16 = dlen16[t_perm].contiguous()
    recs, payload = zeros(N * 64, ic.FILL), zeros(N * stride, ic.FILL)
    lib.wire_parse(N, ds, dgram.data_ptr(), dlen16.data_ptr(), stride, capacity, recs.data_ptr(), payload.data_ptr(),
                   st)
    shape = rc.new_outputs(plan, G, N, stride)

    def outs():
        return (zeros(G * 16, 0xEE), zeros(G * E * stride, 0x3C), zeros(G * E * 20, 0x3C), zeros(G * E, 0x3C))

    # the chain under test: tables only, then the decode through the map
    t = {name: zeros(shape[name].nbytes) for name in ic.TABLES}
    lib.wire_regroup_index(plan, G, fec_id0, N, recs.data_ptr(), capacity, *(t[name].data_ptr() for name in ic.TABLES),
                           st)
    rec_b, osh_b, ohd_b, oix_b = outs()
    ws = zeros(lib.workspace_size(plan, G), 0x11)
    lib.recover_indexed_out(plan, G, stride, capacity, payload.data_ptr(), N, t["src_of"].data_ptr(),
                            *(t[name].data_ptr() for name in ("hdr", "present", "meta", "fec_size", "parity_present")),
                            rec_b.data_ptr(), E, osh_b.data_ptr(), ohd_b.data_ptr(), oix_b.data_ptr(), ws.data_ptr(),
                            st)
    # the existing chain on the same parse output
    o = {name: zeros(shape[name].nbytes) for name in rc.OUTPUTS}
    lib.wire_regroup(plan, G, fec_id0, N, recs.data_ptr(), payload.data_ptr(), stride, capacity,
                     *(o[name].data_ptr() for name in rc.OUTPUTS), st)
    rec_a, osh_a, ohd_a, oix_a = outs()
    lib.recover_batch_out(plan, G, stride, capacity, *(o[name].data_ptr() for name in rc.OUTPUTS[:7]),
                          rec_a.data_ptr(), E, osh_a.data_ptr(), ohd_a.data_ptr(), oix_a.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize(dev)

    def down(tt, dtype, shp):
        nb = int(np.prod(shp)) * np.dtype(dtype).itemsize
        return tt[:nb].cpu().numpy().view(dtype).reshape(shp)

    have = ~lost
    present = np.zeros((G, 2), np.uint64)
    for g, i in zip(*np.nonzero(have[:ns].reshape(G, k))):
        present[g, i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    pp = np.zeros(G, np.uint64)
    for g, l in zip(*np.nonzero(have[ns:].reshape(G, n))):
        pp[g] |= np.uint64(1) << np.uint64(l)
    e_sh, e_hd, e_ix, e_rec = oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp,
                                                       capacity, E)
    w = rc.cd16(capacity)
    assert np.array_equal(down(t["present"], np.uint64, (G, 2)), present)
    assert np.array_equal(down(t["parity_present"], np.uint64, (G,)), pp)
    ok = e_ix != 0xFF
    assert ok.any()
    for what, (rec_, osh, ohd, oix) in (("indexed", (rec_b, osh_b, ohd_b, oix_b)), ("batch", (rec_a, osh_a, ohd_a, oix_a))):
        assert np.array_equal(down(oix, np.uint8, (G, E)), e_ix), what
        assert np.array_equal(down(rec_, np.uint64, (G, 2)), e_rec), what
        assert np.array_equal(down(ohd, rc.po.HDR_DTYPE, (G, E))[ok], e_hd[ok]), what
        assert np.array_equal(down(osh, np.uint8, (G, E, stride))[ok][:, :w], e_sh[ok][:, :w]), what
    # the two chains' four outputs, one against the other
    assert torch.equal(rec_a, rec_b) and torch.equal(oix_a, oix_b)
    okt = torch.from_numpy(ok.reshape(-1)).to(dev)
    assert torch.equal(ohd_a[:G * E * 20].view(G * E, 20)[okt], ohd_b[:G * E * 20].view(G * E, 20)[okt])
    assert torch.equal(osh_a[:G * E * stride].view(G * E, stride)[okt][:, :w],
                       osh_b[:G * E * stride].view(G * E, stride)[okt][:, :w])
    assert (down(osh_b, np.uint8, (G, E, stride))[:, :, w:] == 0x3C).all()
    return int(ok.sum())
