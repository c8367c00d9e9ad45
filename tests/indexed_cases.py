"""Cases, inputs, the reference and engines for rfec_recover_indexed_out (the
dense decode with payload rows read through a slot map from a row pool) and
rfec_wire_regroup_index (rfec_wire_regroup's tables without the row copy),
shared by the CPU and the GPU tests of test_recover_indexed.py.

A case is (plan, geometry, groups, per_group, sparse).  Its row pool and slot
map come from regroup_cases: sender_batch (the oracle's sender path, framed and
parsed) -> an arrival order with losses, later copies with other bytes and
refused records -> regroup_ref (the placement rule in numpy), whose tables
(hdr, present, meta, fec_size, parity_present, src_of) are the call's inputs.
A sparse case then scatters the pool's rows over a larger pool by hand, so that
winning row indices pass 65,535.

The reference of every comparison: gather the rows by src_of in numpy into the
batch layout -> oracle.recover_batch_out.  Each `wrong` switch bends the gather
one way; the case set must tell every bent gather from the right one.
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import regroup_cases as rc

FILL = rc.FILL
NONE = rc.NONE
FEC_ID0 = 65530  # every window of more than 5 groups crosses 65535 -> 1

PLANS = dict(rc.PLANS)
PLANS["rows32x4"] = lambda o: o.plan_matrix(32, 8, 4, rc.ROWS)   # the fused row decode compiled for K = 32
PLANS["rows12x3"] = lambda o: o.plan_matrix(12, 4, 3, rc.ROWS)   # a row layout with k and col at run time
GEOMS = rc.GEOMS

# tags of rfec_indexed_last_path (rfec_internal.h)
ROWS_FUSED, PEEL_REPLAY = 1, 2
# plan -> the tag under the default kernel selection (RFEC_TUNE_GENERIC: (PEEL_REPLAY, MAXC) for all)
DEFAULT_PATH = {"rows10x4": (ROWS_FUSED, 10), "rows32x4": (ROWS_FUSED, 32), "rows12x3": (ROWS_FUSED, 0),
                "k2": (ROWS_FUSED, 0), "full3x4k10": (PEEL_REPLAY, 4), "hand6": (PEEL_REPLAY, 4),
                "strip65": (PEEL_REPLAY, 8), "strip128": (PEEL_REPLAY, 8)}

# (plan, geometry, groups, per_group, sparse).  Group counts 1, 63, 64, 65, 129 and 600 at c0 / c15: the edges of
# the header blocks' groups-per-block rules (256 >> lg groups per line_headers block, 64 or fewer per peel block)
# and of the payload blocks, with more header than payload blocks; c20 has a tail (stride 48, CD = 2); c1200 has
# CD = 75, so a wave straddles out slots and groups.
CASES = [
    ("rows10x4", "c1200", 7, 3, False), ("rows10x4", "c1000", 5, 1, False), ("rows10x4", "c20", 7, 2, False),
    ("rows10x4", "c0", 1, 1, False), ("rows10x4", "c15", 63, 2, False), ("rows10x4", "c0", 64, 3, False),
    ("rows10x4", "c15", 65, 10, False), ("rows10x4", "c0", 129, 2, False), ("rows10x4", "c15", 600, 3, False),
    ("rows32x4", "c1200", 3, 3, False), ("rows32x4", "c15", 65, 32, False), ("rows32x4", "c20", 7, 2, False),
    ("rows32x4", "c1000", 2, 1, False),
    ("rows12x3", "c1200", 4, 3, False), ("rows12x3", "c15", 129, 1, False), ("rows12x3", "c20", 7, 12, False),
    ("rows12x3", "c1000", 3, 2, False), ("rows12x3", "c0", 64, 3, False),
    ("full3x4k10", "c1000", 12, 3, False), ("full3x4k10", "c1200", 4, 10, False), ("full3x4k10", "c15", 64, 2, False),
    ("full3x4k10", "c20", 7, 3, False), ("full3x4k10", "c0", 600, 3, False), ("full3x4k10", "c15", 5, 1, False),
    ("strip65", "c15", 7, 1, False), ("strip65", "c20", 3, 2, False), ("strip65", "c1200", 2, 65, False),
    ("strip65", "c1000", 2, 1, False),
    ("strip128", "c0", 1, 1, False), ("strip128", "c1000", 2, 3, False), ("strip128", "c15", 63, 128, False),
    ("strip128", "c20", 3, 2, False),
    ("hand6", "c20", 7, 3, False), ("hand6", "c1200", 4, 6, False), ("hand6", "c0", 65, 1, False),
    ("hand6", "c1000", 5, 2, False),
    ("k2", "c15", 7, 1, False), ("k2", "c1200", 2, 2, False), ("k2", "c0", 129, 2, False), ("k2", "c20", 3, 1, False),
    # pools of 70,000 rows at stride 16: winning row indices above 65,535
    ("rows10x4", "c15", 7, 3, True), ("full3x4k10", "c0", 7, 3, True),
]
SPARSE_ROWS = 70000

WRONG = ("slot_is_row", "parity_from_members", "cd_pitch", "trunc16")


def case_id(c):
    plan, geom, G, E, sparse = c
    return f"{plan}-{geom}-G{G}-E{E}{'-sparse' if sparse else ''}"


class Inputs:
    pass


def _lose(plan, G, rng, pname):
    """lost [G (k + n)] bool over the sender's datagrams (segments [G k], then parities [G n]).  Group 0 loses
    its last member alone and keeps every parity, so it recovers a segment in every case; group 1 its first
    member alone (the refused line, make_inputs); group 2 one member (the descending group); group 3 of the
    3 x 4 plan members 0 and 1 and the parity of column 1, so member 1 comes from row 0 after column 0 gave
    member 0; the others 0..3 random members and now and then a parity."""
    k, n = plan.k, plan.n_lines
    ls, lp = np.zeros((G, k), bool), np.zeros((G, n), bool)
    for g in range(G):
        if g == 0:
            ls[g, k - 1] = True
        elif g == 1:
            ls[g, 0] = True
        elif g == 2:
            ls[g, rng.integers(0, k)] = True
        elif g == 3 and pname == "full3x4k10":
            ls[g, :2] = True
            lp[g, plan.n_row_lines + 1] = True
        else:
            ls[g, rng.choice(k, min(k - 1, int(rng.integers(0, 4))), replace=False)] = True
            lp[g] = rng.random(n) < 0.15
    return np.concatenate([ls.reshape(-1), lp.reshape(-1)])


def make_inputs(oracle, c):
    """The case's pool, map and tables (see the module's text)."""
    pname, gname, G, E, sparse = c
    capacity, stride = GEOMS[gname]
    plan = PLANS[pname](oracle)
    k, n = plan.k, plan.n_lines
    slots = k + n
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    b = rc.sender_batch(oracle, plan, G, FEC_ID0, capacity, stride, rng)
    recs0, pay0 = b.recs.copy(), b.pay.copy()
    refused_line = None
    if G > 1 and capacity:
        # group 1, line 0: the parity's data_size below a present member's -> the header checks refuse the line
        ln = plan.line[0]
        others = [ln.first + q * ln.stride for q in range(ln.count)][1:]
        if ln.first == 0 and max(int(b.hdr["size"][1, i]) for i in others) > 0:
            recs0["data_size"][G * k + 1 * n + 0] = 0
            refused_line = (1, 0)
    lost = _lose(plan, G, rng, pname)
    arr = rng.permutation(np.nonzero(~lost)[0])
    group_of = np.where(arr < G * k, arr // k, (arr - G * k) // max(n, 1))
    slot_of = np.where(arr < G * k, arr % k, k + (arr - G * k) % max(n, 1))
    if G > 2:  # group 2: the higher the slot, the earlier its datagram
        pos = np.nonzero(group_of == 2)[0]
        arr[pos] = arr[pos][np.argsort(-slot_of[pos], kind="stable")]
    recs, pay = recs0[arr], pay0[arr]
    # later copies with other bytes, each somewhere behind its source: they lose their slots
    nd = len(arr) // 2 + 1
    src = rng.integers(0, len(arr), nd)
    drec, dpay = recs[src].copy(), pay[src].copy()
    rc._changed(drec, dpay)
    at = rng.integers(src + 1, len(arr) + 1)
    order = np.argsort(at, kind="stable")
    recs, pay = np.insert(recs, at[order], drec[order]), np.insert(pay, at[order], dpay[order], axis=0)
    # refused records ahead of everything: a fec_id outside the window, a failed parse status
    head_r, head_p = recs0[:5].copy(), pay0[:5].copy() ^ 0xA5
    head_r["fec_id"][:3] = rc.fec_id_of(FEC_ID0, G)
    head_r["status"][3:] = -1
    recs, pay = np.concatenate([head_r, recs]), np.concatenate([head_p, pay])
    x = Inputs()
    x.case, x.plan, x.G, x.k, x.nl, x.E, x.fec_id0 = c, plan, G, k, n, E, FEC_ID0
    x.capacity, x.stride, x.batch, x.refused_line = capacity, stride, b, refused_line
    x.recs, x.rows, x.n_rows = np.ascontiguousarray(recs), np.ascontiguousarray(pay), len(recs)
    t = rc.regroup_ref(plan, G, FEC_ID0, x.recs, x.rows, capacity, rc.new_outputs(plan, G, x.n_rows, stride))
    x.hdr, x.present, x.meta, x.fec_size, x.parity_present = (t[name] for name in (
        "hdr", "present", "meta", "fec_size", "parity_present"))
    x.src_of = t["src_of"]
    x.tables = t
    if sparse:  # the same rows scattered over a larger pool, the map rewritten by hand
        assert stride == 16 and x.n_rows <= 8000
        where = np.sort(rng.choice(np.arange(SPARSE_ROWS - 9000, SPARSE_ROWS), x.n_rows, replace=False))
        big = rng.integers(0, 256, (SPARSE_ROWS, stride), dtype=np.uint8)
        big[where] = x.rows
        filled = x.src_of != NONE
        so = x.src_of.copy()
        so[filled] = where[x.src_of[filled]].astype(np.uint32)
        x.rows, x.n_rows, x.src_of, x.recs = big, SPARSE_ROWS, so, None
    assert slots * G == len(x.src_of)
    return x


# -- the reference ----------------------------------------------------------------------------------------------------
def gather(x, wrong=()):
    """The batch layout's shards [G][k][stride] and parity [G][n][stride] with row src_of[slot] copied over
    [0, 16 CD) of each filled slot; every other byte holds FILL.  wrong: names of WRONG, each one way to bend it."""
    assert set(wrong) <= set(WRONG)
    G, k, n, stride = x.G, x.k, x.nl, x.stride
    slots, w = k + n, rc.cd16(x.capacity)
    so = x.src_of.reshape(G, slots).astype(np.int64)
    filled = so != NONE
    flat = x.rows.reshape(-1)

    def fetch(a):
        if "trunc16" in wrong:
            a = a & 0xFFFF
        a = np.minimum(a, x.n_rows - 1)
        if "cd_pitch" in wrong:  # rows taken as 16 CD bytes apart
            return flat[(a * w)[:, None] + np.arange(w)[None, :]]
        return x.rows[a, :w]

    shards = np.full((G, k, stride), FILL, np.uint8)
    parity = np.full((G, n, stride), FILL, np.uint8)
    g_, s_ = np.nonzero(filled[:, :k])
    shards[g_, s_, :w] = fetch(g_ * slots + s_ if "slot_is_row" in wrong else so[g_, s_])
    g_, l_ = np.nonzero(filled[:, k:])
    if len(g_):
        a = so[g_, l_] if "parity_from_members" in wrong else so[g_, k + l_]
        parity[g_, l_, :w] = fetch(g_ * slots + k + l_ if "slot_is_row" in wrong else a)
    return shards, parity


def reference(oracle, x, wrong=()):
    """(out_shards [G][E][stride], out_hdr [G][E], out_index [G][E], recovered [G][2]) of
    oracle.recover_batch_out on the gathered batch."""
    shards, parity = gather(x, wrong)
    return oracle.recover_batch_out(x.plan, shards, x.hdr, x.present, parity, x.meta, x.fec_size, x.parity_present,
                                    x.capacity, x.E)


def compare(got, exp, x, what, fill=FILL):
    """recovered, out_index, out_hdr and out_shards over [0, 16 CD) of the slots whose out_index is not 0xFF,
    byte for byte; bytes [16 CD, stride) of every out slot hold the pre-fill."""
    g_sh, g_hd, g_ix, g_rec = got
    e_sh, e_hd, e_ix, e_rec = exp
    w = rc.cd16(x.capacity)
    bad = []
    if not np.array_equal(g_rec, e_rec):
        bad.append(f"recovered: {int((g_rec != e_rec).any(1).sum())} groups differ")
    if not np.array_equal(g_ix, e_ix):
        bad.append(f"out_index: {int((g_ix != e_ix).sum())} slots differ")
    ok = e_ix != 0xFF
    if g_hd[ok].tobytes() != e_hd[ok].tobytes():
        bad.append(f"out_hdr: {int((g_hd[ok] != e_hd[ok]).sum())} records differ")
    d = (g_sh[ok][:, :w] != e_sh[ok][:, :w])
    if d.any():
        bad.append(f"out_shards: {int(d.any(1).sum())} slots differ")
    if (g_sh[:, :, w:] != fill).any():
        bad.append("out_shards: a slot's tail was written")
    assert not bad, f"{what}: " + "; ".join(bad)


def conditions(x, ref):
    """What the case exercises, from the reference's own outputs."""
    e_sh, e_hd, e_ix, e_rec = ref
    k, n, G = x.k, x.nl, x.G
    pres = ga.present_rows(x.present, k).reshape(G, k)
    pp = ((x.parity_present[:, None] >> np.arange(max(n, 1), dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    rec = ga.present_rows(e_rec, k).reshape(G, k)
    c = {"recovered": bool(rec.any()), "target_64": bool((e_ix[e_ix != 0xFF] >= 64).any())}
    # an erased segment with an out slot that stays 0xFF
    erased_rank = np.cumsum(~pres, 1) - 1
    c["unrecovered_slot"] = bool(((~pres) & (erased_rank < x.E) & ~rec).any())
    members = [[x.plan.line[l].first + q * x.plan.line[l].stride for q in range(x.plan.line[l].count)]
               for l in range(n)]
    # the refused line: its parity is there, one member is missing, every size but the patched one is in bounds
    c["refused_line"] = False
    if x.refused_line is not None:
        g, l = x.refused_line
        miss = [i for i in members[l] if not pres[g, i]]
        c["refused_line"] = bool(pp[g, l] and len(miss) == 1 and not rec[g, miss[0]] and
                                 any(pres[g, i] and x.hdr["size"][g, i] > x.fec_size[g, l] for i in members[l]))
    # a cascade: more segments recovered than lines that can fire on the received masks
    first = np.zeros(G, int)
    for g in range(G):
        t = {next(i for i in m if not pres[g, i]) for l, m in enumerate(members)
             if pp[g, l] and sum(not pres[g, i] for i in m) == 1}
        first[g] = len(t)
    c["cascade"] = bool((rec.sum(1) > first).any())
    so = x.src_of.reshape(G, k + n).astype(np.int64)
    desc = False
    for g in range(G):
        a = so[g][so[g] != NONE]
        desc = desc or (len(a) >= 3 and bool((np.diff(a) < 0).all()))
    c["descending_group"] = desc
    c["pool_above_slots"] = x.n_rows > G * (k + n)
    c["row_above_65535"] = bool((x.src_of[x.src_of != NONE] > 65535).any())
    return c


# -- engines ----------------------------------------------------------------------------------------------------------
_IN = (("rows", 16), ("src_of", 4), ("hdr", 4), ("present", 8), ("meta", 4), ("fec_size", 2), ("parity_present", 8))


class IndexedEngine:
    """run(x) -> (out_shards, out_hdr, out_index, recovered) of one rfec_recover_indexed_out call with every buffer
    in one guarded arena at exactly its documented alignment, the outputs pre-filled with FILL; guards and inputs
    are checked after the call.  mutate (tests): called with the arena before the call (a bent input)."""

    be = None
    mutate = None
    last_path = 0

    def _workspace_size(self, x):
        return 16

    def run(self, x):
        G, E, stride = x.G, x.E, x.stride
        src = {"rows": x.rows, "src_of": x.src_of, "hdr": x.hdr, "present": x.present, "meta": x.meta,
               "fec_size": x.fec_size, "parity_present": x.parity_present}
        bufs = [ga.Buf(name, src[name].nbytes, src[name], "in", align) for name, align in _IN]
        bufs += [ga.Buf("recovered", G * 16, FILL, "out", 8), ga.Buf("out_shards", G * E * stride, FILL, "out", 16),
                 ga.Buf("out_hdr", G * E * 20, FILL, "out", 4), ga.Buf("out_index", G * E, FILL, "out", 1),
                 ga.Buf("workspace", max(16, self._workspace_size(x)), 0x11, "scratch", 16)]
        A = ga.Arena(self.be, bufs)
        if self.mutate is not None:
            self.mutate(A)
            A.snap = {b.name: self.be.clone(A.view(b.name)) for b in bufs if b.role == "in"}
        self._run(x, A)
        self.be.sync()
        A.check(f"recover_indexed_out {case_id(x.case)}")
        return (A.get("out_shards", np.uint8, (G, E, stride)), A.get("out_hdr", po.HDR_DTYPE, (G, E)),
                A.get("out_index", np.uint8, (G, E)), A.get("recovered", np.uint64, (G, 2)))


class RefIndexed(IndexedEngine):
    """The reference behind the same arena (the CPU run of the checks): reads the arena's inputs, writes
    [0, 16 CD) of every out slot."""

    def __init__(self, oracle):
        self.be, self.o = ga.NumpyBackend(), oracle

    def _run(self, x, A):
        y = Inputs()
        y.__dict__.update(x.__dict__)
        y.rows = A.view("rows").reshape(x.rows.shape)
        y.src_of = A.view("src_of").view(np.uint32)
        sh, hd, ix, rec = reference(self.o, y)
        w = rc.cd16(x.capacity)
        A.view("out_shards").reshape(sh.shape)[:, :, :w] = sh[:, :, :w]
        A.view("out_hdr")[...] = hd.view(np.uint8).reshape(-1)
        A.view("out_index")[...] = ix.reshape(-1)
        A.view("recovered")[...] = rec.view(np.uint8).reshape(-1)


class GpuIndexed(IndexedEngine):
    def __init__(self, lib, device="cuda:0", tuning=0):
        import ctypes as C

        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib, self.tuning = torch, lib, tuning
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        lib.lib.rfec_indexed_last_path.restype = C.c_uint32
        lib.lib.rfec_indexed_last_path.argtypes = []

    def _workspace_size(self, x):
        return self.lib.workspace_size(x.plan, x.G)

    def _run(self, x, A):
        self.lib.set_tuning(self.tuning)
        try:
            self.lib.recover_indexed_out(x.plan, x.G, x.stride, x.capacity, A.ptr("rows"), x.n_rows, A.ptr("src_of"),
                                         A.ptr("hdr"), A.ptr("present"), A.ptr("meta"), A.ptr("fec_size"),
                                         A.ptr("parity_present"), A.ptr("recovered"), x.E, A.ptr("out_shards"),
                                         A.ptr("out_hdr"), A.ptr("out_index"), A.ptr("workspace"),
                                         self.torch.cuda.current_stream(self.device).cuda_stream)
            self.last_path = int(self.lib.lib.rfec_indexed_last_path())
        finally:
            self.lib.set_tuning(0)


def swap_two_members(oracle, x, ref):
    """A mutation of the arena's src_of: the entries of two present members of one group swapped (both stay
    valid rows), the first such pair for which the reference's own outputs change (two members of one line, or
    of lines that recover nothing, would change none)."""
    w = rc.cd16(x.capacity)
    slots = x.k + x.nl
    so = x.src_of.reshape(x.G, slots)
    rec = None
    for g in np.nonzero((ref[2] != 0xFF).any(1))[0][:4]:
        s = [i for i in range(x.k) if so[g, i] != NONE]
        for i, j in [(i, j) for i in s for j in s if i < j][:40]:
            y = Inputs()
            y.__dict__.update(x.__dict__)
            y.src_of = x.src_of.copy()
            y.src_of[[g * slots + i, g * slots + j]] = y.src_of[[g * slots + j, g * slots + i]]
            out = reference(oracle, y)
            ok = ref[2] != 0xFF
            if (out[0][ok][:, :w] != ref[0][ok][:, :w]).any():
                rec = (int(g) * slots + i, int(g) * slots + j)
                break
        if rec:
            break
    assert rec is not None

    def mutate(A):
        v = A.view("src_of")
        a, b = rec
        if isinstance(v, np.ndarray):
            t = v[4 * a:4 * a + 4].copy()
            v[4 * a:4 * a + 4] = v[4 * b:4 * b + 4]
            v[4 * b:4 * b + 4] = t
        else:
            t = v[4 * a:4 * a + 4].clone()
            v[4 * a:4 * a + 4] = v[4 * b:4 * b + 4]
            v[4 * b:4 * b + 4] = t

    return mutate, rec


# -- rfec_wire_regroup_index ------------------------------------------------------------------------------------------
TABLES = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")
_TAB_ALIGN = {"hdr": 4, "present": 8, "meta": 4, "fec_size": 2, "parity_present": 8, "base_id": 4, "src_of": 4,
              "slot_of": 4}


def regroup_index_gpu(lib, x, device="cuda:0"):
    """One rfec_wire_regroup_index call on a regroup_cases input: the eight tables, each in the guarded arena
    over FILL.  The arena holds recs and the tables only: no payload, shards or parity buffer exists."""
    import torch
    from gpu_engine import TorchBackend
    dev = torch.device(device)
    shape = rc.new_outputs(x.plan, x.G, x.n, x.stride)
    bufs = [ga.Buf("recs", x.n * 64, x.recs, "in", 16)]
    bufs += [ga.Buf(name, shape[name].nbytes, FILL, "out", _TAB_ALIGN[name]) for name in TABLES]
    A = ga.Arena(TorchBackend(dev), bufs)
    lib.wire_regroup_index(x.plan, x.G, x.fec_id0, x.n, A.ptr("recs"), x.capacity, *(A.ptr(name) for name in TABLES),
                           torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    A.check(f"wire_regroup_index {rc.case_id(x.case)}")
    return {name: A.get(name, shape[name].dtype, shape[name].shape) for name in TABLES}


def compare_tables(got, exp, what):
    bad = []
    for name in TABLES:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad.append(f"{name}: {int((a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)).sum())} bytes differ")
    assert not bad, f"{what}: " + "; ".join(bad)
