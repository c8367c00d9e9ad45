"""Cases, a numpy restatement of the rule and engines for rfec_recover_deliver
(the outputs of rfec_recover_indexed_shapes_out as a dense list of delivered
segments in window order), shared by the CPU and the GPU tests of
test_recover_deliver.py.

The call is a pure function of the decode's outputs and of the regroup's
shape_of / rank_of / group_of, so a case feeds synthetic ones: `synth` draws a
window (which groups were sent, the shape of each), ranks the groups of a shape
in window order as rfec_wire_regroup_shapes does, gives every section its room
and rows, and fills out_index with the hole patterns, out_hdr and out_shards
with random bytes.  A case's id is its name and its seed derives from it.

deliver_ref restates rules 1-7 of include/razor_fec.h (rfec_recover_deliver) in
numpy, in place over pre-filled outputs.  Each `wrong` switch bends one rule:
the case set must tell every bent rule from the right one.

An engine runs one call with every buffer in a guarded arena (guarded_arena.py),
each at exactly its documented alignment, the outputs pre-filled with FILL:
    RefDeliver   numpy memory, deliver_ref (the CPU run of the checks)
    GpuDeliver   torch memory in HBM, the product library
After the call the arena checks the guards and every input, and check_untouched
the tails [16 CD, stride) of the delivered rows and every seg / seg_payload
entry at or past min(T, max_out) against the pre-fill.
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import regroup_cases as rc

FILL = rc.FILL
NONE = rc.NONE
NOSHAPE = 0xFF
HOLE = 0xFF
DELIVER = 5  # tag of rfec_indexed_last_path for this entry (rfec_internal.h): DELIVER | launches << 8
GEOMS = rc.GEOMS

WRONG = ("section_order", "fec_id_no_wrap", "n_out_clamped", "rank_past_groups_delivered",
         "slot_order_by_index_byte")


def launches(G):
    """The documented number (razor_fec.h): three launches, two when window_groups <= 256."""
    return 2 if G <= 256 else 3


def hand_plan():
    """A valid plan: the call checks its plans and reads nothing else of them."""
    return rc._hand_plan(2, 1, 2, [(0, 1, 2, 0)])


class Case:
    pass


# window positions of decoded groups in the 65,535-group window: the first and last lane of a wave and of a block of
# the count pass, and the first and last block of the totals pass
BIG_POSITIONS = (0, 63, 64, 255, 256, 257, 65279, 65280, 65534)


def _patterns(rng, R, E, unsorted):
    """out_index [R][E]: row o takes pattern (o + 1) % 6 -- all holes, all delivered (row 0), a hole before, a hole
    after, holes between (E >= 3; else a random mask), a random mask.  Delivered slots hold distinct segment indices,
    ascending with the slot as the decodes write them, descending when `unsorted`."""
    ix = np.full((R, E), HOLE, np.uint8)
    for o in range(R):
        kind = (o + 1) % 6
        m = np.ones(E, bool)
        if kind == 0:
            m[:] = False
        elif kind == 2:
            m[0] = False
        elif kind == 3:
            m[-1] = False
        elif kind == 4 and E >= 3:
            m[1:-1] = False
        elif kind >= 4:
            m = rng.random(E) < 0.5
        v = np.sort(rng.choice(200, int(m.sum()), replace=False)).astype(np.uint8)
        ix[o, m] = v[::-1] if unsorted else v
    return ix


def synth(name, geom="c20", G=40, E=2, P=3, fec_id0=65530, sent=None, positions=(), room="fit", zero=(), max_out="T+3",
          unsorted=False, balanced=False):
    """One synthetic case.
    sent      None: every group of the window has a shape; else the number of groups drawn from the seed that have
              one, besides those at `positions`
    room      "fit": cap = counts and groups = counts; "null": cap = counts + 3 and groups NULL (the trailing rows
              have group_of NONE, and junk in out_index); "below": cap = counts, groups = counts - 1 where counts >= 2
              (the last rank of such a shape delivers nothing)
    zero      sections with groups[p] == 0 and a NULL group_of (their groups keep shape and rank)
    max_out   an int, or "T", "T-1", "T+3" of the rule's own total
    balanced  every shape has as many groups (G a multiple of P)"""
    x = Case()
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x.name, x.geom, x.G, x.E, x.P, x.fec_id0 = name, geom, G, E, P, fec_id0
    x.capacity, x.stride = GEOMS[geom]
    x.plans = [hand_plan() for _ in range(P)]
    has = np.ones(G, bool)
    if sent is not None:
        has[:] = False
        has[rng.choice(G, min(sent, G), replace=False)] = True
        has[list(positions)] = True
    shape = np.where(has, rng.integers(0, P, G), NOSHAPE).astype(np.uint8)
    if balanced:
        shape = rng.permutation(np.arange(G) % P).astype(np.uint8)
    elif G >= 2 * P and sent is None:
        where = rng.permutation(G)[:2 * P]
        shape[where] = np.arange(2 * P) % P
    rank = np.full(G, NONE, np.uint32)
    counts = [0] * P
    for g in np.nonzero(shape != NOSHAPE)[0]:
        rank[g] = counts[shape[g]]
        counts[shape[g]] += 1
    x.shape_of, x.rank_of, x.counts = shape, rank, counts
    x.caps = [c + 3 if room == "null" else c for c in counts]
    groups = None if room == "null" else [c - 1 if room == "below" and c >= 2 else c for c in counts]
    if zero:
        groups = list(x.caps) if groups is None else groups
        for p in zero:
            groups[p] = 0
    x.groups = groups
    x.rows = list(x.caps) if groups is None else list(groups)
    x.first = np.concatenate([[0], np.cumsum(x.rows)]).astype(np.int64)
    x.R = R = int(x.first[-1])
    x.group_of = []
    for p in range(P):
        if not x.rows[p]:
            x.group_of.append(None)
            continue
        go = np.full(x.caps[p], NONE, np.uint32)
        gs = np.nonzero((shape == p) & (rank < x.caps[p]))[0]
        go[rank[gs]] = gs
        x.group_of.append(go)
    x.out_index = _patterns(rng, R, E, unsorted)
    x.out_hdr = rng.integers(0, 256, (R, E, 20), dtype=np.uint8).view(po.HDR_DTYPE).reshape(R, E)
    x.out_shards = rng.integers(0, 256, (R, E, x.stride), dtype=np.uint8)
    x.max_out = 0
    x.T = T = int(deliver_ref(x, new_outputs(x))["n_out"][0])
    x.max_out = max_out if isinstance(max_out, int) else T + {"T": 0, "T-1": -1, "T+3": 3}[max_out]
    assert x.max_out >= 0
    return x


def from_tables(name, plans, caps, groups, G, fec_id0, shape_of, rank_of, group_of, capacity, stride, E, out_shards,
                out_hdr, out_index, max_out):
    """A case over given tables (the composed chain's, the comparison with the reference's receiver)."""
    x = Case()
    x.name, x.geom, x.G, x.E, x.P, x.fec_id0 = name, None, G, E, len(plans), fec_id0
    x.capacity, x.stride, x.plans, x.caps, x.groups = capacity, stride, plans, list(caps), groups
    x.rows = list(caps) if groups is None else list(groups)
    x.first = np.concatenate([[0], np.cumsum(x.rows)]).astype(np.int64)
    x.R = R = int(x.first[-1])
    x.shape_of, x.rank_of = np.ascontiguousarray(shape_of, np.uint8), np.ascontiguousarray(rank_of, np.uint32)
    x.group_of = [np.ascontiguousarray(g, np.uint32) if x.rows[p] else None for p, g in enumerate(group_of)]
    x.out_index = np.ascontiguousarray(out_index, np.uint8).reshape(R, E)
    x.out_hdr = np.ascontiguousarray(out_hdr).view(po.HDR_DTYPE).reshape(R, E)
    x.out_shards = np.ascontiguousarray(out_shards, np.uint8).reshape(R, E, stride)
    x.max_out = 0
    x.T = int(deliver_ref(x, new_outputs(x))["n_out"][0])
    x.max_out = max_out if max_out is not None else x.T + 3
    return x


# -- the rule ---------------------------------------------------------------------------------------------------
OUTPUTS = ("seg", "seg_payload", "first_of", "n_out")


def shapes_of(x):
    return {"seg": (po.RX_SEG, (x.max_out,)), "seg_payload": (np.uint8, (x.max_out, x.stride)),
            "first_of": (np.uint32, (x.G + 1,)), "n_out": (np.uint32, (1,))}


def new_outputs(x, fill=FILL):
    o = {name: np.zeros(shp, dt) for name, (dt, shp) in shapes_of(x).items()}
    for a in o.values():
        a.view(np.uint8)[...] = fill
    return o


def deliver_ref(x, out, wrong=()):
    """Rules 1-7 of rfec_recover_deliver (include/razor_fec.h), in place over `out` (new_outputs' arrays, or views of
    an arena).  wrong: names of WRONG, each one rule bent."""
    assert set(wrong) <= set(WRONG)
    P, G, E, R = x.P, x.G, x.E, x.R
    first = x.first  # rule 1
    w = rc.cd16(x.capacity)
    limit = np.array(x.caps if "rank_past_groups_delivered" in wrong else x.rows, np.int64)
    p, c = x.shape_of.astype(np.int64), x.rank_of.astype(np.int64)
    ok = p < P  # rule 2
    pp = np.where(ok, p, 0)
    o = first[pp] + c
    dec = ok & (c < limit[pp]) & (o < R)  # (o < R: the bent rule stays inside the arrays)
    ix = x.out_index.reshape(R, E)
    hit = np.zeros((G, E), bool)  # rule 3
    hit[dec] = ix[o[dec]] != HOLE
    n = hit.sum(1)
    order = np.arange(G)  # rule 4
    if "section_order" in wrong:
        order = np.argsort(np.where(dec, o, R + np.arange(G)), kind="stable")
    start = np.zeros(G, np.int64)
    start[order] = np.cumsum(n[order]) - n[order]
    T = int(n.sum())
    out["first_of"][:G] = start
    out["first_of"][G] = T
    out["n_out"][0] = min(T, x.max_out) if "n_out_clamped" in wrong else T
    for g in np.nonzero(n)[0]:  # rules 5-7
        es = np.nonzero(hit[g])[0]
        if "slot_order_by_index_byte" in wrong:
            es = es[np.argsort(ix[o[g], es], kind="stable")]
        for r, e in enumerate(es):
            j = int(start[g]) + r
            if j >= x.max_out:
                continue
            fid = (x.fec_id0 + int(g)) & 0xFFFF if "fec_id_no_wrap" in wrong else (x.fec_id0 - 1 + int(g)) % 65535 + 1
            out["seg"]["hdr"][j], out["seg"]["fec_id"][j], out["seg"]["reserved"][j] = x.out_hdr[o[g], e], fid, 0
            out["seg_payload"][j, :w] = x.out_shards[o[g], e, :w]
    return out


def compare(got, exp, what):
    """The six outputs -- seg's hdr, fec_id and reserved, seg_payload, first_of, n_out -- byte for byte (what the call
    leaves alone holds FILL in both)."""
    bad = []
    pairs = [(f"seg.{f}", got["seg"][f], exp["seg"][f]) for f in ("hdr", "fec_id", "reserved")]
    pairs += [(name, got[name], exp[name]) for name in OUTPUTS[1:]]
    for name, a, b in pairs:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            d = np.nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1))[0]
            bad.append(f"{name}: {len(d)} bytes differ, the first at offset {int(d[0])}")
    assert not bad, f"{what}: " + "; ".join(bad)


def check_untouched(x, out, what):
    """From the call's own n_out: the tails [16 CD, stride) of the delivered rows and every seg / seg_payload entry at
    or past min(T, max_out) hold the pre-fill."""
    T = int(out["n_out"][0])
    m = min(T, x.max_out)
    w = rc.cd16(x.capacity)
    assert (out["seg_payload"][:m, w:] == FILL).all(), f"{what}: the tail of a delivered row was written"
    assert (out["seg"][m:].view(np.uint8) == FILL).all(), f"{what}: seg was written at or past entry {m}"
    assert (out["seg_payload"][m:] == FILL).all(), f"{what}: seg_payload was written at or past row {m}"


def conditions(x, ref):
    """What the case exercises, from the rule's own outputs."""
    G, E, R = x.G, x.E, x.R
    cd = rc.cd16(x.capacity) // 16
    ix = x.out_index.reshape(R, E)
    hit = ix != HOLE
    p, c = x.shape_of.astype(np.int64), x.rank_of.astype(np.int64)
    rows = np.array(x.rows, np.int64)
    ok = p < x.P
    dec = ok & (c < rows[np.where(ok, p, 0)])
    o = (x.first[np.where(ok, p, 0)] + c)[dec]
    live = np.zeros(R, bool)
    live[o] = True
    h = hit[live]
    cnd = {"decoded": int(dec.sum()), "T": x.T}
    cnd["row_all_holes"] = bool((~h).all(1).any()) if len(h) else False
    cnd["row_all_delivered"] = bool(h.all(1).any()) if len(h) else False
    cnd["hole_before"] = bool((~h[:, 0] & h.any(1)).any()) if len(h) else False
    cnd["hole_after"] = bool((~h[:, -1] & h.any(1)).any()) if len(h) else False
    cnd["hole_between"] = any(E >= 3 and r[0] and r[-1] and not r.all() for r in h)
    s = np.nonzero((hit & live[:, None]).reshape(-1))[0]
    cnd["last_entry_mid_wave"] = bool(len(s)) and ((int(s[-1]) + 1) * cd) % 64 != 0
    cnd["wrap"] = x.fec_id0 + G > 65536
    cnd["overflow"] = x.T > x.max_out
    cnd["trailing_none_rows"] = x.groups is None and any(cap > cnt for cap, cnt in zip(x.caps, x.counts)) \
        if hasattr(x, "counts") else False
    cnd["rank_past_groups"] = bool((ok & ~dec & (c != NONE) & (rows[np.where(ok, p, 0)] > 0)).any())
    cnd["zero_sections"] = [q for q in range(x.P) if not x.rows[q] and hasattr(x, "counts") and x.counts[q]]
    cnd["no_shape_group"] = bool((~ok).any())
    cnd["unsorted_index"] = any((np.diff(r[r != HOLE].astype(int)) < 0).any() for r in ix[live])
    return cnd


# -- the case set -----------------------------------------------------------------------------------------------
# name -> keyword arguments of synth
CASES = {
    # the window's size: the count pass's workgroup scan at its edge, several blocks and the totals pass
    "G1": dict(G=1, P=1, fec_id0=9), "G255": dict(G=255), "G256": dict(G=256), "G257": dict(G=257),
    "G600": dict(G=600),
    # 65,535 groups from fec_id 65530: a few hundred decoded
    "big": dict(G=65535, sent=300, positions=BIG_POSITIONS, E=2),
    # out-slot patterns
    "E1": dict(E=1), "E2": dict(E=2), "E4": dict(E=4), "E6": dict(E=6),
    "unsorted": dict(E=4, unsorted=True, G=12),
    # payload lanes: CD = 1, 2, 75
    "cd1": dict(geom="c15", E=3), "cd2": dict(geom="c20", E=3), "cd75": dict(geom="c1200", E=2),
    # overflow
    "max-T": dict(max_out="T"), "max-T-1": dict(max_out="T-1"), "max-1": dict(max_out=1), "max-0": dict(max_out=0),
    # section variants
    "null-groups": dict(room="null", sent=30), "below-counts": dict(room="below"),
    "zero-first": dict(zero=(0,)), "zero-middle": dict(zero=(1,)), "zero-last": dict(zero=(2,)),
    "thirty-two": dict(P=32, G=100, zero=(3, 17)), "one-section": dict(P=1), "no-rows": dict(zero=(0, 1, 2)),
    # two sections with as many rows: the self-test swaps their group_of pointers
    "swap": dict(P=2, G=24, E=2, fec_id0=100, balanced=True),
}


def make(name):
    return synth(name, **CASES[name])


# -- engines ----------------------------------------------------------------------------------------------------
_IN = (("shape_of", 1), ("rank_of", 4), ("out_shards", 16), ("out_hdr", 4), ("out_index", 1))
_OUT = (("seg", 4), ("seg_payload", 16), ("first_of", 4), ("n_out", 4))


class DeliverEngine:
    """run(x) -> the four outputs (new_outputs' names, shapes and types) of one call with every buffer in one guarded
    arena: the decode's outputs, shape_of, rank_of and the group_of of every section with rows as inputs, the
    outputs pre-filled, a workspace of random bytes.  With max_out == 0 seg and seg_payload are NULL, with no rows the
    decode's outputs are, and a section without rows has a NULL group_of."""

    be = None

    def run(self, x, swap=None):
        shp = shapes_of(x)
        src = {"shape_of": x.shape_of, "rank_of": x.rank_of, "out_shards": x.out_shards, "out_hdr": x.out_hdr,
               "out_index": x.out_index}
        bufs = [ga.Buf(name, src[name].nbytes, src[name], "in", align) for name, align in _IN]
        bufs += [ga.Buf(f"group_of{p}", g.nbytes, g, "in", 4) for p, g in enumerate(x.group_of) if g is not None]
        bufs += [ga.Buf(name, int(np.prod(shp[name][1])) * np.dtype(shp[name][0]).itemsize, FILL, "out", align)
                 for name, align in _OUT]
        nws = max(16, self._workspace_size(x.G))
        bufs.append(ga.Buf("workspace", nws, np.random.default_rng(nws).integers(0, 256, nws, dtype=np.uint8),
                           "scratch", 16))
        A = ga.Arena(self.be, bufs)

        def group_of(p):
            if x.group_of[p] is None:
                return None
            q = p if swap is None or p not in swap else swap[1 - swap.index(p)]
            return A.ptr(f"group_of{q}")

        sections = [dict(cap=x.caps[p], group_of=group_of(p)) for p in range(x.P)]
        ptr = {name: A.ptr(name) for name, _ in _IN + _OUT}
        if not x.max_out:
            ptr["seg"] = ptr["seg_payload"] = None
        if not x.R:
            ptr["out_shards"] = ptr["out_hdr"] = ptr["out_index"] = None
        self._run(x, sections, ptr, A)
        self.be.sync()
        A.check(f"recover_deliver {x.name}")
        out = {name: A.get(name, *shp[name]) for name in OUTPUTS}
        check_untouched(x, out, f"recover_deliver {x.name}")
        return out


class RefDeliver(DeliverEngine):
    def __init__(self, wrong=()):
        self.be, self.wrong = ga.NumpyBackend(), wrong

    def _workspace_size(self, G):
        return 16

    def _run(self, x, sections, ptr, A):
        shp = shapes_of(x)
        out = {name: A.view(name).view(shp[name][0]).reshape(shp[name][1]) for name in OUTPUTS}
        deliver_ref(x, out, self.wrong)


class GpuDeliver(DeliverEngine):
    """last_path and last_launches: the tag and rfec_timing_launches() of the call."""

    def __init__(self, lib, device="cuda:0"):
        import ctypes as C

        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        lib.lib.rfec_indexed_last_path.restype = C.c_uint32
        lib.lib.rfec_indexed_last_path.argtypes = []

    def _workspace_size(self, G):
        return self.lib.recover_deliver_workspace_size(G)

    def _run(self, x, sections, ptr, A):
        self.lib.lib.rfec_timing_events(None, None)
        self.lib.recover_deliver(x.plans, sections, x.groups, x.G, x.fec_id0, ptr["shape_of"], ptr["rank_of"],
                                 x.stride, x.capacity, x.E, ptr["out_shards"], ptr["out_hdr"], ptr["out_index"],
                                 x.max_out, ptr["seg"], ptr["seg_payload"], ptr["first_of"], ptr["n_out"],
                                 A.ptr("workspace"), self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_launches = int(self.lib.lib.rfec_timing_launches())
        self.last_path = int(self.lib.lib.rfec_indexed_last_path())


# -- the in-order stream of the comparison with the reference's receiver ------------------------------------------
def inorder_window(oracle, seed, G=40, fec_id0=65520, geom="c1000"):
    """regroup_cases.inorder_stream for a window of several shapes: the plans of shapes_cases.PLANSETS["decode3"],
    their groups interleaved across the window, base ids ascending with the window index, group by group the
    segments, then the parities; 15 % of the datagrams lost, 10 % delivered twice (the copy a few places later, within
    its part).  Returns (plans, the window's shapes [G], recs, payload, capacity, stride)."""
    import shapes_cases as sc
    capacity, stride = GEOMS[geom]
    plans = [sc.PLANS[name](oracle) for name in sc.PLANSETS["decode3"]]
    P = len(plans)
    rng = np.random.default_rng(seed)
    shape = rng.permutation(np.arange(G) % P)
    batches, j_of = [], np.zeros(G, np.int64)
    for p, plan in enumerate(plans):
        gs = np.nonzero(shape == p)[0]
        j_of[gs] = np.arange(len(gs))
        b = rc.sender_batch(oracle, plan, len(gs), 1, capacity, stride, rng,
                            (5000 + gs.astype(np.uint64) * 140).astype(np.uint32))
        assert plan.n_lines and not b.status.any()
        b.recs["fec_id"] = [rc.fec_id_of(fec_id0, int(g))
                            for g in np.concatenate([np.repeat(gs, plan.k), np.repeat(gs, plan.n_lines)])]
        batches.append(b)
    recs, pay = [], []
    for g in range(G):
        p, j = int(shape[g]), int(j_of[g])
        k, n, Gp = plans[p].k, plans[p].n_lines, int((shape == p).sum())
        for part in ([j * k + i for i in range(k)], [Gp * k + j * n + l for l in range(n)]):
            got = []
            for d in part:
                if rng.random() < 0.15:
                    continue
                got.append(d)
                if rng.random() < 0.10:
                    got.append(d)
            for i in range(len(got) - 1):
                if got[i] == got[i + 1] and i + 2 < len(got) and rng.random() < 0.5:
                    got[i + 1], got[i + 2] = got[i + 2], got[i + 1]
            recs.append(batches[p].recs[got])
            pay.append(batches[p].pay[got])
    return plans, shape, np.concatenate(recs), np.concatenate(pay), capacity, stride


def decode_sections(oracle, plans, caps, rows, sec, payload, capacity, stride, E):
    """oracle.recover_batch_out per section over the regroup's tables (regroup_shapes_ref's `sec`), the member and
    parity rows gathered through src_of: the decode's outputs, dense over the sections' first rows[p] rows."""
    osh, ohd, oix = [], [], []
    for p, plan in enumerate(plans):
        g = rows[p]
        if not g:
            continue
        k, n, s = plan.k, plan.n_lines, sec[p]
        so = s["src_of"].reshape(caps[p], k + n)[:g].astype(np.int64)
        rows_ = np.where((so != NONE)[:, :, None], payload[np.minimum(so, len(payload) - 1)], 0).astype(np.uint8)
        sh, hd, ix, _ = oracle.recover_batch_out(plan, rows_[:, :k], s["hdr"][:g], s["present"][:g], rows_[:, k:],
                                                 s["meta"][:g], s["fec_size"][:g], s["parity_present"][:g], capacity,
                                                 E)
        osh.append(sh), ohd.append(hd), oix.append(ix)
    return np.concatenate(osh), np.concatenate(ohd), np.concatenate(oix)
