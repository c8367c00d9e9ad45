"""Cases, inputs, a numpy restatement of the rule and engines for
rfec_wire_regroup_shapes (one regroup pass over a window whose groups have
different shapes), shared by the CPU and the GPU tests of
test_wire_regroup_shapes.py.

A case is (plan set, geometry, groups, fec_id0, room, layout); its id holds
every field and its seed derives from the id.  The window is built from one
regroup_cases.sender_batch per plan: the parsed records' fec_ids are rewritten so
that the shapes interleave across the window in a pattern drawn from the seed,
then the records are edited as regroup_cases.make_inputs edits them (shuffled,
about 15 % lost, about 15 % duplicated with other bytes, the refused kinds) and
the two shape conflicts are added (see make_inputs).

regroup_shapes_ref restates rules 1-7 of include/razor_fec.h
(rfec_wire_regroup_shapes) and "Written" in numpy, in place over pre-filled
outputs.  Each `wrong` switch bends one rule: the case set must tell every bent
rule from the right one.

An engine runs one call with every buffer in a guarded arena (guarded_arena.py):
    RefShapes   numpy memory, regroup_shapes_ref (the CPU run of the checks)
    GpuShapes   torch memory in HBM, the product library
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import indexed_cases as ic
import pyoracle as po
import regroup_cases as rc

FILL = rc.FILL
NONE = rc.NONE
NOSHAPE = 0xFF
ENOTFEC, EWINDOW, ESHAPE, ENOPARITY, EBASE, EDUP = rc.ENOTFEC, rc.EWINDOW, rc.ESHAPE, rc.ENOPARITY, rc.EBASE, rc.EDUP
EFULL = -7
SEG, FEC = rc.SEG, rc.FEC
MAX_SHAPES = 32

WRONG = ("anchor_per_plan", "rank_by_arrival", "counts_clamped", "full_wraps", "other_shape_placed")

PLANS = ic.PLANS
GEOMS = rc.GEOMS
PLANSETS = {
    "mix3": ("full3x4k10", "k2", "hand6"),
    "mask2": ("strip65", "k2"),           # the second mask word
    "noanchor": ("k1", "rows10x4"),       # k1 has no line: a plan that can never anchor
    # the composed chain: every plan recovers, and every line has an index of its own (hand6 puts one index on two
    # lines, so its second such parity never reaches its line over the wire)
    "decode3": ("full3x4k10", "rows32x4", "rows12x3"),
}

# (plan set, geometry, groups, fec_id0, room, layout)
#   room    "fit": every section has cap = groups; "tight": the first section that has two groups or more gets
#           cap = count - 1 and the last of the others cap = 0; "c64": every cap = 64
#   layout  "mixed": every group of the window is sent, its shape drawn from the seed; "edges": 65,535 groups of
#           which only a few hundred are sent, the first plan's at the edges of the rank pass
CASES = [
    ("mix3", "c20", 12, 65530, "fit", "mixed"),     # the window crosses 65535 -> 1
    ("mix3", "c15", 12, 65530, "tight", "mixed"),
    ("mix3", "c20", 1, 9, "fit", "mixed"),          # G = 1
    ("mask2", "c15", 12, 65530, "fit", "mixed"),
    ("mask2", "c20", 12, 65530, "tight", "mixed"),
    ("mask2", "c15", 1, 65535, "fit", "mixed"),
    ("noanchor", "c20", 12, 65530, "fit", "mixed"),
    ("noanchor", "c15", 12, 65530, "tight", "mixed"),
    ("noanchor", "c15", 1, 1, "fit", "mixed"),
    ("mix3", "c15", 65535, 65530, "c64", "edges"),  # the rank pass at its edges
]
# three plans, 3,000 groups, about 70,000 records, every slot contended by several copies
LOOP_CASE = ("mix3", "c32", 3000, 64000, "fit", "mixed")
# window positions of the first plan's groups in the "edges" layout: the issue's, and the first and last group of a
# lane's run of 16 and of a tile of 8,192 of the rank kernel
EDGE_POSITIONS = (0, 15, 16, 63, 64, 1023, 1024, 8191, 8192, 65534)


def case_id(c):
    pset, geom, G, fec_id0, room, layout = c
    return f"{pset}-{geom}-G{G}-id{fec_id0}-{room}-{layout}"


class Inputs:
    pass


def _shapes_of_window(c, P, rng):
    """sent [G] bool and shape [G] (a plan index; meaningless where not sent)."""
    G, layout = c[2], c[5]
    if layout == "edges":
        sent = np.zeros(G, bool)
        shape = np.zeros(G, np.int64)
        other = rng.choice(G, 260, replace=False)
        sent[other] = True
        shape[other] = rng.integers(0, P, len(other))
        sent[list(EDGE_POSITIONS)] = True
        shape[list(EDGE_POSITIONS)] = 0
        return sent, shape
    shape = rng.integers(0, P, G)
    if G >= 2 * P:  # every plan has two groups or more, wherever the draw put them
        where = rng.permutation(G)[:2 * P]
        shape[where] = np.arange(2 * P) % P
    return np.ones(G, bool), shape


def make_inputs(oracle, c):
    """The case's records (and their payload rows, which the call does not read: the per-plan rule and the
    composed decode do).  x.batches[p] is plan p's sender batch, x.groups_of[p] the window indices of its groups
    in window order."""
    pset, gname, G, fec_id0, room, layout = c
    capacity, stride = GEOMS[gname]
    plans = [PLANS[name](oracle) for name in PLANSETS[pset]]
    P = len(plans)
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    loop = c == LOOP_CASE
    sent, shape = _shapes_of_window(c, P, rng)
    groups_of = [np.nonzero(sent & (shape == p))[0] for p in range(P)]
    batches, recs_l, pay_l = [], [], []
    for p, plan in enumerate(plans):
        gs = groups_of[p]
        if not len(gs):
            batches.append(None)
            continue
        k, n = plan.k, plan.n_lines
        base = (1000 + gs.astype(np.uint64) * 140).astype(np.uint32)
        if len(gs) > 1 and k > 6:
            base[1] = 0xFFFFFFFA  # member ids wrap 32 bits
        b = rc.sender_batch(oracle, plan, len(gs), 1, capacity, stride, rng, base, big=loop or layout == "edges")
        g_of_rec = np.concatenate([np.repeat(gs, k), np.repeat(gs, n)])
        b.recs["fec_id"] = [rc.fec_id_of(fec_id0, int(g)) for g in g_of_rec]
        b.window_fid = np.array([rc.fec_id_of(fec_id0, int(g)) for g in gs], np.uint16)
        batches.append(b)
        recs_l.append(b.recs)
        pay_l.append(b.pay)
    recs0, pay0 = np.concatenate(recs_l), np.concatenate(pay_l)
    keep = np.nonzero(rng.random(len(recs0)) > 0.15)[0]
    order = rng.permutation(keep)
    recs, pay = recs0[order], pay0[order]
    nd = int((1.8 if loop else 0.15) * len(order))
    if len(order) >= 3 and nd:
        third = max(1, len(order) // 3)
        src = rng.integers(0, len(order) if loop else third, nd)
        drec, dpay = recs[src].copy(), pay[src].copy()
        rc._changed(drec, dpay)
        if loop:
            recs, pay = np.concatenate([recs, drec]), np.concatenate([pay, dpay])
            q = rng.permutation(len(recs))
            recs, pay = recs[q], pay[q]
        else:
            at = np.sort(rng.integers(len(order) - third, len(order) + 1, nd))
            recs, pay = np.insert(recs, at, drec), np.insert(pay, at, dpay, axis=0)
    head, tail = [], []

    def seg_of(p, j, i):
        d = j * plans[p].k + i
        return batches[p].recs[d:d + 1].copy(), batches[p].pay[d:d + 1].copy()

    def fec_of(p, j, l):
        d = len(groups_of[p]) * plans[p].k + j * plans[p].n_lines + l
        return batches[p].recs[d:d + 1].copy(), batches[p].pay[d:d + 1].copy()

    conflicts = []  # (kind, window group, its plan, the foreign plan)
    if not loop:
        anchoring = [p for p in range(P) if plans[p].n_lines and len(groups_of[p])]
        # conflict "later": group g of shape A keeps an A parity ahead of everything; a parity B accepts, with g's
        # fec_id and base_id, arrives after everything (ESHAPE, rule 3) -- both ways round, so that the lower and
        # the higher plan index are the first once each
        # conflict "refused": group g's earliest parity is one B would accept but for data_size = capacity + 1,
        # with another base_id; an A parity follows
        for a in anchoring:
            for bb in anchoring:
                if a == bb or len(groups_of[a]) < 2:
                    continue
                for kind, j in (("later", 0), ("refused", len(groups_of[a]) - 1)):
                    g = int(groups_of[a][j])
                    own = fec_of(a, j, 0)
                    r, pl = fec_of(bb, 0, 0)
                    r["fec_id"][0] = rc.fec_id_of(fec_id0, g)
                    if kind == "later":
                        r["base_id"][0] = own[0]["base_id"][0]
                        head.append(own)
                        tail.append((r, pl))
                    else:
                        r["data_size"][0], r["base_id"][0] = capacity + 1, (int(own[0]["base_id"][0]) + 7) % 2**32
                        head.append((r, pl))
                        recs = np.concatenate([own[0], recs])  # behind the head, ahead of the rest
                        pay = np.concatenate([own[1], pay])
                    conflicts.append((kind, g, a, bb))
        for p in anchoring:  # the refused kinds of regroup_cases.make_inputs, per plan
            plan, j = plans[p], len(groups_of[p]) // 2
            for field, val in (("count", plan.k + 1), ("row", plan.row + 1), ("col", plan.col + 1), ("index", 0x7F)):
                r, pl = fec_of(p, j, 0)
                r[field][0], r["base_id"][0] = val, (int(r["base_id"][0]) + 7) % 2**32
                head.append((r, pl))
            r, pl = fec_of(p, j, 0)
            r["base_id"][0] = (int(r["base_id"][0]) + 1) % 2**32  # a later parity with another base_id
            tail.append((r, pl))
        for p in range(P):
            if not len(groups_of[p]):
                continue
            for j in {len(groups_of[p]) // 2, len(groups_of[p]) - 1}:
                for d in (-1, plans[p].k):  # segments below and above the group's range
                    r, pl = seg_of(p, j, 0)
                    r["hdr"]["seq"][0] = (int(batches[p].base[j]) + d) % 2**32
                    tail.append((r, pl))
        p0 = next(p for p in range(P) if len(groups_of[p]))
        outside = [0, (fec_id0 - 2) % 65535 + 1] + ([rc.fec_id_of(fec_id0, G)] if G < 65535 else [])
        for fid in outside:  # fec_id 0, and ids outside the window on both sides (a full window has no outside)
            r, pl = seg_of(p0, 0, 0)
            r["fec_id"][0] = fid
            tail.append((r, pl))
            for p in anchoring[:1]:
                r, pl = fec_of(p, 0, 0)
                r["fec_id"][0] = fid
                tail.append((r, pl))
        for status in (-1, -2, -3, 1):
            r, pl = seg_of(p0, 0, 0)
            r["status"][0] = status
            tail.append((r, pl))
        r, pl = seg_of(p0, 0, 0)
        r["mid"][0] = 0x12
        tail.append((r, pl))
    if head or tail:
        nh, nt = len(head), len(tail)
        recs = np.concatenate([x[0] for x in head] + [recs] + [x[0] for x in tail])
        pay = np.concatenate([x[1] for x in head] + [pay] + [x[1] for x in tail])
        q = np.concatenate([rng.permutation(nh), nh + np.arange(len(recs) - nh - nt),
                            len(recs) - nt + rng.permutation(nt)])
        recs, pay = recs[q], pay[q]
    x = Inputs()
    x.case, x.plans, x.P, x.G, x.fec_id0 = c, plans, P, G, fec_id0
    x.capacity, x.stride, x.n = capacity, stride, len(recs)
    x.recs, x.payload = np.ascontiguousarray(recs), np.ascontiguousarray(pay)
    x.batches, x.groups_of, x.conflicts = batches, groups_of, conflicts
    # the sections' room, from the rule's own counts
    counts = regroup_shapes_ref(plans, [G] * P, G, fec_id0, x.recs, capacity, new_outputs(plans, [G] * P, G, x.n))["counts"]
    caps = [G] * P
    if room == "tight":
        big = next(p for p in range(P) if counts[p] >= 2)
        caps[big] = int(counts[big]) - 1
        caps[max(p for p in range(P) if p != big)] = 0
    elif room == "c64":
        caps = [64] * P
    x.caps = caps
    return x


# -- the rule ---------------------------------------------------------------------------------------------------
WINDOW = ("shape_of", "rank_of", "anchor_of", "counts", "slot_of")
SECTION = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "group_of")
_ALIGN = {"shape_of": 1, "rank_of": 4, "anchor_of": 4, "counts": 4, "slot_of": 4, "hdr": 4, "present": 8, "meta": 4,
          "fec_size": 2, "parity_present": 8, "base_id": 4, "src_of": 4, "group_of": 4}


def shapes_of(plans, caps, G, n):
    """name -> (dtype, shape) of the window outputs, and per section."""
    w = {"shape_of": (np.uint8, (G,)), "rank_of": (np.uint32, (G,)), "anchor_of": (np.uint32, (G,)),
         "counts": (np.uint32, (len(plans),)), "slot_of": (np.int32, (n,))}
    secs = []
    for plan, cap in zip(plans, caps):
        k, nl = plan.k, plan.n_lines
        secs.append({"hdr": (po.HDR_DTYPE, (cap, k)), "present": (np.uint64, (cap, 2)),
                     "meta": (po.HDR_DTYPE, (cap, nl)), "fec_size": (np.uint16, (cap, nl)),
                     "parity_present": (np.uint64, (cap,)), "base_id": (np.uint32, (cap,)),
                     "src_of": (np.uint32, (cap * (k + nl),)), "group_of": (np.uint32, (cap,))})
    return w, secs


def new_outputs(plans, caps, G, n, fill=FILL):
    w, secs = shapes_of(plans, caps, G, n)
    o = {name: np.zeros(shp, dt) for name, (dt, shp) in w.items()}
    o["sec"] = [{name: np.zeros(shp, dt) for name, (dt, shp) in s.items()} for s in secs]
    for a in list(o.values())[:-1] + [a for s in o["sec"] for a in s.values()]:
        a.view(np.uint8)[...] = fill
    return o


def regroup_shapes_ref(plans, caps, G, fec_id0, recs, capacity, out, wrong=()):
    """Rules 1-7 of rfec_wire_regroup_shapes (include/razor_fec.h) and what the call writes, in place over `out`
    (new_outputs' arrays, or views of an arena).  wrong: names of WRONG, each one rule bent."""
    assert set(wrong) <= set(WRONG)
    P, n = len(plans), len(recs)
    ks, nls = [p.k for p in plans], [p.n_lines for p in plans]
    slots = [k + nl for k, nl in zip(ks, nls)]
    key = {(p.k, p.row, p.col): i for i, p in enumerate(plans)}
    assert len(key) == P
    index = [[p.line[l].index for l in range(p.n_lines)] for p in plans]
    status, mid = recs["status"].tolist(), recs["mid"].tolist()
    fec_id, count, row, col = recs["fec_id"].tolist(), recs["count"].tolist(), recs["row"].tolist(), recs["col"].tolist()
    idx, dsize, rbase = recs["index"].tolist(), recs["data_size"].tolist(), recs["base_id"].tolist()
    seq = recs["hdr"]["seq"].tolist()
    code, group, line, acc = [0] * n, [0] * n, [0] * n, [None] * n
    anchor = [None] * G
    per_plan = {}  # (g, p) -> the first arrival accepted by p
    for r in range(n):  # rules 1-3
        if status[r] != 0 or mid[r] not in (SEG, FEC):
            code[r] = ENOTFEC
            continue
        f = fec_id[r]
        g = (f - fec_id0 if f >= fec_id0 else f + 65535 - fec_id0) if f else G
        if g >= G:
            code[r] = EWINDOW
            continue
        group[r] = g
        if mid[r] == FEC:
            p = key.get((count[r], row[r], col[r]))
            if p is None or idx[r] not in index[p] or dsize[r] > capacity:
                code[r] = ESHAPE
                continue
            acc[r], line[r] = p, index[p].index(idx[r])
            if anchor[g] is None:
                anchor[g] = r  # ascending r: the first stays
            per_plan.setdefault((g, p), r)
    if "anchor_per_plan" in wrong:  # the lowest plan that has an anchor of its own, not the first arrival
        for g in range(G):
            own = [per_plan[(g, p)] for p in range(P) if (g, p) in per_plan]
            anchor[g] = own[0] if own else None
    shape = [NOSHAPE if anchor[g] is None else acc[anchor[g]] for g in range(G)]
    base = [0 if anchor[g] is None else rbase[anchor[g]] for g in range(G)]
    rank, counts = [NONE] * G, [0] * P  # rule 4
    order = range(G)
    if "rank_by_arrival" in wrong:
        order = sorted(range(G), key=lambda g: NONE if anchor[g] is None else anchor[g])
    for g in order:
        if shape[g] != NOSHAPE:
            rank[g] = counts[shape[g]]
            counts[shape[g]] += 1
    src = [[NONE] * (caps[p] * slots[p]) for p in range(P)]
    slot_of = [0] * n
    for r in range(n):  # rules 3, 5, 6 and the contention of 7
        if code[r]:
            slot_of[r] = code[r]
            continue
        g = group[r]
        p = shape[g]
        if mid[r] == FEC:
            if acc[r] != p and not ("other_shape_placed" in wrong and line[r] < nls[p]):
                slot_of[r] = ESHAPE
                continue
            if rbase[r] != base[g]:
                slot_of[r] = EBASE
                continue
            s = ks[p] + line[r]
        else:
            if anchor[g] is None:
                slot_of[r] = ENOPARITY
                continue
            s = (seq[r] - base[g]) % 2**32
            if s >= ks[p]:
                slot_of[r] = EBASE
                continue
        c = rank[g]
        if c >= caps[p]:
            if "full_wraps" in wrong and caps[p]:
                c %= caps[p]
            else:
                slot_of[r] = EFULL
                continue
        slot_of[r] = c * slots[p] + s
        if src[p][slot_of[r]] == NONE:
            src[p][slot_of[r]] = r
    for r in range(n):
        if slot_of[r] >= 0 and src[shape[group[r]]][slot_of[r]] != r:
            slot_of[r] = EDUP
    out["shape_of"][...] = np.array(shape, np.uint8)
    out["rank_of"][...] = np.array(rank, np.uint32)
    out["anchor_of"][...] = np.array([NONE if a is None else a for a in anchor], np.uint32)
    out["counts"][...] = np.array([min(counts[p], caps[p]) if "counts_clamped" in wrong else counts[p]
                                   for p in range(P)], np.uint32)
    out["slot_of"][...] = np.array(slot_of, np.int32).reshape(out["slot_of"].shape)
    bits = np.uint64(1) << (np.arange(64, dtype=np.uint64))
    for p in range(P):  # "Written", per section
        cap, k, nl, o = caps[p], ks[p], nls[p], out["sec"][p]
        if not cap:
            continue
        group_of = np.full(cap, NONE, np.uint32)
        base_id = np.zeros(cap, np.uint32)
        for g in range(G):
            if shape[g] == p and rank[g] < cap:
                group_of[rank[g]], base_id[rank[g]] = g, base[g]
        o["group_of"][...], o["base_id"][...] = group_of, base_id
        o["src_of"][...] = np.array(src[p], np.uint32)
        srca = np.array(src[p], np.int64).reshape(cap, slots[p])
        filled = srca != NONE
        c_, s_ = np.nonzero(filled[:, :k])
        o["hdr"][c_, s_] = recs["hdr"][srca[c_, s_]]
        c_, l_ = np.nonzero(filled[:, k:])
        a = srca[c_, k + l_]
        o["meta"][c_, l_] = recs["hdr"][a]
        o["fec_size"][c_, l_] = recs["data_size"][a]
        m = np.zeros((cap, 128), bool)
        m[:, :k] = filled[:, :k]
        o["present"][:, 0] = (m[:, :64] * bits).sum(1, dtype=np.uint64)
        o["present"][:, 1] = (m[:, 64:] * bits).sum(1, dtype=np.uint64)
        pp = np.zeros((cap, 64), bool)
        pp[:, :nl] = filled[:, k:]
        o["parity_present"][...] = (pp * bits).sum(1, dtype=np.uint64)
    return out


def ref_outputs(x, wrong=()):
    return regroup_shapes_ref(x.plans, x.caps, x.G, x.fec_id0, x.recs, x.capacity,
                              new_outputs(x.plans, x.caps, x.G, x.n), wrong)


def compare(got, exp, what):
    """The five window outputs and every section's eight tables, byte for byte (what the call leaves alone holds
    FILL in both)."""
    bad = []
    pairs = [(name, got[name], exp[name]) for name in WINDOW]
    pairs += [(f"sections[{p}].{name}", got["sec"][p][name], exp["sec"][p][name])
              for p in range(len(exp["sec"])) for name in SECTION]
    for name, a, b in pairs:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            d = np.nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1))[0]
            bad.append(f"{name}: {len(d)} bytes differ, the first at offset {int(d[0])}")
    assert not bad, f"{what}: " + "; ".join(bad)


def check_equivalence(x, out, per_plan, what):
    """The header's "Equivalence": `out` (the shapes call's outputs) against per_plan[p], the eight tables of
    rfec_wire_regroup_index(&plans[p], ...) on the same records (ic.TABLES).  Returns the rows compared."""
    G, rows = x.G, 0
    f = x.recs["fec_id"].astype(np.int64)
    g_rec = np.where(f >= x.fec_id0, f - x.fec_id0, f + 65535 - x.fec_id0)
    valid = (x.recs["status"] == 0) & np.isin(x.recs["mid"], (SEG, FEC)) & (f != 0) & (g_rec < G)
    for p, plan in enumerate(x.plans):
        k, nl, cap = plan.k, plan.n_lines, x.caps[p]
        slots, t, s = k + nl, per_plan[p], out["sec"][p]
        gs = np.nonzero((out["shape_of"] == p) & (out["rank_of"] < cap))[0]
        cs = out["rank_of"][gs].astype(np.int64)
        rows += len(gs)
        for name, a, b in (("hdr", s["hdr"][cs], t["hdr"][gs]), ("present", s["present"][cs], t["present"][gs]),
                           ("meta", s["meta"][cs], t["meta"][gs]), ("fec_size", s["fec_size"][cs], t["fec_size"][gs]),
                           ("parity_present", s["parity_present"][cs], t["parity_present"][gs]),
                           ("base_id", s["base_id"][cs], t["base_id"][gs]),
                           ("src_of", s["src_of"].reshape(cap, slots)[cs], t["src_of"].reshape(G, slots)[gs])):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (what, p, name)
        assert np.array_equal(s["group_of"][cs], gs), (what, p, "group_of")
        rank_of_g = np.full(G, -1, np.int64)
        rank_of_g[gs] = cs
        r = np.nonzero(valid & (rank_of_g[np.minimum(g_rec, G - 1)] >= 0))[0]
        theirs = t["slot_of"][r].astype(np.int64)
        g = g_rec[r]
        mine = np.where(theirs >= 0, theirs - (g - rank_of_g[g]) * slots, theirs)
        assert np.array_equal(out["slot_of"][r], mine), (what, p, "slot_of")
    return rows


def conditions(x, ref):
    """What the case's records exercise, from the rule's own outputs."""
    so = ref["slot_of"]
    c = {f"code{e}": bool((so == e).any()) for e in (ENOTFEC, EWINDOW, ESHAPE, ENOPARITY, EBASE, EDUP, EFULL)}
    c["placed"] = bool((so >= 0).any())
    c["wrap"] = x.fec_id0 + x.G > 65536 and x.G < 65535
    c["shapes"] = len(set(ref["shape_of"].tolist()) - {NOSHAPE})
    c["no_shape_group"] = bool((ref["shape_of"] == NOSHAPE).any())
    c["overflow"] = bool((ref["counts"] > np.array(x.caps)).any())
    c["cap0"] = 0 in x.caps
    c["mask_hi"] = any(bool(s["present"][:, 1].any()) for s, cap in zip(ref["sec"], x.caps) if cap)
    # conflict "later": the foreign parity is ESHAPE and the group kept its own shape; "refused": likewise, and the
    # refused parity has the lowest arrival index of the group's SIM_FECs
    later = refused = 0
    for kind, g, a, b in x.conflicts:
        fid = rc.fec_id_of(x.fec_id0, g)
        mine = np.nonzero((x.recs["mid"] == FEC) & (x.recs["fec_id"] == fid))[0]
        foreign = [r for r in mine if x.recs["count"][r] == x.plans[b].k and x.recs["row"][r] == x.plans[b].row]
        ok = ref["shape_of"][g] == a and all(so[r] == ESHAPE for r in foreign) and len(foreign) >= 1
        if kind == "later":
            later += ok and all(x.recs["data_size"][r] <= x.capacity for r in foreign) and \
                max(foreign) > ref["anchor_of"][g]
        else:
            refused += ok and min(foreign) == mine[0] and x.recs["data_size"][min(foreign)] == x.capacity + 1
    c["conflict_later"], c["conflict_refused"] = later, refused
    c["rank_edges"] = x.case[5] == "edges" and all(ref["shape_of"][g] == 0 for g in EDGE_POSITIONS)
    return c


# -- engines ----------------------------------------------------------------------------------------------------
class ShapesEngine:
    """run(x) -> the outputs (new_outputs' names, shapes and types) of one call with every buffer in one guarded
    arena: recs, the five window outputs and the eight tables of every section with cap > 0 (a section with
    cap == 0 gets NULL pointers).  mutate (tests): called with the arena after the call and before its checks."""

    be = None
    mutate = None

    def run(self, x):
        w, secs = shapes_of(x.plans, x.caps, x.G, x.n)
        bufs = [ga.Buf("recs", x.n * 64, x.recs, "in", 16)]
        for name, (dt, shp) in w.items():
            bufs.append(ga.Buf(name, int(np.prod(shp)) * np.dtype(dt).itemsize, FILL, "out", _ALIGN[name]))
        for p, s in enumerate(secs):
            if x.caps[p]:
                for name, (dt, shp) in s.items():
                    bufs.append(ga.Buf(f"{name}{p}", int(np.prod(shp)) * np.dtype(dt).itemsize, FILL, "out",
                                       _ALIGN[name]))
        A = ga.Arena(self.be, bufs)
        self._run(x, A)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_regroup_shapes {case_id(x.case)}")
        out = {name: A.get(name, dt, shp) for name, (dt, shp) in w.items()}
        out["sec"] = [{name: A.get(f"{name}{p}", dt, shp) if x.caps[p] else np.zeros(shp, dt)
                       for name, (dt, shp) in s.items()} for p, s in enumerate(secs)]
        return out


class RefShapes(ShapesEngine):
    def __init__(self, wrong=()):
        self.be, self.wrong = ga.NumpyBackend(), wrong

    def _run(self, x, A):
        w, secs = shapes_of(x.plans, x.caps, x.G, x.n)
        out = {name: A.view(name).view(dt).reshape(shp) for name, (dt, shp) in w.items()}
        out["sec"] = [{name: A.view(f"{name}{p}").view(dt).reshape(shp) if x.caps[p] else np.zeros(shp, dt)
                       for name, (dt, shp) in s.items()} for p, s in enumerate(secs)]
        regroup_shapes_ref(x.plans, x.caps, x.G, x.fec_id0, A.view("recs").view(po.WIRE_REC), x.capacity, out,
                           self.wrong)


def sections_of(x, ptr):
    """The call's `sections` argument: ptr(name, p) -> the device address of section p's table."""
    return [dict(cap=x.caps[p], **{name: ptr(name, p) if x.caps[p] else None for name in SECTION})
            for p in range(x.P)]


class GpuShapes(ShapesEngine):
    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)

    def _run(self, x, A):
        self.lib.wire_regroup_shapes(x.plans, sections_of(x, lambda name, p: A.ptr(f"{name}{p}")), x.G, x.fec_id0,
                                     x.n, A.ptr("recs"), x.capacity, *(A.ptr(name) for name in WINDOW),
                                     self.torch.cuda.current_stream(self.device).cuda_stream)


def swap_two_group_of(x, ref):
    """A mutation of the arena: two filled group_of entries of one section swapped."""
    p = next(p for p in range(x.P) if min(x.caps[p], int(ref["counts"][p])) >= 2)

    def mutate(A):
        v = A.view(f"group_of{p}")
        t = v[0:4].copy() if isinstance(v, np.ndarray) else v[0:4].clone()
        v[0:4] = v[4:8]
        v[4:8] = t

    return mutate
