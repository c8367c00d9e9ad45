"""Windows, the ragged numbering, numpy restatements and engines for
rfec_recover_indexed_window_each_out and rfec_recover_deliver_each (the one-launch
window decode and the deliver with an out-slot count per section), shared by the
CPU and the GPU tests of test_recover_window_each.py and
test_recover_deliver_each.py.  Everything is built on window_cases,
deliver_cases, guarded_arena and gpu_engine, which stay as they are.

The ragged numbering (include/razor_fec.h): first[p] is the sum of groups[q]
over q < p and slot_first[p] the sum of groups[q] * per_group[q] over q < p;
recovered is indexed by output row first[p] + c; out_index, out_hdr and
out_shards by slot slot_first[p] + c * per_group[p] + e with e < per_group[p].

A window is (name, geometry, variant, sections); a section is a window_cases
spec with the section's own per_group behind its groups:
  ("ic" | "mw" | "rw", what, groups, E[, sparse])   and   ("stairs", k, None, E)
so each section's Inputs and reference (indexed_cases.reference: the oracle over
the gathered batch) are those of its single-shape call at ITS per_group.
window_each_ref lays the sections' references out ragged; section_view reads a
section back out of ragged arrays by the rule, or by one of the bent rules of
WRONG_VIEW.  deliver_each_ref restates rfec_recover_deliver_each's rule, with
deliver_cases' bent rules and those of WRONG_DELIVER.
"""
from __future__ import annotations

import copy
import zlib

import numpy as np

import deliver_cases as dc
import guarded_arena as ga
import indexed_cases as ic
import matrix_wide_cases as mw
import pyoracle as po
import recover_shapes_cases as rsc
import regroup_cases as rc
import rows_wide_cases as rw
import window_cases as wc

FILL = ic.FILL
NONE = ic.NONE
HOLE = dc.HOLE
WINDOW_EACH_TAG = 9  # rfec_indexed_last_path (rfec_internal.h): WINDOW_EACH_TAG | sections launched << 8
DELIVER_EACH = 10    # DELIVER_EACH | launches << 8
GEOMS = wc.GEOMS

# bent readings of the ragged arrays: a slot taken as o * (the call's largest E) + e; slot_first[p] taken as
# first[p] * E[p]; the row pitch of the neighbouring section
WRONG_VIEW = ("o_times_max_E", "slot_first_is_first_times_E", "neighbour_E")
# the same three in the deliver's rule, and the count taken over the least E of the call
WRONG_DELIVER = WRONG_VIEW + ("count_over_min_E",)


def first_slots(groups, E):
    """(first, slot_first), each [n + 1] (razor_amd.fec.window_first_slots restated)."""
    first, slot_first = [0], [0]
    for g, e in zip(groups, E):
        first.append(first[-1] + g)
        slot_first.append(slot_first[-1] + (g * e if g else 0))
    return np.array(first, np.int64), np.array(slot_first, np.int64)


def _slot_index(W, p, wrong=()):
    """[groups[p]][E[p]] slot numbers of section p's out slots, by the rule or a bent one (kept inside the arrays)."""
    g, E = W.groups[p], W.E[p]
    c, e = np.arange(g)[:, None], np.arange(E)[None, :]
    live = [q for q in range(len(W.groups)) if W.groups[q]]
    if "o_times_max_E" in wrong:
        s = (W.first[p] + c) * max(W.E[q] for q in live) + e
    elif "slot_first_is_first_times_E" in wrong:
        s = W.first[p] * E + c * E + e
    elif "neighbour_E" in wrong:
        i = live.index(p)
        s = W.slot_first[p] + c * W.E[live[i + 1 if i + 1 < len(live) else i - 1]] + e
    else:
        s = W.slot_first[p] + c * E + e
    return s % max(int(W.slot_first[-1]), 1)


def section_view(W, arrays, p, wrong=()):
    """Section p's (out_shards [g][E][stride], out_hdr [g][E], out_index [g][E], recovered [g][2]) out of the
    call's ragged arrays (out_shards [S][stride], out_hdr [S], out_index [S], recovered [R][2])."""
    sh, hd, ix, rec = arrays
    s = _slot_index(W, p, wrong)
    return sh[s], hd[s], ix[s], rec[int(W.first[p]):int(W.first[p + 1])]


def window_each_ref(W, prefilled=False):
    """The call's four arrays from the sections' own references, laid out ragged.  prefilled: bytes [16 CD, stride)
    of every out slot hold FILL (what a run over pre-filled arrays leaves)."""
    S, R = int(W.slot_first[-1]), int(W.first[-1])
    sh = np.full((S, W.stride), FILL, np.uint8)
    hd = np.zeros(S, po.HDR_DTYPE)
    ix = np.full(S, HOLE, np.uint8)
    rec = np.zeros((R, 2), np.uint64)
    for p in wc.launched(W):
        a, b = int(W.slot_first[p]), int(W.slot_first[p + 1])
        r = W.ref[p]
        sh[a:b], hd[a:b], ix[a:b] = r[0].reshape(b - a, W.stride), r[1].reshape(-1), r[2].reshape(-1)
        rec[int(W.first[p]):int(W.first[p + 1])] = r[3]
    if prefilled:
        sh[:, rc.cd16(W.capacity):] = FILL
    return sh, hd, ix, rec


# -- windows --------------------------------------------------------------------------------------------------------------
def _spec3(spec):
    return spec[:3] + spec[4:] if spec[0] != "stairs" else spec[:2]


def _mixed(sizes):
    """Five sections, all four families, a small E before a large one and after: one group of 1 x 3 rows at E = 3
    first (an odd slot count: the slot base of every later section is no multiple of its own E), the (10, 3, 4)
    matrix at E = 6, rows 4 x 3 at E = 2, the k = 17 matrix at E = 17, rows 1 x 30 at E = 1."""
    a, b, c, d = sizes
    return [("rw", (3, 3), 1, 3), ("ic", "full3x4k10", a, 6), ("ic", "rows12x3", b, 2), ("mw", 17, c, 17),
            ("rw", (30, 30), d, 1)]


def _reversed_keep_first(secs):
    return secs[:1] + secs[:0:-1]


def _thirty_two():
    """32 sections cycling the four families with 2..5 groups, every seventh empty; E cycles 1, 2, 3 and k."""
    ks = {"full3x4k10": 10, "rows12x3": 12, 17: 17, (5, 5): 5}
    out = []
    for p in range(32):
        kind, what = wc._CYCLE[p % 4]
        E = (1, 2, 3, ks[what])[(p // 4 + p) % 4]
        out.append((kind, what, 0 if p % 7 == 3 else 2 + (p * 3) % 4, E))
    return out


# (the last size is even or odd so that in both orders every section's slot base is no multiple of its E > 1)
_SIZES = {"c15": (257, 255, 256, 4), "c20": (7, 5, 5, 63), "c1200": (3, 2, 2, 4)}
MIXED = [(f"each-{g}{'-reversed' if r else ''}-{v}", g, v, _reversed_keep_first(_mixed(n)) if r else _mixed(n))
         for g, n in _SIZES.items() for r in (False, True) for v in ("clean", "tampered")]
WINDOWS = MIXED + [
    # the staircases of k = 100 at E = 10 between two sections at E = 3: a cascade's intermediates go through the
    # group's own out slots, which lie slot_first[1] = 9 slots into the arrays -- no multiple of 10
    ("staircase", "c20", "clean", [("ic", "rows12x3", 3, 3), ("stairs", 100, None, 10), ("ic", "full3x4k10", 4, 3)]),
    ("thirty-two", "c20", "tampered", _thirty_two()),
    # an empty first, middle and last section, of plans the call refuses and with a per_group out of range
    ("empties", "c20", "tampered", [("ic", "hand6", 0, 0), ("mw", 17, 4, 5), ("ic", "k10col3", 0, 200),
                                    ("rw", (5, 5), 3, 2), ("ic", "k1", 0, 7)]),
    ("sparse", "c15", "tampered", [("ic", "rows10x4", 7, 3, True), ("mw", 17, 40, 4, True),
                                   ("rw", (11, 5), 40, 11, True), ("ic", "full3x4k10", 7, 2, True)]),
    # two wide sections whose maps have as many words (5 x 26 = 10 x 13): the self-tests swap them
    ("swap", "c20", "clean", [("mw", 17, 5, 3), ("rw", (11, 5), 10, 2)]),
]
WINDOW = {w[0]: w for w in WINDOWS}


def window_id(w):
    return w[0]


def join_each(name, geom, plans, xs, refs, Es):
    """window_cases.join with an E per section."""
    W = wc.Window()
    W.name, W.geom, W.E = name, geom, [int(e) for e in Es]
    W.capacity, W.stride = GEOMS[geom]
    W.plans, W.x, W.ref = list(plans), list(xs), list(refs)
    W.groups = [x.G if x is not None else 0 for x in xs]
    W.names = [x.case[0] if x is not None else None for x in xs]
    W.src_of, pools, base = [], [], 0
    for x, E in zip(xs, W.E):
        if x is None:
            W.src_of.append(None)
            continue
        assert (x.capacity, x.stride, x.E) == (W.capacity, W.stride, E)
        so = x.src_of.copy()
        so[so != NONE] += np.uint32(base)
        W.src_of.append(so)
        pools.append(x.rows)
        base += x.n_rows
    W.rows = np.concatenate(pools) if base else np.zeros((0, W.stride), np.uint8)
    W.n_rows = base
    W.first, W.slot_first = first_slots(W.groups, W.E)
    return W


def make_window(o, w, cache=None):
    name, geom, variant, secs = w
    cache = {} if cache is None else cache
    plans, xs, refs, Es = [], [], [], []
    for spec in secs:
        Es.append(spec[3])
        if spec[0] != "stairs" and not spec[2]:
            plans.append(ic.PLANS[spec[1]](o) if spec[0] == "ic" else mw.wide_plan(o, spec[1]) if spec[0] == "mw"
                         else rw.rows_plan(o, *spec[1]))
            xs.append(None), refs.append(None)
            continue
        key = (spec, geom, variant)
        if key not in cache:
            x = wc.section_inputs(o, _spec3(spec), geom, spec[3], variant == "tampered")
            cache[key] = (x, ic.reference(o, x))
        x, ref = cache[key]
        plans.append(x.plan), xs.append(x), refs.append(ref)
    return join_each(name, geom, plans, xs, refs, Es)


def from_uniform(W):
    """A window_cases window (one E) as one of these."""
    V = copy.copy(W)
    V.E = [W.E] * len(W.plans)
    V.first, V.slot_first = first_slots(V.groups, V.E)
    return V


def padded(W, extra):
    xs, refs = [], []
    for x, ref in zip(W.x, W.ref):
        if x is None:
            xs.append(None), refs.append(None)
        else:
            y, r = wc.pad_section(x, ref, extra)
            xs.append(y), refs.append(r)
    return join_each(W.name + "-padded", W.geom, W.plans, xs, refs, W.E)


def empty_pool_window(o, geom="c20"):
    """A section of each family over an empty pool (n_rows == 0, rows NULL), all-absent tables, E = 3, 1, 17, 2."""
    import indexed_matrix_cases as imc
    Es = [3, 1, 17, 2]
    xs = [imc.empty_pool_inputs(o, 5, Es[0], geom), rsc.empty_rows_inputs(o, 6, Es[1], geom),
          mw.empty_pool_inputs(o, 17, 300, Es[2], geom), rw.empty_pool_inputs(o, 11, 5, 300, Es[3], geom)]
    for x in xs:
        x.family = wc.family_of(o, x.plan)
    assert [x.family for x in xs] == [1, 2, 3, 4]
    return join_each("empty-pool", geom, [x.plan for x in xs], xs, [None] * 4, Es)


# -- the window engine ----------------------------------------------------------------------------------------------------
_TABLES, _OUTS = rsc._TABLES, rsc._OUTS


def _ragged_bytes(name, rows, slots, stride):
    return {"recovered": rows * 16, "out_shards": slots * stride, "out_hdr": slots * 20, "out_index": slots}[name]


class GpuWindowEachDecode(wc.GpuWindowDecode):
    """run(W) -> per launched section p (its view of rfec_recover_indexed_window_each_out's ragged arrays, the four
    outputs of its single-shape call with per_group[p], its rows of rfec_recover_indexed_window_out when `uniform`),
    every buffer of all the calls in one guarded arena, the outputs pre-filled with FILL; guards and inputs are
    checked after the calls, the tags as they are made.  self.arrays: the call's four ragged arrays."""

    def run(self, W, pass_groups=True, swap=None, singles=True, uniform=False):
        stride = W.stride
        live = wc.launched(W)
        R, S = int(W.first[-1]), int(W.slot_first[-1])
        bufs = [ga.Buf("rows", W.rows.nbytes, W.rows, "in", 16)]
        for p in live:
            x = W.x[p]
            src = {"src_of": W.src_of[p], "hdr": x.hdr, "present": x.present, "meta": x.meta, "fec_size": x.fec_size,
                   "parity_present": x.parity_present}
            bufs += [ga.Buf(f"{name}{p}", src[name].nbytes, src[name], "in", align) for name, align in _TABLES]
        bufs += [ga.Buf(name, _ragged_bytes(name, R, S, stride), FILL, "out", align) for name, align in _OUTS]
        if uniform:
            assert len({W.E[p] for p in live}) == 1 and S == R * W.E[live[0]]
            bufs += [ga.Buf(f"u_{name}", _ragged_bytes(name, R, S, stride), FILL, "out", align)
                     for name, align in _OUTS]
        if singles:
            for p in live:
                g = W.groups[p]
                bufs += [ga.Buf(f"{name}{p}", rsc._out_bytes(name, g, W.E[p], stride), FILL, "out", align)
                         for name, align in _OUTS]
                if W.x[p].family == 2:
                    bufs.append(ga.Buf(f"workspace{p}", max(16, self.lib.workspace_size(W.plans[p], g)), 0x11,
                                       "scratch", 16))
        A = ga.Arena(self.be, bufs)
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        sections = []
        for p in range(len(W.plans)):
            if not W.groups[p]:
                sections.append(dict(cap=0))
                continue
            q = p if swap is None or p not in swap else swap[1 - swap.index(p)]
            sections.append(dict(cap=W.groups[p], src_of=A.ptr(f"src_of{q}"),
                                 **{name: A.ptr(f"{name}{p}") for name, _ in _TABLES[1:]}))
        rows = A.ptr("rows") if W.n_rows else None
        groups = W.groups if pass_groups else None
        assert self.lib.recover_window_slots(sections, groups, W.E) == S
        self.lib.recover_indexed_window_each_out(W.plans, sections, groups, stride, W.capacity, rows, W.n_rows,
                                                 A.ptr("recovered"), W.E, A.ptr("out_shards"), A.ptr("out_hdr"),
                                                 A.ptr("out_index"), st)
        self.last_path = self._path()
        if uniform:
            self.lib.recover_indexed_window_out(W.plans, sections, groups, stride, W.capacity, rows, W.n_rows,
                                                A.ptr("u_recovered"), W.E[live[0]], A.ptr("u_out_shards"),
                                                A.ptr("u_out_hdr"), A.ptr("u_out_index"), st)
            self.uniform_path = self._path()
        self.single_paths = {}
        if singles:
            for p in live:
                g = W.groups[p]
                args = (W.plans[p], g, stride, W.capacity, rows, W.n_rows,
                        *(A.ptr(f"{name}{p}") for name, _ in _TABLES), A.ptr(f"recovered{p}"), W.E[p],
                        A.ptr(f"out_shards{p}"), A.ptr(f"out_hdr{p}"), A.ptr(f"out_index{p}"))
                family = W.x[p].family
                if family == 1:
                    self.lib.recover_indexed_matrix_out(*args, st)
                elif family == 2:
                    self.lib.recover_indexed_out(*args, A.ptr(f"workspace{p}"), st)
                elif family == 3:
                    self.lib.recover_indexed_matrix_wide_out(*args, st)
                else:
                    self.lib.recover_indexed_rows_wide_out(*args, st)
                self.single_paths[p] = self._path()
        self.be.sync()
        A.check(f"recover_indexed_window_each_out {W.name}")

        def ragged(prefix):
            return (A.get(f"{prefix}out_shards", np.uint8, (S, stride)), A.get(f"{prefix}out_hdr", po.HDR_DTYPE, (S,)),
                    A.get(f"{prefix}out_index", np.uint8, (S,)), A.get(f"{prefix}recovered", np.uint64, (R, 2)))

        self.arrays = ragged("")
        self.uniform_arrays = ragged("u_") if uniform else None
        out = {}
        for p in live:
            g, E = W.groups[p], W.E[p]
            single = (A.get(f"out_shards{p}", np.uint8, (g, E, stride)), A.get(f"out_hdr{p}", po.HDR_DTYPE, (g, E)),
                      A.get(f"out_index{p}", np.uint8, (g, E)), A.get(f"recovered{p}", np.uint64, (g, 2))) \
                if singles else None
            out[p] = (section_view(W, self.arrays, p), single,
                      section_view(W, self.uniform_arrays, p) if uniform else None)
        return out


# -- the deliver: cases, rule, engines ------------------------------------------------------------------------------------
def _Es(x):
    return list(x.E) if isinstance(x.E, (list, tuple)) else [int(x.E)] * x.P


def synth_each(name, Es, **kw):
    """deliver_cases.synth's window (shapes, ranks, sections, rooms) with Es[p % len(Es)] out slots a row in section
    p: the ragged out_index from deliver_cases' hole patterns per section, out_hdr and out_shards random bytes."""
    max_out = kw.pop("max_out", "T+3")
    unsorted = kw.pop("unsorted", False)
    x = dc.synth(name, E=1, **kw)
    rng = np.random.default_rng(zlib.crc32(f"each-{name}".encode()))
    x.E = [Es[p % len(Es)] for p in range(x.P)]
    x.first, x.slot_first = first_slots(x.rows, x.E)
    x.S = S = int(x.slot_first[-1])
    parts = [dc._patterns(rng, x.rows[p], x.E[p], unsorted).reshape(-1) for p in range(x.P) if x.rows[p]]
    x.out_index = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    x.out_hdr = rng.integers(0, 256, (S, 20), dtype=np.uint8).view(po.HDR_DTYPE).reshape(S)
    x.out_shards = rng.integers(0, 256, (S, x.stride), dtype=np.uint8)
    x.max_out = 0
    x.T = T = int(deliver_each_ref(x, dc.new_outputs(x))["n_out"][0])
    x.max_out = max_out if isinstance(max_out, int) else T + {"T": 0, "T-1": -1, "T+3": 3}[max_out]
    assert x.max_out >= 0
    return x


def each_from_tables(name, plans, caps, groups, G, fec_id0, shape_of, rank_of, group_of, capacity, stride, Es,
                     out_shards, out_hdr, out_index, max_out):
    """deliver_cases.from_tables over ragged tables."""
    x = dc.Case()
    x.name, x.geom, x.G, x.E, x.P, x.fec_id0 = name, None, G, list(Es), len(plans), fec_id0
    x.capacity, x.stride, x.plans, x.caps, x.groups = capacity, stride, plans, list(caps), groups
    x.rows = list(caps) if groups is None else list(groups)
    x.first, x.slot_first = first_slots(x.rows, x.E)
    x.R, x.S = int(x.first[-1]), int(x.slot_first[-1])
    x.shape_of, x.rank_of = np.ascontiguousarray(shape_of, np.uint8), np.ascontiguousarray(rank_of, np.uint32)
    x.group_of = [np.ascontiguousarray(g, np.uint32) if x.rows[p] else None for p, g in enumerate(group_of)]
    x.out_index = np.ascontiguousarray(out_index, np.uint8).reshape(x.S)
    x.out_hdr = np.ascontiguousarray(out_hdr).view(po.HDR_DTYPE).reshape(x.S)
    x.out_shards = np.ascontiguousarray(out_shards, np.uint8).reshape(x.S, stride)
    x.max_out = 0
    x.T = int(deliver_each_ref(x, dc.new_outputs(x))["n_out"][0])
    x.max_out = max_out if max_out is not None else x.T + 3
    return x


def uniform_as_each(x):
    """A deliver_cases case (one E) as one of these: the same bytes, the slot arrays flat."""
    y = copy.copy(x)
    y.E = [x.E] * x.P
    y.first, y.slot_first = first_slots(x.rows, y.E)
    y.S = int(y.slot_first[-1])
    assert y.S == x.R * x.E
    y.out_index, y.out_hdr = x.out_index.reshape(y.S), x.out_hdr.reshape(y.S)
    y.out_shards = x.out_shards.reshape(y.S, x.stride)
    return y


def deliver_each_ref(x, out, wrong=()):
    """rfec_recover_deliver_each's rule (include/razor_fec.h: rfec_recover_deliver's rules 1-7 with rule 3 counting
    e < per_group[p] at slot slot_first[p] + c per_group[p] + e and rules 5 and 6 reading that slot), in place over
    `out`.  wrong: names of deliver_cases.WRONG or WRONG_DELIVER, each one rule bent."""
    assert set(wrong) <= set(dc.WRONG) | set(WRONG_DELIVER)
    P, G = x.P, x.G
    Es = _Es(x)
    first, slot_first = first_slots(x.rows, Es)  # rule 1
    S = int(slot_first[-1])
    w = rc.cd16(x.capacity)
    ix = x.out_index.reshape(-1)
    hdr, sh = x.out_hdr.reshape(-1), x.out_shards.reshape(-1, x.stride)
    limit = x.caps if "rank_past_groups_delivered" in wrong else x.rows
    live = [q for q in range(P) if x.rows[q]]
    slots = [[] for _ in range(G)]  # per window group, the slots of its row that deliver, in out-slot order
    o_of = np.full(G, -1, np.int64)
    for g in range(G):
        p, c = int(x.shape_of[g]), int(x.rank_of[g])
        if p >= P or c >= limit[p] or first[p] + c >= first[-1]:  # rule 2 (the last: a bent limit stays inside)
            continue
        E = Es[p]
        o_of[g] = first[p] + c
        if "o_times_max_E" in wrong:
            base = (first[p] + c) * max(Es[q] for q in live)
        elif "slot_first_is_first_times_E" in wrong:
            base = first[p] * E + c * E
        elif "neighbour_E" in wrong:
            i = live.index(p)
            base = slot_first[p] + c * Es[live[i + 1 if i + 1 < len(live) else i - 1]]
        else:
            base = slot_first[p] + c * E
        n = min(Es[q] for q in live) if "count_over_min_E" in wrong else E
        es = [int(base + e) % max(S, 1) for e in range(n)]
        es = [s for s in es if ix[s] != HOLE]  # rule 3
        if "slot_order_by_index_byte" in wrong:
            es = sorted(es, key=lambda s: ix[s])
        slots[g] = es
    n = np.array([len(s) for s in slots], np.int64)
    order = np.arange(G)  # rule 4
    if "section_order" in wrong:
        order = np.argsort(np.where(o_of >= 0, o_of, first[-1] + np.arange(G)), kind="stable")
    start = np.zeros(G, np.int64)
    start[order] = np.cumsum(n[order]) - n[order]
    T = int(n.sum())
    out["first_of"][:G] = start
    out["first_of"][G] = T
    out["n_out"][0] = min(T, x.max_out) if "n_out_clamped" in wrong else T
    for g in np.nonzero(n)[0]:  # rules 5-7
        for r, s in enumerate(slots[g]):
            j = int(start[g]) + r
            if j >= x.max_out:
                continue
            fid = (x.fec_id0 + int(g)) & 0xFFFF if "fec_id_no_wrap" in wrong else (x.fec_id0 - 1 + int(g)) % 65535 + 1
            out["seg"]["hdr"][j], out["seg"]["fec_id"][j], out["seg"]["reserved"][j] = hdr[s], fid, 0
            out["seg_payload"][j, :w] = sh[s, :w]
    return out


# Mixed-E deliver cases: name -> (Es cycled over the sections, keyword arguments of deliver_cases.synth)
_E4 = (3, 10, 1, 6)
CASES = {
    "G1": ((3,), dict(G=1, P=1, fec_id0=9)), "G255": (_E4, dict(G=255, P=4)), "G256": (_E4, dict(G=256, P=4)),
    "G257": (_E4, dict(G=257, P=4)), "G600": (_E4, dict(G=600, P=4)),
    "cd1": (_E4, dict(geom="c15", P=4)), "cd75": ((2, 5, 1), dict(geom="c1200")),
    "max-T": (_E4, dict(max_out="T", P=4)), "max-T-1": (_E4, dict(max_out="T-1", P=4)),
    "max-1": (_E4, dict(max_out=1, P=4)), "max-0": (_E4, dict(max_out=0, P=4)),
    # rows of holes before, between and after delivered slots in a large-E section (deliver_cases._patterns, E = 12)
    "large-E": ((2, 12, 3), dict(G=60)),
    "zero-first": (_E4, dict(zero=(0,), P=4)), "zero-middle": (_E4, dict(zero=(1,), P=4)),
    "zero-last": (_E4, dict(zero=(3,), P=4)),
    "below-counts": (_E4, dict(room="below", P=4)), "null-groups": (_E4, dict(room="null", sent=30, P=4)),
    "thirty-two": ((1, 2, 3, 7, 16), dict(P=32, G=100, zero=(3, 17))),
    "unsorted": (_E4, dict(unsorted=True, G=24, P=4)),
    # two sections with as many rows and as many slots a row: the self-test swaps their group_of pointers
    "swap": ((2,), dict(P=2, G=24, fec_id0=100, balanced=True)),
}


def make(name):
    Es, kw = CASES[name]
    return synth_each(name, Es, **kw)


class RefDeliverEach(dc.RefDeliver):
    def _run(self, x, sections, ptr, A):
        shp = dc.shapes_of(x)
        out = {name: A.view(name).view(shp[name][0]).reshape(shp[name][1]) for name in dc.OUTPUTS}
        deliver_each_ref(x, out, self.wrong)


class GpuDeliverEach(dc.GpuDeliver):
    """deliver_cases.GpuDeliver over rfec_recover_deliver_each."""

    def _run(self, x, sections, ptr, A):
        self.lib.lib.rfec_timing_events(None, None)
        self.lib.recover_deliver_each(x.plans, sections, x.groups, x.G, x.fec_id0, ptr["shape_of"], ptr["rank_of"],
                                      x.stride, x.capacity, _Es(x), ptr["out_shards"], ptr["out_hdr"],
                                      ptr["out_index"], x.max_out, ptr["seg"], ptr["seg_payload"], ptr["first_of"],
                                      ptr["n_out"], A.ptr("workspace"),
                                      self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_launches = int(self.lib.lib.rfec_timing_launches())
        self.last_path = int(self.lib.lib.rfec_indexed_last_path())


# -- the capability window: 1 x 3 groups beside a k = 100 frame -------------------------------------------------------------
class Capability:
    pass


CAP_LOST_100 = tuple(r * 10 + (2 * r + 1) % 10 for r in range(5))  # five members, distinct rows and columns


def capability_stream(o, G=9, fec_id0=65530, geom="c20"):
    """An in-order stream of G groups from fec_id0 (it crosses 65535 -> 1): every third group the planner's k = 100
    matrix at protect_fraction 10 (10 x 10), the others one row of k = 3.  A k = 100 group loses the five members
    CAP_LOST_100 (distinct rows and columns: every one comes back from its row at once) and keeps every parity; a
    k = 3 group loses member g % 3 and keeps its parity.  Group by group the segments, then the parities."""
    cap = Capability()
    cap.G, cap.fec_id0, cap.geom = G, fec_id0, geom
    cap.capacity, cap.stride = GEOMS[geom]
    cap.plans = [o.plan_matrix(3, 1, 3, rc.ROWS), o.plan_from_fraction(100, 10, rc.ROWS | rc.COLS)]
    cap.Es = [3, 10]
    cap.shape = np.array([1 if g % 3 == 1 else 0 for g in range(G)], np.uint8)
    rng = np.random.default_rng(zlib.crc32(b"capability"))
    recs, pay, dgram, dlen = [], [], [], []
    for g in range(G):  # one sender batch per window group: its datagrams carry the group's own fec_id
        plan = cap.plans[int(cap.shape[g])]
        k, n = plan.k, plan.n_lines
        b = rc.sender_batch(o, plan, 1, rc.fec_id_of(fec_id0, g), cap.capacity, cap.stride, rng,
                            np.array([5000 + g * 140], np.uint32))
        assert n and not b.status.any()
        lost = set(CAP_LOST_100) if k == 100 else {g % 3}
        keep = [i for i in range(k) if i not in lost] + [k + l for l in range(n)]
        recs.append(b.recs[keep]), pay.append(b.pay[keep]), dgram.append(b.dgram[keep]), dlen.append(b.dlen[keep])
    cap.recs, cap.pay = np.concatenate(recs), np.concatenate(pay)
    cap.dgram, cap.dlen = np.concatenate(dgram), np.concatenate(dlen).astype(np.uint16)
    return cap
