"""Cases, a numpy restatement of the rule and engines for rfec_wire_window_census
(the shapes of a parsed window, in window order, and the groups of each), shared
by the CPU and the GPU tests of test_wire_window_census.py.

A window is a list of parsed records synthesised in the record dtype (no payload
rows: the call reads none).  census_ref restates rules 1-5 of include/razor_fec.h
(rfec_wire_window_census); which indices a key's plan has comes from the
oracle's planner (lines_of_key), not from the product.  Each `wrong` switch
bends one rule: the case set must tell every bent rule from the right one.

An engine runs one call with every buffer in a guarded arena (guarded_arena.py):
    RefCensus   numpy memory, census_ref (the CPU run of the checks)
    GpuCensus   torch memory in HBM, the product library
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import regroup_cases as rc

FILL = rc.FILL
NONE = rc.NONE
SEG, FEC = rc.SEG, rc.FEC
MAX_SHAPES = 32
MAX_K = 128
TILE = 1024   # the groups of one tile of the shapes pass (fec.CENSUS_TILE, rfec_census_tile())
AHEAD = 4     # tiles whose keys a lane loads together (rfec_census.hip)

SHAPE = np.dtype([("k", "<u2"), ("row", "u1"), ("col", "u1"), ("groups", "<u4"), ("first_g", "<u4"),
                  ("reserved", "<u4")])
CENSUS = np.dtype([("n_shapes", "<u4"), ("other_groups", "<u4"), ("anchored", "<u4"), ("g_first", "<u4"),
                   ("g_end", "<u4"), ("n_seg", "<u4"), ("n_fec", "<u4"), ("n_refused", "<u4"), ("n_notfec", "<u4"),
                   ("n_window", "<u4"), ("reserved", "<u4", (6,)), ("shape", SHAPE, (MAX_SHAPES,))])
assert CENSUS.itemsize == 576

WRONG = ("anchor_first_fec", "shapes_by_arrival", "groups_count_records", "column_on_rows_only", "size_below_capacity")


# -- the plan of a key, from the oracle's planner ---------------------------------------------------------------------
def plannable(count, row, col):
    return 1 <= count <= MAX_K and row >= 1 and col >= 2 and row * col >= count


_lines = {}


def key_layers(o, count, row, col):
    """ROWS | COLS for the matrix key of its count (the planner's matrix mode), ROWS for any other key."""
    if count >= 6:
        _, mrow, mcol = o.num_packets(count, 255)
        if (row, col) == (mrow, mcol):
            return rc.ROWS | rc.COLS
    return rc.ROWS


def plan_of_key(o, count, row, col):
    return o.plan_matrix(count, row, col, key_layers(o, count, row, col))


def lines_of_key(o, count, row, col):
    """{index: line} of the plan a receiver takes for the key (the first line of an index), {} when unplannable."""
    key = (count, row, col)
    if key not in _lines:
        d = {}
        if plannable(*key):
            p = plan_of_key(o, *key)
            for l in range(p.n_lines - 1, -1, -1):
                d[p.line[l].index] = l
        _lines[key] = d
    return _lines[key]


# -- the rule ------------------------------------------------------------------------------------------------------
def census_ref(o, G, fec_id0, recs, capacity, wrong=()):
    """Rules 1-5 of rfec_wire_window_census: {"census": CENSUS scalar array [1], "anchor_of", "key_of"}."""
    assert set(wrong) <= set(WRONG)
    n = len(recs)
    status, mid = recs["status"].tolist(), recs["mid"].tolist()
    fec_id, count, row, col = recs["fec_id"].tolist(), recs["count"].tolist(), recs["row"].tolist(), recs["col"].tolist()
    idx, dsize = recs["index"].tolist(), recs["data_size"].tolist()
    c = np.zeros(1, CENSUS)
    anchor, akey, per_key_recs = {}, {}, {}
    g_lo, g_hi = NONE, 0
    for r in range(n):
        if status[r] != 0 or mid[r] not in (SEG, FEC):
            c["n_notfec"] += 1
            continue
        f = fec_id[r]
        g = (f - fec_id0 if f >= fec_id0 else f + 65535 - fec_id0) if f else G
        if g >= G:
            c["n_window"] += 1
            continue
        g_lo, g_hi = min(g_lo, g), max(g_hi, g + 1)
        if mid[r] == SEG:
            c["n_seg"] += 1
            continue
        key = (count[r], row[r], col[r])
        lines = lines_of_key(o, *key)
        ok = idx[r] in lines
        if "column_on_rows_only" in wrong and plannable(*key) and idx[r] >= 0x80 and (idx[r] & 0x7F) < key[2]:
            ok = True
        ok = ok and (dsize[r] < capacity if "size_below_capacity" in wrong else dsize[r] <= capacity)
        c["n_fec" if ok else "n_refused"] += 1
        if ok:
            per_key_recs[key] = per_key_recs.get(key, 0) + 1
        if (ok or "anchor_first_fec" in wrong) and g not in anchor:
            anchor[g], akey[g] = r, key  # ascending r: the first stays
    c["g_first"], c["g_end"] = g_lo, g_hi
    anchor_of = np.full(G, NONE, np.uint32)
    key_of = np.full(G, NONE, np.uint32)
    for g, r in anchor.items():
        k, rw, cl = akey[g]
        anchor_of[g], key_of[g] = r, (k | rw << 8 | cl << 16) & 0xFFFFFFFF
    c["anchored"] = len(anchor)
    first, groups = {}, {}
    for g in sorted(anchor):
        first.setdefault(akey[g], g)
        groups[akey[g]] = groups.get(akey[g], 0) + 1
    order = sorted(first, key=(lambda key: anchor[first[key]]) if "shapes_by_arrival" in wrong else first.get)
    listed = order[:MAX_SHAPES]
    c["n_shapes"] = len(listed)
    c["other_groups"] = sum(groups[key] for key in order[MAX_SHAPES:])
    for i, key in enumerate(listed):
        s = c["shape"]
        s["k"][0, i], s["row"][0, i], s["col"][0, i] = key[0] & 0xFFFF, key[1], key[2]
        s["groups"][0, i] = per_key_recs.get(key, 0) if "groups_count_records" in wrong else groups[key]
        s["first_g"][0, i] = first[key]
    return {"census": c, "anchor_of": anchor_of, "key_of": key_of}


def shapes_of_census(c):
    """[(k, row, col, groups, first_g)] of the listed shapes."""
    c = c.reshape(-1)[0]
    return [(int(s["k"]), int(s["row"]), int(s["col"]), int(s["groups"]), int(s["first_g"]))
            for s in c["shape"][:int(c["n_shapes"])]]


def compare(got, exp, what):
    """The census's 576 bytes, anchor_of and key_of, byte for byte."""
    bad = []
    for name in ("census", "anchor_of", "key_of"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            d = np.nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1))[0]
            detail = f" (got {a[0]}, expected {b[0]})" if name == "census" else ""
            bad.append(f"{name}: {len(d)} bytes differ, the first at offset {int(d[0])}{detail}")
    assert not bad, f"{what}: " + "; ".join(bad)


def check_equivalence(o, x, cen, reg_ref, what, order=None):
    """The header's "Equivalence", for a census with other_groups == 0: reg_ref(plans, caps) -> the outputs of
    rfec_wire_regroup_shapes on the same records (the rule, or the device's) with plans[i] the plan of shape[i] (taken
    in `order`) and cap = the shape's groups.  Returns the plans used."""
    c = cen["census"].reshape(-1)[0]
    assert c["other_groups"] == 0
    shapes = shapes_of_census(cen["census"])
    if order is not None:
        shapes = [shapes[i] for i in order]
    if not shapes:
        assert (cen["anchor_of"] == NONE).all() and (cen["key_of"] == NONE).all(), what
        return []
    plans = [plan_of_key(o, k, row, col) for k, row, col, _, _ in shapes]
    caps = [s[3] for s in shapes]
    out = reg_ref(plans, caps)
    assert np.array_equal(out["anchor_of"], cen["anchor_of"]), (what, "anchor_of")
    assert out["counts"].tolist() == caps, (what, "counts", out["counts"].tolist(), caps)
    index = {(k | row << 8 | col << 16): i for i, (k, row, col, _, _) in enumerate(shapes)}
    index[NONE] = 0xFF
    assert np.array_equal(out["shape_of"], np.array([index[int(k)] for k in cen["key_of"]], np.uint8)), (what, "shape_of")
    assert not (out["slot_of"] == -7).any(), (what, "EFULL")
    return plans


# -- windows ---------------------------------------------------------------------------------------------------------
class Inputs:
    pass


class Builder:
    """Records of one window in arrival order.  fec / seg append one record for window group g (any integer: the
    fec_id is the succession's, so g < 0 and g >= G fall outside the window)."""

    def __init__(self, name, G, fec_id0, capacity=20):
        self.name, self.G, self.fec_id0, self.capacity = name, G, fec_id0, capacity
        self.rows = []
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))

    def _rec(self, kind, g, **kw):
        r = np.zeros(1, po.WIRE_REC)
        r["mid"], r["ver"], r["uid"] = kind, 1, 77
        r["fec_id"] = rc.fec_id_of(self.fec_id0, g % 65535)
        r["base_id"] = 1000 + 140 * (g % 65535)
        r["data_size"] = 10
        r["reserved"] = self.rng.integers(0, 256, 17)  # the call reads none of it
        for k, v in kw.items():
            r[k] = v
        self.rows.append(r)
        return r

    def fec(self, g, key, index=0, **kw):
        return self._rec(FEC, g, count=key[0], row=key[1], col=key[2], index=index, **kw)

    def seg(self, g, i=0, **kw):
        r = self._rec(SEG, g, **kw)
        r["hdr"]["seq"] = 1000 + 140 * (g % 65535) + i
        return r

    def shuffle(self):
        self.rows = [self.rows[i] for i in self.rng.permutation(len(self.rows))]

    def done(self):
        x = Inputs()
        x.name, x.G, x.fec_id0, x.capacity = self.name, self.G, self.fec_id0, self.capacity
        x.recs = np.ascontiguousarray(np.concatenate(self.rows)) if self.rows else np.zeros(0, po.WIRE_REC)
        x.n = len(x.recs)
        return x


def strip(k):
    return (k, 1, k)  # one row of k: index 0 is its line


M10 = (10, 3, 4)      # the matrix key of 10: rows 0..2, columns 0x80..0x83
R9 = (9, 3, 4)        # rows only (the matrix key of 9 is (3, 3)); its last row has one member
M100 = (100, 10, 10)  # the matrix key of 100
KEYS3 = (M10, strip(3), R9)


def _sizes(G):
    """Up to 42 groups anchored, the first and the last among them, three keys, arrival shuffled."""
    b = Builder(f"size-G{G}", G, 65000)
    gs = sorted({0, G - 1} | set(b.rng.choice(G, min(G, 40), replace=False).tolist()))
    for j, g in enumerate(gs):
        key = KEYS3[j % 3]
        b.fec(g, key, index=j % 2)  # row 0 or 1: strip(3) has no row 1
        b.fec(g, key, index=0)
        b.seg(g, 1)
    b.shuffle()
    return b.done()


def _full_window():
    """65,535 groups, a few hundred records: anchors at the edges of the tiles and of the tiles loaded together."""
    G = 65535
    b = Builder("size-G65535", G, 40000)
    edges = [0, TILE - 1, TILE, AHEAD * TILE - 1, AHEAD * TILE, 63 * TILE, 63 * TILE + 1, G - 1]
    gs = sorted(set(edges) | set(b.rng.choice(G, 150, replace=False).tolist()))
    keys = [M10, strip(2), M100, strip(77)]
    for j, g in enumerate(gs):
        # two keys first seen in the window's last tile
        b.fec(g, keys[j % 4] if g not in (63 * TILE + 1, G - 1) else strip(5 + (g == G - 1)))
        if j % 3 == 0:
            b.seg(g)
    b.shuffle()
    return b.done()


def _second_tile():
    """A key first seen in the second tile; the first tile's key goes on there."""
    b = Builder("second-tile", 2 * TILE + 1, 100)
    for g in (3, 500, TILE - 1, TILE + 900, 2 * TILE):
        b.fec(g, M10)
    for g in (TILE + 5, TILE + 6, 2 * TILE - 1):
        b.fec(g, strip(7))
    return b.done()


def _two_in_one_tile():
    """Two keys new in the second tile: B's first group lies before A's in the window, A's parity arrives first, and
    A's lane within its wave (5) is below B's (10).  A third key, new in the same tile, comes after both."""
    b = Builder("two-new-keys", 2 * TILE, 65000)
    A, B, C_ = strip(4), strip(6), strip(8)
    b.fec(TILE + 64 + 5, A)
    b.fec(TILE + 999, C_)
    b.fec(TILE + 10, B)
    b.fec(TILE + 700, B)
    b.fec(TILE + 701, A)
    b.fec(2, M10)
    return b.done()


def _many(S):
    """S shapes, shape i first at group 2 i.  The 33rd shape's groups lie before and after the later groups of the
    first listed shape; with S >= 33 they count in other_groups."""
    b = Builder(f"shapes-{S}", 300, 65400)  # the window crosses 65535 -> 1
    for i in range(S):
        b.fec(2 * i, strip(2 + i))
    for g in (100, 200):
        b.fec(g, strip(2))
    if S >= 33:
        for g in (150, 250):
            b.fec(g, strip(2 + 32))
    b.fec(299, strip(2 + S - 1))
    b.shuffle()
    return b.done()


def _rules():
    """Every refusal and every counter, in a window of 12 groups across 65535 -> 1."""
    cap = 20
    b = Builder("rules", 12, 65530, cap)
    # group 0: its lowest-arrival SIM_FEC is refused (col 1), the next, of another key, accepted
    b.fec(0, (3, 3, 1))
    b.fec(0, strip(3))
    b.fec(0, M10)                      # accepted, later: not the anchor
    # group 1: two accepted parities of one key (the group counts once), segments
    b.fec(1, M10, 0x82)
    b.fec(1, M10, 1)
    b.seg(1, 0), b.seg(1, 1)
    # group 2: segments only
    b.seg(2, 0), b.seg(2, 5)
    # group 3: refused keys only
    b.fec(3, (0, 1, 2))                # k = 0
    b.fec(3, (129, 1, 129))            # k = 129
    b.fec(3, (10, 3, 3))               # row * col < k
    b.fec(3, (2, 2, 1))                # col 1
    # group 4: indices that are no line
    b.fec(4, R9, 3)                    # a row index >= rows
    b.fec(4, R9, 2)                    # the last row, of one member
    b.fec(4, R9, 0x80)                 # a column on a rows-only key
    b.fec(4, R9, 0x81)
    b.fec(4, M10, 0x80 | 4)            # 0x80 | col on a matrix key
    b.fec(4, M10, 0x7F)
    b.fec(4, (4, 2, 4), 1)             # a row that lies past k
    # group 5: data_size = capacity + 1 refused, then capacity accepted
    b.fec(5, strip(5), data_size=cap + 1)
    b.fec(5, strip(5), data_size=cap)
    # group 6: only an oversize parity; group 7: a column of the matrix key; group 11: the last group
    b.fec(6, strip(5), data_size=cap + 1)
    b.fec(7, M10, 0x83)
    b.fec(11, M100, 0x89)
    b.fec(10, M100, 9)
    b.fec(9, (100, 20, 5), 19)         # rows only, 20 rows
    b.fec(8, (128, 64, 2), 63)         # 64 row lines
    b.fec(8, (128, 64, 2), 64)
    # outside the window: fec_id 0, the id before fec_id0, g == groups
    b.fec(0, M10, fec_id=0), b.seg(0, fec_id=0)
    b.fec(-1, M10), b.seg(-1)
    b.fec(12, M10), b.seg(12)
    # not FEC traffic: a status other than OK, control mids
    for status in (-1, -2, -3, 1):
        b.fec(1, M10, status=status)
    b.seg(1, status=-1)
    b.fec(1, M10, mid=0x12), b.seg(1, mid=0x10)
    return b.done()


def _segments_only():
    b = Builder("segments-only", 9, 7)
    for g in (2, 3, 6):
        b.seg(g, 0), b.seg(g, 1)
    return b.done()


def _empty():
    return Builder("no-records", 9, 7).done()


def make_cases():
    return [_sizes(G) for G in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)] + [
        _full_window(), _second_tile(), _two_in_one_tile(), *(_many(S) for S in (31, 32, 33, 34)), _rules(),
        _segments_only(), _empty()]


def conditions(x, ref):
    c = ref["census"][0]
    return {"refused": int(c["n_refused"]), "notfec": int(c["n_notfec"]), "window": int(c["n_window"]),
            "seg": int(c["n_seg"]), "other": int(c["other_groups"]), "full_list": int(c["n_shapes"] == MAX_SHAPES),
            "wrap": int(x.fec_id0 + x.G > 65536 and x.G < 65535), "unanchored": int(c["anchored"] < x.G),
            "empty": int(x.n == 0), "G1": int(x.G == 1), "G65535": int(x.G == 65535)}


# -- engines ---------------------------------------------------------------------------------------------------------
class CensusEngine:
    """run(x) -> {"census", "anchor_of", "key_of"} of one call with recs and the three outputs in one guarded arena,
    each at exactly its documented alignment.  mutate (tests): called with the arena after the call and before its
    checks.  last_path: the call's launch tag (0 where the engine has none)."""

    be = None
    mutate = None
    last_path = 0

    def run(self, x, groups=None):
        G = x.G if groups is None else groups
        A = ga.Arena(self.be, [ga.Buf("recs", x.n * 64, x.recs, "in", 16), ga.Buf("census", 576, FILL, "out", 16),
                               ga.Buf("anchor_of", x.G * 4, FILL, "out", 4), ga.Buf("key_of", x.G * 4, FILL, "out", 4)])
        self._run(x, G, A)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_window_census {x.name}")
        return {"census": A.get("census", CENSUS, (1,)), "anchor_of": A.get("anchor_of", np.uint32, (x.G,)),
                "key_of": A.get("key_of", np.uint32, (x.G,))}


class RefCensus(CensusEngine):
    def __init__(self, o, wrong=()):
        self.be, self.o, self.wrong = ga.NumpyBackend(), o, wrong

    def _run(self, x, G, A):
        if G == 0:
            return
        out = census_ref(self.o, G, x.fec_id0, A.view("recs").view(po.WIRE_REC), x.capacity, self.wrong)
        A.view("census")[...] = out["census"].view(np.uint8).reshape(-1)
        A.view("anchor_of").view(np.uint32)[...] = out["anchor_of"]
        A.view("key_of").view(np.uint32)[...] = out["key_of"]


class GpuCensus(CensusEngine):
    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)

    def _run(self, x, G, A):
        self.lib.wire_window_census(G, x.fec_id0, x.n, A.ptr("recs"), x.capacity, A.ptr("census"), A.ptr("anchor_of"),
                                    A.ptr("key_of"), self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_path = self.lib.census_last_path()


def swap_two_shapes(A):
    """A mutation of the arena: shape[0] and shape[1] of the census swapped."""
    v = A.view("census")
    t = v[64:80].copy() if isinstance(v, np.ndarray) else v[64:80].clone()
    v[64:80] = v[80:96]
    v[80:96] = t
