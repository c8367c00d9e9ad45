"""Windows, inputs and the engine for rfec_recover_indexed_window_out (the
sections of a window of ANY of the planner's shapes decoded in one launch of
k_decode_window_indexed), shared by the CPU and the GPU tests of
test_recover_indexed_window.py.

A window is (name, geometry, per_group, variant, sections); a section is a spec
  ("ic", plan name, groups[, sparse])   indexed_cases.make_inputs: families 1 and 2 (full matrix of k = 6..16, rows
                                        of <= 4 with k <= 64), and with groups 0 any plan at all
  ("mw", k, groups[, sparse])           matrix_wide_cases.build on the planner's full matrix of k: family 3
  ("rw", (k, col), groups[, sparse])    rows_wide_cases.build on rows of col: family 4
  ("stairs", k)                         matrix_wide_cases.staircase_case: cascades of every depth, family 3
A section with groups > 0 becomes an indexed_cases.Inputs (pool, slot map, tables); its reference is
indexed_cases.reference (the oracle over the gathered batch), compared by indexed_cases.compare -- exactly as for the
single-shape calls.  A section with groups == 0 is left out of the launch and passes NULL tables.

What the random losses cannot promise in a section of two groups is set by hand: group 0 of every wide section loses
its last member alone and keeps every parity (random_loss / row_loss), and in the tampered variant the first line
that could recover it carries a fec_data_size above the capacity -- a banned line; group 1 of every wide matrix
section loses members 0 and 1 and the parity of column 1, so member 1 comes from row 0 only after column 0 gave
member 0 -- a cascade within per_group 2.  The random corruptions (matrix_wide_cases.tamper, one per group) go to the
groups after the hand-made ones.

The window's pool is the sections' pools one after the other, each section's map words raised by the first row of
its pool (recover_shapes_cases.make_window's joining).  family_of is the rule of rfec_recover_window_family in
Python; census() reads off the exact peel (matrix_wide_cases.peel, held to the reference's recovered masks) what a
section exercises.
"""
from __future__ import annotations

import copy
import zlib

import numpy as np

import guarded_arena as ga
import indexed_cases as ic
import indexed_matrix_cases as imc
import matrix_wide_cases as mw
import pyoracle as po
import recover_shapes_cases as rsc
import regroup_cases as rc
import rows_wide_cases as rw

FILL = ic.FILL
NONE = ic.NONE
WINDOW_TAG = 8  # tag of rfec_indexed_last_path for this entry (rfec_internal.h): WINDOW_TAG | sections launched << 8
GEOMS = ic.GEOMS


# -- the family rule, in Python -----------------------------------------------------------------------------------------
def lines_of(p):
    return [(p.line[l].first, p.line[l].stride, p.line[l].count) for l in range(p.n_lines)]


def rows_col(p):
    """The row width of a row layout (rows of line[0].count >= 2 consecutive segments in order, a last row of one
    segment without a line), else 0."""
    k, n = p.k, p.n_lines
    if not n or p.line[0].count < 2:
        return 0
    col = p.line[0].count
    return col if n == rw.n_lines(k, col) and lines_of(p) == [(l * col, 1, min(col, k - l * col)) for l in range(n)] \
        else 0


def family_of(o, p):
    """0 refused; 1 the planner's full matrix of k = 6..16; 2 rows of <= 4 with k <= 64, every row with a line; 3 the
    planner's full matrix of k = 17..128 (at most 23 lines); 4 any other row layout of k >= 2."""
    k = p.k
    full = False
    if 6 <= k <= 128:
        q = mw.wide_plan(o, k)
        full = q.n_lines > q.n_row_lines and lines_of(p) == lines_of(q)
    col = rows_col(p)
    if full and k <= 16:
        return 1
    if col and col <= 4 and k <= 64 and p.n_lines == -(-k // col):
        return 2
    if full and p.n_lines <= 23:
        return 3
    if col and k >= 2:
        return 4
    return 0


def single_tag(x):
    """rfec_indexed_last_path's tag of the section's single-shape call."""
    col = x.plan.line[0].count
    return {1: imc.MATRIX | x.k << 8, 2: rw.old_tag(x.k, col), 3: mw.WIDE | x.k << 8,
            4: rw.ROWS_WIDE | x.k << 8 | col << 16}[x.family]


# -- sections -------------------------------------------------------------------------------------------------------------
REFUSED = dict(mw.REFUSED, k1=lambda o: ic.PLANS["k1"](o))
for _n in ("rows10x4", "strip65", "rows_only40"):  # row layouts: the window call takes them
    del REFUSED[_n]
REFUSED["rows_gap"] = lambda o: _bent_rows(o, "gap")
REFUSED["rows_unequal"] = lambda o: _bent_rows(o, "unequal")
REFUSED["strip_from_1"] = lambda o: _bent_rows(o, "from1")


def _bent_rows(o, how):
    """Row layouts bent by hand: a gap between two rows, rows of unequal width, a strip from segment 1."""
    p = o.plan_matrix(12, 3, 4, rc.ROWS)
    if how == "gap":
        p.line[1].first, p.line[1].count = 5, 3
    elif how == "unequal":
        p.line[0].count, p.line[1].first, p.line[1].count = 3, 3, 5
    else:
        p = o.plan_matrix(12, 1, 12, rc.ROWS)
        p.line[0].first, p.line[0].count = 1, 11
    return p


def _present_bits(x):
    return ga.present_rows(x.present, x.k).reshape(x.G, x.k).astype(bool)


def _ban_first_line_of(x, g, t):
    """fec_data_size above the capacity on the first line (plan order) that holds segment t: the line is banned."""
    for l, m in enumerate(mw.line_masks(x.plan)):
        if (m >> t) & 1:
            x.fec_size[g, l] = x.capacity + 1
            return l
    raise AssertionError("no line holds the segment")


def section_inputs(o, spec, geom, E, tampered):
    """The Inputs of one launched section, with .family set."""
    kind, what = spec[0], spec[1]
    sparse = len(spec) > 3 and spec[3]
    if kind == "stairs":
        x = mw.staircase_case(o, what, E)
        assert ic.GEOMS["c20"] == GEOMS[geom]
        x.family = 3
        return x
    G = spec[2]
    tag = f"window-{kind}-{what}-{geom}-G{G}-E{E}{'-sparse' if sparse else ''}"
    rng = np.random.default_rng(zlib.crc32(f"tamper-{tag}".encode()))
    if kind == "ic":
        x = copy.copy(ic.make_inputs(o, (what, geom, G, E, sparse)))
        x.hdr, x.fec_size = x.hdr.copy(), x.fec_size.copy()
        hand = 4  # (indexed_cases._lose: groups 0..3; group 1 holds a refused line already)
    elif kind == "mw":
        k = what
        plan = mw.wide_plan(o, k)
        n = plan.n_lines
        assert G >= 2, "a wide matrix section holds its hand-made cascade in group 1"
        bits, pbits = mw.random_loss(tag, k, n, G, 0.08)
        bits[1], pbits[1] = True, True
        bits[1, :2] = False
        pbits[1, plan.n_row_lines + 1] = False
        x = mw.build(o, tag, k, G, geom, E, bits, pbits, False, sparse)
        hand = 2
    else:
        k, col = what
        bits, pbits = rw.row_loss(tag, k, col, G)
        x = rw.build(o, tag, k, col, G, geom, E, bits, pbits, False, sparse)
        hand = 3
    if tampered:
        if x.G > hand and x.nl:
            mw.tamper(rng, x.hdr[hand:], x.fec_size[hand:], _present_bits(x)[hand:], x.capacity)
        if kind != "ic":  # group 0 loses its last member with a line alone: ban the line that would recover it
            t = int(np.nonzero(~_present_bits(x)[0])[0][0])
            _ban_first_line_of(x, 0, t)
    x.family = family_of(o, x.plan)
    assert x.family and (kind != "mw" or x.family == 3)
    return x


def pad_section(x, ref, extra):
    """The section with `extra` all-absent groups behind it (what rfec_wire_regroup_shapes leaves in the rows past
    counts[p]: no member, no parity, every map word NONE), and its reference: recovered 0, out_index 0xFF."""
    y = copy.copy(x)
    k, n, E = x.k, x.nl, x.E
    y.G = x.G + extra
    y.src_of = np.concatenate([x.src_of, np.full(extra * (k + n), NONE, np.uint32)])
    pad_h = np.zeros((extra, k), po.HDR_DTYPE)
    pad_h.view(np.uint8)[...] = 0xA5
    pad_m = np.zeros((extra, n), po.HDR_DTYPE)
    pad_m.view(np.uint8)[...] = 0xA5
    y.hdr, y.meta = np.concatenate([x.hdr, pad_h]), np.concatenate([x.meta, pad_m])
    y.fec_size = np.concatenate([x.fec_size, np.full((extra, n), 7, np.uint16)])
    y.present = np.concatenate([x.present.reshape(-1, 2), np.zeros((extra, 2), np.uint64)])
    y.parity_present = np.concatenate([x.parity_present, np.zeros(extra, np.uint64)])
    sh, hd, ix, rec = ref
    ref2 = (np.concatenate([sh, np.full((extra, E, x.stride), FILL, np.uint8)]),
            np.concatenate([hd, np.zeros((extra, E), po.HDR_DTYPE)]),
            np.concatenate([ix, np.full((extra, E), 0xFF, np.uint8)]),
            np.concatenate([rec, np.zeros((extra, 2), np.uint64)]))
    return y, ref2


# -- windows --------------------------------------------------------------------------------------------------------------
# The mixed windows: all four families, the smallest shapes that can still go wrong.  Family 1 full3x4k10 and
# full2x3k6; family 2 rows12x3 and k2; family 3 k = 17 and k = 65 (two mask words); family 4 5 x 5, (11, 5) (rows of 5,
# 5 and 1: NL = 2), (65, 65) (bit 64) and (128, 2) (64 lines: 64 header lanes per group).  per_group is the least k, 2.
#  c15 (CD = 1): 1, 255, 256 and 257 groups are x 2 slots 2, 510, 512 and 514 payload lanes -- sections end mid-wave
#  and at a block's edge, and the next starts in the next round of 8; header / checker lanes per group are 4, 4 or 2,
#  1, and 2..64, so the sections have more header than payload blocks ((128, 2): 65 against 3) and fewer (k = 17: 1
#  against 2).
#  c20 (CD = 2, stride 48: a tail); c1200 (CD = 75): a wave straddles out slots and groups.
_M15 = [("ic", "full3x4k10", 257), ("rw", (5, 5), 255), ("mw", 17, 256), ("ic", "rows12x3", 255),
        ("rw", (65, 65), 1), ("ic", "full2x3k6", 256), ("mw", 65, 255), ("ic", "k2", 1), ("rw", (11, 5), 256),
        ("rw", (128, 2), 257)]
_M20 = [("ic", "full3x4k10", 7), ("rw", (5, 5), 64), ("mw", 17, 5), ("ic", "rows12x3", 5), ("rw", (65, 65), 3),
        ("ic", "full2x3k6", 64), ("mw", 65, 7), ("ic", "k2", 9), ("rw", (11, 5), 10), ("rw", (128, 2), 3)]
_M1200 = [("ic", "full3x4k10", 4), ("rw", (5, 5), 3), ("mw", 17, 3), ("ic", "rows12x3", 2), ("rw", (65, 65), 2),
          ("ic", "full2x3k6", 3), ("mw", 65, 2), ("ic", "k2", 2), ("rw", (11, 5), 3), ("rw", (128, 2), 2)]
_CYCLE = [("ic", "full3x4k10"), ("ic", "rows12x3"), ("mw", 17), ("rw", (5, 5))]


def _thirty_two():
    """32 sections cycling the four families with 2..5 groups, every seventh section empty."""
    return [(*_CYCLE[p % 4], 0 if p % 7 == 3 else 2 + (p * 3) % 4) for p in range(32)]


MIXED = [(f"mixed-{g}{'-reordered' if r else ''}-{v}", g, 2, v, rsc._reordered(s) if r else s)
         for g, s in (("c15", _M15), ("c20", _M20), ("c1200", _M1200)) for r in (False, True)
         for v in ("clean", "tampered")]
WINDOWS = MIXED + [
    # only sections of k >= 17: per_group 17
    ("wide-only", "c20", 17, "tampered", [("mw", 17, 5), ("rw", (65, 65), 4), ("mw", 65, 3), ("rw", (128, 2), 3)]),
    # the staircases of k = 100 (cascades of up to 10 steps within per_group 10) neither first nor last: every
    # intermediate goes through the group's own out slots, which lie first[p] = 3 rows into the arrays
    ("staircase", "c20", 10, "clean", [("ic", "rows12x3", 3), ("stairs", 100), ("ic", "full3x4k10", 4)]),
    # an empty first and last section and one between two filled ones; their plans are ones the call refuses
    ("empties", "c20", 3, "tampered", [("ic", "hand6", 0), ("mw", 17, 4), ("ic", "k10col3", 0), ("rw", (5, 5), 3),
                                       ("ic", "k1", 0)]),
    ("thirty-two", "c20", 2, "tampered", _thirty_two()),
    ("one-matrix", "c20", 3, "clean", [("ic", "full3x4k10", 7)]), ("one-rows", "c1200", 3, "clean", [("ic", "rows12x3", 5)]),
    ("one-wide-matrix", "c20", 4, "tampered", [("mw", 65, 6)]), ("one-wide-rows", "c1200", 3, "tampered", [("rw", (11, 5), 4)]),
    # pools of 70,000 rows at stride 16 each: every winning row index of the later sections is above 65,535
    ("sparse", "c15", 3, "tampered", [("ic", "rows10x4", 7, True), ("mw", 17, 40, True), ("rw", (11, 5), 40, True),
                                      ("ic", "full3x4k10", 7, True)]),
    # two wide sections whose maps have as many words (5 x 26 = 10 x 13): the self-tests swap them
    ("swap", "c20", 2, "clean", [("mw", 17, 5), ("rw", (11, 5), 10)]),
]
WINDOW = {w[0]: w for w in WINDOWS}
ic.PLANS.setdefault("k10col3", mw.REFUSED["k10col3"])


def window_id(w):
    return w[0]


class Window:
    pass


def join(name, geom, E, plans, xs, refs):
    """A window from its sections' Inputs (None: an empty section) and references: the joined pool, the maps into
    it, the output rows' prefix."""
    W = Window()
    W.name, W.geom, W.E = name, geom, E
    W.capacity, W.stride = GEOMS[geom]
    W.plans, W.x, W.ref = list(plans), list(xs), list(refs)
    W.groups = [x.G if x is not None else 0 for x in xs]
    W.names = [x.case[0] if x is not None else None for x in xs]
    W.src_of, pools, base = [], [], 0
    for x in xs:
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
    W.first = np.concatenate([[0], np.cumsum(W.groups)]).astype(int)
    return W


def make_window(o, w, cache=None):
    """The window's sections (section_inputs), their references (indexed_cases.reference), joined.  cache: section
    key -> (inputs, reference), shared among windows that hold the same section."""
    name, geom, E, variant, secs = w
    cache = {} if cache is None else cache
    plans, xs, refs = [], [], []
    for spec in secs:
        if spec[0] != "stairs" and not spec[2]:
            plans.append(ic.PLANS[spec[1]](o) if spec[0] == "ic" else mw.wide_plan(o, spec[1]) if spec[0] == "mw"
                         else rw.rows_plan(o, *spec[1]))
            xs.append(None), refs.append(None)
            continue
        key = (spec, geom, E, variant)
        if key not in cache:
            x = section_inputs(o, spec, geom, E, variant == "tampered")
            cache[key] = (x, ic.reference(o, x))
        x, ref = cache[key]
        plans.append(x.plan), xs.append(x), refs.append(ref)
    return join(name, geom, E, plans, xs, refs)


def from_shapes_window(o, V):
    """A recover_shapes_cases window as one of these: the same sections, their families from the rule."""
    W = copy.copy(V)
    W.x = []
    for x in V.x:
        if x is not None:
            x = copy.copy(x)
            x.family = family_of(o, x.plan)
        W.x.append(x)
    return W


def padded(W, extra):
    """Every launched section followed by `extra` all-absent rows: the window a caller decodes with groups NULL and
    cap above the rows in use."""
    xs, refs = [], []
    for x, ref in zip(W.x, W.ref):
        if x is None:
            xs.append(None), refs.append(None)
        else:
            y, r = pad_section(x, ref, extra)
            xs.append(y), refs.append(r)
    return join(W.name + "-padded", W.geom, W.E, W.plans, xs, refs)


def empty_pool_window(o, E=3, geom="c20"):
    """A section of each family over an empty pool (n_rows == 0, rows NULL), all-absent tables."""
    xs = [imc.empty_pool_inputs(o, 5, E, geom), rsc.empty_rows_inputs(o, 6, E, geom),
          mw.empty_pool_inputs(o, 17, 300, E, geom), rw.empty_pool_inputs(o, 11, 5, 300, E, geom)]
    for x in xs:
        x.family = family_of(o, x.plan)
    assert [x.family for x in xs] == [1, 2, 3, 4]
    return join("empty-pool", geom, E, [x.plan for x in xs], xs, [None] * 4)


def launched(W):
    return [p for p, g in enumerate(W.groups) if g]


# -- the census -----------------------------------------------------------------------------------------------------------
def census(x, ref):
    """What a section exercises, from the exact peel over 128-bit masks (matrix_wide_cases.peel), held to the
    reference's recovered masks on every group: segments recovered; steps whose target no line recovers at once
    on the received masks (a cascade: neither its row nor its column fires); groups with a line the header checks
    refuse; recovered targets of a line whose members lie in both mask words."""
    e_rec = ref[3]
    k, E = x.k, x.E
    lm = mw.line_masks(x.plan)
    have, ppm, rec = mw.masks_of(x.present), [int(p) for p in x.parity_present], mw.masks_of(e_rec)
    c = dict(recovered=0, cascade=0, refused=0, straddle=0)
    lo = (1 << 64) - 1
    for g in range(x.G):
        steps, refused = mw.peel(lm, k, have[g], ppm[g], E, x.capacity, x.hdr["size"][g], x.meta["size"][g],
                                 x.fec_size[g])
        got = sum(1 << t for _, t, _ in steps)
        assert got == rec[g], f"{x.case[0]} group {g}: the model recovers {got:#x}, the reference {rec[g]:#x}"
        erased = ~have[g] & ((1 << k) - 1)
        for l, t, _ in steps:
            at_once = any((ppm[g] >> q) & 1 and m & erased == 1 << t and m & have[g] for q, m in enumerate(lm))
            c["cascade"] += not at_once
            c["straddle"] += bool(lm[l] & lo and lm[l] >> 64)
        c["recovered"] += len(steps)
        c["refused"] += bool(refused)
    return c


# -- the engine -----------------------------------------------------------------------------------------------------------
_TABLES = rsc._TABLES
_OUTS = rsc._OUTS
_out_bytes = rsc._out_bytes


class GpuWindowDecode:
    """run(W) -> per launched section p ((out_shards, out_hdr, out_index, recovered) of the window call over the
    section's output rows, the same of the section's single-shape call, the same of rfec_recover_indexed_shapes_out
    when asked), every buffer of all the calls in one guarded arena at exactly its documented alignment, the outputs
    pre-filled with FILL; guards and inputs are checked after the calls, the tags as they are made.  groups: the
    window call's argument (None: NULL, every section's cap = its groups).  swap: two sections whose src_of pointers
    the window call gets swapped."""

    def __init__(self, lib, device="cuda:0"):
        import ctypes as C

        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        lib.lib.rfec_indexed_last_path.restype = C.c_uint32
        lib.lib.rfec_indexed_last_path.argtypes = []
        self.last_path = 0

    def _path(self):
        return int(self.lib.lib.rfec_indexed_last_path())

    def run(self, W, pass_groups=True, swap=None, singles=True, shapes=False):
        E, stride = W.E, W.stride
        live = launched(W)
        total = int(W.first[-1])
        bufs = [ga.Buf("rows", W.rows.nbytes, W.rows, "in", 16)]
        for p in live:
            x = W.x[p]
            src = {"src_of": W.src_of[p], "hdr": x.hdr, "present": x.present, "meta": x.meta, "fec_size": x.fec_size,
                   "parity_present": x.parity_present}
            bufs += [ga.Buf(f"{name}{p}", src[name].nbytes, src[name], "in", align) for name, align in _TABLES]
        bufs += [ga.Buf(name, _out_bytes(name, total, E, stride), FILL, "out", align) for name, align in _OUTS]
        if shapes:
            bufs += [ga.Buf(f"s_{name}", _out_bytes(name, total, E, stride), FILL, "out", align)
                     for name, align in _OUTS]
        if singles:
            for p in live:
                g = W.groups[p]
                bufs += [ga.Buf(f"{name}{p}", _out_bytes(name, g, E, stride), FILL, "out", align)
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
        self.lib.recover_indexed_window_out(W.plans, sections, groups, stride, W.capacity, rows, W.n_rows,
                                            A.ptr("recovered"), E, A.ptr("out_shards"), A.ptr("out_hdr"),
                                            A.ptr("out_index"), st)
        self.last_path = self._path()
        if shapes:
            self.lib.recover_indexed_shapes_out(W.plans, sections, groups, stride, W.capacity, rows, W.n_rows,
                                                A.ptr("s_recovered"), E, A.ptr("s_out_shards"), A.ptr("s_out_hdr"),
                                                A.ptr("s_out_index"), st)
            self.shapes_path = self._path()
        self.single_paths = {}
        if singles:
            for p in live:
                g = W.groups[p]
                args = (W.plans[p], g, stride, W.capacity, rows, W.n_rows,
                        *(A.ptr(f"{name}{p}") for name, _ in _TABLES), A.ptr(f"recovered{p}"), E,
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
        A.check(f"recover_indexed_window_out {W.name}")

        def outs(prefix, n, a=None, b=None):
            o = (A.get(f"{prefix[0]}out_shards{prefix[1]}", np.uint8, (n, E, stride)),
                 A.get(f"{prefix[0]}out_hdr{prefix[1]}", po.HDR_DTYPE, (n, E)),
                 A.get(f"{prefix[0]}out_index{prefix[1]}", np.uint8, (n, E)),
                 A.get(f"{prefix[0]}recovered{prefix[1]}", np.uint64, (n, 2)))
            return o if a is None else tuple(v[a:b] for v in o)

        out = {}
        for p in live:
            a, b, g = int(W.first[p]), int(W.first[p + 1]), W.groups[p]
            out[p] = (outs(("", ""), total, a, b), outs(("", p), g) if singles else None,
                      outs(("s_", ""), total, a, b) if shapes else None)
        return out
