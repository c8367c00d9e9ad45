"""Windows, inputs and the engine for rfec_recover_indexed_shapes_out (the
sections of a window of several shapes decoded in one launch), shared by the CPU
and the GPU tests of test_recover_shapes.py.

A window is (name, geometry, per_group, sections); a section is (plan, groups,
sparse).  A section with groups > 0 is the indexed_cases case (plan, geometry,
groups, per_group, sparse): make_inputs builds its pool, map and tables, and
reference / compare / conditions judge its outputs, exactly as for the
single-shape calls.  A section with groups == 0 is left out of the launch (its
plan may be one the call refuses otherwise) and passes NULL tables.

The window's pool is the sections' pools one after the other, each section's
map words raised by the first row of its pool.  The reference of every section
is the oracle's on the section's own inputs; the engine also runs the
single-shape call of each section -- rfec_recover_indexed_matrix_out for a full
matrix, rfec_recover_indexed_out for a row layout -- on the same arena, into
output arrays of its own.
"""
from __future__ import annotations

import numpy as np

import guarded_arena as ga
import indexed_cases as ic
import indexed_matrix_cases as imc  # (registers full2x3k6 and full4x4k16 in ic.PLANS)
import pyoracle as po
import regroup_cases as rc

FILL = ic.FILL
NONE = ic.NONE
SHAPES = 4  # tag of rfec_indexed_last_path for this entry (rfec_internal.h): SHAPES | sections launched << 8
MATRIX_PLANS = ("full3x4k10", "full2x3k6", "full4x4k16")
# the edge windows' plans: shapes_cases' decode3, the k = 6 and k = 16 matrices, k2
EDGE_PLANS = ("full3x4k10", "rows32x4", "rows12x3", "full2x3k6", "full4x4k16", "k2")

# Payload lanes of a section: groups x per_group x CD, in blocks of 256 (4 waves of 64).  Checker lanes of a matrix
# section: 4 per group; header lanes of a row layout: the least power of two >= n_lines, at least 2, per group.
#  c15 (CD = 1), E = 1: 1, 255, 256 and 257 groups are as many payload lanes; a matrix of 257 groups has 5 checker
#  blocks and 2 payload blocks, rows32x4 (8 header lanes per group) of 255 groups 8 header blocks and 1 payload block;
#  255 and 257 lanes end mid-wave, 1 lane in a block's first wave, and the next section starts in the next round of 8.
#  c20 (CD = 2, stride 48: a tail), E = 2: 64 groups are 256 lanes, 7 groups 28.
#  c1200 (CD = 75), E = 2: a wave straddles out slots and groups; 3 groups are 450 lanes (2 blocks, the last wave 2).
_C15 = [("full3x4k10", 257, False), ("rows32x4", 255, False), ("full2x3k6", 255, False), ("rows12x3", 256, False),
        ("full4x4k16", 1, False), ("k2", 257, False), ("rows12x3", 1, False), ("full2x3k6", 256, False)]
_C20 = [("full3x4k10", 7, False), ("rows32x4", 64, False), ("rows12x3", 5, False), ("full2x3k6", 64, False),
        ("full4x4k16", 3, False), ("k2", 9, False)]
_C1200 = [("full3x4k10", 4, False), ("rows32x4", 3, False), ("rows12x3", 2, False), ("full2x3k6", 3, False),
          ("full4x4k16", 2, False), ("k2", 2, False)]


def _reordered(secs):
    """The same sections in another order: reversed, then the two halves swapped."""
    r = secs[::-1]
    return r[len(r) // 2:] + r[:len(r) // 2]


def _thirty_two():
    """32 sections: the edge plans in turn with 1..5 groups, every seventh section empty."""
    out = []
    for p in range(32):
        name = EDGE_PLANS[p % len(EDGE_PLANS)]
        out.append((name, 0 if p % 7 == 3 else 1 + (p * 3) % 5, False))
    return out


WINDOWS = [
    ("edges-c15", "c15", 1, _C15), ("edges-c15-reordered", "c15", 1, _reordered(_C15)),
    ("edges-c20", "c20", 2, _C20), ("edges-c20-reordered", "c20", 2, _reordered(_C20)),
    ("edges-c1200", "c1200", 2, _C1200), ("edges-c1200-reordered", "c1200", 2, _reordered(_C1200)),
    # an empty first and last section and one between two filled ones; their plans are ones the call refuses
    ("empties", "c20", 3, [("strip65", 0, False), ("full3x4k10", 5, False), ("hand6", 0, False),
                           ("rows10x4", 6, False), ("k1", 0, False)]),
    # pools of 70,000 rows at stride 16 each: every winning row index of the second section is above 65,535
    ("sparse", "c15", 3, [("rows10x4", 7, True), ("full3x4k10", 7, True)]),
    ("thirty-two", "c20", 1, _thirty_two()),
    ("one-matrix", "c20", 3, [("full3x4k10", 7, False)]), ("one-rows", "c1200", 3, [("rows12x3", 5, False)]),
    # two sections whose maps have as many words (11 x 17 = 17 x 11): the self-test swaps their pointers
    ("swap", "c20", 2, [("full3x4k10", 11, False), ("full2x3k6", 17, False)]),
]
WINDOW = {w[0]: w for w in WINDOWS}


def window_id(w):
    return w[0]


def is_matrix(name):
    return name in MATRIX_PLANS


def single_tag(x):
    """rfec_indexed_last_path's tag of the section's single-shape call."""
    if is_matrix(x.case[0]):
        return imc.MATRIX | x.k << 8
    path, K = ic.DEFAULT_PATH[x.case[0]]
    assert path == ic.ROWS_FUSED
    return path | K << 8


class Window:
    pass


def make_window(oracle, w, cache=None):
    """The window's sections' inputs (indexed_cases.make_inputs; None for an empty section), their references, the
    joined pool and the maps into it.  cache: (plan, geometry, groups, per_group, sparse) -> (inputs, reference),
    shared among windows that hold the same section."""
    name, geom, E, secs = w
    cache = {} if cache is None else cache
    W = Window()
    W.name, W.geom, W.E = name, geom, E
    W.capacity, W.stride = ic.GEOMS[geom]
    W.plans = [ic.PLANS[p](oracle) for p, _, _ in secs]
    W.names = [p for p, _, _ in secs]
    W.groups = [g for _, g, _ in secs]
    W.x, W.ref, W.src_of, pools, base = [], [], [], [], 0
    for p, g, sparse in secs:
        if not g:
            W.x.append(None), W.ref.append(None), W.src_of.append(None)
            continue
        c = (p, geom, g, E, sparse)
        if c not in cache:
            x = ic.make_inputs(oracle, c)
            cache[c] = (x, ic.reference(oracle, x))
        x, ref = cache[c]
        W.x.append(x), W.ref.append(ref)
        so = x.src_of.copy()
        so[so != NONE] += np.uint32(base)
        W.src_of.append(so)
        pools.append(x.rows)
        base += x.n_rows
    W.rows = np.concatenate(pools) if pools else np.zeros((0, W.stride), np.uint8)
    W.n_rows = base
    W.first = np.concatenate([[0], np.cumsum(W.groups)]).astype(int)
    return W


def launched(W):
    return [p for p, g in enumerate(W.groups) if g]


_TABLES = (("src_of", 4), ("hdr", 4), ("present", 8), ("meta", 4), ("fec_size", 2), ("parity_present", 8))
_OUTS = (("recovered", 8), ("out_shards", 16), ("out_hdr", 4), ("out_index", 1))


def _out_bytes(name, rows, E, stride):
    return rows * {"recovered": 16, "out_shards": E * stride, "out_hdr": E * 20, "out_index": E}[name]


class GpuShapesDecode:
    """run(W) -> per launched section p ((out_shards, out_hdr, out_index, recovered) of the window call over the
    section's output rows, the same of the section's single-shape call), every buffer of all the calls in one guarded
    arena at exactly its documented alignment, the outputs pre-filled with FILL; guards and inputs are checked after
    the calls, the tags as they are made.  groups: the window call's argument (None: NULL, every section's cap =
    its groups).  swap: two sections whose src_of pointers the window call gets swapped."""

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

    def run(self, W, pass_groups=True, swap=None, singles=True):
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
        if singles:
            for p in live:
                g = W.groups[p]
                bufs += [ga.Buf(f"{name}{p}", _out_bytes(name, g, E, stride), FILL, "out", align)
                         for name, align in _OUTS]
                if not is_matrix(W.names[p]):
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
        self.lib.recover_indexed_shapes_out(W.plans, sections, W.groups if pass_groups else None, stride, W.capacity,
                                            rows, W.n_rows, A.ptr("recovered"), E, A.ptr("out_shards"),
                                            A.ptr("out_hdr"), A.ptr("out_index"), st)
        self.last_path = self._path()
        self.single_paths = {}
        if singles:
            for p in live:
                x, g = W.x[p], W.groups[p]
                args = (W.plans[p], g, stride, W.capacity, rows, W.n_rows,
                        *(A.ptr(f"{name}{p}") for name, _ in _TABLES), A.ptr(f"recovered{p}"), E,
                        A.ptr(f"out_shards{p}"), A.ptr(f"out_hdr{p}"), A.ptr(f"out_index{p}"))
                if is_matrix(W.names[p]):
                    self.lib.recover_indexed_matrix_out(*args, st)
                else:
                    self.lib.recover_indexed_out(*args, A.ptr(f"workspace{p}"), st)
                self.single_paths[p] = self._path()
        self.be.sync()
        A.check(f"recover_indexed_shapes_out {W.name}")
        sh = A.get("out_shards", np.uint8, (total, E, stride))
        hd = A.get("out_hdr", po.HDR_DTYPE, (total, E))
        ix = A.get("out_index", np.uint8, (total, E))
        rec = A.get("recovered", np.uint64, (total, 2))
        out = {}
        for p in live:
            a, b, g = int(W.first[p]), int(W.first[p + 1]), W.groups[p]
            single = None
            if singles:
                single = (A.get(f"out_shards{p}", np.uint8, (g, E, stride)), A.get(f"out_hdr{p}", po.HDR_DTYPE, (g, E)),
                          A.get(f"out_index{p}", np.uint8, (g, E)), A.get(f"recovered{p}", np.uint64, (g, 2)))
            out[p] = ((sh[a:b], hd[a:b], ix[a:b], rec[a:b]), single)
        return out


def empty_rows_inputs(oracle, G=6, E=3, geom="c20"):
    """indexed_matrix_cases.empty_pool_inputs for a row layout: all-absent tables over an empty pool."""
    x = imc.empty_pool_inputs(oracle, G, E, geom)
    plan = ic.PLANS["rows12x3"](oracle)
    k, n = plan.k, plan.n_lines
    x.case = ("rows12x3", geom, G, E, False)
    x.plan, x.k, x.nl = plan, k, n
    x.src_of = np.full(G * (k + n), NONE, np.uint32)
    x.hdr = np.zeros((G, k), po.HDR_DTYPE)
    x.hdr.view(np.uint8)[...] = 0xA5
    x.meta = np.zeros((G, n), po.HDR_DTYPE)
    x.meta.view(np.uint8)[...] = 0xA5
    x.fec_size = np.full((G, n), 7, np.uint16)
    return x


def empty_pool_window(oracle, E=3, geom="c20"):
    """A matrix and a row-layout section over an empty pool (n_rows == 0, rows NULL)."""
    W = Window()
    W.name, W.geom, W.E = "empty-pool", geom, E
    W.capacity, W.stride = ic.GEOMS[geom]
    W.x = [imc.empty_pool_inputs(oracle, 5, E, geom), empty_rows_inputs(oracle, 6, E, geom)]
    W.names = [x.case[0] for x in W.x]
    W.plans = [x.plan for x in W.x]
    W.groups = [x.G for x in W.x]
    W.src_of = [x.src_of for x in W.x]
    W.ref = [None, None]
    W.rows, W.n_rows = np.zeros((0, W.stride), np.uint8), 0
    W.first = np.concatenate([[0], np.cumsum(W.groups)]).astype(int)
    return W


def pattern_window(sweeps, E):
    """pattern_cases' sweeps (one per k, one geometry) as the sections of one window at per_group E."""
    import pattern_cases as pc
    W = Window()
    sw0 = sweeps[0]
    W.name, W.geom, W.E = f"patterns-{sw0.variant}-E{E}", sw0.geom, E
    W.capacity, W.stride = sw0.cap, sw0.stride
    W.x = [pc.indexed_inputs(sw, E) for sw in sweeps]
    W.names = ["full3x4k10"] * len(sweeps)  # (every section a matrix: is_matrix)
    W.plans = [sw.plan for sw in sweeps]
    W.groups = [sw.G for sw in sweeps]
    W.ref = [None] * len(sweeps)
    W.src_of, pools, base = [], [], 0
    for x in W.x:
        so = x.src_of.copy()
        so[so != NONE] += np.uint32(base)
        W.src_of.append(so)
        pools.append(x.rows)
        base += x.n_rows
    W.rows, W.n_rows = np.concatenate(pools), base
    W.first = np.concatenate([[0], np.cumsum(W.groups)]).astype(int)
    return W
