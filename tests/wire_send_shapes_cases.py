"""Cases, inputs, expected values and engines for rfec_wire_encode_send_shapes
(a send window of several shapes into its SIM_SEG and SIM_FEC datagrams in one
launch), shared by the CPU and the GPU tests of test_wire_send_shapes.py.  Built
on wire_send_cases.py (its plans, geometries, comparison and guarded arena).

A case is (shapes, geometry, per-group sequence, row layout, descriptor order,
seg order?, fec order?).  The sequence holds, in window order, a shape's index
per group or ("skip", reason, shape): a descriptor the call must skip, which owns
a block of rows and lines of that shape that must keep the fill.  Row layouts:
"window" (the groups' rows and lines follow each other in window order), "perm"
(the groups' blocks lie in a random order) and "gaps" (rows and lines that no
group covers between the blocks).  Descriptor orders: "window", "byshape" (a
stable sort by shape) and "random".

Expected values come from the oracle composed per shape: each shape's groups are
gathered, framed and encoded as wire_send_cases.compose does, and the datagrams
are scattered to row0 + i / line0 + l; slots that no live group covers expect
DGRAM_FILL / DLEN_FILL.  On the GPU the same gather / scatter runs through the
product's own rfec_wire_encode_send, one call per shape.
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import wire_cases as wc
import wire_encode_cases as wec
import wire_send_cases as wsc
from wire_send_cases import DGRAM_FILL, DLEN_FILL, POISON, compare_all, permuted  # noqa: F401

GEOMS = wsc.GEOMS
SEND_GROUP = np.dtype([("row0", "<u4"), ("line0", "<u4"), ("shape", "<u4"), ("reserved", "<u4")])
MAX_SHAPES, MAX_LINES = 32, 512


def _wide_plan(i):
    """Plan i of the 32-shape case: 24 (even i) or 8 (odd i) lines of 2-3 neighbours, k = 26 + i % 5."""
    n = 24 if i % 2 == 0 else 8
    return wec._hand_plan(26 + i % 5, [(l, 1, 2 + (i + l) % 2) for l in range(n)])


PLANS = dict(wsc.PLANS)
PLANS["k3"] = lambda o: wec._hand_plan(3, [(0, 1, 2)])  # member 2 on no line
for _i in range(MAX_SHAPES):
    PLANS[f"wide{_i}"] = (lambda i: lambda o: _wide_plan(i))(_i)

Q4 = ["rows10x4", "full3x4k10", "hand7", "k1"]
SKIPS = ("shape", "rows", "lines")


def _seq(rng_seed, n, n_shapes):
    return np.random.default_rng(rng_seed).integers(0, n_shapes, n).tolist()


# (shapes, geometry, sequence, layout, descriptor order, seg order?, fec order?)
CASES = {
    # quad compositions at c1200w: 4 of one shape, 2 + 2, 3 + 1, 1 + 1 + 1 + 1, 2 + 1 + 1; trailing quads of 1, 2, 3
    "quads-tail1": (Q4, "c1200w", [0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 3, 0, 1, 2, 3, 2, 2, 1, 3, 1], "window", "window",
                    False, False),
    "quads-tail2": (Q4, "c1200w", [2, 2, 2, 2, 1, 2, 1, 2, 3, 0], "window", "window", False, False),
    "quads-tail3": (Q4, "c1200w", [1, 1, 1, 1, 0, 2, 1], "window", "window", True, True),
    "one-group": (Q4, "c1200w", [2], "window", "window", False, False),
    # the 8-bit limits, an orphan and strided lines in one window
    "big-shapes": (["k255", "k2", "rows9x4", "cols10x4"], "c1200w", [0, 1, 2, 3, 3, 0, 1, 2, 2], "window", "window",
                   False, False),
    # both kernel instances, the smallest slots and the poisoned tails
    "c463": (Q4, "c463", [0, 1, 2, 3, 1, 1, 0], "window", "window", False, False),
    "c464": (Q4, "c464", [0, 1, 2, 3, 1, 1, 0], "window", "window", False, False),
    "c15": (Q4, "c15", [3, 2, 1, 0, 0, 2], "window", "window", False, False),
    "c1000p": (Q4, "c1000p", [0, 1, 1, 2, 3, 0, 2, 2, 1], "gaps", "window", False, False),
    # rows permuted against descriptor order; descriptors sorted by shape over window-order rows
    "rows-perm": (Q4, "c1000", _seq(1, 14, 4), "perm", "window", False, False),
    "desc-byshape": (Q4, "c1000", _seq(2, 15, 4), "window", "byshape", True, True),
    "desc-random": (Q4, "c256", _seq(3, 13, 4), "perm", "random", False, True),
    # rows and lines that no group covers keep the fill
    "gaps": (Q4, "c1200w", _seq(4, 10, 4), "gaps", "window", False, False),
    # a skipped group for each reason, each among live groups of its quad
    "skips": (Q4, "c1200w", [0, ("skip", "shape", 1), 1, 2, ("skip", "rows", 0), 0, 3, 1, 2, 1, ("skip", "lines", 2), 0,
                             ("skip", "rows", 1), ("skip", "shape", 0)], "window", "window", False, False),
    # every combination of the two orders on one small case
    "orders-00": (Q4, "c1000", [1, 0, 2, 1, 3], "gaps", "window", False, False),
    "orders-10": (Q4, "c1000", [1, 0, 2, 1, 3], "gaps", "window", True, False),
    "orders-01": (Q4, "c1000", [1, 0, 2, 1, 3], "gaps", "window", False, True),
    "orders-11": (Q4, "c1000", [1, 0, 2, 1, 3], "gaps", "window", True, True),
    # 32 plans whose lines sum to exactly 512, each used at least once
    "shapes32": ([f"wide{i}" for i in range(MAX_SHAPES)], "c64",
                 np.random.default_rng(5).permutation(np.arange(37) % MAX_SHAPES).tolist(), "window", "window", False,
                 False),
    # a one-shape window: also byte-equal to rfec_wire_encode_send on the same buffers
    "one-shape": (["full3x4k10"], "c1000", [0] * 9, "window", "window", False, False),
    "one-shape-orders": (["hand7"], "c1200w", [0] * 6, "window", "window", True, True),
}
# four descriptors per wave, 16 waves per block, one block per CU: more units than the waves resident at once
LOOP_CASE = (["k2", "k3"], "c64", _seq(6, 4 * 4099 + 1, 2), "window", "window", False, False)


class Inputs:
    pass


def make_inputs(oracle, name, c=None):
    """The case's inputs, its descriptors and what the oracle composed per shape expects of them."""
    shapes, gname, seq, layout, dorder, with_so, with_fo = c if c is not None else CASES[name]
    capacity, stride, dstride = GEOMS[gname]
    plans = [(PLANS.get(s) or wsc.LOOP_PLANS[s])(oracle) for s in shapes]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    G = len(seq)
    big = G > 5000  # the loop case: cheap inputs
    # every descriptor owns a block of k rows and n lines of its shape, live or not
    shape_of = np.array([s if isinstance(s, (int, np.integer)) else s[2] for s in seq])
    skip = [None if isinstance(s, (int, np.integer)) else s[1] for s in seq]
    ks = np.array([plans[p].k for p in shape_of])
    nl = np.array([plans[p].n_lines for p in shape_of])
    place = rng.permutation(G) if layout == "perm" else np.arange(G)  # the order the blocks lie in
    gap_r = rng.integers(0, 4, G + 1) if layout == "gaps" else np.zeros(G + 1, np.int64)
    gap_l = rng.integers(0, 3, G + 1) if layout == "gaps" else np.zeros(G + 1, np.int64)
    if layout == "gaps":
        gap_r[min(2, G)], gap_l[min(1, G)], gap_r[G], gap_l[G] = 3, 2, 2, 1
    row0, line0 = np.zeros(G, np.int64), np.zeros(G, np.int64)
    r = l = 0
    for j, w in enumerate(place):
        r, l = r + int(gap_r[j]), l + int(gap_l[j])
        row0[w], line0[w] = r, l
        r, l = r + int(ks[w]), l + int(nl[w])
    n_rows, n_fec = r + int(gap_r[G]), l + int(gap_l[G])
    covered_r, covered_l = np.zeros(n_rows, bool), np.zeros(n_fec, bool)
    for w in range(G):
        if skip[w] is None:
            covered_r[row0[w]:row0[w] + ks[w]] = True
            covered_l[line0[w]:line0[w] + nl[w]] = True

    # headers of every width (random_batch: half of seq, fid and total narrow), remb 0 and not
    N = n_rows
    _, hdr, _, sstamps = wc.random_batch(rng, N, 16, 0, seg=True)
    # the first live group: packet ids that straddle 65,535 / 65,536 with the other fields narrow
    w0 = next(w for w in range(G) if skip[w] is None)
    m0 = slice(int(row0[w0]), int(row0[w0] + ks[w0]))
    hdr["seq"][m0] = 65536 - (int(ks[w0]) + 1) // 2 + np.arange(int(ks[w0]))
    hdr["fid"][m0], hdr["total"][m0] = 77, 255
    sizes = rng.integers(0, capacity + 1, N)
    u = rng.random(N)
    sizes[u < 0.12] = 0
    sizes[(u >= 0.12) & (u < 0.18)] = min(1, capacity)
    sizes[u > 0.90] = capacity
    hs = wsc.seg_hs(hdr)
    if capacity >= 512 and not big:
        # SIM_SEG trailers (at byte hs + L) across a 64-lane row's edge (256 bytes) and across a chunk's
        for d in rng.choice(N, max(2, N // 10), replace=False):
            sizes[d] = 256 * int(rng.integers(1, capacity // 256)) + 254 - hs[d] + int(rng.integers(0, 2))
        # a SIM_FEC trailer (at byte 45 + max L) likewise: every member of a live group's line 0 at most Lf
        for w in range(G):
            if skip[w] is None and nl[w]:
                Lf = 256 + 254 - 45
                m = int(row0[w]) + np.array(plans[shape_of[w]].members(0))
                sizes[m] = np.minimum(sizes[m], Lf)
                sizes[m[-1]] = Lf
                break
    shards = np.zeros((N, stride), np.uint8) if big else rng.integers(0, 256, (N, stride), dtype=np.uint8)
    if big:
        shards[:, :capacity] = rng.integers(0, 256, (1, capacity), dtype=np.uint8) ^ \
            ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)[:, None]
    shards[np.arange(stride)[None, :] >= sizes[:, None]] = 0
    cd16 = 16 * ((capacity + 15) // 16)
    if gname.endswith("p"):
        assert cd16 + 16 <= stride
        shards[:, cd16:] = POISON
    hdr["size"] = sizes
    # about 6 % of the segments (at least one covered): data_size above the capacity
    over = np.nonzero(rng.random(N) < 0.06)[0]
    over = over if covered_r[over].any() else np.append(over, np.nonzero(covered_r)[0][N // 3 % covered_r.sum()])
    hdr["size"][over] = np.minimum(65535, capacity + 1 + (rng.integers(0, 40, len(over)) * (rng.random(len(over)) < 0.5)))
    _, _, _, fstamps = wc.random_batch(rng, max(n_fec, 1), 16, 0, seg=False)
    fstamps = fstamps[:n_fec]

    # the descriptors, then their order
    desc = np.zeros(G, SEND_GROUP)
    desc["row0"], desc["line0"], desc["shape"] = row0, line0, shape_of
    seen = {}
    for w in range(G):
        if skip[w] is None:
            continue
        nth = seen[skip[w]] = seen.get(skip[w], 0) + 1
        if skip[w] == "shape":  # shape >= n_plans
            desc["shape"][w] = len(plans) if nth == 1 else 0xFFFFFFFF
        elif skip[w] == "rows":  # row0 + k > n_rows: by one row, or past 2^32
            desc["row0"][w] = n_rows - ks[w] + 1 if nth == 1 else 0xFFFFFFFF
        else:  # line0 + n > n_fec
            assert nl[w] >= 1
            desc["line0"][w] = n_fec - nl[w] + 1 if nth == 1 else 0xFFFFFFFE
    if dorder == "byshape":
        perm = np.argsort(desc["shape"], kind="stable")
    elif dorder == "random":
        perm = rng.permutation(G)
    else:
        perm = np.arange(G)
    desc = np.ascontiguousarray(desc[perm])
    live = np.array([skip[w] is None for w in perm])

    x = Inputs()
    x.name, x.plans, x.G, x.n_rows, x.n_fec = name, plans, G, n_rows, n_fec
    x.capacity, x.stride, x.dstride = capacity, stride, dstride
    x.shards, x.hdr, x.sstamps, x.fstamps = shards, hdr, sstamps, fstamps
    x.desc, x.live, x.skip = desc, live, [skip[w] for w in perm]
    x.covered_r, x.covered_l = covered_r, covered_l
    x.sorder = rng.permutation(n_rows).astype(np.uint32) if with_so else None
    x.forder = rng.permutation(n_fec).astype(np.uint32) if with_fo and n_fec else None
    x.exp, x.enc = compose_shapes(x, lambda p, sub: wsc.compose(oracle, sub, sub.shards, sub.hdr, sub.sstamps,
                                                               sub.fstamps, None, None))
    return x


def gathered(x, p):
    """Shape p's live groups as one rfec_wire_encode_send batch: (its inputs, the member rows, the SIM_FEC lines)."""
    plan = x.plans[p]
    d = x.desc[x.live & (x.desc["shape"] == p)]
    k, n, Gp = plan.k, plan.n_lines, len(d)
    rows = (d["row0"].astype(np.int64)[:, None] + np.arange(k)[None, :]).reshape(-1)
    lines = (d["line0"].astype(np.int64)[:, None] + np.arange(n)[None, :]).reshape(-1)
    sub = Inputs()
    sub.plan, sub.G, sub.k, sub.n, sub.ns, sub.nf = plan, Gp, k, n, Gp * k, Gp * n
    sub.capacity, sub.stride, sub.dstride = x.capacity, x.stride, x.dstride
    sub.shards = np.ascontiguousarray(x.shards[rows]).reshape(Gp, k, x.stride)
    sub.hdr = np.ascontiguousarray(x.hdr[rows]).reshape(Gp, k)
    sub.sstamps = np.ascontiguousarray(x.sstamps[rows])
    sub.fstamps = np.ascontiguousarray(x.fstamps[lines])
    return sub, rows, lines


def compose_shapes(x, send_one):
    """((seg_dgram [n_rows], seg_dlen, fec_dgram [n_fec], fec_dlen), {shape: enc}): send_one(p, sub) -> ((sd, sl, fd,
    fl), enc) frames one shape's gathered groups; the datagrams are scattered to their rows and lines over the fill
    and moved by the orders."""
    sd = np.full((x.n_rows, x.dstride), DGRAM_FILL, np.uint8)
    sl = np.full(x.n_rows, DLEN_FILL * 0x0101, np.uint16)
    fd = np.full((x.n_fec, x.dstride), DGRAM_FILL, np.uint8)
    fl = np.full(x.n_fec, DLEN_FILL * 0x0101, np.uint16)
    encs = {}
    for p in range(len(x.plans)):
        sub, rows, lines = gathered(x, p)
        if sub.G == 0:
            continue
        (a, b, c, d), encs[p] = send_one(p, sub)
        sd[rows], sl[rows] = a, b
        if sub.nf:
            fd[lines], fl[lines] = c, d
    sd, sl = permuted(sd, sl, x.sorder)
    fd, fl = permuted(fd, fl, x.forder)
    return (sd, sl, fd, fl), encs


def quad_kinds(x):
    """Per wave (four consecutive descriptors): the sorted counts of its live groups' shapes, and its size."""
    out = []
    for q in range(0, x.G, 4):
        d, live = x.desc[q:q + 4], x.live[q:q + 4]
        _, cnt = np.unique(d["shape"][live], return_counts=True)
        out.append((len(d), tuple(sorted(cnt.tolist(), reverse=True))))
    return out


def conditions(x):
    """What the case exercises, from the oracle's outputs (in row / line order: the orders undone)."""
    sd, sl, fd, fl = x.exp
    if x.sorder is not None:
        sl = sl[x.sorder]
    sl = sl.astype(np.int64)
    size = x.hdr["size"].astype(np.int64)
    cov = x.covered_r
    live = cov & (sl > 0)
    hs = np.where(live, sl - 4 - size, 0)
    end = sl - 4
    used = sorted(set(x.desc["shape"][x.live].tolist()))
    own = [o for p in used for o in wsc.owners(x.plans[p])]
    c = {
        "hs": set(np.unique(hs[hs > 0]).tolist()),
        "seg_oversize": bool((cov & (size > x.capacity) & (sl == 0)).any()),
        "seg_crc_chunk": bool((live & (end % 16 > 12)).any()),
        "seg_crc_row": bool((live & (end % 256 > 252)).any()),
        "orphan": any(len(o) == 0 for o in own),
        "on_two_lines": any(len(o) == 2 for o in own),
        "one_member_line": any(x.plans[p].line[l].count == 1 for p in used for l in range(x.plans[p].n_lines)),
        "fec_refused": False, "fec_crc_chunk": False, "fec_crc_row": False,
        "gap_rows": bool((~cov).any()) and bool((sl[~cov] == DLEN_FILL * 0x0101).all()),
        "gap_lines": bool((~x.covered_l).any()),
        "quads": set(quad_kinds(x)),
        "skips": {s for s in x.skip if s},
    }
    for enc in x.enc.values():
        if enc is None:
            continue
        fsize, status = enc[2].reshape(-1).astype(np.int64), enc[3].reshape(-1)
        ok = status == 0
        c["fec_refused"] |= bool((status == -1).any())
        c["fec_crc_chunk"] |= bool((ok & ((45 + fsize) % 16 > 12)).any())
        c["fec_crc_row"] |= bool((ok & ((45 + fsize) % 256 > 252)).any())
    return c


# -- engines -----------------------------------------------------------------------------------------------------
class ShapesEngine:
    """send(x) -> (seg_dgram [n_rows][dstride], seg_dlen, fec_dgram [n_fec][dstride], fec_dlen) with the call's
    buffers in one guarded arena (no SIM_FEC buffers when n_fec == 0: the call gets NULL).  mutate (tests): called
    with the arena after the call and before its checks."""

    be = None
    mutate = None

    def arena(self, x):
        bufs = [ga.Buf("group", x.G * 16, x.desc, "in", 4), ga.Buf("shards", x.shards.size, x.shards, "in", 16),
                ga.Buf("hdr", x.hdr.size * 20, x.hdr, "in", 4), ga.Buf("seg_stamps", x.n_rows * 12, x.sstamps, "in", 4)]
        if x.n_fec:
            bufs.append(ga.Buf("fec_stamps", x.n_fec * 24, x.fstamps, "in", 4))
        if x.sorder is not None:
            bufs.append(ga.Buf("seg_order", x.n_rows * 4, x.sorder, "in", 4))
        if x.forder is not None:
            bufs.append(ga.Buf("fec_order", x.n_fec * 4, x.forder, "in", 4))
        bufs += self.out_bufs(x)
        return ga.Arena(self.be, bufs)

    @staticmethod
    def out_bufs(x):
        bufs = [ga.Buf("seg_dgram", x.n_rows * x.dstride, DGRAM_FILL, "out", 16),
                ga.Buf("seg_dlen", x.n_rows * 2, DLEN_FILL, "out", 2)]
        if x.n_fec:
            bufs += [ga.Buf("fec_dgram", x.n_fec * x.dstride, DGRAM_FILL, "out", 16),
                     ga.Buf("fec_dlen", x.n_fec * 2, DLEN_FILL, "out", 2)]
        return bufs

    @staticmethod
    def outputs(A, x):
        sd, sl = A.get("seg_dgram", np.uint8, (x.n_rows, x.dstride)), A.get("seg_dlen", np.uint16, (x.n_rows,))
        if not x.n_fec:
            return sd, sl, np.zeros((0, x.dstride), np.uint8), np.zeros(0, np.uint16)
        return sd, sl, A.get("fec_dgram", np.uint8, (x.n_fec, x.dstride)), A.get("fec_dlen", np.uint16, (x.n_fec,))

    def send(self, x):
        A = self.arena(x)
        self._send(x, A)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_encode_send_shapes {x.name}")
        self.last_arena = A
        return self.outputs(A, x)


class OracleShapes(ShapesEngine):
    """The oracle composed per shape, on the arena's own copies of the inputs."""

    def __init__(self, oracle):
        self.o, self.be = oracle, ga.NumpyBackend()

    def _send(self, x, A):
        y = Inputs()
        y.__dict__.update(x.__dict__)
        y.desc = A.get("group", SEND_GROUP, (x.G,))
        y.shards = A.get("shards", np.uint8, x.shards.shape)
        y.hdr = A.get("hdr", po.HDR_DTYPE, x.hdr.shape)
        y.sstamps = A.get("seg_stamps", po.SEG_STAMP, (x.n_rows,))
        y.fstamps = A.get("fec_stamps", po.FEC_STAMP, (x.n_fec,)) if x.n_fec else x.fstamps
        y.sorder = A.get("seg_order", np.uint32, (x.n_rows,)) if x.sorder is not None else None
        y.forder = A.get("fec_order", np.uint32, (x.n_fec,)) if x.forder is not None else None
        (sd, sl, fd, fl), _ = compose_shapes(y, lambda p, sub: wsc.compose(self.o, sub, sub.shards, sub.hdr,
                                                                          sub.sstamps, sub.fstamps, None, None))
        A.view("seg_dgram")[...] = sd.reshape(-1)
        A.view("seg_dlen")[...] = sl.view(np.uint8).reshape(-1)
        if x.n_fec:
            A.view("fec_dgram")[...] = fd.reshape(-1)
            A.view("fec_dlen")[...] = fl.view(np.uint8).reshape(-1)


class GpuShapes(ShapesEngine):
    """The product library on torch memory.  per_shape(x): the product's own rfec_wire_encode_send, one call per
    shape on gathered copies, scattered as the oracle's; same_buffers(x): rfec_wire_encode_send on the device
    buffers of the last call (a one-shape window in window order is one of its batches)."""

    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        self.single = wsc.GpuSend(lib, device)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    @staticmethod
    def _p(A, name):
        return A.ptr(name) if name in A.bufs else None

    def _send(self, x, A):
        p = self._p
        self.lib.timing_events(None, None)  # resets the launch count
        self.lib.wire_encode_send_shapes(x.plans, x.G, A.ptr("group"), x.n_rows, x.n_fec, x.stride, x.capacity,
                                         A.ptr("shards"), A.ptr("hdr"), A.ptr("seg_stamps"), A.ptr("seg_dgram"),
                                         A.ptr("seg_dlen"), p(A, "fec_stamps"), p(A, "fec_dgram"), p(A, "fec_dlen"),
                                         x.dstride, self._stream(), seg_order=p(A, "seg_order"),
                                         fec_order=p(A, "fec_order"))
        self.launches = self.lib.timing_launches()

    def per_shape(self, x):
        def one(p, sub):
            sub.case = (f"{x.name}/shape{p}", "", sub.G, False, False)
            sub.sorder = sub.forder = None
            return self.single.send(sub), None

        return compose_shapes(x, one)[0]

    def same_buffers(self, x):
        A, p = self.last_arena, self._p
        B = ga.Arena(self.be, self.out_bufs(x))
        self.lib.wire_encode_send(x.plans[0], x.G, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"),
                                  A.ptr("seg_stamps"), B.ptr("seg_dgram"), B.ptr("seg_dlen"), p(A, "fec_stamps"),
                                  p(B, "fec_dgram"), p(B, "fec_dlen"), x.dstride, self._stream(),
                                  seg_order=p(A, "seg_order"), fec_order=p(A, "fec_order"))
        self.be.sync()
        A.check(f"rfec_wire_encode_send after wire_encode_send_shapes {x.name}")
        B.check(f"rfec_wire_encode_send {x.name}")
        return self.outputs(B, x)
