"""Cases, inputs, expected values and engines for rfec_wire_encode_send (a
batch's SIM_SEG and SIM_FEC datagrams in one kernel), shared by the CPU and the
GPU tests of test_wire_send.py.  Built on wire_encode_cases.py.

A case is (plan, geometry, groups, seg order?, fec order?); its id holds every
field and its seed derives from the id.  Expected values come from the oracle
composed -- frame_seg_batch for the segments, frame_fec_batch(*encode_batch(...))
for the parities, each permuted by its order -- and, on the GPU, from the
product's own rfec_wire_frame_seg + rfec_wire_encode_fec on the same device
buffers; whole [count][dstride] slots and every length are compared.

An engine runs one fused call with every buffer in a guarded arena
(guarded_arena.py: the four outputs between canary guards, the inputs compared
with what was uploaded after the call):
    OracleSend   numpy memory, the oracle composed (the CPU run of the checks)
    GpuSend      torch memory in HBM, the product library
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import wire_cases as wc
import wire_encode_cases as wec
from wire_encode_cases import DGRAM_FILL, DLEN_FILL, POISON, compare, permuted  # noqa: F401

ROWS, COLS = wec.ROWS, wec.COLS

PLANS = {
    "rows10x4": wec.PLANS["rows10x4"],                                # lines of 4 / 4 / 2
    "full3x4k10": wec.PLANS["full3x4k10"],                            # every member on a row and a column
    "rows9x4": lambda o: o.plan_matrix(9, 3, 4, ROWS),                # member 8: the one-member last row, dropped
    "full3x4k9": lambda o: o.plan_matrix(9, 3, 4, ROWS | COLS),       # member 8 on a column only
    "cols10x4": lambda o: o.plan_matrix(10, 3, 4, COLS),              # strided lines only
    # member 2 on no line, member 3 on a one-member line (refused), member 5 on two lines
    "hand7": lambda o: wec._hand_plan(7, [(0, 1, 2), (3, 1, 1), (4, 1, 3), (5, 1, 2)]),
    "k2": wec.PLANS["k2"],
    "k1": lambda o: wec._hand_plan(1, []),                            # no line: segments only
    "k255": wec.PLANS["k255"],                                        # a strip of all 255 members
}
# plans of the capped-grid loop cases (wire_loop_cases.py) alone: a line of 18 members is two SIM_SEG header batches
# of 16 in k_encode_send_q / k_encode_send_shapes_q, beside a line of 2
LOOP_PLANS = {"row18k20": lambda o: wec._hand_plan(20, [(0, 1, 18), (18, 1, 2)])}

# (capacity, stride, dstride); "p": every shard byte in [16 CD, stride) poisoned
GEOMS = {
    "c1200w": (1200, 1216, 1280), "c1000": (1000, 1008, 1056), "c1231": (1231, 1232, 1280), "c15": (15, 16, 64),
    "c256": (256, 256, 320), "c1000p": (1000, 1040, 1280), "c64": (64, 64, 128),
    # the kernel's two instances: slots up to 512 bytes take two rows of 16 chunks (463 + 49 = 512: a full-size
    # SIM_FEC ends at the two-row window's end), wider ones five
    "c463": (463, 464, 512), "c464": (464, 464, 528),
}

# (plan, geometry, groups, seg order?, fec order?).  ns = G k and nf = G n each hit 0-3 (mod 4); one group.
CASES = [
    ("rows10x4", "c1200w", 7, False, False),   # ns 70 = 2, nf 21 = 1
    ("rows10x4", "c1000", 6, True, True),      # ns 60 = 0, nf 18 = 2
    ("full3x4k10", "c1200w", 5, False, False),  # nf 35 = 3
    ("full3x4k10", "c1231", 4, True, False),   # nf 28 = 0
    ("rows9x4", "c1200w", 3, False, False),    # ns 27 = 3, nf 6
    ("rows9x4", "c256", 50, False, True),      # 13 units: more than one wave
    ("full3x4k9", "c1000p", 5, False, False),  # ns 45 = 1
    ("cols10x4", "c1000", 3, False, False),
    ("hand7", "c1200w", 9, False, False),      # ns 63 = 3
    ("hand7", "c15", 2, True, True),
    ("k2", "c15", 1, False, False),            # one group
    ("k2", "c256", 5, False, False),
    ("k1", "c1200w", 6, False, False),         # n_lines == 0: the FEC pointers are NULL
    ("k1", "c15", 1, True, False),
    ("k255", "c1200w", 3, False, False),
    ("rows10x4", "c1000p", 13, False, False),
    ("rows10x4", "c15", 2, False, False),
    ("rows10x4", "c463", 5, False, False), ("full3x4k10", "c464", 5, False, False),
    # every combination of the two orders on one small case
    ("full3x4k10", "c1000", 3, False, False), ("full3x4k10", "c1000", 3, True, False),
    ("full3x4k10", "c1000", 3, False, True), ("full3x4k10", "c1000", 3, True, True),
]
# the kernel's unit of work is four groups per wave: more units than the waves resident at once
LOOP_CASE = ("rows10x4", "c64", 4 * 4099 + 1, False, False)
CHUNK_CASE = ("full3x4k10", "c1000", 50, None, None)  # run with and without orders


def case_id(c):
    plan, geom, groups, so, fo = c
    return f"{plan}-{geom}-G{groups}-seg{'perm' if so else 'inorder'}-fec{'perm' if fo else 'inorder'}"


class Inputs:
    pass


def seg_hs(hdr):
    """The SIM_SEG header's size by the field widths (sim_proto.inl:83-125)."""
    return (26 + 2 * (hdr["seq"] > 65535).astype(np.int64) + 2 * (hdr["fid"] > 65535) + 2 * (hdr["total"] > 255))


def make_inputs(oracle, c):
    """The case's inputs and what the oracle composed expects of them."""
    pname, gname, G, with_so, with_fo = c
    capacity, stride, dstride = GEOMS[gname]
    plan = (PLANS.get(pname) or LOOP_PLANS[pname])(oracle)
    k, n = plan.k, plan.n_lines
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    N = G * k
    big = N > 5000  # the loop case: cheap inputs
    # headers of every width (random_batch: half of seq, fid and total narrow), remb 0 and not
    _, hdr, _, sstamps = wc.random_batch(rng, N, 16, 0, seg=True)
    hdr = hdr.reshape(G, k)
    # group 0: packet ids that straddle 65,535 / 65,536 with the other fields narrow, so its lines' members differ
    # in header size by the packet id alone; groups 0 and 1 (one quad): total 255 and 256
    hdr["seq"][0] = 65536 - (k + 1) // 2 + np.arange(k)
    hdr["fid"][0] = 77
    hdr["total"][0] = 255
    if G > 1:
        hdr["total"][1] = 256
    hdr = hdr.reshape(-1)
    sizes = rng.integers(0, capacity + 1, N)
    u = rng.random(N)
    sizes[u < 0.12] = 0
    sizes[(u >= 0.12) & (u < 0.18)] = min(1, capacity)
    sizes[u > 0.90] = capacity
    hs = seg_hs(hdr)
    if capacity >= 512 and not big:
        # SIM_SEG trailers (at byte hs + L) across a 64-lane row's edge (256 bytes) and across a chunk's
        for d in rng.choice(N, max(2, N // 10), replace=False):
            sizes[d] = 256 * int(rng.integers(1, capacity // 256)) + 254 - hs[d] + int(rng.integers(0, 2))
        # a SIM_FEC trailer (at byte 45 + max L) likewise: every member of the last group's line 0 at most Lf
        if n:
            Lf = 256 + 254 - 45
            m = (G - 1) * k + np.array(plan.members(0))
            sizes[m] = np.minimum(sizes[m], Lf)
            sizes[m[-1]] = Lf
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
    # about 6 % of the segments (at least one): data_size above the capacity -- SEG length 0, its lines refused
    over = np.nonzero(rng.random(N) < 0.06)[0]
    over = over if len(over) else np.array([N // 2])
    hdr["size"][over] = np.minimum(65535, capacity + 1 + (rng.integers(0, 40, len(over)) * (rng.random(len(over)) < 0.5)))
    ns, nf = N, G * n
    _, _, _, fstamps = wc.random_batch(rng, max(nf, 1), 16, 0, seg=False)
    fstamps = fstamps[:nf]

    x = Inputs()
    x.case, x.plan, x.G, x.k, x.n, x.ns, x.nf = c, plan, G, k, n, ns, nf
    x.capacity, x.stride, x.dstride = capacity, stride, dstride
    x.shards, x.hdr, x.sstamps, x.fstamps = shards.reshape(G, k, stride), hdr.reshape(G, k), sstamps, fstamps
    x.sorder = rng.permutation(ns).astype(np.uint32) if with_so else None
    x.forder = rng.permutation(nf).astype(np.uint32) if with_fo and nf else None
    x.exp, x.enc = compose(oracle, x, x.shards, x.hdr, x.sstamps, x.fstamps, x.sorder, x.forder)
    return x


def compose(oracle, x, shards, hdr, sstamps, fstamps, sorder, forder):
    """((seg_dgram, seg_dlen, fec_dgram, fec_dlen), enc): the oracle's framing of the segments and its encode +
    framing of the parities; enc: what its encode_batch returned (None without lines)."""
    sd, sl = oracle.frame_seg_batch(shards, hdr.reshape(-1), sstamps, x.capacity, x.dstride)
    sd, sl = permuted(sd, sl, sorder)
    if x.nf:
        enc = oracle.encode_batch(x.plan, shards, hdr, x.capacity)
        fd, fl = oracle.frame_fec_batch(*enc, fstamps, x.capacity, x.dstride)
        fd, fl = permuted(fd, fl, forder)
    else:
        enc = None
        fd, fl = np.zeros((0, x.dstride), np.uint8), np.zeros(0, np.uint16)
    return (sd, sl, fd, fl), enc


def owners(plan):
    """Per member: the lines that hold it."""
    own = [[] for _ in range(plan.k)]
    for l in range(plan.n_lines):
        for m in plan.members(l):
            own[m].append(l)
    return own


def conditions(x):
    """What the case's inputs exercise, from the oracle's outputs (in input order: the orders undone)."""
    sd, sl, fd, fl = x.exp
    if x.sorder is not None:
        sl = sl[x.sorder]
    sl = sl.astype(np.int64)
    size = x.hdr["size"].reshape(-1).astype(np.int64)
    live = sl > 0
    hs = np.where(live, sl - 4 - size, 0).reshape(x.G, x.k)
    mixed = False
    for l in range(x.n):
        h = hs[:, x.plan.members(l)]
        ok = (h > 0).all(1)
        mixed = mixed or bool((ok & (h.min(1) != h.max(1))).any())
    own = owners(x.plan)
    end = sl - 4  # the trailer's first byte
    c = {
        "hs": set(np.unique(hs[hs > 0]).tolist()),
        "mixed_hs_line": mixed,
        "seg_oversize": bool(((size > x.capacity) & (sl == 0)).any()) and bool((size == x.capacity + 1).any()),
        "seg_size_0": bool((live & (size == 0)).any()),
        "seg_size_1": bool((live & (size == 1)).any()),
        "seg_size_cap": bool((live & (size == x.capacity)).any()),
        "seg_crc_chunk": bool((live & (end % 16 > 12)).any()),
        "seg_crc_row": bool((live & (end % 256 > 252)).any()),
        "remb_0": bool((x.sstamps["remb"] == 0).any()), "remb_set": bool((x.sstamps["remb"] != 0).any()),
        "fid_wide": bool((x.hdr["fid"] > 65535).any()), "fid_narrow": bool((x.hdr["fid"] <= 65535).any()),
        "orphan": any(len(o) == 0 for o in own),
        "on_two_lines": any(len(o) == 2 for o in own),
        "one_member_line": any(x.plan.line[l].count == 1 for l in range(x.n)),
        "no_lines": x.n == 0,
        "fec_refused": False, "fec_crc_chunk": False, "fec_crc_row": False, "ragged_line": False,
    }
    # total 255 and 256 in two groups of one quad of groups
    tot = x.hdr["total"]
    c["total_255_256"] = any({255, 256} <= set(tot[q:q + 4].reshape(-1).tolist()) for q in range(0, x.G, 4))
    if x.nf:
        _, _, fsize, status = x.enc
        fsize, status = fsize.reshape(-1).astype(np.int64), status.reshape(-1)
        ok = status == 0
        c["fec_refused"] = bool((status == -1).any())
        c["fec_crc_chunk"] = bool((ok & ((45 + fsize) % 16 > 12)).any())
        c["fec_crc_row"] = bool((ok & ((45 + fsize) % 256 > 252)).any())
        sz = x.hdr["size"]
        c["ragged_line"] = any(len(set(sz[g, x.plan.members(l)].tolist())) > 1 for g in range(min(x.G, 8))
                               for l in range(x.n))
    return c


def compare_all(got, exp, what):
    compare(got[0], got[1], exp[0], exp[1], f"{what}, SIM_SEG")
    compare(got[2], got[3], exp[2], exp[3], f"{what}, SIM_FEC")


# -- engines -----------------------------------------------------------------------------------------------------
class SendEngine:
    """send(x) -> (seg_dgram [ns][dstride], seg_dlen [ns], fec_dgram [nf][dstride], fec_dlen [nf]) with the call's
    buffers in one guarded arena (no SIM_FEC buffers when the plan has no line: the call gets NULL).  mutate
    (tests): called with the arena after the call and before its checks."""

    be = None
    mutate = None

    def arena(self, x):
        bufs = [ga.Buf("shards", x.shards.size, x.shards, "in", 16), ga.Buf("hdr", x.hdr.size * 20, x.hdr, "in", 4),
                ga.Buf("seg_stamps", x.ns * 12, x.sstamps, "in", 4)]
        if x.nf:
            bufs.append(ga.Buf("fec_stamps", x.nf * 24, x.fstamps, "in", 4))
        if x.sorder is not None:
            bufs.append(ga.Buf("seg_order", x.ns * 4, x.sorder, "in", 4))
        if x.forder is not None:
            bufs.append(ga.Buf("fec_order", x.nf * 4, x.forder, "in", 4))
        bufs += [ga.Buf("seg_dgram", x.ns * x.dstride, DGRAM_FILL, "out", 16),
                 ga.Buf("seg_dlen", x.ns * 2, DLEN_FILL, "out", 2)]
        if x.nf:
            bufs += [ga.Buf("fec_dgram", x.nf * x.dstride, DGRAM_FILL, "out", 16),
                     ga.Buf("fec_dlen", x.nf * 2, DLEN_FILL, "out", 2)]
        return ga.Arena(self.be, bufs)

    @staticmethod
    def outputs(A, x):
        sd, sl = A.get("seg_dgram", np.uint8, (x.ns, x.dstride)), A.get("seg_dlen", np.uint16, (x.ns,))
        if not x.nf:
            return sd, sl, np.zeros((0, x.dstride), np.uint8), np.zeros(0, np.uint16)
        return sd, sl, A.get("fec_dgram", np.uint8, (x.nf, x.dstride)), A.get("fec_dlen", np.uint16, (x.nf,))

    def send(self, x):
        A = self.arena(x)
        self._send(x, A)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_encode_send {case_id(x.case)}")
        self.last_arena = A
        return self.outputs(A, x)


class OracleSend(SendEngine):
    def __init__(self, oracle):
        self.o, self.be = oracle, ga.NumpyBackend()

    def _send(self, x, A):
        shards = A.get("shards", np.uint8, x.shards.shape)
        hdr = A.get("hdr", po.HDR_DTYPE, x.hdr.shape)
        ss = A.get("seg_stamps", po.SEG_STAMP, (x.ns,))
        fs = A.get("fec_stamps", po.FEC_STAMP, (x.nf,)) if x.nf else None
        so = A.get("seg_order", np.uint32, (x.ns,)) if x.sorder is not None else None
        fo = A.get("fec_order", np.uint32, (x.nf,)) if x.forder is not None else None
        (sd, sl, fd, fl), _ = compose(self.o, x, shards, hdr, ss, fs, so, fo)
        A.view("seg_dgram")[...] = sd.reshape(-1)
        A.view("seg_dlen")[...] = sl.view(np.uint8).reshape(-1)
        if x.nf:
            A.view("fec_dgram")[...] = fd.reshape(-1)
            A.view("fec_dlen")[...] = fl.view(np.uint8).reshape(-1)


class GpuSend(SendEngine):
    """The product library on torch memory; two_calls(x): rfec_wire_frame_seg + rfec_wire_encode_fec on the device
    buffers of the last fused call (its arena is checked again afterwards: the inputs are still as uploaded)."""

    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    @staticmethod
    def _p(A, name):
        return A.ptr(name) if name in A.bufs else None

    def _send(self, x, A):
        p = self._p
        self.lib.wire_encode_send(x.plan, x.G, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"),
                                  A.ptr("seg_stamps"), A.ptr("seg_dgram"), A.ptr("seg_dlen"), p(A, "fec_stamps"),
                                  p(A, "fec_dgram"), p(A, "fec_dlen"), x.dstride, self._stream(),
                                  seg_order=p(A, "seg_order"), fec_order=p(A, "fec_order"))

    def two_calls(self, x):
        A, p = self.last_arena, self._p
        bufs = [ga.Buf("seg_dgram", x.ns * x.dstride, DGRAM_FILL, "out", 16),
                ga.Buf("seg_dlen", x.ns * 2, DLEN_FILL, "out", 2)]
        if x.nf:
            bufs += [ga.Buf("fec_dgram", x.nf * x.dstride, DGRAM_FILL, "out", 16),
                     ga.Buf("fec_dlen", x.nf * 2, DLEN_FILL, "out", 2)]
        B = ga.Arena(self.be, bufs)
        self.lib.wire_frame_seg(x.ns, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"), A.ptr("seg_stamps"),
                                x.dstride, B.ptr("seg_dgram"), B.ptr("seg_dlen"), self._stream(),
                                order=p(A, "seg_order"))
        if x.nf:
            self.lib.wire_encode_fec(x.plan, x.G, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"),
                                     A.ptr("fec_stamps"), x.dstride, B.ptr("fec_dgram"), B.ptr("fec_dlen"),
                                     self._stream(), order=p(A, "fec_order"))
        self.be.sync()
        A.check(f"two calls after wire_encode_send {case_id(x.case)}")
        B.check(f"two calls {case_id(x.case)}")
        return self.outputs(B, x)


# -- the chunked run, in a process of its own (RFEC_WIRE_ENCODE_CHUNK_GROUPS is read from the environment) ---------
def chunk_child():
    """Prints one line per order variant: the launches the fused call took and a checksum of its output."""
    import hashlib

    from razor_amd.fec import native
    o = po.Oracle(1000)
    eng = GpuSend(native(1000))
    for with_order in (False, True):
        x = make_inputs(o, CHUNK_CASE[:3] + (with_order, with_order))
        eng.lib.timing_events(None, None)  # resets the launch count
        got = eng.send(x)
        launches = eng.lib.timing_launches()
        compare_all(got, x.exp, "chunked fused call vs the oracle")
        print("chunk", int(with_order), launches, hashlib.sha256(b"".join(a.tobytes() for a in got)).hexdigest(),
              flush=True)


if __name__ == "__main__":
    chunk_child()
