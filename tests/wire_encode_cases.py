"""Cases, inputs, expected values and engines for rfec_wire_encode_fec (the
fused encode + SIM_FEC framing), shared by the CPU and the GPU tests of
test_wire_encode.py.

A case is (plan, geometry, groups, order); its id holds every field and its
seed derives from the id.  Expected values come from the oracle composed --
frame_fec_batch(*encode_batch(...)) permuted by `order` -- and, on the GPU,
from the product's own rfec_encode_batch + rfec_wire_frame_fec on the same
device buffers; whole [count][dstride] slots and every length are compared.

An engine runs one fused call with every buffer in a guarded arena
(guarded_arena.py: dgram and dlen between canary guards, the inputs compared
with what was uploaded after the call):
    OracleFused   numpy memory, the oracle composed (the CPU run of the checks)
    GpuFused      torch memory in HBM, the product library
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import wire_cases as wc

ROWS, COLS = 1, 2
DGRAM_FILL, DLEN_FILL = 0xEE, 0x77  # differ from guarded_arena.CANARY
assert ga.CANARY not in (DGRAM_FILL, DLEN_FILL)


# -- plans -------------------------------------------------------------------------------------------------------
def _hand_plan(k, lines):
    p = po.rfec_plan()
    p.k, p.n_lines, p.n_row_lines = k, len(lines), len(lines)
    for i, (first, stride, count) in enumerate(lines):
        p.line[i].first, p.line[i].stride, p.line[i].count, p.line[i].index = first, stride, count, i
    return p


PLANS = {
    "rows10x4": lambda o: o.plan_matrix(10, 3, 4, ROWS),          # lines of 4 / 4 / 2
    "full3x4k10": lambda o: o.plan_matrix(10, 3, 4, ROWS | COLS),  # the sender's plan: 3 rows + 4 strided columns
    "full4x4k16": lambda o: o.plan_matrix(16, 4, 4, ROWS | COLS),
    "rows4k32": lambda o: o.plan_matrix(32, 8, 4, ROWS),
    "k2": lambda o: o.plan_matrix(2, 1, 2, ROWS),                  # one line
    "k200pf10": lambda o: o.plan_from_fraction(200, 10),           # 14 rows of 15 (the last of 5) + 15 columns
    # the 8-bit limits of first / stride / count: a line of all 255 members beside lines of 1-3 (a line of one
    # member is refused, as flex_fec_generate refuses it)
    "k255": lambda o: _hand_plan(255, [(0, 1, 255), (254, 1, 1), (0, 127, 3), (0, 254, 2), (253, 1, 2)]),
}

# (capacity, stride, dstride); "p": every shard byte in [16 CD, stride) poisoned with 0xA5
GEOMS = {
    "c1200": (1200, 1200, 1264), "c1200w": (1200, 1216, 1280), "c1000": (1000, 1008, 1056),
    "c1000p": (1000, 1040, 1280), "c1231": (1231, 1232, 1280),  # 1231 + 49 = 1280: the largest the kernel takes
    "c256": (256, 256, 320), "c15": (15, 16, 64), "c0": (0, 16, 64), "c48": (48, 48, 112),
}
POISON = 0xA5

# (plan, geometry, groups, order?): counts = 0, 1, 2, 3 (mod 4) and 1; more than one block (64 datagrams)
CASES = [
    ("rows10x4", "c1200w", 7, False),    # 21 = 1 (mod 4)
    ("rows10x4", "c1200", 6, True),      # 18 = 2
    ("full3x4k10", "c1200w", 5, False),  # 35 = 3
    ("full3x4k10", "c1000", 4, True),    # 28 = 0
    ("full3x4k10", "c1200w", 300, True),  # 2,100 datagrams: 33 blocks
    ("full4x4k16", "c1000p", 3, False),  # 24 = 0
    ("rows4k32", "c256", 9, True),       # 72: two blocks
    ("rows4k32", "c1200", 2, False),
    ("k2", "c15", 1, False),             # count == 1
    ("k2", "c0", 5, True),
    ("k200pf10", "c1231", 2, False),     # 58 = 2
    ("k255", "c1200w", 3, False),        # 15 = 3
    ("rows10x4", "c1231", 11, True),     # 33 = 1
    ("rows10x4", "c1000p", 13, True),    # 39 = 3
    ("full3x4k10", "c15", 3, False),
]
LOOP_CASE = ("k2", "c48", 40003, False)  # more datagrams than the resident waves' first quads
CHUNK_CASE = ("full3x4k10", "c1000", 50, None)  # run with and without order


def case_id(c):
    plan, geom, groups, order = c
    return f"{plan}-{geom}-G{groups}-{'perm' if order else 'inorder'}"


class Inputs:
    pass


def make_inputs(oracle, c):
    """The case's inputs and what the oracle composed expects of them."""
    pname, gname, G, with_order = c
    capacity, stride, dstride = GEOMS[gname]
    plan = PLANS[pname](oracle)
    k, n = plan.k, plan.n_lines
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    N = G * k
    # data_size uniform in [0, capacity], the edges more often; shard bytes zero past it
    sizes = rng.integers(0, capacity + 1, N)
    u = rng.random(N)
    sizes[u < 0.15] = 0
    sizes[u > 0.90] = capacity
    shards = rng.integers(0, 256, (N, stride), dtype=np.uint8)
    shards[np.arange(stride)[None, :] >= sizes[:, None]] = 0
    cd16 = 16 * ((capacity + 15) // 16)
    if gname.endswith("p"):
        assert cd16 < stride
        shards[:, cd16:] = POISON
    hdr = np.zeros(N, po.HDR_DTYPE)
    for f in ("seq", "fid", "ts"):
        hdr[f] = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    for f in ("index", "total"):
        hdr[f] = rng.integers(0, 2**16, N)
    for f in ("ftype", "payload_type"):
        hdr[f] = rng.integers(0, 256, N)
    hdr["size"] = sizes
    # about 5 % of the lines: one member with size > capacity (the line is refused)
    for d in np.nonzero(rng.random(G * n) < 0.05)[0]:
        g, l = divmod(int(d), n)
        m = plan.members(l)
        hdr["size"][g * k + m[int(rng.integers(len(m)))]] = min(65535, capacity + 1 + int(rng.integers(0, 40)))
    count = G * n
    _, _, _, stamps = wc.random_batch(rng, count, 16, 0, seg=False)
    order = rng.permutation(count).astype(np.uint32) if with_order else None

    x = Inputs()
    x.case, x.plan, x.G, x.k, x.n, x.count = c, plan, G, k, n, count
    x.capacity, x.stride, x.dstride = capacity, stride, dstride
    x.shards, x.hdr, x.stamps, x.order = shards.reshape(G, k, stride), hdr.reshape(G, k), stamps, order
    x.enc = oracle.encode_batch(plan, x.shards, x.hdr, capacity)  # parity, meta, fec_size, status
    dgram, dlen = oracle.frame_fec_batch(*x.enc, stamps, capacity, dstride)
    x.exp_dgram, x.exp_dlen = permuted(dgram, dlen, order)
    return x


def permuted(dgram, dlen, order):
    """Datagram i in slot order[i]."""
    if order is None:
        return dgram, dlen
    d, l = np.empty_like(dgram), np.empty_like(dlen)
    d[order], l[order] = dgram, dlen
    return d, l


def conditions(x):
    """What the case's inputs exercise, from the oracle's encode_batch."""
    _, _, fsize, status = x.enc
    fsize, status = fsize.reshape(-1).astype(np.int64), status.reshape(-1)
    ok = status == 0
    counts = np.array([x.plan.line[d % x.n].count for d in range(x.count)])
    quads = [set(counts[q:q + 4].tolist()) for q in range(0, x.count - 3, 4)]
    return {
        "refused": bool((status == -1).any()),
        "full": bool((ok & (fsize == x.capacity)).any()),
        "empty": bool((ok & (fsize == 0)).any()),
        # the 4-byte trailer at byte 45 + L crosses a 16-byte chunk
        "crc_straddles": bool((ok & ((45 + fsize) % 16 > 12)).any()),
        "mixed_quad": any(len(s) > 1 for s in quads),
    }


def compare(dgram, dlen, exp_dgram, exp_dlen, what):
    """Whole slots (the zeros past each length included) and every length."""
    assert dgram.shape == exp_dgram.shape and dlen.shape == exp_dlen.shape, what
    bad = np.nonzero(dlen != exp_dlen)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} lengths differ, the first at slot {int(bad[0])}: " \
                          f"{int(dlen[bad[0]])} != {int(exp_dlen[bad[0]])}"
    bad = np.nonzero((dgram != exp_dgram).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} slots differ, the first slot {int(bad[0])} at byte " \
                          f"{int(np.nonzero(dgram[bad[0]] != exp_dgram[bad[0]])[0][0])}"


# -- engines -----------------------------------------------------------------------------------------------------
class FusedEngine:
    """fused(x) -> (dgram [count][dstride], dlen [count]) with the call's buffers in one guarded arena.  mutate
    (tests): called with the arena after the call and before its checks."""

    be = None
    mutate = None

    def arena(self, x):
        bufs = [ga.Buf("shards", x.shards.size, x.shards, "in", 16), ga.Buf("hdr", x.hdr.size * 20, x.hdr, "in", 4),
                ga.Buf("stamps", x.count * 24, x.stamps, "in", 4)]
        if x.order is not None:
            bufs.append(ga.Buf("order", x.count * 4, x.order, "in", 4))
        bufs += [ga.Buf("dgram", x.count * x.dstride, DGRAM_FILL, "out", 16),
                 ga.Buf("dlen", x.count * 2, DLEN_FILL, "out", 2)]
        return ga.Arena(self.be, bufs)

    def fused(self, x):
        A = self.arena(x)
        self._fused(x, A)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_encode_fec {case_id(x.case)}")
        self.last_arena = A
        return A.get("dgram", np.uint8, (x.count, x.dstride)), A.get("dlen", np.uint16, (x.count,))


class OracleFused(FusedEngine):
    def __init__(self, oracle):
        self.o, self.be = oracle, ga.NumpyBackend()

    def _fused(self, x, A):
        shards = A.get("shards", np.uint8, x.shards.shape)
        hdr = A.get("hdr", po.HDR_DTYPE, x.hdr.shape)
        stamps = A.get("stamps", po.FEC_STAMP, (x.count,))
        order = A.get("order", np.uint32, (x.count,)) if x.order is not None else None
        d, l = self.o.frame_fec_batch(*self.o.encode_batch(x.plan, shards, hdr, x.capacity), stamps, x.capacity,
                                      x.dstride)
        d, l = permuted(d, l, order)
        A.view("dgram")[...] = d.reshape(-1)
        A.view("dlen")[...] = l.view(np.uint8).reshape(-1)


class GpuFused(FusedEngine):
    """The product library on torch memory; two_calls(x): rfec_encode_batch + rfec_wire_frame_fec on the device
    buffers of the last fused call (its arena is checked again afterwards: the inputs are still as uploaded)."""

    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _fused(self, x, A):
        self.lib.wire_encode_fec(x.plan, x.G, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"), A.ptr("stamps"),
                                 x.dstride, A.ptr("dgram"), A.ptr("dlen"), self._stream(),
                                 order=A.ptr("order") if x.order is not None else None)

    def two_calls(self, x):
        A = self.last_arena
        B = ga.Arena(self.be, [ga.Buf("parity", x.count * x.stride, 0x5A, "out"),
                               ga.Buf("meta", x.count * 20, 0x5A, "out"), ga.Buf("fec_size", x.count * 2, 0, "out"),
                               ga.Buf("status", x.count, 7, "out"),
                               ga.Buf("dgram", x.count * x.dstride, DGRAM_FILL, "out", 16),
                               ga.Buf("dlen", x.count * 2, DLEN_FILL, "out", 2)])
        self.lib.encode_batch(x.plan, x.G, x.stride, x.capacity, A.ptr("shards"), A.ptr("hdr"), B.ptr("parity"),
                              B.ptr("meta"), B.ptr("fec_size"), B.ptr("status"), self._stream())
        self.lib.wire_frame_fec(x.count, x.stride, x.capacity, B.ptr("parity"), B.ptr("meta"), B.ptr("fec_size"),
                                B.ptr("status"), A.ptr("stamps"), x.dstride, B.ptr("dgram"), B.ptr("dlen"),
                                self._stream(), order=A.ptr("order") if x.order is not None else None)
        self.be.sync()
        A.check(f"two calls after wire_encode_fec {case_id(x.case)}")
        B.check(f"two calls {case_id(x.case)}")
        return B.get("dgram", np.uint8, (x.count, x.dstride)), B.get("dlen", np.uint16, (x.count,))


# -- the chunked run, in a process of its own (RFEC_WIRE_ENCODE_CHUNK_GROUPS is read from the environment) ---------
def chunk_child():
    """Prints one line per order variant: the launches the fused call took and a checksum of its output."""
    import hashlib

    from razor_amd.fec import native
    o = po.Oracle(1000)
    eng = GpuFused(native(1000))
    for with_order in (False, True):
        x = make_inputs(o, CHUNK_CASE[:3] + (with_order,))
        eng.lib.timing_events(None, None)  # resets the launch count
        d, l = eng.fused(x)
        launches = eng.lib.timing_launches()
        compare(d, l, x.exp_dgram, x.exp_dlen, "chunked fused call vs the oracle")
        print("chunk", int(with_order), launches, hashlib.sha256(d.tobytes() + l.tobytes()).hexdigest(), flush=True)


if __name__ == "__main__":
    chunk_child()
