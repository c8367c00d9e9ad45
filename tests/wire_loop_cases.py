"""Loop cases of the wire kernels (rfec_wire.hip) at a capped grid, shared by the CPU and the GPU tests of
test_wire_loops.py.

Every wire kernel runs on a persistent grid: a wave strides over its units (a quad of four datagrams in the
quarter-wave kernels, one datagram in the wave kernels) by nw = 16 * blocks and keeps state from one unit to the
next -- rows or datagrams loaded ahead, a header batch of 16 quads (64 datagrams in the wave parse) whose slot the
unit reads, a rotation of three buffers.  On the whole device a wave takes a second unit only above 16,384
datagrams and a second batch only above 262,144; with rfec_wire_set_grid_cap(c) (rfec_internal.h) the same depth is
reached by N of a few thousand, so whole slots, whole records and every length are compared with the oracle.

A case is (kernel, geometry, N, cap); it states the batches its deepest wave takes, which the test checks by
arithmetic from the grid that rfec_wire_last_path reports.  Engines: wire_cases.WireEngine (OracleWire on the CPU,
gpu_engine.GpuWire in HBM), every call's buffers in one guarded arena.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

import aux_kernel_cases as ac
import pyoracle as po
import wire_cases as wc

RFEC_TUNE_WAVE_PARSE = 1 << 3
WAVES = 16  # waves per block: nw = WAVES * blocks

# rfec_wire_last_path's kernel ids (rfec_internal.h RFEC_WIRE_K_*)
K_FRAME_FEC_32, K_FRAME_SEG_32, K_PARSE_20, K_PARSE_32, K_FRAME_SEG_Q, K_FRAME_FEC_Q, K_PARSE_Q = 1, 3, 4, 5, 6, 7, 8
K_ENCODE_FEC_Q, K_ENCODE_SEND_Q, K_ENCODE_SEND_Q2, K_ENCODE_SEND_SHAPES_Q, K_ENCODE_SEND_SHAPES_Q2 = 9, 10, 11, 12, 13

# kernel name -> (id, call, datagrams per unit, units per header batch, tuning)
KERNELS = {
    "parse_q": (K_PARSE_Q, "parse", 4, 16, 0),
    "seg_q": (K_FRAME_SEG_Q, "seg", 4, 16, 0),
    # k_frame_fec_q keeps no header batch (its fields come with each quad's rows); the depth is counted alike
    "fec_q": (K_FRAME_FEC_Q, "fec", 4, 16, 0),
    "parse20": (K_PARSE_20, "parse", 1, 64, RFEC_TUNE_WAVE_PARSE),
    "parse32": (K_PARSE_32, "parse", 1, 64, 0),
    # the wave framing keeps two buffers in turn and no batch; the depth is counted as the wave parse's
    "seg32": (K_FRAME_SEG_32, "seg", 1, 64, 0),
    "fec32": (K_FRAME_FEC_32, "fec", 1, 64, 0),
}

Case = namedtuple("Case", "kernel geom N cap")

# (capacity, stride, dstride)
Q_GEOMS = [(1200, 1216, 1264), (1200, 1200, 1280), (1000, 1008, 1056), (230, 240, 288), (15, 16, 64),
           # datagram slots that end exactly at a row of 16 chunks (chunk 32 / 48 would be the next slot's first):
           # no other framing test has a slot of 512 to 1,008 bytes
           (463, 464, 512), (700, 704, 768)]
# cap 1 (nw = 16): fewer quads than waves (the idle waves leave after the barrier); every wave ends exactly at a
# batch's end; one wave opens a second batch on a quad of one datagram; every wave in its second batch with a
# partial last quad; a third batch.  cap 3: nw = 48 is no power of two
Q_N1 = [1, 3, 4, 5, 63, 64, 65, 1024, 1025, 1024 + 64 + 3, 4 * 16 * 33 + 2]
Q_N3 = 4 * 48 * 16 + 4 * 48 + 1
Q_DEEP = [(1024 + 64 + 3, 1), (4 * 16 * 33 + 2, 1), (Q_N3, 3)]

# the wave kernels: cap 1; N - 1 = 0, 16, 32 (mod 48) past 1,024: wave 0 leaves the rotation of three in its first,
# second and third step (the other waves one step earlier); 16 * 129 + 7: a third batch
W_N1 = [1, 2, 15, 16, 17, 33, 49, 1024, 1025, 1057, 1073, 1089, 16 * 129 + 7]
W_N3 = 48 * 64 + 48 + 5
W_DEEP = [(1057, 1), (1073, 1), (1089, 1), (16 * 129 + 7, 1), (W_N3, 3)]
assert [(n - 1) % 48 for n in (1057, 1073, 1089)] == [0, 16, 32]
W_GEOMS = {
    "parse20": [(1200, 1216, 1264), (1000, 1008, 1056)],  # RFEC_TUNE_WAVE_PARSE at slots up to 1,280 bytes
    "parse32": [(1200, 1200, 1504), (1984, 2000, 2048)],
    "seg32": [(1300, 1312, 1344), (1984, 1984, 2048)],
    # a SIM_FEC of 1,300 bytes needs 1,349: the next multiple of 16 that rfec_wire_frame_fec takes
    "fec32": [(1300, 1312, 1360), (1984, 1984, 2048)],
}


def _cases():
    out = []
    for kern in ("parse_q", "seg_q", "fec_q"):
        out += [Case(kern, Q_GEOMS[0], n, 1) for n in Q_N1] + [Case(kern, Q_GEOMS[0], Q_N3, 3)]
        out += [Case(kern, g, n, 1) for g in Q_GEOMS[1:] for n in Q_N1[-2:]]  # every geometry at two deep N
    for kern, geoms in W_GEOMS.items():
        out += [Case(kern, geoms[0], n, 1) for n in W_N1] + [Case(kern, geoms[0], W_N3, 3)]
        out += [Case(kern, geoms[1], n, 1) for n in (1073, 16 * 129 + 7)]
    return out


CASES = _cases()


def case_id(c):
    return f"{c.kernel}-c{c.geom[0]}s{c.geom[1]}d{c.geom[2]}-N{c.N}-cap{c.cap}"


def is_deep(c):
    per = KERNELS[c.kernel][2]
    return (c.N, c.cap) in (Q_DEEP if per == 4 else W_DEEP)


def depth(c, blocks=None):
    """(units of the deepest wave, header batches it takes) on a grid of `blocks` blocks."""
    _, _, per, batch, _ = KERNELS[c.kernel]
    nw = WAVES * (c.cap if blocks is None else blocks)
    units = (c.N + per - 1) // per
    steps = (units + nw - 1) // nw
    return steps, (steps + batch - 1) // batch


# the batches each deep N claims (checked against depth() from the reported grid)
CLAIM = {(1024 + 64 + 3, 1): 2, (4 * 16 * 33 + 2, 1): 3, (Q_N3, 3): 2,
         (1057, 1): 2, (1073, 1): 2, (1089, 1): 2, (16 * 129 + 7, 1): 3, (W_N3, 3): 2}

# cases whose first batch of inputs misses a condition of conditions(): another seed (found by the CPU test)
SEEDS = {"parse20-c1200s1216d1264-N1057-cap1": 1}


def seed_of(c):
    return SEEDS.get(case_id(c), 0)


class Inputs:
    pass


@functools.lru_cache(maxsize=3)
def make_inputs(c):
    """The case's inputs and the oracle's outputs for them (computed once, shared, left unchanged)."""
    o = po.Oracle(1000)
    capacity, stride, dstride = c.geom
    call = KERNELS[c.kernel][1]
    x = Inputs()
    x.case, x.call = c, call
    N = c.N
    if call == "parse":
        # (bad_len: mixed_corrupt_batch alone yields no RFEC_WIRE_EBODY record)
        x.dgram, x.dlen = wc.mixed_corrupt_batch(o, capacity, stride, dstride, N, zero_ids=0.1, seed=seed_of(c),
                                                 bad_len=0.03)
        x.recs, x.pay = o.parse_batch(x.dgram, x.dlen, stride, capacity)
        return x
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()) + seed_of(c))
    seg = call == "seg"
    data, hdr, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=seg)
    garbage = rng.integers(0, 256, data.shape, dtype=np.uint8)  # past each size: the kernel masks it itself
    data = np.where(np.arange(stride)[None, :] >= sizes[:, None], garbage, data)
    big = rng.random(N) < 0.02
    over = (capacity + 1 + rng.integers(0, 40, int(big.sum()))).astype(np.uint16)
    x.status = None
    if seg:
        hdr["size"][big] = over
    else:
        sizes = sizes.astype(np.uint16)
        sizes[big] = over
        x.status = np.where(rng.random(N) < 0.05, -1, 0).astype(np.int8)
    x.data, x.hdr, x.sizes, x.stamps = data, hdr, sizes, stamps
    x.order = rng.permutation(N).astype(np.uint32)
    if seg:
        x.dgram, x.dlen = o.frame_seg_batch(data, hdr, stamps, capacity, dstride)
    else:
        x.dgram, x.dlen = o.frame_fec_batch(data, hdr, sizes, x.status, stamps, capacity, dstride)
    return x


def conditions(c, x):
    """What a deep case's inputs exercise, from the oracle's outputs alone; d + step is the datagram the same
    lanes of the same wave take in their next unit."""
    _, call, per, batch, _ = KERNELS[c.kernel]
    nw = WAVES * c.cap
    step = per * nw
    N = c.N
    d = np.arange(N)
    nxt = d + step
    has_next = nxt < N
    unit = d // per // nw  # the index of d's unit in its wave
    if call == "parse":
        st = x.recs["status"].astype(np.int64)
        ok_data = (st == 0) & (x.recs["data_size"] > 0)
        bad = st == -1
        follow = np.zeros(N, bool)
        follow[has_next] = ok_data[nxt[has_next]]
        return {
            "statuses": set(st.tolist()) >= {0, 1, -1, -2, -3},
            "half_ok": int((st == 0).sum()) * 2 > N,
            "badcrc_then_data": bool((bad & has_next & follow).any()),
            "badcrc_in_second_batch": bool((bad & (unit >= batch) & (unit < 2 * batch)).any()),
        }
    zero = x.dlen == 0
    follow = np.zeros(N, bool)
    follow[has_next] = x.dlen[nxt[has_next]] > 0
    return {"zero_then_valid": bool((zero & follow).any())}


# -- comparisons -----------------------------------------------------------------------------------------------
def same_frames(dgram, dlen, exp_dgram, exp_dlen, what):
    """Whole slots (the zeros past each length included) and every length."""
    assert dgram.shape == exp_dgram.shape and dlen.shape == exp_dlen.shape, what
    bad = np.nonzero(dlen != exp_dlen)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} lengths differ, the first at slot {int(bad[0])}: " \
                          f"{int(dlen[bad[0]])} != {int(exp_dlen[bad[0]])}"
    bad = np.nonzero((dgram != exp_dgram).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} slots differ, the first slot {int(bad[0])} at byte " \
                          f"{int(np.nonzero(dgram[bad[0]] != exp_dgram[bad[0]])[0][0])}"


def same_parse(recs, pay, exp_recs, exp_pay, what):
    """All 64 bytes of every record and whole payload slots."""
    n = len(exp_recs)
    assert recs.shape == exp_recs.shape and pay.shape == exp_pay.shape, what
    bad = np.nonzero((recs.view(np.uint8).reshape(n, 64) != exp_recs.view(np.uint8).reshape(n, 64)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, the first record {int(bad[0])}: " \
                          f"{recs[bad[0]]} != {exp_recs[bad[0]]}"
    bad = np.nonzero((pay != exp_pay).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} payload slots differ, the first slot {int(bad[0])} (status " \
                          f"{int(exp_recs['status'][bad[0]])}) at byte {int(np.nonzero(pay[bad[0]] != exp_pay[bad[0]])[0][0])}"


def same_split(split, exp_recs, T, what):
    want = ac.ref_rx_split(exp_recs, T)
    bad = np.nonzero(split.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} split entries differ, the first entry {int(bad[0])}: " \
                          f"{split[bad[0]]} != {want[bad[0]]} (status {int(exp_recs['status'][bad[0]])})"


SPLIT_T = (1, 3, 8)


def check_tag(engine, c, what):
    """The launch was the case's kernel on exactly `cap` blocks, and its deepest wave takes the batches claimed."""
    if not getattr(engine, "has_tag", False):
        return
    tag = engine.last_path
    kid, blocks = tag & 0xFF, tag >> 8
    assert kid == KERNELS[c.kernel][0], f"{what}: kernel id {kid}, the case is written for {KERNELS[c.kernel][0]}"
    assert blocks == c.cap, f"{what}: a grid of {blocks} blocks, not the cap's {c.cap}"
    if is_deep(c):
        steps, batches = depth(c, blocks)
        assert batches == CLAIM[(c.N, c.cap)] and steps > KERNELS[c.kernel][3], (what, steps, batches)


def run_case(engine, c):
    """The case on an engine: every call's outputs against the oracle's, byte for byte (the arena's guards and
    inputs are checked inside the engine).  A GPU engine runs it under the case's grid cap."""
    x = make_inputs(c)
    capacity, stride, dstride = c.geom
    what = case_id(c)
    cap = getattr(engine, "set_grid_cap", None)
    if cap is not None:
        cap(c.cap)
    try:
        if x.call == "parse":
            tuning = KERNELS[c.kernel][4]
            engine.tuning = tuning
            recs, pay = engine.parse(x.dgram, x.dlen, stride, capacity)
            check_tag(engine, c, what)
            same_parse(recs, pay, x.recs, x.pay, what)
            for T in SPLIT_T:
                w = f"{what} split T={T}"
                recs, pay, split = engine.parse_split(x.dgram, x.dlen, stride, capacity, 0, T, tuning)
                check_tag(engine, c, w)
                same_parse(recs, pay, x.recs, x.pay, w)
                same_split(split, x.recs, T, w)
        else:
            for order in (None, x.order):
                w = f"{what} {'in order' if order is None else 'permuted'}"
                if x.call == "seg":
                    g, gl = engine.frame_seg(x.data, x.hdr, x.stamps, capacity, dstride, order=order)
                else:
                    g, gl = engine.frame_fec(x.data, x.hdr, x.sizes, x.status, x.stamps, capacity, dstride,
                                             order=order)
                check_tag(engine, c, w)
                if order is not None:
                    g, gl = g[order], gl[order]  # datagram i was written to slot order[i]
                same_frames(g, gl, x.dgram, x.dlen, w)
    finally:
        if cap is not None:
            cap(0)


# -- the fused kernels: one case each at cap 1, on their own engines (wire_encode_cases.py, wire_send_cases.py,
# -- wire_send_shapes_cases.py), at a full-size geometry ------------------------------------------------------------
def _shape_seq(n):
    return [i % 3 for i in range(n)]


# name -> (family, kernel id, the family's case, units of work, what a wave carries from unit to unit)
FUSED = {
    # k_encode_frame_fec_q: a quad of SIM_FEC per step; the next quad's first member rows, header dword and stamp
    # are loaded at the bottom of the loop (load_first) and consumed at its top; no header batch.  45 groups of 3
    # lines = 135 datagrams = 34 quads on 16 waves: waves 0-1 take three quads (the prefetch is consumed twice),
    # the rest two, and the last quad holds 3 datagrams.
    "encode_fec": ("fec", K_ENCODE_FEC_Q, ("rows10x4", "c1200w", 45, True), 34),
    # k_encode_send_q<., 5>: 4 groups per step, nothing loaded ahead across units; inside a unit the SIM_SEG
    # headers of a line come in batches of 16 members (pass() when j & ~15 changes, through the wave's LDS buffer
    # HB): the 18-member line takes a second batch, the 2-member line after it a fresh one.  73 groups = 19 units
    # on 16 waves: waves 0-2 take a second unit (HB rewritten after the previous unit's last read), the last unit
    # holds one group.
    "send": ("send", K_ENCODE_SEND_Q, ("row18k20", "c1200w", 73, True, True), 19),
    # k_encode_send_q<., 2>, the instance for slots up to 512 bytes (463 + 49 = 512: the largest it takes)
    "send2": ("send", K_ENCODE_SEND_Q2, ("row18k20", "c463", 73, False, False), 19),
    # k_encode_send_shapes_q: 4 descriptors per step, one pass per distinct shape of the four, the same header
    # batches; shapes 0, 1, 2 in turn, so every quad mixes them and an 18-member line lies in a wave's second unit
    # (descriptor 66).  73 descriptors = 19 units on 16 waves, the last unit holds one.
    "shapes": ("shapes", K_ENCODE_SEND_SHAPES_Q,
               (["row18k20", "k2", "hand7"], "c1200w", _shape_seq(73), "window", "window", True, False), 19),
    "shapes2": ("shapes", K_ENCODE_SEND_SHAPES_Q2,
                (["row18k20", "k2", "hand7"], "c463", _shape_seq(73), "window", "window", False, True), 19),
}


@functools.lru_cache(maxsize=None)
def fused_inputs(name):
    import wire_encode_cases as wec
    import wire_send_cases as wsc
    import wire_send_shapes_cases as wss
    o = po.Oracle(1000)
    family, _, case, _ = FUSED[name]
    if family == "fec":
        return wec.make_inputs(o, case)
    if family == "send":
        return wsc.make_inputs(o, case)
    return wss.make_inputs(o, "loop-" + name, case)


def run_fused(name, engine, last_path=None, set_grid_cap=None):
    """The fused case on its family's engine (OracleFused / OracleSend / OracleShapes on the CPU, their Gpu
    counterparts with the grid capped at one block): whole slots and lengths against the oracle composed, and from
    the tag the kernel, the grid of one block and more units than its 16 waves."""
    import wire_encode_cases as wec
    import wire_send_cases as wsc
    family, kid, _, units = FUSED[name]
    x = fused_inputs(name)
    if set_grid_cap is not None:
        set_grid_cap(1)
    try:
        got = engine.fused(x) if family == "fec" else engine.send(x)
        tag = last_path() if last_path is not None else None
    finally:
        if set_grid_cap is not None:
            set_grid_cap(0)
    if tag is not None:
        assert tag & 0xFF == kid and tag >> 8 == 1, (name, hex(tag))
        assert units > WAVES * (tag >> 8), (name, units)
    if family == "fec":
        assert (x.count + 3) // 4 == units and units > 2 * WAVES and x.count % 4
        wec.compare(got[0], got[1], x.exp_dgram, x.exp_dlen, f"{name} vs the oracle composed")
    else:
        assert (x.G + 3) // 4 == units and x.G % 4
        wsc.compare_all(got, x.exp, f"{name} vs the oracle composed")
