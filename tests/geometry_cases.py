"""Geometry cases of the batched encode / recover kernels, shared by the CPU run
(OracleArenaEngine: the oracle behind guarded arenas) and the GPU run
(GpuEngine), both from tests/test_geometry.py.

What they add to parity_cases.py's fixtures: every written slot is compared
over its WHOLE stride ("Slot tails" of include/razor_fec.h), at strides with a
tail past the last chunk; group counts at the edges of every kernel's
groups-per-block rule; capacities on both sides of the thresholds that switch
kernels; and every case names the dispatch tag (rfec_internal.h RFEC_PATH) it
expects and asserts it, so a dispatch change cannot drop a kernel out of the
suite unnoticed.  Shapes are the smallest that reach a branch.  The launchers'
rules (groups per block, the period `every` of the header blocks in a grid) are
restated here, and a case written for more header than payload blocks asserts
every == 0 from them.

An engine is parity_cases.py's (encode, recover, recover_out; the GPU ones also
recover_packed or recover_packed_matrix, with `pack_path`) with `last_path` (0:
the engine has no dispatch).  Inputs come
from a seeded numpy generator: ragged sizes, zeros past data_size, and the
erasure / lost parity / header corruption recipe of the random-batch tests.
Expected values come from the oracle (oracle/rfec_oracle.c).
"""
from __future__ import annotations

import zlib

import numpy as np

import pyoracle as po

# -- dispatch tags: rfec_internal.h ----------------------------------------------------------------------------
KIND = {n: i for i, n in enumerate(
    ["NONE", "ENC_ROWS", "ENC_ROWS_RT", "ENC_MATRIX", "ENC_PLAN", "DEC_ROWS", "DEC_OUT", "DEC_FLAT", "CASCADE",
     "CASCADE_DENSE", "MATRIX_DENSE", "PEEL_FLAT", "PACK_ROWS", "PACK_MATRIX", "MATRIX_PACKED"])}
SLOTS, PACKED, FAST, DENSE = 0x40, 0x80, 0x40, 0x80
TUNE_GENERIC, TUNE_PLAN_CASCADE = 1, 1 << 2


def tag(kind, arg=0):
    return KIND[kind] | arg << 8


def tag_name(t):
    return f"{[n for n, i in KIND.items() if i == (t & 0xFF)][0]}:{t >> 8:#x}"


# every value the launchers can store
ALL_TAGS = set(
    [tag("ENC_ROWS", 10), tag("ENC_ROWS", 32), tag("ENC_ROWS_RT", 4), tag("ENC_ROWS_RT", 16), tag("ENC_PLAN")] +
    [tag("ENC_MATRIX", k) for k in range(6, 17)] +
    [tag("DEC_ROWS", K | f) for K in (0, 10, 32) for f in (0, SLOTS, SLOTS | PACKED)] +
    [tag("DEC_OUT", c | f) for c in (4, 8) for f in (0, SLOTS)] +
    [tag("DEC_FLAT", 4), tag("DEC_FLAT", 8)] +
    [tag("CASCADE", 32), tag("CASCADE", 64), tag("CASCADE_DENSE", 32), tag("CASCADE_DENSE", 64)] +
    [tag("MATRIX_DENSE", k) for k in range(6, 17)] +
    [tag("PEEL_FLAT", c | d) for c in (4 | FAST, 8 | FAST, 8) for d in (0, DENSE)] +
    [tag("PACK_ROWS"), tag("PACK_MATRIX")] + [tag("MATRIX_PACKED", k) for k in range(6, 17)])
# Tags no case here reaches, each with its reason: none.
NOT_REACHED = {}


# -- plans -------------------------------------------------------------------------------------------------------
def make_plan(o, spec):
    """("rows", k, col): rows of col (a last row of one member has no line and the plan is then no row layout for
    the dispatch, so the cases keep k % col != 1); ("cols", k, row, col): the column layer alone (disjoint, not a
    row layout);
    ("full", k): the sender's plan at protect fraction 80; ("sub", k): the full 4x4 plan of 16 segments inside a
    group of k > 32 (segments 16.. on no line): lines cascade, k needs 64-bit masks, 8 lines of 4."""
    if spec[0] == "rows":
        _, k, col = spec
        return o.plan_matrix(k, (k + col - 1) // col, col, 1)
    if spec[0] == "cols":
        _, k, row, col = spec
        return o.plan_matrix(k, row, col, 2)
    if spec[0] == "full":
        return o.plan_from_fraction(spec[1], 80, 3)
    if spec[0] == "sub":
        p = o.plan_matrix(16, 4, 4, 3)
        assert p.n_lines == 8
        p.k = spec[1]
        return p
    raise ValueError(spec)


def cd_of(capacity):
    return (capacity + 15) // 16 if capacity else 1


# -- inputs ------------------------------------------------------------------------------------------------------
def make_batch(k, G, capacity, stride, rng):
    """Ragged segments: data_size in [1, capacity] (a fifth of them exactly capacity), random bytes, zeros past
    data_size up to the stride; random header fields."""
    if capacity:
        size = rng.integers(1, capacity + 1, (G, k))
        size[rng.random((G, k)) < 0.2] = capacity
    else:
        size = np.zeros((G, k), np.int64)
    data = rng.integers(0, 256, (G, k, stride), dtype=np.uint8)
    shards = np.where(np.arange(stride)[None, None, :] < size[:, :, None], data, 0).astype(np.uint8)
    hdr = np.zeros((G, k), po.HDR_DTYPE)
    hdr["seq"] = rng.integers(0, 2**32, (G, k), dtype=np.uint64)
    hdr["fid"] = rng.integers(0, 2**32, (G, k), dtype=np.uint64)
    hdr["ts"] = rng.integers(0, 2**32, (G, k), dtype=np.uint64)
    hdr["index"] = rng.integers(0, 2**16, (G, k))
    hdr["total"] = rng.integers(0, 2**16, (G, k))
    hdr["ftype"] = rng.integers(0, 256, (G, k))
    hdr["payload_type"] = rng.integers(0, 256, (G, k))
    hdr["size"] = size
    return shards, hdr


def lossy_rx(o, plan, shards, hdr, capacity, rng, n_erase, corrupt, p_lost_parity=0.2, events=1):
    """The received batch of the random-batch tests (test_gpu_parity._lossy_rx): n_erase(rng) erasures per group
    (slot poisoned with 0xA5, header zeroed), a lost parity with p_lost_parity, and `events` times with probability
    `corrupt` a header corruption that makes the exact peel reject a line (plans whose lines cross need several
    before the peel's result, not only its order, changes): fec_data_size above capacity, fec_data_size below a
    member's size, a member's data_size above fec_data_size.  Returns (rx, rh, present, parity, meta, fs, pp,
    clean [G] bool: no corruption was applied)."""
    G, k, _ = shards.shape
    parity, meta, fsize, _ = o.encode_batch(plan, shards, hdr, capacity)
    present = np.zeros((G, 2), np.uint64)
    pp = np.full(G, (1 << plan.n_lines) - 1, np.uint64)
    rx, rh, fs = shards.copy(), hdr.copy(), fsize.copy()
    clean = np.ones(G, bool)
    for g in range(G):
        m = (1 << k) - 1
        for i in rng.choice(k, int(n_erase(rng)), replace=False):
            m &= ~(1 << int(i))
            rx[g, i] = 0xA5
            rh[g, i] = np.zeros((), po.HDR_DTYPE)
        present[g, 0], present[g, 1] = m & (2**64 - 1), m >> 64
        if rng.random() < p_lost_parity:
            pp[g] &= ~np.uint64(1 << int(rng.integers(plan.n_lines)))
        for _ in range(events):
            r = rng.random() / corrupt if corrupt else 1.0
            if r < 1:
                clean[g] = False
            if r < 1 / 3:
                fs[g, rng.integers(plan.n_lines)] = capacity + 1
            elif r < 2 / 3:
                l = int(rng.integers(plan.n_lines))
                fs[g, l] = max(1, int(fs[g, l]) - 3)
            elif r < 1:
                i = int(rng.integers(k))
                if (m >> i) & 1:
                    rh[g, i]["size"] = min(capacity, int(rh[g, i]["size"]) + 5)
    return rx, rh, present, parity, meta, fs, pp, clean


def _w(a, g):
    return int(a[g, 0]) | int(a[g, 1]) << 64


def mask_peel(plan, present, pp):
    """Recovered mask of the canonical peel over the masks alone (no header checks)."""
    have, rec, progress = int(present), 0, True
    while progress:
        progress = False
        for l in range(plan.n_lines):
            if not (int(pp) >> l) & 1:
                continue
            mem = plan.members(l)
            miss = [i for i in mem if not (have >> i) & 1]
            if len(miss) == 1 and len(miss) < len(mem):
                have |= 1 << miss[0]
                rec |= 1 << miss[0]
                progress = True
    return rec


# -- the full-slot comparison ----------------------------------------------------------------------------------
def check_slot(name, where, got, exp, L, cd16, rest, zeros_past_L=True):
    """One written slot of buffer `name` against the contract of razor_fec.h ("Slot tails"): [0, L) the oracle's
    bytes; [L, 16 CD) zero where the contract says so (always the oracle's: both XOR whole chunks); [16 CD, stride)
    what the slot held before the call (`rest`: an array, or the pre-fill byte)."""
    assert np.array_equal(got[:L], exp[:L]), f"{name} {where}: bytes [0, {L}) differ from the oracle's"
    if zeros_past_L:
        assert not got[L:cd16].any(), f"{name} {where}: bytes [{L}, 16 CD = {cd16}) are not zero"
    assert np.array_equal(got[L:cd16], exp[L:cd16]), (
        f"{name} {where}: bytes [{L}, 16 CD = {cd16}) differ from the whole-chunk XOR")
    tail = got[cd16:]
    ok = np.array_equal(tail, rest[cd16:]) if isinstance(rest, np.ndarray) else bool((tail == rest).all())
    assert ok, f"{name} {where}: bytes [16 CD = {cd16}, stride = {len(got)}) were written"


def _assert_tag(engine, c):
    if engine.last_path:
        assert engine.last_path == c["tag"], (
            f"{c['id']}: took {tag_name(engine.last_path)}, the case is written for {tag_name(c['tag'])}")
    return c["tag"]


def run_encode(make_engine, o, c):
    """Returns the tags the case asserted."""
    plan = make_plan(o, c["plan"])
    k, G, cap, stride = plan.k, c["G"], c["cap"], 16 * cd_of(c["cap"]) + c["extra"]
    rng = np.random.default_rng(c["seed"])
    shards, hdr = make_batch(k, G, cap, stride, rng)
    e_p, e_m, e_f, e_s = o.encode_batch(plan, shards, hdr, cap)
    eng = make_engine(c["tuning"])
    p, m, f, s = eng.encode(plan, shards, hdr, cap)
    t = _assert_tag(eng, c)
    assert np.array_equal(s, e_s) and not s.any(), "status"
    assert np.array_equal(f, e_f), "fec_size"
    assert np.array_equal(m, e_m), "meta"
    cd16 = 16 * cd_of(cap)
    for g in range(G):
        for l in range(plan.n_lines):
            check_slot("parity", f"group {g} line {l}", p[g, l], e_p[g, l], int(e_f[g, l]), cd16, 0x5A)
    return [t]


def build_rx(o, c):
    """The received batch of a recover case and the oracle's in-place result, with the conditions that keep the
    case honest asserted on the latter."""
    plan = make_plan(o, c["plan"])
    k, G, cap, stride, E = plan.k, c["G"], c["cap"], 16 * cd_of(c["cap"]) + c["extra"], c["E"]
    rng = np.random.default_rng(c["seed"])
    shards, hdr = make_batch(k, G, cap, stride, rng)
    covered = sorted({i for l in range(plan.n_lines) for i in plan.members(l)})
    if G <= 2:  # one constructed erasure per group, nothing else: it must be recovered
        corrupt = 0.0
        rx, rh, present, parity, meta, fs, pp, clean = lossy_rx(o, plan, shards, hdr, cap, np.random.default_rng(0),
                                                                 lambda r: 0, 0.0, p_lost_parity=0.0)
        for g in range(G):
            i = covered[(3 * g + 1) % len(covered)]
            rx[g, i], rh[g, i] = 0xA5, np.zeros((), po.HDR_DTYPE)
            present[g, i >> 6] &= ~np.uint64(1 << (i & 63))
    else:
        corrupt = c["corrupt"]
        hi = c.get("max_erase", 4)
        rx, rh, present, parity, meta, fs, pp, clean = lossy_rx(o, plan, shards, hdr, cap, rng,
                                                                 lambda r: r.integers(1, hi + 1), corrupt,
                                                                 events=c.get("events", 1))
    e_s, e_h, e_rec = o.recover_batch(plan, rx, rh, present, parity, meta, fs, pp, cap)
    # the conditions that keep the case honest, on the oracle's output
    n_rec_groups = sum(_w(e_rec, g) != 0 for g in range(G))
    if G <= 2:
        assert n_rec_groups == G, f"{c['id']}: the constructed erasure was not recovered"
    else:
        assert 4 * n_rec_groups >= G, f"{c['id']}: only {n_rec_groups} of {G} groups recover a segment"
        if corrupt:
            differ = sum(_w(e_rec, g) != mask_peel(plan, _w(present, g), pp[g]) for g in range(G))
            assert 20 * differ >= G, f"{c['id']}: header checks change the peel in only {differ} of {G} groups"
    return plan, rx, rh, present, parity, meta, fs, pp, clean, e_s, e_h, e_rec


def run_recover(make_engine, o, c):
    """In place (E == 0), dense (E > 0) or dense through the packed records (c["packed"]).  Returns the tags the
    case asserted."""
    plan, rx, rh, present, parity, meta, fs, pp, clean, e_s, e_h, e_rec = build_rx(o, c)
    k, G, cap, E = plan.k, c["G"], c["cap"], c["E"]
    eng = make_engine(c["tuning"])
    cd16 = 16 * cd_of(cap)
    if E == 0:
        out_s, out_h, rec = eng.recover(plan, rx, rh, present, parity, meta, fs, pp, cap)
        t = _assert_tag(eng, c)
        assert np.array_equal(rec, e_rec), "recovered masks"
        for g in range(G):
            for i in range(k):
                where = f"group {g} segment {i}"
                if (_w(rec, g) >> i) & 1:
                    assert out_h[g, i] == e_h[g, i], f"hdr {where}"
                    check_slot("shards", where, out_s[g, i], e_s[g, i], int(e_h[g, i]["size"]), cd16, rx[g, i],
                               zeros_past_L=bool(clean[g]))
                elif (_w(present, g) >> i) & 1:
                    assert out_h[g, i] == rh[g, i] and np.array_equal(out_s[g, i], rx[g, i]), f"received {where}"
                else:  # erased and not recovered: unspecified up to 16 CD, untouched from there
                    assert np.array_equal(out_s[g, i, cd16:], rx[g, i, cd16:]), f"shards {where}: tail written"
        return [t]
    x_s, x_h, x_i, x_rec = o.recover_batch_out(plan, rx, rh, present, parity, meta, fs, pp, cap, E)
    pack = {"rows": "PACK_ROWS", "matrix": "PACK_MATRIX"}.get(c.get("packed"))
    extra_tags = [tag(pack)] if pack else []
    call = {"rows": "recover_packed", "matrix": "recover_packed_matrix"}.get(c.get("packed"))
    if call and hasattr(eng, call):  # (an engine without the records: the call they equal)
        o_s, o_h, o_i, rec, _ = getattr(eng, call)(plan, rx, rh, present, parity, meta, fs, pp, cap, E)
        assert eng.pack_path == tag(pack), tag_name(eng.pack_path)
    else:
        o_s, o_h, o_i, rec = eng.recover_out(plan, rx, rh, present, parity, meta, fs, pp, cap, E)
    t = _assert_tag(eng, c)
    assert np.array_equal(rec, x_rec), "recovered masks"
    assert np.array_equal(o_i, x_i), "out_index"
    if E >= k:
        assert np.array_equal(x_rec, e_rec)
    for g in range(G):
        for e in range(E):
            where = f"group {g} slot {e}"
            if x_i[g, e] == 0xFF:
                assert (o_s[g, e, cd16:] == 0x3C).all(), f"out_shards {where}: tail written"
                continue
            assert o_h[g, e] == x_h[g, e], f"out_hdr {where}"
            check_slot("out_shards", where, o_s[g, e], x_s[g, e], int(x_h[g, e]["size"]), cd16, 0x3C,
                       zeros_past_L=bool(clean[g]))
    return [t] + extra_tags


def run_case(make_engine, o, c):
    if "every" in c:  # the header blocks' period the case is written for, from the launcher's rule
        plan = make_plan(o, c["plan"])
        assert plan.n_lines == n_lines_of(c["plan"]), (c["id"], plan.n_lines)
        assert every_of_case(c) == c["every"], (c["id"], every_of_case(c))
    return run_encode(make_engine, o, c) if c["op"] == "encode" else run_recover(make_engine, o, c)


# -- the rules of the launchers, restated ----------------------------------------------------------------------
EXTRAS = (0, 16, 112)  # stride - 16 CD: none, one chunk, seven chunks (the tail region exists)
G_SWEEP = (1, 2, 63, 64, 65, 257)


def _cdiv(a, b):
    return -(-a // b)


def _clog2(m, least=0):
    return max(least, (m - 1).bit_length())


def enc_gpb(k):
    """Encode meta blocks: gpb = min(64, 4096 / (5 k)) groups per block, rounded down to a multiple of 4
    (launch_encode: kMetaDwords / (5 k), `gpb &= ~3u` from 4 up)."""
    g = max(1, min(64, 4096 // (5 * k)))
    return g & ~3 if g >= 4 else g


def peel_gpb(k, n):
    """The LDS peel: gpb = (kPeelDwords - 8) / (5 k + 6 n) groups per block, at most 64, rounded down to a
    multiple of 8 from 8 up (launch_recover)."""
    g = min(64, (8192 - 8) // (5 * k + 6 * n))
    return max(1, g & ~7 if g >= 8 else g)


def fused_gpb(n):
    """The fused decodes' header lanes: groups << ceil_log2(n_lines) lanes (at least 2 per group), 256 per block."""
    return 256 >> _clog2(n, 1)


CASCADE_GPB = 64  # the cascade checker: 4 lanes per group (kCheckLanes), 256 per block


def g_list(gpb):
    return sorted({1, 2, gpb - 1, gpb, gpb + 1, *G_SWEEP} - {0})


def g_for_blocks(lanes_per_group, blocks):
    """The smallest G whose payload lanes fill exactly `blocks` blocks of 256."""
    G = 1
    while _cdiv(G * lanes_per_group, 256) < blocks:
        G += 1
    assert _cdiv(G * lanes_per_group, 256) == blocks, (lanes_per_group, blocks)
    return G


def n_lines_of(spec):
    """Lines of make_plan(spec), for the rules below (run_case checks it against the plan itself)."""
    if spec[0] == "rows":
        return _cdiv(spec[1], spec[2])
    if spec[0] == "cols":
        return spec[3]
    if spec[0] == "sub":
        return 8
    k = spec[1]  # the sender's full plan of k = 6..16: rows of 3 (k <= 9) or 4, then columns, lines of >= 2 members
    assert spec[0] == "full"
    if not 6 <= k <= 16:  # (larger groups take the LDS peel, whose grid has no rule that counts lines here)
        return None
    col = 3 if k <= 9 else 4
    return (sum(min(col, k - r * col) >= 2 for r in range(_cdiv(k, col))) +
            sum(_cdiv(k - c, col) >= 2 for c in range(col)))


def hdr_every(kind, flags, k, col, n, G, cap, E=0):
    """`every`, the period of the header (meta, checker) blocks in the grid of one launch, by its launcher's rule:
    payload units // header units, 0 when there are fewer payload than header units (the header blocks then stay at
    the head of the grid: the `!every` branch of header_block / header_block_xcd).  The XCD-swizzled kernels count
    both in rounds of 8 blocks of 256 lanes, k_decode_out and k_decode_disjoint in blocks.  None: the grid holds no
    header blocks (k_encode keeps its meta blocks at the head; the in-place cascade and the LDS peel check in a
    launch of their own; the pack kernels have none)."""
    cd = cd_of(cap)
    blocks = lambda lanes: _cdiv(lanes, 256)
    rounds = lambda lanes: _cdiv(blocks(lanes), 8)
    R = _cdiv(k, col) if col else 0
    slots = flags & SLOTS
    if kind in ("ENC_ROWS", "ENC_ROWS_RT", "ENC_MATRIX"):
        # enc_payload_block: n_mr = ceil(meta blocks / 8) rounds, meta blocks = ceil(G / gpb); lanes per (group,
        # row or line, chunk)
        return rounds(G * (n if kind == "ENC_MATRIX" else R) * cd) // _cdiv(_cdiv(G, enc_gpb(k)), 8)
    if kind == "DEC_ROWS":
        # launch_fused_rows: header lanes G << ceil_log2(n_lines) (>= 2 a group); launch_packed_rows: G <<
        # ceil_log2(per_group); payload lanes per (group, row or slot, chunk)
        hl = G << (_clog2(E) if flags & PACKED else _clog2(n, 1))
        return rounds(G * (E if slots else R) * cd) // rounds(hl)
    if kind == "DEC_OUT":  # launch_fused_out: hdr_every(F, npay) on blocks; lanes per (group, line or slot, chunk)
        return blocks(G * (E if slots else n) * cd) // blocks(G << _clog2(n, 1))
    if kind == "DEC_FLAT":  # launch_fused_flat: lanes per (group, chunk)
        return blocks(G * cd) // blocks(G << _clog2(n, 1))
    if kind in ("MATRIX_DENSE", "CASCADE_DENSE", "MATRIX_PACKED"):
        # launch_cascade (dense), rfec_launch_recover_packed_matrix: rounds of checker blocks, 4 lanes a group
        return rounds(G * E * cd) // rounds(4 * G)
    assert kind in ("ENC_PLAN", "CASCADE", "PEEL_FLAT", "PACK_ROWS", "PACK_MATRIX"), kind
    return None


def _shape(plan):
    """(k, col, n_lines) of a plan spec, as hdr_every takes them."""
    k = plan[1]
    col = plan[2] if plan[0] == "rows" else (3 if k <= 9 else 4) if plan[0] == "full" else 0
    return k, col, n_lines_of(plan)


def every_of(t, plan, G, cap, E=0):
    kind = [n for n, i in KIND.items() if i == (t & 0xFF)][0]
    return hdr_every(kind, t >> 8, *_shape(plan), G, cap, E)


def every_of_case(c):
    return every_of(c["tag"], c["plan"], c["G"], c["cap"], c["E"])


def g_hdr_heavy(t, plan, cap, E=0):
    """The smallest G >= 3 at which the path has more header than payload units (every == 0)."""
    return next(G for G in range(3, 1025) if every_of(t, plan, G, cap, E) == 0)


R10, R32, R14, R64 = ("rows", 10, 4), ("rows", 32, 4), ("rows", 14, 3), ("rows", 64, 2)
C4, C8, W8, W10 = ("cols", 12, 3, 4), ("cols", 12, 6, 2), ("rows", 16, 8), ("rows", 20, 10)

# Paths whose grid holds header blocks but can never hold more header than payload units, so that no case reaches
# every == 0 for them: tag -> (why, a plan of the path, its smallest capacity, its per_group values).
# test_geometry.test_hdr_heavy_cases checks each claim by brute force over G on that plan.
NO_HDR_HEAVY = {
    **{tag("ENC_MATRIX", k): ("a group has >= 5 lines, so >= 5 payload lanes, and 1/64 meta block (4 lanes' worth) "
                              "at the most: payload blocks >= meta blocks at every G", ("full", k), 1, (0,))
       for k in range(6, 17)},
    **{tag("DEC_ROWS", K): ("in place it runs from 64 chunks a slot: 64 R payload lanes a group against fewer "
                            "than 2 R header lanes", p, 1009, (0,))
       for K, p in ((10, R10), (32, R32), (0, R64))},
    tag("DEC_ROWS", 10 | SLOTS): ("dense slots run from 16 chunks: >= 16 payload lanes a group against 4 header "
                                  "lanes (3 lines)", R10, 241, (1, 2, 3)),
    tag("DEC_ROWS", 32 | SLOTS): ("dense slots run from 16 chunks: >= 16 payload lanes a group against 8 header "
                                  "lanes (8 lines)", R32, 241, tuple(range(1, 9))),
    **{tag("DEC_OUT", c | f): ("it runs from 64 chunks a slot: >= 64 payload lanes a group; more header lanes need "
                               "more than 64 disjoint lines, which is more than RFEC_MAX_K = 128 segments", p, 1009,
                               tuple(range(1, n + 1)) if f else (0,))
       for c, p, n in ((4, C4, 4), (8, C8, 2)) for f in (0, SLOTS)},
}


# Seeds of the cases whose own seed (1000 + a checksum of the id) misses a share condition of build_rx on the
# oracle: the first of seed + 1000 j that meets it.
SEEDS = {'recover-cols3-cap-G21-cap1009-E4-x0': 2657,
         'recover-cols6-G21-cap1009-E3-x16': 2624,
         'recover-cols6-G21-cap1009-x0': 2803,
         'recover-cols6-nb7-G13-cap1009-x16': 2071,
         'recover-rows10x4-E-G21-cap1009-E3-x0': 2848,
         'recover-rows10x4-G21-cap256-E2-x112': 2271,
         'recover-rows10x4-G9-cap1009-x112': 3041,
         'recover-rows32x4-G21-cap1009-E9-x16': 2199,
         'recover-rows32x4-G21-cap1009-x0': 2031,
         'recover-rows64x2-hdr-heavy-G65-cap256-E1-x0': 4010,
         'recover-sub40-G70-cap100-E3-x0': 7306,
         'recover-sub40-G70-cap100-E3-x112': 5285,
         'recover-sub40-G70-cap100-x112': 2368,
         'recover-sub40-G70-cap100-x16': 6116,
         'recover-sub40-g257-G257-cap16-x112': 2254,
         'recover-sub40-hdr-heavy-G513-cap16-E1-x16': 39944}


def _cases():
    out = {}

    def add(op, name, plan, G, cap, t, tuning=0, E=0, extra=None, corrupt=0.6, **kw):
        """The id holds every field that tells two cases apart; the default stride tail and the seed come from a
        checksum of the case's own fields, not from its place in the table."""
        base = (f"{op}-{name}-G{G}-cap{cap}" + (f"-E{E}" if E else "") +
                (f"-p{kw['packed']}" if kw.get("packed") else "") + (f"-t{tuning}" if tuning else ""))
        if extra is None:
            extra = EXTRAS[zlib.crc32(base.encode()) % 3]
        cid = f"{base}-x{extra}"
        c = dict(op=op, plan=plan, G=G, cap=cap, tag=t, tuning=tuning, E=E, corrupt=corrupt, extra=extra, id=cid,
                 seed=SEEDS.get(cid, 1000 + zlib.crc32(cid.encode()) % 1000), **kw)
        if plan[0] in ("full", "sub"):
            c.setdefault("events", 3)
        assert out.setdefault(cid, c) == c, f"two different cases named {cid}"  # (two sweeps may meet in one case)

    def sweep(op, name, plan, cap, t, gpb, lanes, **kw):
        """Group counts at the edges of the path's groups-per-block rule and payload block counts of 1, 7, 8 and 9
        (rounds of 8 blocks)."""
        for G in g_list(gpb):
            add(op, name, plan, G, cap, t, **kw)
        for nb in (1, 7, 8, 9):
            add(op, f"{name}-nb{nb}", plan, g_for_blocks(lanes, nb), cap, t, **kw)

    def hdr_heavy(op, name, plan, cap, t, **kw):
        """More header than payload units, every == 0: the smallest such G at this capacity (run_case asserts the
        period from the launcher's rule).  Paths without header blocks in the grid: 257 groups of one chunk."""
        if every_of(t, plan, 257, cap, kw.get("E", 0)) is None:
            add(op, f"{name}-g257", plan, 257, cap, t, **kw)
        else:
            add(op, f"{name}-hdr-heavy", plan, g_hdr_heavy(t, plan, cap, kw.get("E", 0)), cap, t, every=0, **kw)

    # ---- encode paths: every stride tail, default and RFEC_TUNE_GENERIC ----
    enc = [("rows10x4", R10, tag("ENC_ROWS", 10)), ("rows32x4", R32, tag("ENC_ROWS", 32)),
           ("rt4-col2", ("rows", 8, 2), tag("ENC_ROWS_RT", 4)), ("rt4-col3", ("rows", 9, 3), tag("ENC_ROWS_RT", 4)),
           ("rt4-col4", ("rows", 12, 4), tag("ENC_ROWS_RT", 4)), ("rt16-col5", ("rows", 12, 5), tag("ENC_ROWS_RT", 16)),
           ("rt16-col16", ("rows", 34, 16), tag("ENC_ROWS_RT", 16)), ("plan-col17", ("rows", 36, 17), tag("ENC_PLAN")),
           ("plan-cols", C4, tag("ENC_PLAN"))]
    enc += [(f"matrix{k}", ("full", k), tag("ENC_MATRIX", k)) for k in range(6, 17)]
    for name, plan, t in enc:
        for x in EXTRAS:
            add("encode", name, plan, 37, 40, t, extra=x)
        add("encode", name, plan, 37, 40, tag("ENC_PLAN"), tuning=TUNE_GENERIC)
    # group counts: k = 10 (gpb 64), k = 34 in rows of 16 (gpb 24), the 4x4 matrix (gpb 48), k = 36 in rows of 17,
    # plan-driven (gpb 20)
    sweep("encode", "rows10x4", R10, 64, tag("ENC_ROWS", 10), enc_gpb(10), 3 * 4)
    sweep("encode", "rt16-col16", ("rows", 34, 16), 48, tag("ENC_ROWS_RT", 16), enc_gpb(34), 3 * 3)
    sweep("encode", "matrix16", ("full", 16), 48, tag("ENC_MATRIX", 16), enc_gpb(16), 8 * 3)
    sweep("encode", "plan-col17", ("rows", 36, 17), 48, tag("ENC_PLAN"), enc_gpb(36), 3)
    # more meta than payload rounds, one chunk a slot (the matrix encodes: NO_HDR_HEAVY; 257 groups all the same)
    for name, plan, t in (("rows10x4", R10, tag("ENC_ROWS", 10)), ("rows32x4", R32, tag("ENC_ROWS", 32)),
                          ("rt4-col4", ("rows", 12, 4), tag("ENC_ROWS_RT", 4)),
                          ("rt16-col16", ("rows", 34, 16), tag("ENC_ROWS_RT", 16)),
                          ("plan-col17", ("rows", 36, 17), tag("ENC_PLAN"))):
        hdr_heavy("encode", name, plan, 16, t)
    add("encode", "matrix16-g257", ("full", 16), 257, 16, tag("ENC_MATRIX", 16))

    # ---- recover paths ----
    # k_decode_rows<K, 4, slots>: in place from 64 chunks per slot; dense with E <= n_lines from 16 (lanes per slot)
    for name, plan, K, n in (("rows10x4", R10, 10, 3), ("rows32x4", R32, 32, 8), ("rows14x3", R14, 0, 5)):
        for x in EXTRAS:
            add("recover", name, plan, 21, 1009, tag("DEC_ROWS", K), extra=x)
            add("recover", name, plan, 21, 256, tag("DEC_ROWS", K | SLOTS), E=2, extra=x)
        add("recover", name, plan, 21, 1009, tag("DEC_ROWS", K), E=n + 1)
        add("recover", name, plan, 21, 256, tag("DEC_ROWS", K | SLOTS | PACKED), E=2, packed="rows")
        add("recover", name, plan, 21, 40, tag("DEC_ROWS", K | SLOTS | PACKED), E=1, packed="rows", extra=112)
    # k_decode_out<MAXC, slots>: disjoint plans that are no row layout of <= 4 columns, from 64 chunks
    for name, plan, mc, n in (("cols3", C4, 4, 4), ("cols6", C8, 8, 2), ("rows16x8", W8, 8, 2)):
        for x in EXTRAS:
            add("recover", name, plan, 21, 1009, tag("DEC_OUT", mc), extra=x)
        add("recover", name, plan, 21, 1009, tag("DEC_OUT", mc | SLOTS), E=n)
        add("recover", name, plan, 21, 1009, tag("DEC_OUT", mc), E=n + 1)
        # k_decode_disjoint<MAXC>: below 64 chunks
        for x in EXTRAS:
            add("recover", name, plan, 70, 100, tag("DEC_FLAT", mc), extra=x)
        add("recover", name, plan, 70, 100, tag("DEC_FLAT", mc), E=n)
    # cascades: the sender's matrix plans (32-bit masks) and 16 of 40 segments in a 4x4 matrix (64-bit masks: k > 32,
    # 8 lines of 4).  In place: k_cascade_check + k_decode_cascade; dense: the kernel compiled for the shape, the
    # plan-driven one under RFEC_TUNE_PLAN_CASCADE and for the 40-segment group; the packed matrix records
    for x in EXTRAS:
        add("recover", "full10", ("full", 10), 70, 100, tag("CASCADE", 32), extra=x, max_erase=5)
        add("recover", "sub40", ("sub", 40), 70, 100, tag("CASCADE", 64), extra=x, max_erase=5)
        add("recover", "full10", ("full", 10), 70, 100, tag("CASCADE_DENSE", 32), E=3, extra=x, max_erase=5,
            tuning=TUNE_PLAN_CASCADE)
        add("recover", "sub40", ("sub", 40), 70, 100, tag("CASCADE_DENSE", 64), E=3, extra=x, max_erase=5)
    for k in range(6, 17):
        add("recover", f"full{k}", ("full", k), 70, 100, tag("MATRIX_DENSE", k), E=2, max_erase=5)
        add("recover", f"full{k}", ("full", k), 70, 100, tag("CASCADE", 32), max_erase=5)
        add("recover", f"full{k}", ("full", k), 70, 100, tag("MATRIX_PACKED", k), E=2, max_erase=5, packed="matrix")
    # the LDS peel + replay: RFEC_TUNE_GENERIC on every plan shape, and by default plans beyond the cascade decode
    for name, plan, arg in (("rows10x4", R10, 4 | FAST), ("full10", ("full", 10), 4 | FAST), ("rows16x8", W8, 8 | FAST),
                            ("rows20x10", W10, 8)):
        for x in EXTRAS:
            add("recover", name, plan, 70, 100, tag("PEEL_FLAT", arg), tuning=TUNE_GENERIC, extra=x)
            add("recover", name, plan, 70, 100, tag("PEEL_FLAT", arg | DENSE), tuning=TUNE_GENERIC, E=2, extra=x)
    add("recover", "rows20x10", W10, 70, 100, tag("PEEL_FLAT", 8))
    add("recover", "rows20x10", W10, 70, 100, tag("PEEL_FLAT", 8 | DENSE), E=2)
    add("recover", "full36", ("full", 36), 70, 100, tag("PEEL_FLAT", 8 | FAST), max_erase=8)
    add("recover", "full36", ("full", 36), 70, 100, tag("PEEL_FLAT", 8 | FAST | DENSE), E=4, max_erase=8)
    add("recover", "rows10x4", R10, 70, 1009, tag("PEEL_FLAT", 4 | FAST), tuning=TUNE_GENERIC)

    # group counts per path (rule restated in fused_gpb / CASCADE_GPB / peel_gpb), in place and dense
    sweep("recover", "rows10x4", R10, 64, tag("DEC_FLAT", 4), fused_gpb(3), 4)
    sweep("recover", "rows10x4", R10, 256, tag("DEC_ROWS", 10 | SLOTS), fused_gpb(3), 2 * 16, E=2)
    sweep("recover", "rows32x4", R32, 64, tag("DEC_FLAT", 4), fused_gpb(8), 4)
    sweep("recover", "rows32x4", R32, 256, tag("DEC_ROWS", 32 | SLOTS), fused_gpb(8), 2 * 16, E=2)
    sweep("recover", "full10", ("full", 10), 64, tag("CASCADE", 32), CASCADE_GPB, 7 * 4, max_erase=5)
    sweep("recover", "full10", ("full", 10), 64, tag("MATRIX_DENSE", 10), CASCADE_GPB, 2 * 4, E=2, max_erase=5)
    sweep("recover", "full36", ("full", 36), 64, tag("PEEL_FLAT", 8 | FAST), peel_gpb(36, 12), 4, max_erase=8)
    sweep("recover", "full36", ("full", 36), 64, tag("PEEL_FLAT", 8 | FAST | DENSE), peel_gpb(36, 12), 4, E=4,
          max_erase=8)
    sweep("recover", "rows10x4", R10, 64, tag("DEC_ROWS", 10 | SLOTS | PACKED), fused_gpb(2), 2 * 4, E=2,
          packed="rows")
    # in place from 64 chunks: 3 rows x 64 chunks a group; 1, 7, 8, 9 blocks and the sweep's small counts
    for G in sorted({1, 2} | {g_for_blocks(3 * 64, nb) for nb in (1, 7, 8, 9)}):
        add("recover", "rows10x4", R10, G, 1009, tag("DEC_ROWS", 10))
    # k_decode_out, its own launcher (header blocks spread by hdr_every over plain blocks): 4 lines (or 4 slots) x 64
    # chunks are one payload block a group, 2 lines of 6 half a block; header lanes 4 (2) a group
    sweep("recover", "cols3", C4, 1009, tag("DEC_OUT", 4), fused_gpb(4), 4 * 64)
    sweep("recover", "cols3", C4, 1009, tag("DEC_OUT", 4 | SLOTS), fused_gpb(4), 4 * 64, E=4)
    sweep("recover", "cols6", C8, 1009, tag("DEC_OUT", 8), fused_gpb(2), 2 * 64)
    sweep("recover", "cols6", C8, 1009, tag("DEC_OUT", 8 | SLOTS), fused_gpb(2), 2 * 64, E=2)
    # one and two groups on the paths that share a swept path's rule
    for name, plan, cap, t, kw in (
            ("cols6", C8, 100, tag("DEC_FLAT", 8), {}),
            ("rows32x4", R32, 1009, tag("DEC_ROWS", 32), {}),
            ("rows14x3", R14, 1009, tag("DEC_ROWS", 0), {}),
            ("rows14x3", R14, 256, tag("DEC_ROWS", 0 | SLOTS), dict(E=2)),
            ("rows14x3", R14, 40, tag("DEC_ROWS", 0 | SLOTS | PACKED), dict(E=2, packed="rows")),
            ("rows32x4", R32, 40, tag("DEC_ROWS", 32 | SLOTS | PACKED), dict(E=2, packed="rows")),
            ("sub40", ("sub", 40), 100, tag("CASCADE", 64), {}),
            ("sub40", ("sub", 40), 100, tag("CASCADE_DENSE", 64), dict(E=3)),
            ("full10", ("full", 10), 100, tag("CASCADE_DENSE", 32), dict(E=3, tuning=TUNE_PLAN_CASCADE)),
            ("full10", ("full", 10), 100, tag("MATRIX_PACKED", 10), dict(E=2, packed="matrix")),
            ("rows20x10", W10, 100, tag("PEEL_FLAT", 8), {}),
            ("rows20x10", W10, 100, tag("PEEL_FLAT", 8 | DENSE), dict(E=2)),
            ("rows10x4", R10, 100, tag("PEEL_FLAT", 4 | FAST), dict(tuning=TUNE_GENERIC)),
            ("rows10x4", R10, 100, tag("PEEL_FLAT", 4 | FAST | DENSE), dict(tuning=TUNE_GENERIC, E=2))):
        for G in (1, 2):
            add("recover", name, plan, G, cap, t, **kw)
    # more header than payload units (every == 0) on every path that can have them (the others: NO_HDR_HEAVY): one
    # chunk a slot; the dense row slots of k_decode_rows<0, 4, true> need 16 chunks and 32 rows of 2
    for name, plan, t, kw in (
            [("rows10x4", R10, tag("DEC_FLAT", 4), {}), ("cols3", C4, tag("DEC_FLAT", 4), {}),
             ("cols6", C8, tag("DEC_FLAT", 8), dict(E=2)),
             ("rows10x4", R10, tag("DEC_ROWS", 10 | SLOTS | PACKED), dict(E=3, packed="rows")),
             ("rows32x4", R32, tag("DEC_ROWS", 32 | SLOTS | PACKED), dict(E=3, packed="rows")),
             ("rows14x3", R14, tag("DEC_ROWS", 0 | SLOTS | PACKED), dict(E=3, packed="rows")),
             ("full10", ("full", 10), tag("CASCADE", 32), dict(max_erase=5)),
             ("full10", ("full", 10), tag("CASCADE_DENSE", 32), dict(E=1, max_erase=5, tuning=TUNE_PLAN_CASCADE)),
             ("sub40", ("sub", 40), tag("CASCADE", 64), dict(max_erase=5)),
             ("sub40", ("sub", 40), tag("CASCADE_DENSE", 64), dict(E=1, max_erase=5)),
             ("full36", ("full", 36), tag("PEEL_FLAT", 8 | FAST), dict(max_erase=8)),
             ("full36", ("full", 36), tag("PEEL_FLAT", 8 | FAST | DENSE), dict(E=4, max_erase=8)),
             ("rows20x10", W10, tag("PEEL_FLAT", 8), {})] +
            [(f"full{k}", ("full", k), tag("MATRIX_DENSE", k), dict(E=1, max_erase=5)) for k in range(6, 17)] +
            [(f"full{k}", ("full", k), tag("MATRIX_PACKED", k), dict(E=1, max_erase=5, packed="matrix"))
             for k in range(6, 17)]):
        hdr_heavy("recover", name, plan, 16, t, **kw)
    hdr_heavy("recover", "rows64x2", R64, 256, tag("DEC_ROWS", 0 | SLOTS), E=1)

    # ---- capacity thresholds: 16 CD chunks; launch_recover goes output-mapped at CD >= 64 and to dense row slots
    # at CD >= 16 (E <= n_lines); capacity 0 counts as one chunk ----
    for cap in (0, 1, 15, 16, 17, 240, 241, 256, 1008, 1009, 1024):
        cd = cd_of(cap)
        G = 70 if cd < 16 else 21
        corrupt = 0.6 if cap >= 15 else 0.0  # (the recipe's corruptions need sizes to move by 3..5 bytes)
        add("recover", "rows10x4-cap", R10, G, cap, tag("DEC_ROWS", 10) if cd >= 64 else tag("DEC_FLAT", 4), extra=0,
            corrupt=corrupt)
        add("recover", "rows10x4-cap", R10, G, cap, tag("DEC_ROWS", 10 | SLOTS) if cd >= 16 else tag("DEC_FLAT", 4),
            E=3, extra=0, corrupt=corrupt)
        add("recover", "cols3-cap", C4, G, cap, tag("DEC_OUT", 4) if cd >= 64 else tag("DEC_FLAT", 4), extra=0,
            corrupt=corrupt)
        add("recover", "cols3-cap", C4, G, cap, tag("DEC_OUT", 4 | SLOTS) if cd >= 64 else tag("DEC_FLAT", 4), E=4,
            extra=0, corrupt=corrupt)
        add("encode", "rows10x4-cap", R10, G, cap, tag("ENC_ROWS", 10), extra=0)
    # ---- per_group on both sides of the `slots` predicate (E <= n_lines), n_lines = 3, k = 10 ----
    for E in (1, 3, 4, 10):
        add("recover", "rows10x4-E", R10, 21, 256, tag("DEC_ROWS", 10 | SLOTS) if E <= 3 else tag("DEC_FLAT", 4), E=E)
        add("recover", "rows10x4-E", R10, 21, 1009, tag("DEC_ROWS", 10 | (SLOTS if E <= 3 else 0)), E=E)
    return list(out.values())


CASES = _cases()

