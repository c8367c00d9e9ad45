"""Cases, a two-word model of the exact peel and the engine for
rfec_recover_indexed_matrix_wide_out (the one-launch indexed decode of the
sender's full row + column plan of any k = 6..128), shared by the CPU and the
GPU tests of test_recover_indexed_matrix_wide.py.

A case is an indexed_cases.Inputs (pool, slot map, tables): `build` makes one
from a seeded batch of the oracle's (fill_groups -> encode_batch), a received
mask per group and, for the tampered variant, one header corruption per group
(pattern_cases.Sweep._tamper's three kinds); the rows lie in the pool under a
seeded permutation, as pattern_cases.indexed_inputs has them.  The reference of
every comparison is indexed_cases.reference (the oracle over the gathered
batch); compare, the guarded-arena engines and the sparse pool are
indexed_cases' too.

peel(): the exact peel of one group over Python integers as 128-bit masks --
lines in plan order to a fixpoint, the header checks of flex_fec_xor.c:88-89,
98-99 on the size fields, a refused line left out.  census() reads off it, and
off the reference's outputs, what a case exercises.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import indexed_cases as ic
import pyoracle as po
import regroup_cases as rc

WIDE = 6  # tag of rfec_indexed_last_path for this entry (rfec_internal.h): WIDE | k << 8
CHECK_GROUPS = 256  # groups per checker block: one lane per group

# k -> (rows, col, lines) of the sender's plan, each the smallest shape that can break one thing: 17 the smallest
# wide shape (a last row of 2), 21 a last row without a line, 33 past 32 bits, 64 exactly one mask word, 65 bit 64
# alone in the second word (the planner's column count is sqrt(k) rounded up only when it is more than 0.1 above the
# integer, so k = 65 is 9 x 8 with a last row of one segment, not 8 x 9), 66 (8 x 9) a row straddling bits 63 / 64,
# 100 the sender's largest, 128 the ABI's largest (23 lines)
SHAPES = {17: (4, 5, 9), 21: (5, 5, 9), 33: (6, 6, 12), 64: (8, 8, 16), 65: (9, 8, 16), 66: (8, 9, 17),
          100: (10, 10, 20), 128: (11, 12, 23)}
RATES = (0.03, 0.15)
VARIANTS = ("clean", "tampered")
GEOMS = dict(rc.GEOMS, s16=(16, 16))


def PER_GROUP(k):
    return (1, 4, 9, 17, k)


def wide_plan(o, k, pf=80):
    return o.plan_from_fraction(k, pf, 3)


# the new plans go where indexed_cases.make_inputs looks plans up (names no other case file uses)
PLANS = ic.PLANS
for _k in (*SHAPES, 40):
    PLANS[f"wide{_k}"] = functools.partial(lambda o, k: wide_plan(o, k), k=_k)

# plans the entry refuses (each a valid plan of rfec_recover_indexed_out)
REFUSED = {
    "rows10x4": lambda o: ic.PLANS["rows10x4"](o),
    "strip65": lambda o: ic.PLANS["strip65"](o),
    "hand6": lambda o: ic.PLANS["hand6"](o),
    "k10col3": lambda o: o.plan_matrix(10, 4, 3, rc.ROWS | rc.COLS),   # a full matrix, but not in the planner's col
    "k40col6": lambda o: o.plan_matrix(40, 7, 6, rc.ROWS | rc.COLS),
    "rows_only40": lambda o: o.plan_from_fraction(40, 80, rc.ROWS),
    "cols_only40": lambda o: o.plan_from_fraction(40, 80, rc.COLS),
    "k5": lambda o: o.plan_matrix(5, 2, 3, rc.ROWS | rc.COLS),
}


def line_masks(plan):
    return [sum(1 << i for i in plan.members(l)) for l in range(plan.n_lines)]


def masks_of(words):
    """[G] Python integers from [G][2] uint64 words."""
    return [int(a) | int(b) << 64 for a, b in np.asarray(words, np.uint64).reshape(-1, 2)]


def words_of(masks):
    w = np.zeros((len(masks), 2), np.uint64)
    for g, m in enumerate(masks):
        w[g] = (m & (2**64 - 1), m >> 64)
    return w


# -- the model --------------------------------------------------------------------------------------------------------
def peel(lm, k, have, ppm, E, capacity=None, sizes=None, meta_size=None, fsize=None):
    """The canonical schedule of one group: lines in plan order, repeated to a fixpoint; a line fires with its parity
    received, exactly one member missing and one present; only erased segments of rank < E are targets.  With
    sizes / meta_size / fsize (the size fields of the members' records and of the lines' meta records, and the
    lines' fec_data_size) the header checks run at every firing and a line that fails is left out: the exact peel.
    Returns (steps [(line, target, reads a recovered member)], refused [(line, steps before it)])."""
    erased = ~have & ((1 << k) - 1)
    steps, refused, banned = [], [], 0
    sizes = None if sizes is None else [int(s) for s in sizes]
    progress = True
    while progress:
        progress = False
        for l, m in enumerate(lm):
            x = m & ~have
            if not (ppm >> l) & 1 or (banned >> l) & 1 or bin(x).count("1") != 1 or not m & have:
                continue
            t = x.bit_length() - 1
            if bin(erased & (x - 1)).count("1") >= E:
                continue
            if sizes is not None:
                L = int(fsize[l])
                others = [i for i in range(k) if (m >> i) & 1 and i != t]
                size = int(meta_size[l])
                for i in others:
                    size ^= sizes[i]
                if L > capacity or any(sizes[i] > L for i in others) or size > L:
                    banned |= 1 << l
                    refused.append((l, len(steps)))
                    continue
                sizes[t] = size
            steps.append((l, t, bool(m & erased & ~x)))
            have |= x
            progress = True
    return steps, refused


# -- inputs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _batch(o, k, G, geom):
    capacity, stride = GEOMS[geom]
    plan = wide_plan(o, k)
    shards, hdr = o.fill_groups(311 + k, G, k, capacity, stride, ragged=True)
    parity, meta, fsize, status = o.encode_batch(plan, shards, hdr, capacity)
    assert not status.any()
    return plan, shards, hdr, parity, meta, fsize


def tamper(rng, rh, fs, bits, capacity):
    """One corruption per group, in place: a line's fec_data_size above the capacity, a line's fec_data_size
    shortened by 3 (floored at 1), or a present member's size raised by 5 (capped at the capacity)."""
    G, k = bits.shape
    n = fs.shape[1]
    kind, line, mem = rng.integers(0, 3, G), rng.integers(0, n, G), rng.integers(0, k, G)
    gi = np.arange(G)
    a, b = kind == 0, kind == 1
    c = (kind == 2) & bits[gi, mem]
    fs[gi[a], line[a]] = capacity + 1
    fs[gi[b], line[b]] = np.maximum(1, fs[gi[b], line[b]].astype(np.int64) - 3)
    size = rh["size"]
    size[gi[c], mem[c]] = np.minimum(capacity, size[gi[c], mem[c]].astype(np.int64) + 5)


def build(o, name, k, G, geom, E, bits, pbits, tampered=False, sparse=False):
    """The Inputs of one case: bits [G][k] / pbits [G][n] bool = received.  The seed derives from the name."""
    capacity, stride = GEOMS[geom]
    plan, shards, hdr, parity, meta, fsize = _batch(o, k, G, geom)
    n = plan.n_lines
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rx, rh, fs = shards.copy(), hdr.copy(), fsize.copy()
    rx[~bits] = 0xA5
    rh.view(np.uint8).reshape(G, k, 20)[~bits] = 0xA5
    if tampered:
        tamper(rng, rh, fs, bits, capacity)
    rows = np.concatenate([rx.reshape(G * k, stride), parity.reshape(G * n, stride)])
    pos = rng.permutation(len(rows))
    pool = np.empty_like(rows)
    pool[pos] = rows
    src = np.concatenate([pos[:G * k].reshape(G, k), pos[G * k:].reshape(G, n)], axis=1)
    filled = np.concatenate([bits, pbits], axis=1)
    x = ic.Inputs()
    x.case = (name, geom, G, E, sparse)
    x.plan, x.G, x.k, x.nl, x.E = plan, G, k, n, E
    x.capacity, x.stride = capacity, stride
    x.rows, x.n_rows = pool, len(pool)
    x.src_of = np.where(filled, src, ic.NONE).astype(np.uint32).reshape(-1)
    x.hdr, x.meta, x.fec_size = rh, meta, fs
    x.present = words_of([sum(1 << int(i) for i in np.nonzero(r)[0]) for r in bits])
    x.parity_present = np.array([sum(1 << int(l) for l in np.nonzero(r)[0]) for r in pbits], np.uint64)
    x.sent = (shards, hdr)
    if sparse:  # the same rows scattered over a larger pool: row indices above 65,535
        assert stride == 16 and x.n_rows <= 8000
        where = np.sort(rng.choice(np.arange(ic.SPARSE_ROWS - 9000, ic.SPARSE_ROWS), x.n_rows, replace=False))
        big = rng.integers(0, 256, (ic.SPARSE_ROWS, stride), dtype=np.uint8)
        big[where] = x.rows
        so = x.src_of.copy()
        so[so != ic.NONE] = where[so[so != ic.NONE]].astype(np.uint32)
        x.rows, x.n_rows, x.src_of = big, ic.SPARSE_ROWS, so
    return x


def random_loss(name, k, n, G, rate):
    """Independent loss of members and parities at `rate`; group 0 loses its last member alone and keeps every
    parity, so every case recovers a segment."""
    rng = np.random.default_rng(zlib.crc32(f"loss-{name}".encode()))
    bits, pbits = rng.random((G, k)) >= rate, rng.random((G, n)) >= rate
    bits[0], pbits[0] = True, True
    bits[0, k - 1] = False
    return bits, pbits


WIDE_GROUPS = 200


def wide_case(o, k, rate, variant, E, G=WIDE_GROUPS, geom="s16"):
    name = f"wide{k}-r{int(rate * 100)}-{variant}"
    n = SHAPES[k][2]
    bits, pbits = random_loss(name, k, n, G, rate)
    return build(o, name, k, G, geom, E, bits, pbits, variant == "tampered")


# (k, geometry, groups, per_group, sparse): CD = 1 (c15), CD = 2 with a tail (c20: stride 48, capacity 40 at s48 in the
# sweeps, 20 here), CD = 75 (c1200: a wave straddles out slots and groups); 255, 256, 257 and 513 groups are the edges
# of the checker blocks (256 groups each); at per_group 1 and CD = 1 the checker blocks are as many as the payload
# blocks (one lane per group: never more, but for the empty pool); 257 groups x 17 x 1 lanes and 513 x 2 cross the
# payload blocks' edges mid-group; the sparse pool has row indices above 65,535
GEOMETRY = [(k, *c) for k in (17, 65) for c in (
    ("c15", 7, 3, False), ("c20", 7, 4, False), ("c1200", 5, 3, False),
    ("c15", 255, 2, False), ("c15", 256, 1, False), ("c15", 257, 17, False), ("c15", 513, 2, False),
    ("c15", 40, 3, True))]


def geometry_case(o, c, rate=0.08):
    k, geom, G, E, sparse = c
    name = f"geom{k}-{geom}-G{G}-E{E}{'-sparse' if sparse else ''}"
    bits, pbits = random_loss(name, k, SHAPES[k][2], G, rate)
    return build(o, name, k, G, geom, E, bits, pbits, tampered=G >= 40, sparse=sparse)


def staircase(k, col, r0, length, mirror):
    """(lost members, the lost parity's line as (is_row, index)) of a staircase of `length` from (r0, r0): (r, r),
    (r, r + 1), (r + 1, r + 1), ... -- or mirrored (r, r), (r + 1, r), (r + 1, r + 1), ... -- so that the only line
    that fires on the received masks is the first loss's column (its row when mirrored), and every later step reads
    the previous step's result; the far end is blocked by losing the parity of the last loss's other line."""
    cells = []
    for s in range(length):
        a, b = r0 + s // 2, r0 + (s + 1) // 2  # (a, b): (r, r), (r, r + 1), (r + 1, r + 1), ...
        cells.append((b, a) if mirror else (a, b))
    assert all(r * col + c < k and c < col for r, c in cells), (k, col, cells)
    r, c = cells[-1]
    # the last loss shares its row with the previous one when it moved along the row (c changed)
    along_row = length >= 2 and cells[-2][0] == r
    blocked = (False, c) if along_row else (True, r)
    if length == 1:
        blocked = (False, c) if not mirror else (True, r)
    return [r * col + c for r, c in cells], blocked


STAIR_LENGTHS = (2, 8, 9, 16, 17, 19)


def staircase_case(o, k=100, E=None):
    """At k = 100 (10 x 10): one group per (length, mirror); at k = 128 (11 x 12): staircases from row 4 of lengths 4,
    9 and 11, both ways, which cross bits 63 / 64 (row 5 holds segments 60..71)."""
    rows, col, n = SHAPES[k]
    specs = [(0, L, m) for L in STAIR_LENGTHS for m in (False, True)] if k == 100 else \
        [(4, L, m) for L in (4, 9, 11) for m in (False, True)]
    G = len(specs)
    plan = wide_plan(o, k)
    n_row_lines = plan.n_row_lines
    bits, pbits = np.ones((G, k), bool), np.ones((G, n), bool)
    for g, (r0, L, m) in enumerate(specs):
        lost, (is_row, idx) = staircase(k, col, r0, L, m)
        bits[g, lost] = False
        pbits[g, idx if is_row else n_row_lines + idx] = False
    x = build(o, f"stairs{k}", k, G, "c20", E or k, bits, pbits)
    x.specs = specs
    return x


def empty_pool_inputs(o, k=17, G=600, E=3, geom="c20"):
    """All-absent tables over an empty pool: no member, no parity, every map word NONE; 600 groups are three checker
    blocks and no payload block."""
    capacity, stride = GEOMS[geom]
    plan = wide_plan(o, k)
    n = plan.n_lines
    x = ic.Inputs()
    x.case = (f"wide{k}-empty", geom, G, E, False)
    x.plan, x.G, x.k, x.nl, x.E = plan, G, k, n, E
    x.capacity, x.stride = capacity, stride
    x.rows, x.n_rows = np.zeros((0, stride), np.uint8), 0
    x.src_of = np.full(G * (k + n), ic.NONE, np.uint32)
    x.hdr = np.zeros((G, k), po.HDR_DTYPE)
    x.hdr.view(np.uint8)[...] = 0xA5
    x.meta = np.zeros((G, n), po.HDR_DTYPE)
    x.meta.view(np.uint8)[...] = 0xA5
    x.fec_size = np.full((G, n), 7, np.uint16)
    x.present = np.zeros((G, 2), np.uint64)
    x.parity_present = np.zeros(G, np.uint64)
    return x


# -- the census -------------------------------------------------------------------------------------------------------
def census(x, ref):
    """What a case exercises: from the exact model (held to the reference's recovered masks on every group: an
    AssertionError otherwise) and from the reference's own outputs."""
    e_sh, e_hd, e_ix, e_rec = ref
    k, n, G, E = x.k, x.nl, x.G, x.E
    lm = line_masks(x.plan)
    have, ppm, rec = masks_of(x.present), [int(p) for p in x.parity_present], masks_of(e_rec)
    c = dict(row_at_once=0, col_at_once=0, cascade=0, steps_gt8=0, steps_gt16=0, refused_reschedules=0, word2=0,
             hole_between=0, recovered=0, max_steps=0)
    nr = x.plan.n_row_lines
    for g in range(G):
        steps, refused = peel(lm, k, have[g], ppm[g], E, x.capacity, x.hdr["size"][g], x.meta["size"][g],
                              x.fec_size[g])
        got = sum(1 << t for _, t, _ in steps)
        assert got == rec[g], f"{x.case[0]} group {g}: the model recovers {got:#x}, the reference {rec[g]:#x}"
        erased = ~have[g] & ((1 << k) - 1)
        for l, t, casc in steps:
            at_once = [q for q, m in enumerate(lm) if (ppm[g] >> q) & 1 and m & erased == 1 << t and m & have[g]]
            if not at_once:
                c["cascade"] += 1
            elif at_once[0] < nr:
                c["row_at_once"] += 1
            else:
                c["col_at_once"] += 1
        c["steps_gt8"] += len(steps) > 8
        c["steps_gt16"] += len(steps) > 16
        c["max_steps"] = max(c["max_steps"], len(steps))
        # a refused line with steps after it: the peel went on without the line
        c["refused_reschedules"] += any(len(steps) > before for _, before in refused)
        c["word2"] += bool((erased | rec[g]) >> 64)
        ok = np.nonzero(e_ix[g] != 0xFF)[0]
        c["hole_between"] += bool(len(ok) >= 2 and (e_ix[g, ok[0]:ok[-1]] == 0xFF).any())
        c["recovered"] += len(steps)
    return c


# -- results bent on purpose (the comparisons must catch each) ------------------------------------------------------------
WRONG = ("intermediate_left_out", "second_word_dropped", "column_before_row", "flipped_byte", "wrong_index")


def bent(o, x, ref, kind):
    """The reference's outputs bent one way:
      intermediate_left_out  one step of a cascade XORs without the member an earlier step recovered;
      second_word_dropped    the masks' second word is ignored: nothing at or above segment 64 is recovered;
      column_before_row      the peel tries the columns before the rows (the oracle on the plan's lines reordered);
      flipped_byte           one payload byte of a recovered segment flipped;
      wrong_index            another segment named in one filled out_index entry."""
    assert kind in WRONG
    sh, hd, ix, rec = (a.copy() for a in ref)
    k, E = x.k, x.E
    if kind == "intermediate_left_out":
        lm = line_masks(x.plan)
        have, ppm = masks_of(x.present), [int(p) for p in x.parity_present]
        w = rc.cd16(x.capacity)
        for g in range(x.G):
            steps, _ = peel(lm, k, have[g], ppm[g], E, x.capacity, x.hdr["size"][g], x.meta["size"][g], x.fec_size[g])
            erased = ~have[g] & ((1 << k) - 1)
            for l, t, casc in steps:
                if not casc:
                    continue
                i = (lm[l] & erased & ~(1 << t)).bit_length() - 1  # a member recovered earlier
                qt, qi = bin(erased & ((1 << t) - 1)).count("1"), bin(erased & ((1 << i) - 1)).count("1")
                if ix[g, qt] == t and ix[g, qi] == i and sh[g, qi, :w].any():
                    sh[g, qt, :w] ^= sh[g, qi, :w]
                    return sh, hd, ix, rec
        raise AssertionError("no cascade in the case")
    if kind == "second_word_dropped":
        assert rec[:, 1].any()
        rec[:, 1] = 0
        ix[(ix >= 64) & (ix != 0xFF)] = 0xFF
    if kind == "column_before_row":
        p = x.plan
        nr, n = p.n_row_lines, p.n_lines
        order = list(range(nr, n)) + list(range(nr))
        q = po.rfec_plan()
        q.k, q.row, q.col, q.n_lines, q.n_row_lines = p.k, p.row, p.col, n, n - nr
        for a, b in enumerate(order):
            q.line[a].first, q.line[a].stride, q.line[a].count, q.line[a].index = \
                p.line[b].first, p.line[b].stride, p.line[b].count, p.line[b].index
        shards, parity = ic.gather(x)
        pp = np.array([sum(((int(v) >> b) & 1) << a for a, b in enumerate(order)) for v in x.parity_present], np.uint64)
        return o.recover_batch_out(q, shards, x.hdr, x.present, parity[:, order], x.meta[:, order],
                                   x.fec_size[:, order], pp, x.capacity, E)
    if kind in ("flipped_byte", "wrong_index"):
        g, q = (int(v[0]) for v in np.nonzero(ix != 0xFF))
        if kind == "flipped_byte":
            sh[g, q, 0] ^= 0x10
        else:
            ix[g, q] ^= 1
    return sh, hd, ix, rec


# -- engines ----------------------------------------------------------------------------------------------------------
class GpuIndexedWide(ic.GpuIndexed):
    """One rfec_recover_indexed_matrix_wide_out call behind indexed_cases' arena; rows is NULL for an empty pool."""

    def _workspace_size(self, x):
        return 16  # none is passed: the arena's workspace buffer only has to stay as it was

    def _run(self, x, A):
        self.lib.recover_indexed_matrix_wide_out(x.plan, x.G, x.stride, x.capacity,
                                                 A.ptr("rows") if x.n_rows else None, x.n_rows, A.ptr("src_of"),
                                                 A.ptr("hdr"), A.ptr("present"), A.ptr("meta"), A.ptr("fec_size"),
                                                 A.ptr("parity_present"), A.ptr("recovered"), x.E,
                                                 A.ptr("out_shards"), A.ptr("out_hdr"), A.ptr("out_index"),
                                                 self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_path = int(self.lib.lib.rfec_indexed_last_path())
