"""Cases, a two-word numpy model of the row rule and the engine for
rfec_recover_indexed_rows_wide_out (the one-launch indexed decode of a row
layout of any width: the sender's strip-mode plans), shared by the CPU and the
GPU tests of test_recover_indexed_rows_wide.py.

A case is an indexed_cases.Inputs (pool, slot map, tables): `build` makes one
from a seeded batch of the oracle's (fill_groups -> encode_batch), a received
mask per group and, for the tampered variant, one header corruption per group
(matrix_wide_cases.tamper's three kinds); the rows lie in the pool under a
seeded permutation.  The reference of every comparison is
indexed_cases.reference (the oracle over the gathered batch); compare, the
guarded-arena engines and the sparse pool are indexed_cases' too.

model(): the kernel's rule restated in numpy over two 64-bit mask words -- line
l of (k, col, NL) is row l, its mask arithmetic; a line fires with its parity,
exactly one member missing and one present; the header checks of
flex_fec_xor.c:88-89, 98-99 on the size fields; the target's rank below
per_group; the tables' pitch k + NL / NL; the member loads in rounds of four with
the target skipped.  Its `wrong` switches bend it one way each.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import indexed_cases as ic
import matrix_wide_cases as mw
import pyoracle as po
import regroup_cases as rc

ROWS_WIDE = 7  # tag of rfec_indexed_last_path for this entry (rfec_internal.h): ROWS_WIDE | k << 8 | col << 16
M64 = (1 << 64) - 1

# (k, col): the smallest shapes at which each piece can go wrong -- one full round of four member loads (5, 5), a
# round plus one (6, 6), two full rounds (9, 9), a strip (10, 10), rows 5, 5, 1 with NL = 2 while ceil(k / col) = 3
# (11, 5), a last row of two (12, 5), a last row of one (5, 2), the shapes rfec_recover_indexed_out decodes in one
# launch itself (10, 4) and (32, 4), the first mask word full (64, 64), bit 0 of the second (65, 65), a row across
# bits 63 / 64 (66, 33), the sender's flush size as a strip (100, 100) and at pf = 9 (100, 25), both words full with
# 127 member loads (128, 128), and 64 lines, a whole wave of header lanes per group, parity bit 63 (128, 2)
SHAPES = [(5, 5), (6, 6), (9, 9), (10, 10), (11, 5), (12, 5), (5, 2), (10, 4), (32, 4), (64, 64), (65, 65), (66, 33),
          (100, 100), (100, 25), (128, 128), (128, 2)]
VARIANTS = ("clean", "tampered")
GEOMS = dict(rc.GEOMS, s16=(16, 16))
GROUPS = 200


def n_lines(k, col):
    nr = -(-k // col)
    return nr if k - (nr - 1) * col >= 2 else nr - 1


def per_groups(k, col):
    return sorted({1, min(2, k), min(col, k), k})


def rows_plan(o, k, col):
    p = o.plan_matrix(k, -(-k // col), col, rc.ROWS)
    assert p.k == k and p.n_lines == n_lines(k, col), (k, col, p.n_lines)
    return p


def old_tag(k, col):
    """rfec_recover_indexed_out's own tag for the shape: one launch of k_decode_rows_indexed<K, 4> (rows of <= 4,
    k <= 64 and every row with a line: rfec_rows_indexed_col), else the peel and the replay for lines of <= 4 or
    <= 8 and more members."""
    if col <= 4 and k <= 64 and n_lines(k, col) == -(-k // col):
        return ic.ROWS_FUSED | (k if (k, col) in ((10, 4), (32, 4)) else 0) << 8
    return ic.PEEL_REPLAY | (4 if col <= 4 else 8) << 8


# -- the model --------------------------------------------------------------------------------------------------------
WRONG = ("pitch_rows", "second_word_dropped", "last_round_skipped", "target_row_xored", "wrong_index")


def row_words(k, col, l):
    """Row l's member mask as two 64-bit words, from (k, col, l) alone."""
    m = (((1 << col) - 1) << (l * col)) & ((1 << k) - 1)
    return m & M64, m >> 64


def model(x, wrong=()):
    """(out_shards, out_hdr, out_index, recovered) of the row rule on the case's tables and pool, FILL where the
    rule writes nothing.  wrong (names of WRONG): pitch_rows -- the tables' pitch taken as ceil(k / col) instead
    of NL; second_word_dropped -- the masks' second word read as all present; last_round_skipped -- the last
    round of four member loads of a line left out; target_row_xored -- the target's own (absent) slot XORed in;
    wrong_index -- another segment named in one filled out_index entry."""
    assert set(wrong) <= set(WRONG)
    G, k, E, stride = x.G, x.k, x.E, x.stride
    col = x.plan.line[0].count
    NL = x.nl
    assert NL == n_lines(k, col)
    pitch = -(-k // col) if "pitch_rows" in wrong else NL
    w = rc.cd16(x.capacity)
    so = x.src_of
    hdr = x.hdr.view(np.uint8).reshape(G, k, 20)
    meta = x.meta.view(np.uint8).reshape(-1, 20)
    fsz = x.fec_size.reshape(-1)
    sh = np.full((G, E, stride), ic.FILL, np.uint8)
    hd = np.full((G, E, 20), ic.FILL, np.uint8)
    ix = np.full((G, E), 0xFF, np.uint8)
    rec = np.zeros((G, 2), np.uint64)
    size = x.hdr["size"]

    def row_of(g, slot):
        a = int(so[g * (k + pitch) + slot]) if g * (k + pitch) + slot < len(so) else 0
        return x.rows[min(a, x.n_rows - 1), :w]

    for g in range(G):
        h0, h1 = int(x.present[g, 0]), int(x.present[g, 1])
        if "second_word_dropped" in wrong:
            h1 = M64
        have = h0 | h1 << 64
        erased = ~have & ((1 << k) - 1)
        ppm = int(x.parity_present[g])
        got = 0
        for l in range(NL):
            m0, m1 = row_words(k, col, l)
            x0, x1 = m0 & ~h0 & M64, m1 & ~h1 & M64
            if not (ppm >> l) & 1 or bin(x0).count("1") + bin(x1).count("1") != 1 or not (m0 & h0 | m1 & h1):
                continue
            t = x0.bit_length() - 1 if x0 else 64 + x1.bit_length() - 1
            first, count = l * col, min(col, k - l * col)
            others = [first + p + (p >= t - first) for p in range(count - 1)]
            if "last_round_skipped" in wrong and len(others) > 0:
                others = others[:4 * ((len(others) - 1) // 4)]
            if "target_row_xored" in wrong:
                others = others + [t]
            ml = min(g * pitch + l, len(fsz) - 1)
            L = int(fsz[ml])
            r = meta[ml].copy()
            for i in others:
                r ^= hdr[g, i]
            if L > x.capacity or any(int(size[g, i]) > L for i in others if i != t) or int(r.view("<u2")[9]) > L:
                continue
            e = bin(erased & ((1 << t) - 1)).count("1")
            if e >= E:
                continue
            acc = row_of(g, k + l).copy()
            for i in others:
                acc ^= row_of(g, i)
            sh[g, e, :w], hd[g, e] = acc, r
            got |= 1 << t
        rec[g] = (got & M64, got >> 64)
        q, m = 0, erased
        while m and q < E:
            i = (m & -m).bit_length() - 1
            m &= m - 1
            if (got >> i) & 1:
                ix[g, q] = i
            q += 1
    if "wrong_index" in wrong:
        g, q = (int(v[0]) for v in np.nonzero(ix != 0xFF))
        ix[g, q] ^= 1
    return sh, hd.view(po.HDR_DTYPE).reshape(G, E), ix, rec


# -- inputs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _batch(o, k, col, G, geom):
    capacity, stride = GEOMS[geom]
    plan = rows_plan(o, k, col)
    shards, hdr = o.fill_groups(733 + k + col, G, k, capacity, stride, ragged=True)
    parity, meta, fsize, status = o.encode_batch(plan, shards, hdr, capacity)
    assert not status.any()
    return plan, shards, hdr, parity, meta, fsize


def build(o, name, k, col, G, geom, E, bits, pbits, tampered=False, sparse=False):
    """The Inputs of one case: bits [G][k] / pbits [G][NL] bool = received.  The seed derives from the name."""
    capacity, stride = GEOMS[geom]
    plan, shards, hdr, parity, meta, fsize = _batch(o, k, col, G, geom)
    n = plan.n_lines
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rx, rh, fs = shards.copy(), hdr.copy(), fsize.copy()
    rx[~bits] = 0xA5
    rh.view(np.uint8).reshape(G, k, 20)[~bits] = 0xA5
    if tampered:
        mw.tamper(rng, rh, fs, bits, capacity)
    rows = np.concatenate([rx.reshape(G * k, stride), parity.reshape(G * n, stride)])
    pos = rng.permutation(len(rows))
    pool = np.empty_like(rows)
    pool[pos] = rows
    src = np.concatenate([pos[:G * k].reshape(G, k), pos[G * k:].reshape(G, n)], axis=1)
    filled = np.concatenate([bits, pbits], axis=1)
    x = ic.Inputs()
    x.case = (name, geom, G, E, sparse)
    x.plan, x.G, x.k, x.nl, x.E, x.col = plan, G, k, n, E, col
    x.capacity, x.stride = capacity, stride
    x.rows, x.n_rows = pool, len(pool)
    x.src_of = np.where(filled, src, ic.NONE).astype(np.uint32).reshape(-1)
    x.hdr, x.meta, x.fec_size = rh, meta, fs
    x.present = mw.words_of([sum(1 << int(i) for i in np.nonzero(r)[0]) for r in bits])
    x.parity_present = np.array([sum(1 << int(l) for l in np.nonzero(r)[0]) for r in pbits], np.uint64)
    if sparse:  # the same rows scattered over a larger pool: row indices above 65,535
        assert stride == 16 and x.n_rows <= 8000
        where = np.sort(rng.choice(np.arange(ic.SPARSE_ROWS - 9000, ic.SPARSE_ROWS), x.n_rows, replace=False))
        big = rng.integers(0, 256, (ic.SPARSE_ROWS, stride), dtype=np.uint8)
        big[where] = x.rows
        so = x.src_of.copy()
        so[so != ic.NONE] = where[so[so != ic.NONE]].astype(np.uint32)
        x.rows, x.n_rows, x.src_of = big, ic.SPARSE_ROWS, so
    return x


def row_loss(name, k, col, G):
    """Per (group, row) 0, 1, 1, 1 or 2 members lost (the numbers drawn evenly from that list), a parity lost with probability 0.15, the segment of a last row without a line with probability
    0.3.  The first groups are set by hand where the shape allows: group 0 loses the last member of the last line
    alone and keeps every parity, group 1 the first member of row 0 alone, group 2 the last member of row 0 and the
    first of row 1 (targets at both ends of a row; both words and a straddling row where k > 64)."""
    rng = np.random.default_rng(zlib.crc32(f"rows-loss-{name}".encode()))
    n = n_lines(k, col)
    bits, pbits = np.ones((G, k), bool), rng.random((G, n)) >= 0.15
    for g in range(G):
        for l in range(n):
            first, count = l * col, min(col, k - l * col)
            lose = (0, 1, 1, 1, 2)[int(rng.integers(0, 5))]
            bits[g, first + rng.choice(count, lose, replace=False)] = False
        if n * col < k:
            bits[g, n * col:] = rng.random(k - n * col) >= 0.3
    last = min(k, n * col) - 1
    for g, lost in enumerate(([last], [0], [col - 1] + ([col] if n > 1 else []))[:G]):
        bits[g], pbits[g] = True, True
        bits[g, lost] = False
    return bits, pbits


def shape_case(o, k, col, variant, E, G=GROUPS, geom="s16"):
    name = f"rows{k}x{col}-{variant}"
    bits, pbits = row_loss(name, k, col, G)
    return build(o, name, k, col, G, geom, E, bits, pbits, variant == "tampered")


# (k, col, geometry, groups, per_group, sparse): CD = 1 (c15), CD = 2 with a tail (c20: stride 48), CD = 75 (c1200: a
# wave straddles out slots and groups).  Header blocks hold 256 >> lg groups (lg = 1: 128 groups per block at both
# shapes), payload blocks 256 lanes: 127, 128, 129 and 257 groups are the header blocks' edges; at per_group 1 and
# CD = 1 a block of 256 payload lanes holds twice a header block's groups, so those cases have more header than payload
# blocks; 257 groups x 1 and 129 x 2 lanes cross a payload block's edge; the sparse pool has row indices above 65,535
GEOMETRY = [(k, col, *c) for k, col in ((65, 65), (11, 5)) for c in (
    ("c15", 7, 2, False), ("c20", 7, 3, False), ("c1200", 5, 2, False),
    ("c15", 127, 1, False), ("c15", 128, 2, False), ("c15", 129, 2, False), ("c15", 257, 1, False),
    ("c15", 40, 3, True))]


def geometry_case(o, c):
    k, col, geom, G, E, sparse = c
    name = f"rowsgeom{k}x{col}-{geom}-G{G}-E{E}{'-sparse' if sparse else ''}"
    bits, pbits = row_loss(name, k, col, G)
    return build(o, name, k, col, G, geom, E, bits, pbits, tampered=G >= 40, sparse=sparse)


def empty_pool_inputs(o, k, col, G=600, E=3, geom="c20"):
    """All-absent tables over an empty pool: no member, no parity, every map word NONE; no payload block."""
    capacity, stride = GEOMS[geom]
    plan = rows_plan(o, k, col)
    n = plan.n_lines
    x = ic.Inputs()
    x.case = (f"rows{k}x{col}-empty", geom, G, E, False)
    x.plan, x.G, x.k, x.nl, x.E, x.col = plan, G, k, n, E, col
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
    """What a case exercises, from the reference's outputs and the received masks alone."""
    e_sh, e_hd, e_ix, e_rec = ref
    k, col, n, G, E = x.k, x.col, x.nl, x.G, x.E
    have, ppm, rec = mw.masks_of(x.present), [int(p) for p in x.parity_present], mw.masks_of(e_rec)
    c = dict(fires=0, two_lost=0, parity_lost=0, refused=0, rank_left_out=0, fire_left_out=0, first_of_row=0,
             last_of_row=0, word1=0, word2=0, straddle=0, recovered=0)
    for g in range(G):
        erased = ~have[g] & ((1 << k) - 1)
        c["rank_left_out"] += bin(erased).count("1") > E
        for l in range(n):
            m = (((1 << col) - 1) << (l * col)) & ((1 << k) - 1)
            miss = m & erased
            nm = bin(miss).count("1")
            c["two_lost"] += nm >= 2
            c["parity_lost"] += nm == 1 and not (ppm[g] >> l) & 1
            if nm != 1 or not (ppm[g] >> l) & 1:
                continue
            t = miss.bit_length() - 1
            if bin(erased & (miss - 1)).count("1") >= E:
                c["fire_left_out"] += 1
                assert not rec[g] & miss
                continue
            if not rec[g] & miss:
                c["refused"] += 1
                continue
            c["fires"] += 1
            first, count = l * col, min(col, k - l * col)
            c["first_of_row"] += t == first
            c["last_of_row"] += t == first + count - 1
            c["word1"] += t < 64
            c["word2"] += t >= 64
            c["straddle"] += first < 64 <= first + count - 1
        c["recovered"] += bin(rec[g]).count("1")
    return c


# -- engines ----------------------------------------------------------------------------------------------------------
class GpuIndexedRowsWide(ic.GpuIndexed):
    """One rfec_recover_indexed_rows_wide_out call behind indexed_cases' arena; rows is NULL for an empty pool."""

    def _workspace_size(self, x):
        return 16  # none is passed: the arena's workspace buffer only has to stay as it was

    def _run(self, x, A):
        self.lib.recover_indexed_rows_wide_out(x.plan, x.G, x.stride, x.capacity,
                                               A.ptr("rows") if x.n_rows else None, x.n_rows, A.ptr("src_of"),
                                               A.ptr("hdr"), A.ptr("present"), A.ptr("meta"), A.ptr("fec_size"),
                                               A.ptr("parity_present"), A.ptr("recovered"), x.E,
                                               A.ptr("out_shards"), A.ptr("out_hdr"), A.ptr("out_index"),
                                               self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_path = int(self.lib.lib.rfec_indexed_last_path())
