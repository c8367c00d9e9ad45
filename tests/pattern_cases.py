"""The exhaustive erasure-pattern sweep of the matrix-plan decoders (the sender's
row + column plans of k = 6..16, 5-8 lines), shared by the CPU and the GPU tests
of test_erasure_patterns.py.  No GPU import; everything here is numpy array
operations over the whole sweep -- there is no Python loop over groups.

One group per erasure pattern.  A pattern is (member mask, parity mask): bit i
of the member mask = segment i was received, bit l of the parity mask = the
parity of line l was received.
  k <= 10   the full product, 2^(k + lines) groups;
  k >= 11   every member mask three times: with all parities, and twice with a
            parity mask drawn uniformly from all 2^lines.
Geometry "s16": stride 16, capacity 16 (one chunk a slot); "s48" (k = 10 and 16
only): stride 48, capacity 40, three chunk columns, the last one reaching past
the capacity.  Erased payloads and header records are 0xA5 bytes.

model(): the canonical schedule over the masks (packed_matrix_cases.
mask_schedule, vectorised over groups).  Variant "clean": nothing tampered, the
expected result is the model's mask and the original group.  Variant
"tampered": one seeded header corruption per group, the expected result is the
oracle's (oracle/rfec_oracle.c).

An engine is parity_cases.py's (recover, recover_out); the packed records and
the indexed decode come in through callables of the same shape as recover_out.
"""
from __future__ import annotations

import functools

import numpy as np

import packed_matrix_cases as pm
import pyoracle as po

KS = tuple(range(6, 17))
GEOMS = {"s16": (16, 16), "s48": (40, 48)}  # name -> (capacity, stride)
S48_KS = (10, 16)
VARIANTS = ("clean", "tampered")


def PER_GROUP(k):
    """per_group values of the dense decodes: both sides of the checker's 4 lanes per group, and every slot."""
    return (1, 3, 4, 5, k)


N_LINES = {6: 5, 7: 5, 8: 6, 9: 6, 10: 7, 11: 7, 12: 7, 13: 7, 14: 8, 15: 8, 16: 8}
PP_SEED, TAMPER_SEED, SAMPLE_SEED = 7100, 4200, 99

_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.int64)


def popcount(a):
    """Bits set in each element of an int64 array of values below 2^32."""
    return _POP16[a & 0xFFFF] + _POP16[(a >> 16) & 0xFFFF]


def bits_of(mask, k):
    """[G][k] bool from a [G] integer mask array (or the first word of a [G][2] one)."""
    m = np.asarray(mask)
    if m.ndim == 2:
        m = m[:, 0]
    return ((m.astype(np.int64)[:, None] >> np.arange(k, dtype=np.int64)[None, :]) & 1).astype(bool)


def full_plan(o, k):
    plan = o.plan_from_fraction(k, 80, 3)
    col, rows = pm.shape_of(k)
    assert (plan.k, plan.col, plan.n_lines) == (k, col, N_LINES[k]), (k, plan.col, plan.n_lines)
    # rows of col consecutive segments (a last row of one member has no line), then the col columns
    n_rows = sum(min(col, k - r * col) >= 2 for r in range(rows))
    assert plan.n_lines == n_rows + col, (k, plan.n_lines, n_rows, col)
    return plan


def line_masks(plan):
    return [sum(1 << i for i in plan.members(l)) for l in range(plan.n_lines)]


def pattern_masks(k, n):
    """(member masks, parity masks) of the sweep, int64 [G] each."""
    if k <= 10:
        g = np.arange(1 << (k + n), dtype=np.int64)
        return g & ((1 << k) - 1), g >> k
    rng = np.random.default_rng(PP_SEED + k)
    mm = np.tile(np.arange(1 << k, dtype=np.int64), 3)
    ppm = np.concatenate([np.full(1 << k, (1 << n) - 1, np.int64), rng.integers(0, 1 << n, 2 << k, dtype=np.int64)])
    return mm, ppm


def model(plan, mm, ppm, E):
    """The canonical schedule over the masks alone, every group at once: lines in plan order, repeated to a
    fixpoint; a line fires with its parity received, exactly one member missing and one present; only erased
    segments of rank < E are targets (E = k: the in-place peel).  Returns (recovered mask, steps, cascade: some
    step reads a segment recovered by an earlier one), [G] each."""
    k = plan.k
    have = mm.copy()
    erased = ~mm & ((1 << k) - 1)
    steps = np.zeros(len(mm), np.int64)
    casc = np.zeros(len(mm), bool)
    lm = line_masks(plan)
    progress = True
    while progress:
        progress = False
        for l, m in enumerate(lm):
            x = m & ~have
            fire = (((ppm >> l) & 1) == 1) & (popcount(x) == 1) & ((m & have) != 0)
            fire &= popcount(erased & (np.maximum(x, 1) - 1)) < E
            if fire.any():
                casc |= fire & ((m & erased & ~x) != 0)
                have = np.where(fire, have | x, have)
                steps += fire
                progress = True
    return have & ~mm, steps, casc


def check_model_sample(plan, mm, ppm, E, count=300):
    """model() against packed_matrix_cases.mask_schedule itself on a seeded sample of groups."""
    rng = np.random.default_rng(SAMPLE_SEED + plan.k + E)
    pick = rng.choice(len(mm), min(count, len(mm)), replace=False)
    rec, steps, casc = model(plan, mm[pick], ppm[pick], E)
    for j, g in enumerate(pick):  # (a few hundred groups: the per-group restatement is the point here)
        s = pm.mask_schedule(plan, int(mm[g]), int(ppm[g]), E)
        assert (int(rec[j]), int(steps[j]), bool(casc[j])) == (sum(1 << t for _, t, _ in s), len(s),
                                                                any(c for _, _, c in s)), (hex(int(mm[g])), s)


class Sweep:
    """One (k, geometry, variant): the received batch of every pattern, the model's result and, lazily, the
    expected outputs.  Everything is computed once and left unchanged."""

    def __init__(self, o, k, geom, variant):
        assert variant in VARIANTS and geom in GEOMS
        self.o, self.k, self.geom, self.variant = o, k, geom, variant
        self.cap, self.stride = GEOMS[geom]
        self.cd16 = 16 * ((self.cap + 15) // 16)
        self.plan = plan = full_plan(o, k)
        self.n = n = plan.n_lines
        self.mm, self.ppm = pattern_masks(k, n)
        self.G = G = len(self.mm)
        self.shards, self.hdr = o.fill_groups(97 + k, G, k, self.cap, self.stride, ragged=True)
        self.parity, self.meta, self.fsize, status = o.encode_batch(plan, self.shards, self.hdr, self.cap)
        assert not status.any()
        self.bits = bits_of(self.mm, k)
        self.rx, self.rh = self.shards.copy(), self.hdr.copy()
        self.rx[~self.bits] = 0xA5
        self.rh.view(np.uint8).reshape(G, k, 20)[~self.bits] = 0xA5
        self.fs = self.fsize.copy()
        self.present = np.zeros((G, 2), np.uint64)
        self.present[:, 0] = self.mm.astype(np.uint64)
        self.pp = self.ppm.astype(np.uint64)
        if variant == "tampered":
            self._tamper()
        self.rec, self.steps, self.casc = model(plan, self.mm, self.ppm, k)
        self._exp = {}

    def _tamper(self):
        """One corruption per group: a line's fec_data_size above the capacity, a line's fec_data_size shortened by
        3 (floored at 1), or a present member's size raised by 5 (capped at the capacity)."""
        G, k, n, cap = self.G, self.k, self.n, self.cap
        rng = np.random.default_rng(TAMPER_SEED + k)
        kind = rng.integers(0, 3, G)
        line = rng.integers(0, n, G)
        mem = rng.integers(0, k, G)
        gi = np.arange(G)
        a, b = kind == 0, kind == 1
        c = (kind == 2) & self.bits[gi, mem]
        self.fs[gi[a], line[a]] = cap + 1
        self.fs[gi[b], line[b]] = np.maximum(1, self.fs[gi[b], line[b]].astype(np.int64) - 3)
        size = self.rh["size"]
        size[gi[c], mem[c]] = np.minimum(cap, size[gi[c], mem[c]].astype(np.int64) + 5)

    def args(self):
        return (self.plan, self.rx, self.rh, self.present, self.parity, self.meta, self.fs, self.pp, self.cap)

    # -- expected ------------------------------------------------------------------------------------------------
    def expected_in_place(self):
        """(shards, hdr, recovered): clean -- the original group and the model's mask; tampered -- the oracle's."""
        if 0 not in self._exp:
            if self.variant == "clean":
                rec = np.zeros((self.G, 2), np.uint64)
                rec[:, 0] = self.rec.astype(np.uint64)
                self._exp[0] = (self.shards, self.hdr, rec)
            else:
                self._exp[0] = self.o.recover_batch(*self.args())
        return self._exp[0]

    def expected_dense(self, E):
        """(out_shards, out_hdr, out_index, recovered) at per_group E; the slots whose out_index is 0xFF hold
        nothing to compare."""
        if E not in self._exp:
            if self.variant == "clean":
                rec = model(self.plan, self.mm, self.ppm, E)[0]
                self._exp[E] = dense_of(self, rec, self.shards, self.hdr, E)
            else:
                self._exp[E] = self.o.recover_batch_out(*self.args(), E)
        return self._exp[E]

    def describe(self, groups, limit=4):
        """The first few of `groups` with their member and parity masks in hex and their step count."""
        groups = np.asarray(groups).reshape(-1)
        txt = ", ".join(f"group {int(g)} (members {int(self.mm[g]):#x}, parities {int(self.ppm[g]):#x}, "
                        f"{int(self.steps[g])} steps)" for g in groups[:limit])
        return f"{len(groups)} groups, the first: {txt}"

    def name(self):
        return f"k={self.k} {self.geom} {self.variant}"


def dense_of(sw, rec, src_s, src_h, E):
    """The dense outputs at per_group E of a recovered mask [G] over whole groups src_s / src_h: the e-th erased
    segment (index order, e < E) in slot e where it was recovered, 0xFF otherwise."""
    G, k = sw.G, sw.k
    eb = ~sw.bits
    order = np.argsort(sw.bits, axis=1, kind="stable")[:, :E]  # erased segments first, each kind in index order
    valid = np.arange(E)[None, :] < eb.sum(1)[:, None]
    gi = np.arange(G)[:, None]
    sel = valid & bits_of(rec, k)[gi, order]
    o_i = np.where(sel, order, 0xFF).astype(np.uint8)
    o_s = np.zeros((G, E, sw.stride), np.uint8)
    o_h = np.zeros((G, E), po.HDR_DTYPE)
    o_s[sel] = src_s[gi, order][sel]
    o_h[sel] = src_h[gi, order][sel]
    r2 = np.zeros((G, 2), np.uint64)
    r2[:, 0] = rec.astype(np.uint64)
    return o_s, o_h, o_i, r2


@functools.lru_cache(maxsize=2)
def _sweep(o, k, geom, variant):
    return Sweep(o, k, geom, variant)


def sweep(o, k, geom="s16", variant="clean"):
    return _sweep(o, k, geom, variant)


# -- the checks ----------------------------------------------------------------------------------------------------------
def _rows_differ(a, b):
    """[N] bool: row i of a differs from row i of b (any trailing shape, any dtype)."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return (a != b).any(1)


def _fail(sw, what, bad_groups):
    raise AssertionError(f"{sw.name()}: {what}: {sw.describe(np.unique(bad_groups))}")


def check_masks(sw, rec, e_rec, what):
    d = (rec != e_rec).any(1)
    if d.any():
        _fail(sw, f"{what}: recovered masks differ", np.nonzero(d)[0])


def check_in_place(sw, got, what="in place"):
    """rfec_recover_batch's outputs against the expected ones: masks; of every recovered segment the header
    record and the whole slot ("Slot tails" of razor_fec.h: [0, 16 CD) the expected bytes, [16 CD, stride) what
    the slot held); every received segment and its header as received; of an erased segment left unrecovered
    the tail past 16 CD untouched."""
    out_s, out_h, rec = got
    e_s, e_h, e_rec = sw.expected_in_place()
    check_masks(sw, rec, e_rec, what)
    w = sw.cd16
    rb = bits_of(e_rec, sw.k)
    g_, i_ = np.nonzero(rb)
    d = _rows_differ(out_h[g_, i_], e_h[g_, i_])
    if d.any():
        _fail(sw, f"{what}: recovered header records differ", g_[d])
    d = _rows_differ(out_s[g_, i_][:, :w], e_s[g_, i_][:, :w])
    if d.any():
        _fail(sw, f"{what}: recovered slots differ over [0, 16 CD = {w})", g_[d])
    # bytes [16 CD, stride) of every slot, and the whole slot and header of every received segment
    d = (out_s[:, :, w:] != sw.rx[:, :, w:]).any(2)
    if d.any():
        _fail(sw, f"{what}: bytes [16 CD = {w}, stride = {sw.stride}) of a slot were written", np.nonzero(d)[0])
    keep = sw.bits
    d = (out_s != sw.rx).any(2) & keep
    d |= _rows_differ(out_h.reshape(-1), sw.rh.reshape(-1)).reshape(sw.G, sw.k) & keep
    if d.any():
        _fail(sw, f"{what}: a received segment or its header was written", np.nonzero(d)[0])


def check_dense(sw, got, E, what="dense", fill=0x3C):
    """rfec_recover_batch_out's outputs (any decode of that contract) at per_group E against the expected ones:
    masks, out_index, and of every slot whose out_index is not 0xFF the header record and bytes [0, 16 CD);
    bytes [16 CD, stride) of every out slot, filled or not, hold the pre-fill.  An unfilled slot's first 16 CD
    bytes and header record are unspecified, as the existing dense checks treat them."""
    o_s, o_h, o_i, rec = got
    e_s, e_h, e_i, e_rec = sw.expected_dense(E)
    what = f"{what} E={E}"
    check_masks(sw, rec, e_rec, what)
    d = (o_i != e_i).any(1)
    if d.any():
        _fail(sw, f"{what}: out_index differs", np.nonzero(d)[0])
    w = sw.cd16
    g_, e_ = np.nonzero(e_i != 0xFF)
    d = _rows_differ(o_h[g_, e_], e_h[g_, e_])
    if d.any():
        _fail(sw, f"{what}: recovered header records differ", g_[d])
    d = _rows_differ(o_s[g_, e_][:, :w], e_s[g_, e_][:, :w])
    if d.any():
        _fail(sw, f"{what}: out slots differ over [0, 16 CD = {w})", g_[d])
    if w < sw.stride:
        d = (o_s[:, :, w:] != fill).any((1, 2))
        if d.any():
            _fail(sw, f"{what}: bytes [16 CD = {w}, stride = {sw.stride}) of an out slot were written",
                  np.nonzero(d)[0])
    return len(g_)


def run_in_place(engine, sw):
    got = engine.recover(*sw.args())
    check_in_place(sw, got)


def run_dense(call, sw, E, what="dense", fill=0x3C):
    """call: recover_out's signature (plan, ..., capacity, per_group) -> (out_shards, out_hdr, out_index,
    recovered, ...)."""
    got = call(*sw.args(), E)[:4]
    return check_dense(sw, got, E, what, fill)


# -- censuses --------------------------------------------------------------------------------------------------------------
def clean_census(sw):
    """Schedule-length histogram of the sweep, from the model, with what the kernels need of it asserted."""
    hist = np.bincount(sw.steps)
    top = len(hist) - 1
    assert (hist > 0).all(), (sw.k, hist)  # every length from 0 to the largest occurs
    assert top <= 8, (sw.k, hist)  # CSched holds 8 steps
    if sw.k >= 7:
        assert top >= 5, (sw.k, hist)
    if 13 <= sw.k <= 16:
        assert top == 7, (sw.k, hist)
    return hist.tolist()


def tampered_census(sw):
    """From the oracle's result on the tampered sweep against the model: groups where the oracle recovers fewer
    than the mask schedule (a line was rejected), those whose schedule has a cascade, those whose schedule has more
    than 4 steps.  The oracle's recovered set is a subset of the model's."""
    e_rec = sw.expected_in_place()[2][:, 0].astype(np.int64)
    assert not (e_rec & ~sw.rec).any(), sw.name()
    rejected = popcount(e_rec) < sw.steps
    c = dict(groups=sw.G, rejected=int(rejected.sum()), cascade_rejected=int((rejected & sw.casc).sum()),
             long_rejected=int((rejected & (sw.steps > 4)).sum()))
    assert 100 * c["rejected"] >= sw.G and 100 * c["cascade_rejected"] >= sw.G, c
    if sw.k >= 8:
        assert 200 * c["long_rejected"] >= sw.G, c
    return c


# -- the indexed decode's inputs --------------------------------------------------------------------------------------------
def indexed_inputs(sw, E, seed=17):
    """indexed_cases.Inputs of the sweep for rfec_recover_indexed_out: the member and parity rows placed in one
    row pool under a seeded permutation, src_of built from it (NONE for an erased member or a lost parity)."""
    import indexed_cases as ic
    G, k, n = sw.G, sw.k, sw.n
    rows = np.concatenate([sw.rx.reshape(G * k, sw.stride), sw.parity.reshape(G * n, sw.stride)])
    pos = np.random.default_rng(seed + k).permutation(len(rows))
    pool = np.empty_like(rows)
    pool[pos] = rows
    src = np.concatenate([pos[:G * k].reshape(G, k), pos[G * k:].reshape(G, n)], axis=1)
    filled = np.concatenate([sw.bits, bits_of(sw.ppm, n)], axis=1)
    x = ic.Inputs()
    x.case = (f"pattern-k{k}-{sw.variant}", sw.geom, G, E, False)
    x.plan, x.G, x.k, x.nl, x.E = sw.plan, G, k, n, E
    x.capacity, x.stride = sw.cap, sw.stride
    x.rows, x.n_rows = pool, len(pool)
    x.src_of = np.where(filled, src, ic.NONE).astype(np.uint32).reshape(-1)
    x.hdr, x.present, x.meta, x.fec_size, x.parity_present = sw.rh, sw.present, sw.meta, sw.fs, sw.pp
    return x


# -- engines that are wrong on purpose (the checks must catch each) -------------------------------------------------------
WRONG = ("drops_long", "mask_peel", "swapped_slots", "flipped_byte", "flipped_header", "wrong_index")


class WrongEngine:
    """The oracle engine `base` bent one way on sweep `sw`:
      drops_long     drops the recoveries of every group whose schedule exceeds 4 steps;
      mask_peel      ignores rejected lines: decodes with the headers and sizes as sent;
      swapped_slots  swaps the payloads of two filled out slots of one group (E >= 2);
      flipped_byte   flips one payload byte of a recovered segment of one group of the longest schedule;
      flipped_header flips one bit of the header record of a recovered segment of one group;
      wrong_index    names another segment in one filled out_index entry."""

    def __init__(self, base, sw, kind):
        assert kind in WRONG
        self.base, self.sw, self.kind = base, sw, kind

    def _args(self, a):
        if self.kind != "mask_peel":
            return a
        sw = self.sw
        rh = sw.hdr.copy()
        rh.view(np.uint8).reshape(sw.G, sw.k, 20)[~sw.bits] = 0xA5
        return (a[0], a[1], rh, a[3], a[4], a[5], sw.fsize) + tuple(a[7:])

    def recover(self, *a):
        s, h, rec = (x.copy() for x in self.base.recover(*self._args(a)))
        sw = self.sw
        if self.kind == "drops_long":
            rec[sw.steps > 4] = 0
        if self.kind == "flipped_byte":
            g = int(np.nonzero((sw.steps == sw.steps.max()) & (rec[:, 0] != 0))[0][0])
            i = int(rec[g, 0]).bit_length() - 1
            s[g, i, 0] ^= 0x10
        if self.kind == "flipped_header":
            g = int(np.nonzero(rec[:, 0] != 0)[0][0])
            h["ts"][g, int(rec[g, 0]).bit_length() - 1] ^= 1 << 20
        return s, h, rec

    def recover_out(self, *a):
        s, h, ix, rec = (x.copy() for x in self.base.recover_out(*self._args(a)))
        sw = self.sw
        if self.kind == "drops_long":
            rec[sw.steps > 4] = 0
            ix[sw.steps > 4] = 0xFF
        if self.kind == "swapped_slots" and ix.shape[1] >= 2:
            g = int(np.nonzero((ix[:, 0] != 0xFF) & (ix[:, 1] != 0xFF) & (s[:, 0] != s[:, 1]).any(1))[0][0])
            s[g, [0, 1]] = s[g, [1, 0]]
        if self.kind == "wrong_index":
            g = int(np.nonzero(ix[:, 0] != 0xFF)[0][0])
            ix[g, 0] ^= 1
        return s, h, ix, rec
