"""Cases, inputs, a numpy restatement of the placement rule and engines for
rfec_wire_regroup (parsed datagrams into recover's batch layout), shared by the
CPU and the GPU tests of test_wire_regroup.py.

A case is (plan, geometry, groups, fec_id0, records taken); its id holds every
field and its seed derives from the id.  Records and payload rows come from the
oracle: frame_seg_batch / frame_fec_batch(*encode_batch(...)) -> parse_batch,
then edited (shuffled, lost, duplicated, patched) as make_inputs says.

regroup_ref restates rules 1-7 of include/razor_fec.h (rfec_wire_regroup) and
"what the call writes" in numpy, in place over the ten outputs, so that what the
call must leave alone keeps what it held.  Each `wrong` switch bends one rule:
the case set must tell every bent rule from the right one.

An engine runs one call with every buffer in a guarded arena (guarded_arena.py:
canaries around all ten outputs, the inputs compared after the call, the outputs
pre-filled with FILL):
    RefRegroup   numpy memory, regroup_ref (the CPU run of the checks)
    GpuRegroup   torch memory in HBM, the product library
"""
from __future__ import annotations

import zlib

import numpy as np

import guarded_arena as ga
import pyoracle as po
import wire_encode_cases as wec

ROWS, COLS = wec.ROWS, wec.COLS
FILL = 0x5A  # what every output holds before the call
assert FILL in ga.PREFILLS

NONE = 0xFFFFFFFF
ENOTFEC, EWINDOW, ESHAPE, ENOPARITY, EBASE, EDUP = -1, -2, -3, -4, -5, -6
SEG, FEC = 0x17, 0x1C

WRONG = ("last_wins", "anchor_highest", "wrap_65536", "fec_id_0_accepted", "signed_index", "ebase_placed",
         "copy_stride", "mask_hi_dropped")


def _hand_plan(k, row, col, lines):
    p = po.rfec_plan()
    p.k, p.row, p.col, p.n_lines, p.n_row_lines = k, row, col, len(lines), len(lines)
    for i, (first, stride, count, index) in enumerate(lines):
        p.line[i].first, p.line[i].stride, p.line[i].count, p.line[i].index = first, stride, count, index
    return p


PLANS = {
    "rows10x4": lambda o: o.plan_matrix(10, 3, 4, ROWS),
    "full3x4k10": lambda o: o.plan_matrix(10, 3, 4, ROWS | COLS),
    "k2": lambda o: o.plan_matrix(2, 1, 2, ROWS),
    "k1": lambda o: _hand_plan(1, 1, 1, []),                      # no line: no group has an anchor
    "strip64": lambda o: o.plan_matrix(64, 1, 64, ROWS),          # the masks' first word, full
    "strip65": lambda o: o.plan_matrix(65, 1, 65, ROWS),          # bit 0 of the second
    "strip128": lambda o: o.plan_matrix(128, 1, 128, ROWS),       # both words full
    # index values that are not 0..n-1, and one value on two lines (the first such line takes it)
    "hand6": lambda o: _hand_plan(6, 2, 3, [(0, 1, 3, 5), (3, 1, 3, 0x81), (0, 3, 2, 2), (1, 3, 2, 5)]),
}

# (capacity, stride)
GEOMS = {"c1200": (1200, 1216), "c1000": (1000, 1008), "c15": (15, 16), "c20": (20, 48), "c0": (0, 16),
         "c32": (32, 32)}

# (plan, geometry, groups, fec_id0, records taken: None = all)
CASES = [
    ("rows10x4", "c1200", 7, 100, None),
    ("full3x4k10", "c1000", 12, 65530, None),   # the window crosses 65535 -> 1
    ("full3x4k10", "c1200", 1, 9, None),        # G = 1
    ("k2", "c15", 7, 1, None),                  # fec_id0 = 1
    ("k1", "c20", 7, 65535, None),
    ("strip64", "c20", 1, 7, None),
    ("strip65", "c15", 7, 65533, None),
    ("strip128", "c0", 1, 1, None),
    ("hand6", "c20", 7, 300, None),
    ("rows10x4", "c0", 7, 1, None),
    ("rows10x4", "c15", 7, 100, 0), ("rows10x4", "c15", 7, 100, 1), ("rows10x4", "c15", 7, 100, 63),
    ("rows10x4", "c15", 7, 100, 64), ("rows10x4", "c15", 7, 100, 65),
    ("rows10x4", "c20", 60, 65500, None),       # four blocks of records; duplicates a block or more apart
]
# about 70,000 records at stride 32, thousands of groups, every slot contended by several copies
LOOP_CASE = ("rows10x4", "c32", 3000, 64000, None)


def case_id(c):
    plan, geom, groups, fec_id0, take = c
    return f"{plan}-{geom}-G{groups}-id{fec_id0}-{'all' if take is None else 'n%d' % take}"


def cd16(capacity):
    return 16 * ((capacity + 15) // 16) if capacity else 16


def fec_id_of(fec_id0, g):
    """The sender's succession: 65535 -> 1, skipping 0 (flex_fec_sender.c:241-243)."""
    return (fec_id0 - 1 + g) % 65535 + 1


class Inputs:
    pass


def sender_batch(oracle, plan, G, fec_id0, capacity, stride, rng, base=None, big=False):
    """A batch of G uniform groups as the sender emits it, framed and parsed by the oracle: the batch
    (shards, hdr, parity, meta, fsize, status) and the parse's records and rows, segments first ([G k]), then
    parities ([G n]).  Timestamps stay within 1 s."""
    k, n = plan.k, plan.n_lines
    N = G * k
    if base is None:
        base = (1000 + np.arange(G, dtype=np.uint64) * (k + 3)).astype(np.uint32)
    sizes = rng.integers(0, capacity + 1, N)
    u = rng.random(N)
    sizes[u < 0.1] = 0
    sizes[u > 0.85] = capacity
    sizes[:k] = capacity  # group 0: every parity's data_size == capacity
    if big:
        shards = np.zeros((N, stride), np.uint8)
        shards[:, :capacity] = rng.integers(0, 256, (1, capacity), dtype=np.uint8) ^ \
            ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)[:, None]
    else:
        shards = rng.integers(0, 256, (N, stride), dtype=np.uint8)
    shards[np.arange(stride)[None, :] >= sizes[:, None]] = 0
    hdr = np.zeros((G, k), po.HDR_DTYPE)
    hdr["seq"] = base[:, None] + np.arange(k, dtype=np.uint32)[None, :]  # wraps 32 bits
    hdr["fid"] = rng.integers(0, 2**32, (G, 1), dtype=np.uint64).astype(np.uint32)
    hdr["ts"] = rng.integers(0, 1000, (G, 1))
    hdr["index"] = np.arange(k)[None, :]
    hdr["total"] = k
    hdr["ftype"] = rng.integers(0, 2, (G, k))  # one bit on the wire (sim_proto.inl:83-125)
    hdr["payload_type"] = rng.integers(0, 256, (G, k))
    hdr["size"] = sizes.reshape(G, k)
    fid = np.array([fec_id_of(fec_id0, g) for g in range(G)], np.uint16)
    ss = np.zeros((G, k), po.SEG_STAMP)
    ss["uid"], ss["fec_id"], ss["send_ts"] = 0x01020304, fid[:, None], rng.integers(0, 1000, (G, k))
    ss["transport_seq"], ss["remb"] = rng.integers(0, 2**16, (G, k)), rng.integers(0, 3, (G, k))
    dstride = max(64, (capacity + 49 + 15) // 16 * 16)
    shards = shards.reshape(G, k, stride)
    dg, dl = oracle.frame_seg_batch(shards, hdr.reshape(-1), ss.reshape(-1), capacity, dstride)
    b = Inputs()
    b.shards, b.hdr, b.base, b.fid, b.dstride, b.sstamps, b.fstamps = shards, hdr, base, fid, dstride, ss, None
    b.parity, b.meta = np.zeros((G, 0, stride), np.uint8), np.zeros((G, 0), po.HDR_DTYPE)
    b.fsize, b.status = np.zeros((G, 0), np.uint16), np.zeros((G, 0), np.int8)
    if n:
        b.parity, b.meta, b.fsize, b.status = oracle.encode_batch(plan, shards, hdr, capacity)
        fs = np.zeros((G, n), po.FEC_STAMP)
        fs["uid"], fs["base_id"], fs["fec_id"] = 0x01020304, base[:, None], fid[:, None]
        fs["send_ts"], fs["count"], fs["row"], fs["col"] = rng.integers(0, 1000, (G, n)), k, plan.row, plan.col
        fs["index"] = np.array([plan.line[l].index for l in range(n)], np.uint8)[None, :]
        fs["transport_seq"] = rng.integers(0, 2**16, (G, n))
        b.fstamps = fs
        fd, fl = oracle.frame_fec_batch(b.parity, b.meta, b.fsize, b.status, fs.reshape(-1), capacity, dstride)
        dg, dl = np.concatenate([dg, fd]), np.concatenate([dl, fl])
    b.dgram, b.dlen = dg, dl
    b.recs, b.pay = oracle.parse_batch(dg, dl, stride, capacity)
    return b


def _changed(recs, pay):
    """Later copies of datagrams that differ in their bytes: header fields and payload (arrays, in place)."""
    recs["hdr"]["fid"] ^= 0x55AA
    recs["hdr"]["ftype"] ^= 1
    pay[:, :16] ^= 0xFF


def make_inputs(oracle, c):
    """The case's records and rows.  From the sender's batch, in a shuffled arrival order: about 15 % of the
    datagrams lost; about 15 % duplicated, the later copy with other bytes and far behind the first; and per
    case, where the shape allows, every record kind of the rule (see `extra` below)."""
    pname, gname, G, fec_id0, take = c
    capacity, stride = GEOMS[gname]
    plan = PLANS[pname](oracle)
    k, n = plan.k, plan.n_lines
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    loop = c == LOOP_CASE
    base = (1000 + np.arange(G, dtype=np.uint64) * (k + 3)).astype(np.uint32)
    if G > 1:
        base[1] = 0xFFFFFFFA  # member ids wrap 32 bits (k > 6)
    b = sender_batch(oracle, plan, G, fec_id0, capacity, stride, rng, base, big=loop)
    N0 = G * (k + n)
    keep = np.nonzero(rng.random(N0) > 0.15)[0]
    order = rng.permutation(keep)
    recs, pay = b.recs[order], b.pay[order]
    # duplicates: sources from the first third of the arrivals, copies inserted into the last third
    nd = int((1.0 if loop else 0.15) * len(order))
    if len(order) >= 3 and nd:
        third = max(1, len(order) // 3)
        src = rng.integers(0, len(order) if loop else third, nd)
        drec, dpay = recs[src].copy(), pay[src].copy()
        _changed(drec, dpay)
        if loop:  # heavy duplication everywhere: a global shuffle
            recs, pay = np.concatenate([recs, drec]), np.concatenate([pay, dpay])
            p = rng.permutation(len(recs))
            recs, pay = recs[p], pay[p]
        else:
            at = np.sort(rng.integers(len(order) - third, len(order) + 1, nd))
            recs, pay = np.insert(recs, at, drec), np.insert(pay, at, dpay, axis=0)
    head, tail = [], []  # records put before / after everything else: (recs [1], rows [1])

    def seg_of(g, i):
        d = g * k + i
        return b.recs[d:d + 1].copy(), b.pay[d:d + 1].copy()

    def fec_of(g, l):
        d = G * k + g * n + l
        return b.recs[d:d + 1].copy(), b.pay[d:d + 1].copy()

    if not loop:
        ga_ = G // 2  # the group the extras aim at
        if n:
            # an earlier shape-rejected parity with another base_id: must not become the anchor (one per reason)
            for field, val in (("count", k + 1), ("row", plan.row + 1), ("col", plan.col + 1), ("index", 0x7F)):
                r, p = fec_of(ga_, 0)
                r[field][0], r["base_id"][0] = val, (int(r["base_id"][0]) + 7) % 2**32
                head.append((r, p))
            # data_size = capacity + 1 cannot come from the parse: patched
            r, p = fec_of(ga_, 0)
            r["data_size"][0], r["base_id"][0] = capacity + 1, (int(r["base_id"][0]) + 7) % 2**32
            head.append((r, p))
            # a later parity with another base_id (EBASE); with two lines or more, line 0's own parity is lost, so
            # a rule that places EBASE parities fills its slot
            r, p = fec_of(ga_, 0)
            r["base_id"][0] = (int(r["base_id"][0]) + 1) % 2**32
            tail.append((r, p))
            if n >= 2:
                lost = (recs["mid"] == FEC) & (recs["fec_id"] == b.fid[ga_]) & (recs["index"] == plan.line[0].index)
                recs, pay = recs[~lost], pay[~lost]
                tail.append(fec_of(ga_, 1))  # the anchor survives (a duplicate when it was not lost)
        # segments below and above the group's range (in a group that has a group before it)
        for g in {ga_, G - 1}:
            for d in (-1, k):
                r, p = seg_of(g, 0)
                r["hdr"]["seq"][0] = (int(b.base[g]) + d) % 2**32
                tail.append((r, p))
        # fec_id 0, and ids outside the window on both sides
        for fid in (0, (fec_id0 - 2) % 65535 + 1, fec_id_of(fec_id0, G)):
            r, p = seg_of(0, 0)
            r["fec_id"][0] = fid
            tail.append((r, p))
            if n:
                r, p = fec_of(0, 0)
                r["fec_id"][0] = fid
                tail.append((r, p))
        # parse statuses other than OK, and another message id with status OK
        for status in (-1, -2, -3, 1):
            r, p = seg_of(G - 1, k - 1)
            r["status"][0] = status
            tail.append((r, p))
        r, p = seg_of(G - 1, k - 1)
        r["mid"][0] = 0x12
        tail.append((r, p))
    if head or tail:
        recs = np.concatenate([x[0] for x in head] + [recs] + [x[0] for x in tail])
        pay = np.concatenate([x[1] for x in head] + [pay] + [x[1] for x in tail])
        if take is None:  # the extras keep their side of the group's other records, but not their places
            nh = len(head)
            p = np.concatenate([rng.permutation(nh), nh + np.arange(len(recs) - nh - len(tail)),
                                len(recs) - len(tail) + rng.permutation(len(tail))])
            recs, pay = recs[p], pay[p]
    if take is not None:
        if take and take < 8:  # n = 1: a record that is placed
            first = np.nonzero((recs["mid"] == FEC) & (recs["count"] == k) & (recs["row"] == plan.row) &
                               (recs["col"] == plan.col) & (recs["index"] == plan.line[0].index) &
                               (recs["data_size"] <= capacity))[0][:1]
            recs, pay = recs[first], pay[first]
        recs, pay = recs[:take], pay[:take]
        assert len(recs) == take
    x = Inputs()
    x.case, x.plan, x.G, x.k, x.nl, x.fec_id0 = c, plan, G, k, n, fec_id0
    x.capacity, x.stride, x.n = capacity, stride, len(recs)
    x.recs, x.payload, x.batch = np.ascontiguousarray(recs), np.ascontiguousarray(pay), b
    return x


# -- the rule ---------------------------------------------------------------------------------------------------
def new_outputs(plan, G, n, stride, fill=FILL):
    k, nl = plan.k, plan.n_lines
    o = {"shards": np.zeros((G, k, stride), np.uint8), "hdr": np.zeros((G, k), po.HDR_DTYPE),
         "present": np.zeros((G, 2), np.uint64), "parity": np.zeros((G, nl, stride), np.uint8),
         "meta": np.zeros((G, nl), po.HDR_DTYPE), "fec_size": np.zeros((G, nl), np.uint16),
         "parity_present": np.zeros(G, np.uint64), "base_id": np.zeros(G, np.uint32),
         "src_of": np.zeros(G * (k + nl), np.uint32), "slot_of": np.zeros(n, np.int32)}
    for a in o.values():
        a.view(np.uint8)[...] = fill
    return o


OUTPUTS = ("shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "base_id", "src_of",
           "slot_of")


def regroup_ref(plan, G, fec_id0, recs, payload, capacity, out, wrong=()):
    """Rules 1-7 of rfec_wire_regroup (include/razor_fec.h) and what the call writes, in place over `out`
    (new_outputs' arrays, or views of an arena).  wrong: names of WRONG, each one rule bent."""
    assert set(wrong) <= set(WRONG)
    k, nl = plan.k, plan.n_lines
    slots = k + nl
    n = len(recs)
    index = [plan.line[l].index for l in range(nl)]
    status, mid = recs["status"].tolist(), recs["mid"].tolist()
    fec_id, count, row, col = recs["fec_id"].tolist(), recs["count"].tolist(), recs["row"].tolist(), recs["col"].tolist()
    idx, dsize, rbase = recs["index"].tolist(), recs["data_size"].tolist(), recs["base_id"].tolist()
    seq = recs["hdr"]["seq"].tolist()
    mod = 65536 if "wrap_65536" in wrong else 65535
    code = [0] * n      # rules 1-3: 0, or the refusal
    group = [0] * n
    line = [0] * n
    anchor = [None] * G
    for r in range(n):
        if status[r] != 0 or mid[r] not in (SEG, FEC):
            code[r] = ENOTFEC
            continue
        f = fec_id[r]
        if f == 0 and "fec_id_0_accepted" not in wrong:
            code[r] = EWINDOW
            continue
        g = f - fec_id0 if f >= fec_id0 else f + mod - fec_id0
        if g >= G:
            code[r] = EWINDOW
            continue
        group[r] = g
        if mid[r] == FEC:
            if not (count[r] == k and row[r] == plan.row and col[r] == plan.col and idx[r] in index
                    and dsize[r] <= capacity):
                code[r] = ESHAPE
                continue
            line[r] = index.index(idx[r])
            if anchor[g] is None or "anchor_highest" in wrong:
                anchor[g] = r  # ascending r: the first stays, unless bent
    base = [0 if anchor[g] is None else rbase[anchor[g]] for g in range(G)]
    src = [NONE] * (G * slots)
    slot_of = [0] * n
    for r in range(n):
        if code[r]:
            slot_of[r] = code[r]
            continue
        g = group[r]
        if mid[r] == FEC:
            if rbase[r] != base[g] and "ebase_placed" not in wrong:
                slot_of[r] = EBASE
                continue
            s = g * slots + k + line[r]
        else:
            if anchor[g] is None:
                slot_of[r] = ENOPARITY
                continue
            i = (seq[r] - base[g]) % 2**32
            if "signed_index" in wrong and i >= 2**31:
                i -= 2**32
            if i >= k or g * slots + i < 0:
                slot_of[r] = EBASE
                continue
            s = g * slots + i
        slot_of[r] = s
        if src[s] == NONE or "last_wins" in wrong:
            src[s] = r
    for r in range(n):
        if slot_of[r] >= 0 and src[slot_of[r]] != r:
            slot_of[r] = EDUP
    out["slot_of"][...] = np.array(slot_of, np.int32).reshape(out["slot_of"].shape)
    out["src_of"][...] = np.array(src, np.uint32).reshape(out["src_of"].shape)
    out["base_id"][...] = np.array(base, np.uint32).reshape(out["base_id"].shape)
    w = payload.shape[1] if "copy_stride" in wrong else cd16(capacity)
    srca = np.array(src, np.int64).reshape(G, slots)
    filled = srca != NONE
    g_, s_ = np.nonzero(filled[:, :k])
    a = srca[g_, s_]
    out["shards"][g_, s_, :w] = payload[a, :w]
    out["hdr"][g_, s_] = recs["hdr"][a]
    g_, l_ = np.nonzero(filled[:, k:])
    a = srca[g_, k + l_]
    out["parity"][g_, l_, :w] = payload[a, :w]
    out["meta"][g_, l_] = recs["hdr"][a]
    out["fec_size"][g_, l_] = recs["data_size"][a]
    bits = np.uint64(1) << (np.arange(64, dtype=np.uint64))
    m = np.zeros((G, 128), bool)
    m[:, :k] = filled[:, :k]
    out["present"][:, 0] = (m[:, :64] * bits).sum(1, dtype=np.uint64)
    out["present"][:, 1] = 0 if "mask_hi_dropped" in wrong else (m[:, 64:] * bits).sum(1, dtype=np.uint64)
    p = np.zeros((G, 64), bool)
    p[:, :nl] = filled[:, k:]
    out["parity_present"][...] = (p * bits).sum(1, dtype=np.uint64)
    return out


def ref_outputs(x, wrong=()):
    return regroup_ref(x.plan, x.G, x.fec_id0, x.recs, x.payload, x.capacity,
                       new_outputs(x.plan, x.G, x.n, x.stride), wrong)


def compare(got, exp, what):
    """All ten outputs, byte for byte (what the call leaves alone holds FILL in both)."""
    bad = []
    for name in OUTPUTS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            d = np.nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1))[0]
            bad.append(f"{name}: {len(d)} bytes differ, the first at offset {int(d[0])}")
    assert not bad, f"{what}: " + "; ".join(bad)


def conditions(x, ref):
    """What the case's records exercise, from the rule's own outputs."""
    so = ref["slot_of"]
    c = {f"code{e}": bool((so == e).any()) for e in (ENOTFEC, EWINDOW, ESHAPE, ENOPARITY, EBASE, EDUP)}
    c["placed"] = bool((so >= 0).any())
    c["empty_slot"] = bool((ref["src_of"] == NONE).any())
    c["status"] = set(x.recs["status"].tolist())
    c["fec_id_0"] = bool((x.recs["fec_id"] == 0).any())
    c["size_cap"] = bool(((x.recs["mid"] == FEC) & (x.recs["data_size"] == x.capacity) & (so >= 0)).any())
    c["size_cap1"] = bool(((x.recs["mid"] == FEC) & (x.recs["data_size"] == x.capacity + 1)).any())
    c["base_wraps"] = bool(((ref["base_id"].astype(np.uint64) + x.k) > 0xFFFFFFFF).any())
    # a beaten duplicate a block of 256 records or more behind its slot's winner, with other bytes
    dup = np.nonzero(so == EDUP)[0]
    far = False
    for d in dup[:2000]:
        same = np.nonzero((x.recs["mid"] == x.recs["mid"][d]) & (x.recs["fec_id"] == x.recs["fec_id"][d]) &
                          (x.recs["hdr"]["seq"] == x.recs["hdr"]["seq"][d]) & (x.recs["index"] == x.recs["index"][d])
                          & (so >= 0))[0]
        if len(same) and d // 256 != same[0] // 256 and x.payload[d].tobytes() != x.payload[same[0]].tobytes():
            far = True
            break
    c["dup_other_block"] = far
    return c


# -- the in-order stream of the comparison with the reference's receiver ------------------------------------------
def inorder_stream(oracle, plan, G, fec_id0, capacity, stride, seed):
    """The sender's batch as the receiver sees it over a network that loses and duplicates but does not reorder:
    group by group, the segments, then the parities; 15 % of the datagrams lost, 10 % delivered twice (the copy a
    few places later, never past the group's first parity for a segment)."""
    rng = np.random.default_rng(seed)
    b = sender_batch(oracle, plan, G, fec_id0, capacity, stride, rng)
    k, n = plan.k, plan.n_lines
    arr = []
    for g in range(G):
        for part in ([g * k + i for i in range(k)], [G * k + g * n + l for l in range(n)]):
            got = []
            for d in part:
                if rng.random() < 0.15:
                    continue
                got.append(d)
                if rng.random() < 0.10:
                    got.append(d)
            # a copy moves a few places back, within its part
            for j in range(len(got) - 1):
                if got[j] == got[j + 1] and j + 2 < len(got) and rng.random() < 0.5:
                    got[j + 1], got[j + 2] = got[j + 2], got[j + 1]
            arr += got
    arr = np.array(arr, np.int64)
    x = Inputs()
    x.plan, x.G, x.k, x.nl, x.fec_id0, x.capacity, x.stride = plan, G, k, n, fec_id0, capacity, stride
    x.recs, x.payload, x.n, x.batch = b.recs[arr].copy(), b.pay[arr].copy(), len(arr), b
    return x


# -- engines ----------------------------------------------------------------------------------------------------
_BUFS = (("shards", 16), ("hdr", 4), ("present", 8), ("parity", 16), ("meta", 4), ("fec_size", 2),
         ("parity_present", 8), ("base_id", 4), ("src_of", 4), ("slot_of", 4))


class RegroupEngine:
    """run(x) -> the ten outputs (new_outputs' names, shapes and types) of one call with every buffer in one
    guarded arena.  mutate (tests): called with the arena after the call and before its checks."""

    be = None
    mutate = None

    def run(self, x):
        shape = new_outputs(x.plan, x.G, x.n, x.stride)
        bufs = [ga.Buf("recs", x.n * 64, x.recs, "in", 16), ga.Buf("payload", x.n * x.stride, x.payload, "in", 16)]
        bufs += [ga.Buf(name, shape[name].nbytes, FILL, "out", align) for name, align in _BUFS]
        A = ga.Arena(self.be, bufs)
        self._run(x, A, shape)
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A)
        A.check(f"wire_regroup {case_id(x.case) if hasattr(x, 'case') else ''}")
        self.last_arena = A
        return {name: A.get(name, shape[name].dtype, shape[name].shape) for name in OUTPUTS}


class RefRegroup(RegroupEngine):
    def __init__(self, wrong=()):
        self.be, self.wrong = ga.NumpyBackend(), wrong

    def _run(self, x, A, shape):
        out = {name: A.view(name).view(shape[name].dtype).reshape(shape[name].shape) for name in OUTPUTS}
        recs = A.view("recs").view(po.WIRE_REC)
        payload = A.view("payload").reshape(x.n, x.stride)
        regroup_ref(x.plan, x.G, x.fec_id0, recs, payload, x.capacity, out, self.wrong)


class GpuRegroup(RegroupEngine):
    def __init__(self, lib, device="cuda:0"):
        import torch
        from gpu_engine import TorchBackend
        self.torch, self.lib = torch, lib
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)

    def _run(self, x, A, shape):
        self.lib.wire_regroup(x.plan, x.G, x.fec_id0, x.n, A.ptr("recs"), A.ptr("payload"), x.stride, x.capacity,
                              *(A.ptr(name) for name in OUTPUTS),
                              self.torch.cuda.current_stream(self.device).cuda_stream)


# -- the device-resident receive path, composed ---------------------------------------------------------------------
def composed(lib, oracle, pname, gname, G, fec_id0=65500, device="cuda:0", per_group=3):
    """rfec_wire_encode_send -> the datagrams concatenated, permuted and some lost (length 0), with torch ->
    rfec_wire_parse -> rfec_wire_regroup -> rfec_recover_batch_out, on device buffers only, against
    oracle.recover_batch_out on the sender's batch with the same losses: out_index, out_hdr, out_shards over
    [0, 16 CD), recovered, the two masks, and the surviving slots of shards and parity against the sender's.
    Returns the number of recovered segments."""
    import torch

    capacity, stride = GEOMS[gname]
    plan = PLANS[pname](oracle)
    k, n, E = plan.k, plan.n_lines, per_group
    rng = np.random.default_rng(zlib.crc32(f"composed-{pname}-{gname}-{G}".encode()))
    b = sender_batch(oracle, plan, G, fec_id0, capacity, stride, rng)
    assert n and not b.status.any()
    dev = torch.device(device)
    st = torch.cuda.current_stream(dev).cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def zeros(nbytes, fill=0):
        return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device=dev)

    ns, nf, N, ds = G * k, G * n, G * (k + n), 1280
    d_sh, d_hd, d_ss, d_fs = up(b.shards), up(b.hdr), up(b.sstamps), up(b.fstamps)
    dgram, dlen = zeros(N * ds, 0xEE), zeros(N * 2, 0x77)
    lib.wire_encode_send(plan, G, stride, capacity, d_sh.data_ptr(), d_hd.data_ptr(), d_ss.data_ptr(),
                         dgram.data_ptr(), dlen.data_ptr(), d_fs.data_ptr(), dgram.data_ptr() + ns * ds,
                         dlen.data_ptr() + ns * 2, ds, st)
    # the network: two segments of every group lost, and one parity of every second group; arrival order shuffled
    lost_seg = np.stack([rng.choice(k, 2, replace=False) for _ in range(G)])
    lost = np.zeros(N, bool)
    lost[(np.arange(G)[:, None] * k + lost_seg).reshape(-1)] = True
    lost[ns + np.arange(0, G, 2) * n + rng.integers(0, n, (G + 1) // 2)] = True
    perm = rng.permutation(N)
    t_perm = torch.from_numpy(perm).to(dev)
    dgram = dgram[:N * ds].view(N, ds)[t_perm].contiguous()
    dlen16 = dlen[:N * 2].view(torch.int16).clone()
    dlen16[torch.from_numpy(lost).to(dev)] = 0
    dlen16 = dlen16[t_perm].contiguous()
    recs, payload = zeros(N * 64, FILL), zeros(N * stride, FILL)
    lib.wire_parse(N, ds, dgram.data_ptr(), dlen16.data_ptr(), stride, capacity, recs.data_ptr(), payload.data_ptr(),
                   st)
    shape = new_outputs(plan, G, N, stride)
    o = {name: zeros(shape[name].nbytes) for name in OUTPUTS}
    lib.wire_regroup(plan, G, fec_id0, N, recs.data_ptr(), payload.data_ptr(), stride, capacity,
                     *(o[name].data_ptr() for name in OUTPUTS), st)
    rec_, osh, ohd, oix = zeros(G * 16, 0xEE), zeros(G * E * stride, 0x3C), zeros(G * E * 20, 0x3C), zeros(G * E, 0x3C)
    ws = zeros(lib.workspace_size(plan, G), 0x11)
    lib.recover_batch_out(plan, G, stride, capacity, *(o[name].data_ptr() for name in OUTPUTS[:7]), rec_.data_ptr(),
                          E, osh.data_ptr(), ohd.data_ptr(), oix.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize(dev)

    def down(t, dtype, shp):
        nb = int(np.prod(shp)) * np.dtype(dtype).itemsize
        return t[:nb].cpu().numpy().view(dtype).reshape(shp)

    got = {name: down(o[name], shape[name].dtype, shape[name].shape) for name in OUTPUTS}
    have = ~lost
    present = np.zeros((G, 2), np.uint64)
    for g, i in zip(*np.nonzero(have[:ns].reshape(G, k))):
        present[g, i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    pp = np.zeros(G, np.uint64)
    for g, l in zip(*np.nonzero(have[ns:].reshape(G, n))):
        pp[g] |= np.uint64(1) << np.uint64(l)
    e_sh, e_hd, e_ix, e_rec = oracle.recover_batch_out(plan, b.shards, b.hdr, present, b.parity, b.meta, b.fsize, pp,
                                                       capacity, E)
    w = cd16(capacity)
    assert np.array_equal(got["present"], present) and np.array_equal(got["parity_present"], pp)
    assert np.array_equal(got["base_id"], b.base)
    hs, hp = have[:ns].reshape(G, k), have[ns:].reshape(G, n)
    assert np.array_equal(got["shards"][hs][:, :w], b.shards[hs][:, :w]) and np.array_equal(got["hdr"][hs], b.hdr[hs])
    assert np.array_equal(got["parity"][hp][:, :w], b.parity[hp][:, :w])
    assert np.array_equal(got["meta"][hp], b.meta[hp]) and np.array_equal(got["fec_size"][hp], b.fsize[hp])
    g_ix, g_rec = down(oix, np.uint8, (G, E)), down(rec_, np.uint64, (G, 2))
    assert np.array_equal(g_ix, e_ix) and np.array_equal(g_rec, e_rec)
    ok = e_ix != 0xFF
    assert ok.any()
    assert np.array_equal(down(ohd, po.HDR_DTYPE, (G, E))[ok], e_hd[ok])
    assert np.array_equal(down(osh, np.uint8, (G, E, stride))[ok][:, :w], e_sh[ok][:, :w])
    return int(ok.sum())
