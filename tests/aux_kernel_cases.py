"""Checks of the helper kernels around the codec -- the receiver's split
summary, its row gathers, its fused stage, the line jobs of large groups, and
the sender's byte-aligned gather -- shared by the host stub (CPU:
tests/host_stub/stub_hip.c, the model the CPU plane tests rest on) and the HIP
kernels (GPU).  Every comparison is bit-exact against a plain numpy
restatement of the rules in razor_amd/csrc/rfec_internal.h.

An *engine* exposes (numpy in, numpy out):
    rx_split(recs[n], T)                               -> split[n + GUARD]
    gather_rows(src[R][stride], map[rows], stride)     -> dst[rows + GUARD][stride]
    rx_stage(src, map, stride, tables[tbytes])         -> (dst[rows + GUARD][stride], tdst[tbytes + GUARD * 16])
    line_jobs(jobs, members, rows, outrows, stride)    -> outrows (same shape, the call's result)
    send_gather(blob, offsets[slots], sizes, stride)   -> dst[slots + GUARD][stride]
It fills every output with CANARY before the call (line_jobs: the check
does, its outputs carry over from level to level) and allocates GUARD rows
past the end of each; the checks assert that those rows stay CANARY.
send_gather: slot s reads blob[offsets[s] : offsets[s] + sizes[s]] from an
address whose low two bits are offsets[s] & 3; offsets[s] < 0 is a zero slot
(source address 0).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from razor_amd.fec import RFEC_WIRE_FEC, RFEC_WIRE_SEG, WIRE_REC_DTYPE

CANARY = 0xA5
GUARD = 2  # canary rows past each output
RX_MAX_THREADS = 64
NONE, SEG_TS, SEG, FEC = 0, 1, 2, 3  # RX_SPLIT_*
SPLIT_DTYPE = np.dtype([("shard", "u1"), ("kind", "u1"), ("reserved", "<u2"), ("value", "<u4")])
JOB_DTYPE = np.dtype([("out", "<i4"), ("parity", "<i4"), ("member0", "<u4"), ("n_members", "<u4")])
assert SPLIT_DTYPE.itemsize == 8 and JOB_DTYPE.itemsize == 16

_P, _U = C.c_void_p, C.c_uint32
LAUNCH_SIGS = {
    "rfec_launch_rx_split": [_P, _U, _U, _P, _P],
    "rfec_launch_gather_rows": [_P, _P, _P, _U, _U, _P],
    "rfec_launch_rx_stage": [_P, _P, _P, _U, _U, _P, _P, C.c_size_t, _P],
    "rfec_launch_line_jobs": [_P, _U, _P, _P, _P, _U, _P],
    "rfec_launch_send_gather": [_P, _P, _U, _U, _P, _P],
    "rfec_launch_wire_parse_split": [_U, _U, _P, _P, _U, _U, _P, _P, _U, _P, _U, _P],
}


def bind_launches(cdll):
    """argtypes of the launch shims (rfec_internal.h) on a loaded library."""
    for name, args in LAUNCH_SIGS.items():
        f = getattr(cdll, name)
        f.restype, f.argtypes = C.c_int, args
    return cdll


def guarded(out, n, what):
    """The first n rows of an engine's output; the rows past them must be CANARY."""
    assert out.shape[0] >= n + 1, f"{what}: the engine returned no canary row"
    assert (out[n:].view(np.uint8) == CANARY).all(), f"{what}: written past the end of the output"
    return out[:n]


# -- rx_split ---------------------------------------------------------------------------------------------------
SPLIT_T = (1, 2, 3, 7, 8, 63, RX_MAX_THREADS)
SPLIT_N = (1, 255, 256, 257, 5000)
SEND_TS_EDGES = (2**32 - 3001, 2**32 - 3000, 2**32 - 2999, 2**32 - 1, 0)


def ref_rx_split(recs, T):
    """The rule of rfec_internal.h: shard 0xFF / NONE / 0 unless the record is
    an OK SIM_SEG (shard by fec_id, else by packet id; SEG_TS with both;
    value ts) or an OK SIM_FEC (shard by fec_id; value send_ts + 3000 mod 2^32)."""
    n = len(recs)
    out = np.zeros(n, SPLIT_DTYPE)
    out["shard"] = 0xFF
    fid = recs["fec_id"].astype(np.uint64)
    seq = recs["hdr"]["seq"].astype(np.uint64)
    ok = recs["status"] == 0
    seg = ok & (recs["mid"] == RFEC_WIRE_SEG)
    fec = ok & (recs["mid"] == RFEC_WIRE_FEC)
    out["shard"][seg] = (np.where(fid != 0, fid, seq) % np.uint64(T))[seg]
    out["kind"][seg] = np.where((fid != 0) & (seq != 0), SEG_TS, SEG)[seg]
    out["value"][seg] = recs["hdr"]["ts"][seg]
    out["shard"][fec] = (fid % np.uint64(T))[fec]
    out["kind"][fec] = FEC
    out["value"][fec] = ((recs["send_ts"].astype(np.uint64) + np.uint64(3000)) % np.uint64(2**32))[fec]
    return out


def split_records(n=5000, seed=20):
    """Random bytes in all 64 of every record, then the fields the rule reads
    drawn to its edges; the first five are OK SIM_FEC at the send_ts wrap."""
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 256, (n, 64), dtype=np.uint8).view(WIRE_REC_DTYPE).reshape(n).copy()
    recs["status"] = rng.choice(np.array([0, 1, -1, -2, -3], np.int8), n, p=[0.44, 0.14, 0.14, 0.14, 0.14])
    recs["mid"] = rng.choice(np.array([RFEC_WIRE_SEG, RFEC_WIRE_FEC, 0x10, 0x33], np.uint8), n)
    recs["fec_id"][rng.random(n) < 0.3] = 0
    recs["hdr"]["seq"][rng.random(n) < 0.3] = 0
    e = len(SEND_TS_EDGES)
    recs["status"][:e] = 0
    recs["mid"][:e] = RFEC_WIRE_FEC
    recs["send_ts"][:e] = np.array(SEND_TS_EDGES, np.uint64).astype(np.uint32)
    return recs


def split_kind_counts(split):
    return [int((split["kind"] == k).sum()) for k in (NONE, SEG_TS, SEG, FEC)]


def same_split(got, want, what):
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:4]], want[bad[:4]])
    assert not got["reserved"].any(), what


def check_rx_split(engine):
    recs = split_records()
    counts = split_kind_counts(ref_rx_split(recs, 8))
    print("rx_split input: NONE / SEG_TS / SEG / FEC =", counts)
    assert min(counts) >= 100, counts  # a condition on the input: every kind is well represented
    assert (ref_rx_split(recs, 8)["value"][:5] == [2**32 - 1, 0, 1, 2999, 3000]).all()  # the wrap is in the input
    for T in SPLIT_T:
        for n in SPLIT_N:
            got = guarded(engine.rx_split(recs[:n], T), n, f"rx_split T={T} n={n}")
            same_split(got, ref_rx_split(recs[:n], T), f"rx_split T={T} n={n}")


# -- gather_rows / rx_stage -------------------------------------------------------------------------------------
GATHER_STRIDES = (16, 48, 1008, 1216)
GATHER_ROWS = (1, 5, 257, 4099)
STAGE_TABLES = (0, 16, 4096, 16 * 1000 + 16)  # the last: no multiple of a block's 256 lanes
MAP_KINDS = ("identity", "permutation", "repeated", "holes")


def ref_gather(src, map_, stride):
    dst = np.zeros((len(map_), stride), np.uint8)
    live = map_ >= 0
    dst[live] = src[map_[live]]
    return dst


def gather_map(rng, kind, rows, src_rows):
    if kind == "identity":
        return np.arange(rows, dtype=np.int32)
    if kind == "permutation":
        return rng.permutation(src_rows)[:rows].astype(np.int32)
    if kind == "repeated":  # few sources, each many times
        return rng.integers(0, max(1, src_rows // 8), rows).astype(np.int32)
    m = rng.permutation(src_rows)[:rows].astype(np.int32)  # holes: runs of -1 at the start, in the middle, at the end
    run = max(1, rows // 7)
    m[:run] = -1
    m[rows // 2:rows // 2 + run] = -1
    m[rows - run:] = -1
    return m


def gather_source(rng, rows, stride):
    src_rows = rows + 3  # (rows the map may leave unread)
    return rng.integers(0, 256, (src_rows, stride), dtype=np.uint8)


def check_gather_rows(engine):
    rng = np.random.default_rng(31)
    for stride in GATHER_STRIDES:
        for rows in GATHER_ROWS:
            src = gather_source(rng, rows, stride)
            for kind in MAP_KINDS:
                m = gather_map(rng, kind, rows, len(src))
                what = f"gather_rows stride={stride} rows={rows} map={kind}"
                got = guarded(engine.gather_rows(src, m, stride), rows, what)
                assert np.array_equal(got, ref_gather(src, m, stride)), what


def check_rx_stage(engine):
    rng = np.random.default_rng(32)
    tables = {t: rng.integers(0, 256, t, dtype=np.uint8) for t in STAGE_TABLES}

    def one(src, m, stride, t, what):
        dst, tdst = engine.rx_stage(src, m, stride, tables[t])
        assert np.array_equal(guarded(dst, len(m), what), ref_gather(src, m, stride)), what
        assert np.array_equal(guarded(tdst.reshape(-1, 16), t // 16, what + " (tables)").reshape(-1), tables[t]), what

    q = 0
    for stride in GATHER_STRIDES:
        for rows in GATHER_ROWS:
            src = gather_source(rng, rows, stride)
            for t in STAGE_TABLES:  # every table size at every shape, the map kinds in turn
                kind = MAP_KINDS[q % len(MAP_KINDS)]
                q += 1
                one(src, gather_map(rng, kind, rows, len(src)), stride, t,
                    f"rx_stage stride={stride} rows={rows} map={kind} tables={t}")
    for stride in (16, 1216):  # no rows, tables only
        for t in STAGE_TABLES[1:]:
            one(gather_source(rng, 0, stride), np.zeros(0, np.int32), stride, t, f"rx_stage stride={stride} rows=0 tables={t}")


# -- line_jobs --------------------------------------------------------------------------------------------------
MEMBER_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 33)  # the 4-wide body, the tail, both
# stride: job counts of the first level; jobs x (stride / 16) = 1, 255, 256, 257, ~20,000 (76 chunks: 76, 228, 304, 19,988)
LINE_JOBS = {16: (1, 255, 256, 257, 20000), 1216: (1, 3, 4, 263)}


def ref_line_jobs(jobs, members, rows, outrows):
    """out = parity ^ XOR(members); code m >= 0: rows[m], m < 0: outrows[-1 - m]
    (an output of an earlier level: every job of a call reads the state before it)."""
    before = outrows
    after = outrows.copy()
    for J in jobs:
        acc = rows[J["parity"]].copy()
        for m in members[J["member0"]:J["member0"] + J["n_members"]]:
            acc ^= rows[m] if m >= 0 else before[-1 - m]
        after[J["out"]] = acc
    return after


def line_job_levels(rng, n1, n_rows, shift):
    """Two dependency levels: n1 jobs over arrived rows, then max(1, n1 // 3)
    jobs whose members include level-1 outputs (negative codes).  Returns
    (levels [(jobs, members)], output rows in all): every fifth output row is
    written by no job."""
    n2 = max(1, n1 // 3)
    n_out = (n1 + n2) + (n1 + n2) // 4 + 1
    outs = rng.permutation(n_out)
    unwritten = outs[n1 + n2:]
    levels = []
    for lvl, (lo, cnt) in enumerate(((0, n1), (n1, n2))):
        jobs = np.zeros(cnt, JOB_DTYPE)
        jobs["out"] = outs[lo:lo + cnt]
        jobs["parity"] = rng.integers(0, n_rows, cnt)
        jobs["n_members"] = np.array(MEMBER_COUNTS)[(np.arange(cnt) + shift + lvl) % len(MEMBER_COUNTS)]
        jobs["member0"] = np.concatenate([[0], np.cumsum(jobs["n_members"])[:-1]]) + 3  # (a list that starts off 0)
        total = int(jobs["n_members"].sum()) + 3
        members = rng.integers(0, n_rows, total).astype(np.int32)
        if lvl == 1:  # about half of the members: outputs of level 1; every job with members reads at least one
            prev = -1 - outs[rng.integers(0, n1, total)].astype(np.int32)
            neg = rng.random(total) < 0.5
            neg[jobs["member0"][jobs["n_members"] > 0]] = True
            members = np.where(neg, prev, members).astype(np.int32)
        levels.append((jobs, members))
    return levels, n_out, unwritten


def check_line_jobs(engine):
    rng = np.random.default_rng(33)
    n_rows = 97
    for stride, counts in LINE_JOBS.items():
        rows = rng.integers(0, 256, (n_rows, stride), dtype=np.uint8)
        runs = [(n1, 0) for n1 in counts] + [(1, s) for s in range(1, len(MEMBER_COUNTS))]  # one job: every count
        for n1, shift in runs:
            levels, n_out, unwritten = line_job_levels(rng, n1, n_rows, shift)
            state = np.full((n_out + GUARD, stride), CANARY, np.uint8)
            want = state.copy()
            for lvl, (jobs, members) in enumerate(levels):
                what = f"line_jobs stride={stride} jobs={n1} level={lvl + 1} first count={int(jobs['n_members'][0])}"
                want = ref_line_jobs(jobs, members, rows, want)
                state = engine.line_jobs(jobs, members, rows, state.copy(), stride)
                assert state.shape == want.shape, what
                bad = np.nonzero((state != want).any(1))[0]
                assert len(bad) == 0, (what, len(bad), bad[:8])
            assert (state[unwritten] == CANARY).all() and (state[n_out:] == CANARY).all()  # (holds in `want` by construction)


# -- send_gather ------------------------------------------------------------------------------------------------
SEND_STRIDES = (16, 1008, 1024)  # 1008: 63 chunks, slot starts slide against the waves; 1024: each slot ends on lane 63
SEND_MARGIN = 64  # every source at least this far inside the blob


def send_sizes(stride):
    s = [0, 1, 2, 3, 4, 5, *range(12, 20), 31, 32, 33, stride - 17, stride - 16, stride - 15, stride - 1, stride]
    return sorted({x for x in s if 0 <= x <= stride})


def ref_send_gather(blob, offsets, sizes, stride):
    dst = np.zeros((len(offsets), stride), np.uint8)
    for s, (o, n) in enumerate(zip(offsets, sizes)):
        if o >= 0:
            dst[s, :n] = blob[o:o + n]
    return dst


def send_slots(rng, stride, blob_len):
    """(offsets, sizes): misalignment 0..3 x the edge sizes; 132 slots of full
    and nearly full size (at 63 chunks a slot every chunk index meets lane 63
    with bytes to fetch from the next dword); 300 random ones, every 11th a
    zero slot."""
    lim = blob_len - SEND_MARGIN - stride - 4

    def at(mis):
        return int(rng.integers(SEND_MARGIN // 4, lim // 4)) * 4 + mis

    slots = [(at(mis), n) for mis in range(4) for n in send_sizes(stride)]
    slots += [(at((i + 1) % 4), stride - (i % 3 == 2)) for i in range(132)]
    for i in range(300):
        slots.append((-1, int(rng.integers(0, stride + 1))) if i % 11 == 10
                     else (at(int(rng.integers(4))), int(rng.integers(0, stride + 1))))
    off = np.array([o for o, _ in slots], np.int64)
    size = np.array([n for _, n in slots], np.uint16)
    live = off >= 0
    assert (off[live] >= SEND_MARGIN).all() and (off[live] + size[live] <= blob_len - SEND_MARGIN).all()
    return off, size


def check_send_gather(engine):
    rng = np.random.default_rng(34)
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    for stride in SEND_STRIDES:
        off, size = send_slots(rng, stride, len(blob))
        got = guarded(engine.send_gather(blob, off, size, stride), len(off), f"send_gather stride={stride}")
        want = ref_send_gather(blob, off, size, stride)
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (f"send_gather stride={stride}", len(bad),
                               [(int(s), int(off[s]) & 3, int(size[s])) for s in bad[:8]])
