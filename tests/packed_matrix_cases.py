"""Shared by the packed matrix record tests (CPU and GPU; no GPU needed here):
the host restatement of the record layout of razor_fec.h
(rfec_pack_erasures_matrix), the lossy batches the decodes run on, and a
census of what those batches exercise (cascades, long schedules, rejected
lines), so the GPU parity test cannot pass on inputs that never reach them.
"""
from __future__ import annotations

import numpy as np

import pyoracle as po

SHAPES = [(6, 16), (9, 100), (10, 64), (13, 48), (16, 32), (10, 1200)]  # (k, S)
G_CASES = 300


def shape_of(k):
    """(COL, R): rows of COL consecutive segments (3 for k <= 9, else 4), R rows."""
    col = 3 if k <= 9 else 4
    return col, (k + col - 1) // col


def slot_bytes(k):
    col, rows = shape_of(k)
    return 24 + 20 * (col - 1), 24 + 20 * (rows - 1)


def stride_of(k, E):
    rh, ch = slot_bytes(k)
    return (16 + E * (rh + ch) + 63) // 64 * 64


def seed_of(k, S):
    return k * 91 + S


def pack_matrix_np(plan, hdr, present, meta, fsize, pp, E):
    """The packed matrix records of a batch, [G][stride] bytes: what a receiver
    that keeps per-group state would write as segments and parities arrive."""
    G, k = hdr.shape
    col, rows = shape_of(k)
    nr = plan.n_lines - col  # row lines (a last row of one member has none)
    rh, ch = slot_bytes(k)
    out = np.zeros((G, stride_of(k, E)), np.uint8)
    hb = np.ascontiguousarray(hdr).view(np.uint8).reshape(G, k, 20)
    mb = np.ascontiguousarray(meta).view(np.uint8).reshape(G, plan.n_lines, 20)

    def half(g, o, line, members, t, h):
        out[g, o:o + 20] = mb[g, line]
        out[g, o + 20:o + 22] = np.frombuffer(np.uint16(int(fsize[g, line])).tobytes(), np.uint8)
        q = o + 24
        for i in members:
            if i == t:
                continue
            if (h >> i) & 1:
                out[g, q:q + 20] = hb[g, i]
            q += 20

    for g in range(G):
        h = int(present[g, 0])
        out[g, 0:8] = np.frombuffer(np.uint64(h).tobytes(), np.uint8)
        out[g, 8:16] = np.frombuffer(np.uint64(int(pp[g])).tobytes(), np.uint8)
        missing = [i for i in range(k) if not (h >> i) & 1]
        for e in range(min(E, len(missing))):
            t = missing[e]
            r, c = divmod(t, col)
            o = 16 + e * (rh + ch)
            if r < nr:
                half(g, o, r, range(r * col, min(k, r * col + col)), t, h)
            half(g, o + rh, nr + c, range(c, k, col), t, h)
    return out


def lossy_matrix_rx(o, k, S, G, seed):
    """A received batch of the sender's full plan of k: 0..6 erasures per group,
    a lost parity with probability 0.2 and one of three header corruptions with
    probability 0.15 each (the generator of test_packed_decode_gpu).  Erased
    header records and payloads are 0xA5 bytes: a packer that copies an erased
    member's record is caught.  Returns (plan, rx, rh, present, parity, meta,
    fec_size, parity_present, capacity)."""
    col, rows = shape_of(k)
    plan = o.plan_matrix(k, rows, col, 3)
    rng = np.random.default_rng(seed)
    shards, hdr = o.fill_groups(53, G, k, S, ragged=True)
    cap = min(o.video_size, S)
    parity, meta, fsize, _ = o.encode_batch(plan, shards, hdr, cap)
    present = np.zeros((G, 2), np.uint64)
    pp = np.full(G, (1 << plan.n_lines) - 1, np.uint64)
    rx, rh, fs_rx = shards.copy(), hdr.copy(), fsize.copy()
    for g in range(G):
        m = (1 << k) - 1
        for i in rng.choice(k, int(rng.integers(0, 7)), replace=False):
            m &= ~(1 << int(i))
            rx[g, i] = 0xA5
            rh[g, i:i + 1].view(np.uint8)[...] = 0xA5
        present[g, 0] = m
        if rng.random() < 0.2:
            pp[g] &= ~np.uint64(1 << int(rng.integers(plan.n_lines)))
        r = rng.random()
        if r < 0.15:
            fs_rx[g, rng.integers(plan.n_lines)] = cap + 1
        elif r < 0.3:
            l = int(rng.integers(plan.n_lines))
            fs_rx[g, l] = max(1, int(fs_rx[g, l]) - 3)
        elif r < 0.45:
            i = int(rng.integers(k))
            if (m >> i) & 1:
                rh[g, i]["size"] = min(cap, int(rh[g, i]["size"]) + 5)
    return plan, rx, rh, present, parity, meta, fs_rx, pp, cap


def mask_schedule(plan, have, ppm, E):
    """The canonical schedule over the masks alone (no header checks): lines in
    plan order, repeated to a fixpoint; a line fires with its parity received,
    exactly one member missing and one present; only erased segments of rank
    < E are targets.  Returns [(line, target, cascade)], cascade = the line
    reads a segment recovered by an earlier step."""
    k = plan.k
    erased = ~have & ((1 << k) - 1)
    masks = [sum(1 << i for i in plan.members(l)) for l in range(plan.n_lines)]
    steps, progress = [], True
    while progress:
        progress = False
        for l, m in enumerate(masks):
            x = m & ~have
            if not (ppm >> l) & 1 or bin(x).count("1") != 1 or not m & have:
                continue
            t = x.bit_length() - 1
            if bin(erased & ((1 << t) - 1)).count("1") >= E:
                continue
            steps.append((l, t, bool(m & erased & ~x)))
            have |= x
            progress = True
    return steps


def coverage(plan, present, pp, recovered, E):
    """What a batch exercises: per group the mask-only schedule against what
    was actually recovered (`recovered` [G][2] of the exact peel)."""
    c = dict(recovering=0, clean_cascades=0, long=0, rejected=0, cascade_rejected=0)
    for g in range(present.shape[0]):
        steps = mask_schedule(plan, int(present[g, 0]), int(pp[g]), E)
        n = bin(int(recovered[g, 0])).count("1")
        casc = any(s[2] for s in steps)
        c["recovering"] += n > 0
        c["clean_cascades"] += casc and n == len(steps)
        c["long"] += n > 4
        c["rejected"] += n < len(steps)
        c["cascade_rejected"] += casc and n < len(steps)
    return c


def check_coverage(c, k, E):
    """The census a parity run needs (asserted on the CPU against the oracle
    and on the GPU against rfec_recover_batch_out)."""
    if E == k:
        assert c["recovering"] >= 100 and c["clean_cascades"] >= 50, c
        assert c["rejected"] >= 3 and c["cascade_rejected"] >= 3, c
        assert k < 9 or c["long"] >= 20, c
    if E == 2:
        assert c["clean_cascades"] >= 30, c
