#!/usr/bin/env python3
"""rfec_wire_regroup_shapes on one GPU: the receive chain after the parse over a
window whose groups have four shapes, with one regroup pass for the window
against one rfec_wire_regroup_index call per shape.

Stream: a window of 65,535 groups, shape p = g mod 4 of
    (10, 3, 4) rows + columns, (32, 8, 4) rows, (16, 4, 4) rows + columns, (6, 2, 3) rows + columns,
1,200-B segments in 1,216-B rows.  Every shape's groups go through the product's
own rfec_wire_encode_send, two segments of every group are lost (length 0), the
datagrams are merged in send order (group after group, a group's segments before
its parities) or, with --shuffle, in a random arrival order, and one
rfec_wire_parse makes the records and rows both chains read.

    chain B   one rfec_wire_regroup_shapes + one rfec_recover_indexed_out per shape over counts[p] groups
    chain A   per shape: rfec_wire_regroup_index into tables of the whole window + rfec_recover_indexed_out over
              the window's groups
    shapes_call   chain B's regroup call alone;  index_x4: chain A's four regroup calls alone

B's recovered segments are compared with A's through shape_of / rank_of before anything is timed (exit status 1
where they differ).  The variants alternate step by step, each bracketed by stream events around the whole chain,
over enough steps for --min-ms (default 250) of timed work each; mean / std / p05 / p95 per variant.  The kernels'
own times need a profiler run of few steps (--steps).  One JSON object per arrival order on stdout.

    python tools/regroup_shapes_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--steps 0]
                                         [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from razor_amd.fec import RFEC_LAYER_COLS, RFEC_LAYER_ROWS, native  # noqa: E402

E = 2  # dense out slots per group: the two lost segments
S, STRIDE, DSTRIDE = 1200, 1216, 1280
SHAPES = ((10, 3, 4, RFEC_LAYER_ROWS | RFEC_LAYER_COLS), (32, 8, 4, RFEC_LAYER_ROWS),
          (16, 4, 4, RFEC_LAYER_ROWS | RFEC_LAYER_COLS), (6, 2, 3, RFEC_LAYER_ROWS | RFEC_LAYER_COLS))
TABLES = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")
SECTION = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "group_of")
DECODE_IN = ("src_of", "hdr", "present", "meta", "fec_size", "parity_present")


def build_stream(lib, plans, G, dev, st, shuffle, seed):
    """recs [N][64], payload [N][STRIDE] of the window, and the groups of every shape."""
    rng = np.random.default_rng(seed)
    u8 = torch.uint8
    dgrams, dlens, keys = [], [], []
    groups_of = [np.arange(p, G, len(plans)) for p in range(len(plans))]
    for p, plan in enumerate(plans):
        gs = groups_of[p]
        Gp, k, n = len(gs), plan.k, plan.n_lines
        shards = torch.empty((Gp, k, STRIDE), dtype=u8, device=dev)
        lib.fill_xorshift(shards.data_ptr(), 3, p * G, Gp, k, S, STRIDE, st)
        hdr_np = bench.make_headers(Gp, k, S, 0)
        hdr_np["seq"] += np.uint32(p << 28)  # packet ids of the shapes apart
        hdr = torch.from_numpy(hdr_np.view(np.uint8).reshape(Gp, k, 20).copy()).to(dev)
        fst, sst = bench.wire_stamps(hdr_np, plan, n)
        fid = (gs % 65535 + 1).astype(np.uint16)  # fec_id0 = 1
        fst["fec_id"], sst["fec_id"] = np.repeat(fid, n), np.repeat(fid, k)
        fstamps = torch.from_numpy(fst.view(np.uint8).copy()).to(dev)
        sstamps = torch.from_numpy(sst.view(np.uint8).copy()).to(dev)
        ns, N = Gp * k, Gp * (k + n)
        dgram = torch.empty((N, DSTRIDE), dtype=u8, device=dev)
        dlen = torch.empty((N,), dtype=torch.int16, device=dev)
        lib.wire_encode_send(plan, Gp, STRIDE, S, shards.data_ptr(), hdr.data_ptr(), sstamps.data_ptr(),
                             dgram.data_ptr(), dlen.data_ptr(), fstamps.data_ptr(), dgram.data_ptr() + ns * DSTRIDE,
                             dlen.data_ptr() + ns * 2, DSTRIDE, st)
        lost = np.argsort(rng.random((Gp, k)), axis=1)[:, :2]
        dlen[torch.from_numpy((np.arange(Gp)[:, None] * k + lost).reshape(-1)).to(dev)] = 0
        torch.cuda.synchronize(dev)
        dgrams.append(dgram)
        dlens.append(dlen)
        # send order: by group, a group's segments before its parities
        keys.append(np.concatenate([np.repeat(gs, k) * 2, np.repeat(gs, n) * 2 + 1]))
        del shards
    key = np.concatenate(keys)
    order = rng.permutation(len(key)) if shuffle else np.argsort(key, kind="stable")
    t_order = torch.from_numpy(order).to(dev)
    dgram = torch.cat(dgrams)[t_order].contiguous()
    dlen = torch.cat(dlens)[t_order].contiguous()
    del dgrams, dlens
    N = len(key)
    recs = torch.empty((N, 64), dtype=u8, device=dev)
    payload = torch.empty((N, STRIDE), dtype=u8, device=dev)
    lib.wire_parse(N, DSTRIDE, dgram.data_ptr(), dlen.data_ptr(), STRIDE, S, recs.data_ptr(), payload.data_ptr(), st)
    torch.cuda.synchronize(dev)
    return recs, payload, groups_of


def tables(plan, rows, n_rec, dev, names):
    k, n = plan.k, plan.n_lines
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    t = dict(hdr=z(rows, k, 20), present=z(rows, 2, dt=torch.int64), meta=z(rows, n, 20),
             fec_size=z(rows, n, dt=torch.int16), parity_present=z(rows, dt=torch.int64),
             base_id=z(rows, dt=torch.int32), src_of=z(rows * (k + n), dt=torch.int32),
             group_of=z(rows, dt=torch.int32), slot_of=z(n_rec, dt=torch.int32))
    return {name: t[name] for name in names}


def decode_out(rows, dev):
    return dict(recovered=torch.zeros((rows, 2), dtype=torch.int64, device=dev),
                out_shards=torch.zeros((rows, E, STRIDE), dtype=torch.uint8, device=dev),
                out_hdr=torch.zeros((rows, E, 20), dtype=torch.uint8, device=dev),
                out_index=torch.full((rows, E), 0x3C, dtype=torch.uint8, device=dev))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65535)
    ap.add_argument("--orders", default="send,shuffled")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regroup_shapes_bench.py: needs a GPU")
    if not 4 <= args.groups <= 65535:
        raise SystemExit("regroup_shapes_bench.py: one window holds 4 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    plans = [lib.plan_matrix(*s) for s in SHAPES]
    P, G = len(plans), args.groups
    cd = (S + 15) // 16
    rc = 0
    for order in args.orders.split(","):
        recs, payload, groups_of = build_stream(lib, plans, G, dev, st, order == "shuffled", 11)
        N = recs.shape[0]
        caps = [len(gs) for gs in groups_of]
        # chain B: the window outputs, a section per shape with room for its groups, decode outputs per section
        win = dict(shape_of=torch.zeros(G, dtype=torch.uint8, device=dev),
                   rank_of=torch.zeros(G, dtype=torch.int32, device=dev),
                   anchor_of=torch.zeros(G, dtype=torch.int32, device=dev),
                   counts=torch.zeros(P, dtype=torch.int32, device=dev),
                   slot_of=torch.zeros(N, dtype=torch.int32, device=dev))
        sec = [tables(plans[p], caps[p], 0, dev, SECTION) for p in range(P)]
        sections = [dict(cap=caps[p], **{name: sec[p][name].data_ptr() for name in SECTION}) for p in range(P)]
        dec_b = [decode_out(caps[p], dev) for p in range(P)]
        # chain A: per shape, tables and decode outputs of the whole window
        tab = [tables(plans[p], G, N, dev, TABLES) for p in range(P)]
        dec_a = [decode_out(G, dev) for p in range(P)]
        ws = [torch.empty(max(16, lib.workspace_size(plans[p], G)), dtype=torch.uint8, device=dev) for p in range(P)]
        counts = [0] * P

        def shapes():
            lib.wire_regroup_shapes(plans, sections, G, 1, N, recs.data_ptr(), S,
                                    *(win[name].data_ptr() for name in ("shape_of", "rank_of", "anchor_of", "counts",
                                                                        "slot_of")), st)

        def decode(p, groups, t, d):
            if groups:
                lib.recover_indexed_out(plans[p], groups, STRIDE, S, payload.data_ptr(), N,
                                        *(t[name].data_ptr() for name in DECODE_IN), d["recovered"].data_ptr(), E,
                                        d["out_shards"].data_ptr(), d["out_hdr"].data_ptr(), d["out_index"].data_ptr(),
                                        ws[p].data_ptr(), st)

        def chain_b():
            shapes()
            for p in range(P):
                decode(p, counts[p], sec[p], dec_b[p])

        def index_x4():
            for p in range(P):
                lib.wire_regroup_index(plans[p], G, 1, N, recs.data_ptr(), S,
                                       *(tab[p][name].data_ptr() for name in TABLES), st)

        def chain_a():
            for p in range(P):
                lib.wire_regroup_index(plans[p], G, 1, N, recs.data_ptr(), S,
                                       *(tab[p][name].data_ptr() for name in TABLES), st)
                decode(p, G, tab[p], dec_a[p])

        # the outputs, before anything is timed: counts read back once (a receiver sizes its decodes by them)
        shapes()
        torch.cuda.synchronize(dev)
        counts = [int(c) for c in win["counts"].cpu().numpy().view(np.uint32)]
        chain_a()
        chain_b()
        torch.cuda.synchronize(dev)
        shape_of = win["shape_of"].cpu().numpy()
        equal = counts == caps and all(bool((shape_of[groups_of[p]] == p).all()) for p in range(P))
        recovered = 0
        for p in range(P):
            gs = torch.from_numpy(groups_of[p]).to(dev)
            a, b = dec_a[p], dec_b[p]
            equal &= bool(torch.equal(sec[p]["group_of"].view(torch.int32), gs.to(torch.int32)))
            ok = b["out_index"] != 0xFF
            recovered += int(ok.sum())
            equal &= bool(torch.equal(a["recovered"][gs], b["recovered"]) and
                          torch.equal(a["out_index"][gs], b["out_index"]) and
                          torch.equal(a["out_hdr"][gs][ok], b["out_hdr"][ok]) and
                          torch.equal(a["out_shards"][gs][ok][:, :16 * cd], b["out_shards"][ok][:, :16 * cd]))
            for name in SECTION[:-1]:
                rows = len(groups_of[p])
                equal &= bool(torch.equal(tab[p][name].view(G, -1)[gs], sec[p][name].view(rows, -1)))
        rc |= 0 if equal and recovered else 1
        variants = {"chain_a": chain_a, "chain_b": chain_b, "shapes_call": shapes, "index_x4": index_x4}

        def run(steps, keep):
            ev = {v: [] for v in variants}
            names = list(variants)
            for step in range(steps):
                for v in names[step % len(names):] + names[:step % len(names)]:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    variants[v]()
                    b.record(stream)
                    ev[v].append((a, b))
            torch.cuda.synchronize(dev)
            return {v: np.array([a.elapsed_time(b) for a, b in e][-keep:]) * 1e3 for v, e in ev.items()}

        est = run(args.warmup + 3, 3)
        steps = args.steps or max(10, int(math.ceil(args.min_ms * 1e3 / min(float(t.mean()) for t in est.values()))))
        us = run(steps, steps)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "std_us": round(float(t.std()), 2),
                    "p05_us": round(float(np.percentile(t, 5)), 2), "p95_us": round(float(np.percentile(t, 95)), 2),
                    "median_us": round(float(np.median(t)), 2), "min_us": round(float(t.min()), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        a_us, b_us = us["chain_a"], us["chain_b"]
        line = {"groups": G, "shapes": [list(s[:3]) + [plans[p].n_lines] for p, s in enumerate(SHAPES)],
                "counts": counts, "S": S, "stride": STRIDE, "records": N, "per_group": E, "arrival": order,
                "steps": steps, "timing": "stream events around the whole chain, variants alternating",
                "outputs_equal": bool(equal), "recovered_segments": recovered,
                **{v: stat(t) for v, t in us.items()},
                "b_over_a": round(float(b_us.mean() / a_us.mean()), 4),
                "b_p95_below_a_p05": bool(np.percentile(b_us, 95) < np.percentile(a_us, 5)),
                "shapes_over_index_x4": round(float(us["shapes_call"].mean() / us["index_x4"].mean()), 4)}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec, tab, dec_a, dec_b, win, ws
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
