#!/usr/bin/env python3
"""rfec_wire_window_census on one GPU: what it costs a receiver to learn a parsed
window's shapes on the device, against what it could do before.

Stream: regroup_shapes_bench.py's: a window of --groups groups,
shape p = g mod 4 of four shapes, 1,200-B segments, two segments of every group
lost, in send order or shuffled; one rfec_wire_parse makes the records.

    (a) census_d2h      the census call + one copy of its 576 bytes to pinned host memory
        records_d2h     the copy of the n 64-byte records to pinned host memory alone: the lower bound of learning
                        the shapes on the host
    (b) census_call     the census call alone
        shapes_call     the rfec_wire_regroup_shapes call it precedes (exact caps)
    (c) chain_census    census, its read-back, plans_from_census on the host, rfec_wire_regroup_shapes with
                        cap = the census's counts, ONE rfec_recover_indexed_window_out with groups = the same
        chain_parent    rfec_wire_regroup_shapes with cap = G per plan (the plans known ahead, which a receiver's
                        are not), counts read back, the same decode with groups = counts

The census's plans and counts, and chain_census's decode outputs, are compared with chain_parent's before anything
is timed (exit status 1 where they differ).  The variants alternate step by step, each bracketed by stream events
around the whole of it (the read-backs and the host work in between included), over enough steps for --min-ms
(default 250) of timed work each; mean / std / p05 / p95 per variant.  One JSON object per arrival order on stdout.

    python tools/window_census_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--steps 0]
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
sys.path.insert(0, str(ROOT / "tools"))

from razor_amd.fec import Native, native  # noqa: E402
from regroup_shapes_bench import E, S, SECTION, SHAPES, STRIDE, build_stream, tables  # noqa: E402

WINDOW = ("shape_of", "rank_of", "anchor_of", "counts", "slot_of")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65535)
    ap.add_argument("--orders", default="send,shuffled")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--census-lib", default="", help="A/B only: another build of librazor_fec_v1200.so whose census "
                                                     "call is timed beside this one's (census_call_alt)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_census_bench.py: needs a GPU")
    if not 4 <= args.groups <= 65535:
        raise SystemExit("window_census_bench.py: one window holds 4 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    alt = Native(1200, args.census_lib) if args.census_lib else None
    known = [lib.plan_matrix(*s) for s in SHAPES]
    P, G = len(known), args.groups
    rc = 0
    for order in args.orders.split(","):
        recs, payload, groups_of = build_stream(lib, known, G, dev, st, order == "shuffled", 11)
        N = recs.shape[0]
        true_counts = [len(gs) for gs in groups_of]

        def window():
            return dict(shape_of=torch.zeros(G, dtype=torch.uint8, device=dev),
                        rank_of=torch.zeros(G, dtype=torch.int32, device=dev),
                        anchor_of=torch.zeros(G, dtype=torch.int32, device=dev),
                        counts=torch.zeros(P, dtype=torch.int32, device=dev),
                        slot_of=torch.zeros(N, dtype=torch.int32, device=dev))

        def decode_out(rows):
            return dict(recovered=torch.zeros((rows, 2), dtype=torch.int64, device=dev),
                        out_shards=torch.zeros((rows, E, STRIDE), dtype=torch.uint8, device=dev),
                        out_hdr=torch.zeros((rows, E, 20), dtype=torch.uint8, device=dev),
                        out_index=torch.full((rows, E), 0x3C, dtype=torch.uint8, device=dev))

        # the census, its outputs and the pinned landing places of the two copies
        d_cen = torch.zeros(576, dtype=torch.uint8, device=dev)
        d_anchor = torch.zeros(G, dtype=torch.int32, device=dev)
        d_key = torch.zeros(G, dtype=torch.int32, device=dev)
        h_cen = torch.zeros(576, dtype=torch.uint8).pin_memory()
        h_recs = torch.zeros((N, 64), dtype=torch.uint8).pin_memory()
        h_counts = torch.zeros(P, dtype=torch.int32).pin_memory()
        # the census's chain: sections of exactly the census's counts (allocated once, from the first census: the
        # window does not change between steps); the parent's chain: sections of the whole window per plan
        win_c, win_p = window(), window()
        sec_p = [tables(known[p], G, 0, dev, SECTION) for p in range(P)]
        sections_p = [dict(cap=G, **{name: sec_p[p][name].data_ptr() for name in SECTION}) for p in range(P)]
        dec_c, dec_p = decode_out(G), decode_out(G)

        def census():
            lib.wire_window_census(G, 1, N, recs.data_ptr(), S, d_cen.data_ptr(), d_anchor.data_ptr(),
                                   d_key.data_ptr(), st)

        def census_d2h():
            census()
            h_cen.copy_(d_cen, non_blocking=True)

        def records_d2h():
            h_recs.copy_(recs, non_blocking=True)

        census_d2h()
        torch.cuda.synchronize(dev)
        plans, groups = lib.plans_from_census(h_cen.numpy().tobytes())
        ok = groups == true_counts and [p.lines() for p in plans] == [p.lines() for p in known]
        sec_c = [tables(plans[p], groups[p], 0, dev, SECTION) for p in range(len(plans))]

        def regroup(pl, sections, win):
            lib.wire_regroup_shapes(pl, sections, G, 1, N, recs.data_ptr(), S,
                                    *(win[name].data_ptr() for name in WINDOW), st)

        def decode(pl, sections, counts, d):
            lib.recover_indexed_window_out(pl, sections, counts, STRIDE, S, payload.data_ptr(), N,
                                           d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                           d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), st)

        def chain_census():
            census_d2h()
            stream.synchronize()
            pl, gr = lib.plans_from_census(h_cen.numpy().tobytes())
            sections = [dict(cap=gr[p], **{name: sec_c[p][name].data_ptr() for name in SECTION})
                        for p in range(len(pl))]
            regroup(pl, sections, win_c)
            decode(pl, sections, gr, dec_c)

        def chain_parent():
            regroup(known, sections_p, win_p)
            h_counts.copy_(win_p["counts"], non_blocking=True)
            stream.synchronize()
            decode(known, sections_p, [int(c) for c in h_counts.numpy().view(np.uint32)], dec_p)

        sections_c = [dict(cap=groups[p], **{name: sec_c[p][name].data_ptr() for name in SECTION})
                      for p in range(len(plans))]

        def shapes_call():
            regroup(plans, sections_c, win_c)

        # the outputs, before anything is timed
        chain_census()
        chain_parent()
        torch.cuda.synchronize(dev)
        R = sum(true_counts)
        recovered = int((dec_c["out_index"][:R] != 0xFF).sum())
        ok = ok and all(bool(torch.equal(win_c[name], win_p[name])) for name in WINDOW)
        ok = ok and bool(torch.equal(win_c["anchor_of"], d_anchor))
        ok = ok and all(bool(torch.equal(dec_c[name][:R], dec_p[name][:R])) for name in dec_c) and recovered > R
        rc |= 0 if ok else 1
        if alt is not None:  # the other build's census into outputs of its own, compared before it is timed
            a_cen, a_anchor, a_key = torch.zeros_like(d_cen), torch.zeros_like(d_anchor), torch.zeros_like(d_key)

            def census_alt():
                alt.wire_window_census(G, 1, N, recs.data_ptr(), S, a_cen.data_ptr(), a_anchor.data_ptr(),
                                       a_key.data_ptr(), st)

            census()
            census_alt()
            torch.cuda.synchronize(dev)
            ok = ok and bool(torch.equal(a_cen, d_cen) and torch.equal(a_anchor, d_anchor) and torch.equal(a_key, d_key))
            rc |= 0 if ok else 1
        variants = {"census_d2h": census_d2h, "records_d2h": records_d2h, "census_call": census,
                    "shapes_call": shapes_call, "chain_census": chain_census, "chain_parent": chain_parent}
        if alt is not None:
            variants["census_call_alt"] = census_alt

        def run(steps, reps, keep):
            """Every step runs every variant, v reps[v] times in a row (each run bracketed by its own events), the
            order of the variants rotating: the variants differ a hundredfold in length, and each gets min-ms."""
            ev = {v: [] for v in variants}
            names = list(variants)
            for step in range(steps):
                for v in names[step % len(names):] + names[:step % len(names)]:
                    for _ in range(reps[v]):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        variants[v]()
                        b.record(stream)
                        ev[v].append((a, b))
            torch.cuda.synchronize(dev)
            return {v: np.array([a.elapsed_time(b) for a, b in e][-keep * reps[v]:]) * 1e3 for v, e in ev.items()}

        est = {v: float(t.mean()) for v, t in run(args.warmup + 3, {v: 1 for v in variants}, 3).items()}
        slowest = max(est.values())
        steps = args.steps or max(10, int(math.ceil(args.min_ms * 1e3 / slowest)))
        reps = {v: max(1, min(64, int(slowest / t))) for v, t in est.items()}
        us = run(steps, reps, steps)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "std_us": round(float(t.std()), 2),
                    "p05_us": round(float(np.percentile(t, 5)), 2), "p95_us": round(float(np.percentile(t, 95)), 2),
                    "median_us": round(float(np.median(t)), 2), "min_us": round(float(t.min()), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        def below(x, y):  # x faster than y, as the project calls it: x's p95 below y's p05
            return bool(np.percentile(us[x], 95) < np.percentile(us[y], 5))

        line = {"groups": G, "shapes": [list(s[:3]) + [known[p].n_lines] for p, s in enumerate(SHAPES)],
                "counts": groups, "S": S, "stride": STRIDE, "records": N, "record_bytes": N * 64, "per_group": E,
                "arrival": order, "steps": steps, "runs_per_step": reps, "census_tag": hex(lib.census_last_path()),
                "timing": "stream events around the whole variant, variants alternating",
                "outputs_equal": bool(ok), "recovered_segments": recovered,
                **{v: stat(t) for v, t in us.items()},
                "census_d2h_over_records_d2h": round(float(us["census_d2h"].mean() / us["records_d2h"].mean()), 4),
                "census_d2h_p95_below_records_d2h_p05": below("census_d2h", "records_d2h"),
                "records_d2h_p95_below_census_d2h_p05": below("records_d2h", "census_d2h"),
                "census_over_shapes_call": round(float(us["census_call"].mean() / us["shapes_call"].mean()), 4),
                "chain_census_over_parent": round(float(us["chain_census"].mean() / us["chain_parent"].mean()), 4),
                "chain_census_p95_below_parent_p05": below("chain_census", "chain_parent"),
                "chain_parent_p95_below_census_p05": below("chain_parent", "chain_census")}
        if alt is not None:
            line.update(census_lib=Path(args.census_lib).name,
                        census_over_alt=round(float(us["census_call"].mean() / us["census_call_alt"].mean()), 4),
                        census_p95_below_alt_p05=below("census_call", "census_call_alt"),
                        alt_p95_below_census_p05=below("census_call_alt", "census_call"))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec_c, sec_p, dec_c, dec_p, win_c, win_p, h_recs
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
