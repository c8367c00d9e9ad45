#!/usr/bin/env python3
"""rfec_recover_indexed_shapes_out on one GPU: the decode behind one
rfec_wire_regroup_shapes over a window whose groups have four shapes, one launch
for the window against one call per shape.

Stream: tools/regroup_shapes_bench.py's (a window of --groups groups, shape
p = g mod 4 of (10, 3, 4) rows + columns, (32, 8, 4) rows, (16, 4, 4) rows +
columns, (6, 2, 3) rows + columns; 1,200-B segments in 1,216-B rows; two segments
of every group lost; send order or shuffled), parsed once and regrouped once by
rfec_wire_regroup_shapes into sections of cap = min(groups, 2 counts[p]) rows.

    per_shape_counts   rfec_recover_indexed_matrix_out for the three matrix sections and rfec_recover_indexed_out
                       for the row layout, each over counts[p] rows into arrays of its own: the best chain without
                       the new call
    per_shape_cap      the same over cap rows (a receiver that did not read the counts back)
    shapes_counts      one rfec_recover_indexed_shapes_out with groups = counts
    shapes_cap         one rfec_recover_indexed_shapes_out with groups = NULL (cap)

Every variant's outputs are compared with per_shape_counts' before anything is timed (exit status 1 where they
differ).  All calls go through prebuilt ctypes arguments, so no variant pays for a binding the other does not.  The
variants alternate step by step, each bracketed by stream events around its calls, over enough steps for --min-ms
(default 250) of timed work each; mean / std / p05 / p95 per variant.  One JSON object per arrival order on stdout.

    python tools/recover_shapes_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--steps 0]
                                         [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from razor_amd.fec import as_plan, native, rfec_plan, rfec_regroup_section  # noqa: E402
from regroup_shapes_bench import DECODE_IN, E, S, SECTION, SHAPES, STRIDE, build_stream, decode_out, tables  # noqa: E402


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
        raise SystemExit("recover_shapes_bench.py: needs a GPU")
    if not 4 <= args.groups <= 65535:
        raise SystemExit("recover_shapes_bench.py: one window holds 4 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    plans = [lib.plan_matrix(*s) for s in SHAPES]
    matrix = [lib.packed_matrix_stride(p, 1) != 0 for p in plans]
    assert matrix == [True, False, True, True]
    P, G = len(plans), args.groups
    cd = (S + 15) // 16
    rc = 0
    for order in args.orders.split(","):
        recs, payload, groups_of = build_stream(lib, plans, G, dev, st, order == "shuffled", 11)
        N = recs.shape[0]
        caps = [min(G, 2 * len(gs)) for gs in groups_of]
        win = dict(shape_of=torch.zeros(G, dtype=torch.uint8, device=dev),
                   rank_of=torch.zeros(G, dtype=torch.int32, device=dev),
                   anchor_of=torch.zeros(G, dtype=torch.int32, device=dev),
                   counts=torch.zeros(P, dtype=torch.int32, device=dev),
                   slot_of=torch.zeros(N, dtype=torch.int32, device=dev))
        sec = [tables(plans[p], caps[p], 0, dev, SECTION) for p in range(P)]
        sections = [dict(cap=caps[p], **{name: sec[p][name].data_ptr() for name in SECTION}) for p in range(P)]
        lib.wire_regroup_shapes(plans, sections, G, 1, N, recs.data_ptr(), S,
                                *(win[name].data_ptr() for name in ("shape_of", "rank_of", "anchor_of", "counts",
                                                                    "slot_of")), st)
        torch.cuda.synchronize(dev)
        counts = [int(c) for c in win["counts"].cpu().numpy().view(np.uint32)]
        assert counts == [len(gs) for gs in groups_of], counts
        # outputs: the per-shape calls' own arrays (cap rows each), the window call's dense arrays
        dec = {v: [decode_out(caps[p], dev) for p in range(P)] for v in ("per_shape_counts", "per_shape_cap")}
        dense = {v: decode_out(sum(caps), dev) for v in ("shapes_counts", "shapes_cap")}
        ws = torch.empty(max(16, lib.workspace_size(plans[1], caps[1])), dtype=torch.uint8, device=dev)
        pa = (rfec_plan * P)(*(as_plan(p) for p in plans))
        sa = (rfec_regroup_section * P)(*(rfec_regroup_section(**s) for s in sections))
        ga = (C.c_uint32 * P)(*counts)
        raw = lib.lib

        def per_shape(rows_of, d):
            def run():
                for p in range(P):
                    a = (C.byref(pa[p]), rows_of[p], STRIDE, S, payload.data_ptr(), N,
                         *(sec[p][name].data_ptr() for name in DECODE_IN), d[p]["recovered"].data_ptr(), E,
                         d[p]["out_shards"].data_ptr(), d[p]["out_hdr"].data_ptr(), d[p]["out_index"].data_ptr())
                    r = raw.rfec_recover_indexed_matrix_out(*a, st) if matrix[p] else \
                        raw.rfec_recover_indexed_out(*a, ws.data_ptr(), st)
                    assert r == 0, raw.rfec_last_error()
            return run

        def shapes(groups, d):
            def run():
                r = raw.rfec_recover_indexed_shapes_out(pa, P, sa, groups, STRIDE, S, payload.data_ptr(), N,
                                                        d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                                        d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), st)
                assert r == 0, raw.rfec_last_error()
            return run

        variants = {"per_shape_counts": per_shape(counts, dec["per_shape_counts"]),
                    "shapes_counts": shapes(ga, dense["shapes_counts"]),
                    "per_shape_cap": per_shape(caps, dec["per_shape_cap"]),
                    "shapes_cap": shapes(None, dense["shapes_cap"])}
        for f in variants.values():
            f()
        torch.cuda.synchronize(dev)
        # the outputs, before anything is timed: every variant's rows [0, counts[p]) of section p against
        # per_shape_counts', and the rows past counts[p] of the cap variants hold nothing
        equal, recovered = True, 0
        first = {"shapes_counts": np.concatenate([[0], np.cumsum(counts)]),
                 "shapes_cap": np.concatenate([[0], np.cumsum(caps)])}
        for p in range(P):
            c = counts[p]
            a = {name: t[:c] for name, t in dec["per_shape_counts"][p].items()}
            ok = a["out_index"] != 0xFF
            recovered += int(ok.sum())
            others = [{name: t[:caps[p]] for name, t in dec["per_shape_cap"][p].items()}]
            for v in ("shapes_counts", "shapes_cap"):
                lo = int(first[v][p])
                hi = lo + (c if v == "shapes_counts" else caps[p])
                others.append({name: t[lo:hi] for name, t in dense[v].items()})
            for b in others:
                equal &= bool(torch.equal(a["recovered"], b["recovered"][:c]) and
                              torch.equal(a["out_index"], b["out_index"][:c]) and
                              torch.equal(a["out_hdr"][ok], b["out_hdr"][:c][ok]) and
                              torch.equal(a["out_shards"][ok][:, :16 * cd], b["out_shards"][:c][ok][:, :16 * cd]))
                equal &= bool((b["out_index"][c:] == 0xFF).all()) and not bool(b["recovered"][c:].any())
        rc |= 0 if equal and recovered else 1

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

        line = {"groups": G, "shapes": [list(s[:3]) + [plans[p].n_lines] for p, s in enumerate(SHAPES)],
                "counts": counts, "caps": caps, "S": S, "stride": STRIDE, "records": N, "per_group": E,
                "arrival": order, "steps": steps,
                "timing": "stream events around each variant's calls, variants alternating",
                "outputs_equal": bool(equal), "recovered_segments": recovered,
                **{v: stat(t) for v, t in us.items()}}
        for s in ("counts", "cap"):
            new, old = us[f"shapes_{s}"], us[f"per_shape_{s}"]
            line[f"shapes_over_per_shape_{s}"] = round(float(new.mean() / old.mean()), 4)
            line[f"shapes_p95_below_per_shape_p05_{s}"] = bool(np.percentile(new, 95) < np.percentile(old, 5))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec, dec, dense, win, ws
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
