#!/usr/bin/env python3
"""rfec_recover_indexed_window_out on one GPU: the decode behind one
rfec_wire_regroup_shapes over a video-like window, one launch for the window
against the best chain without the call.

Stream: tools/regroup_shapes_bench.py's builder over a video-like mix -- shape
p = g mod 5 of rows 1 x 3, the (10, 3, 4) rows + columns plan, rows 1 x 10 and
1 x 30 (strip-mode frames) and the planner's k = 40 matrix (6 x 7); 1,200-B segments in
1,216-B rows; two segments of every group lost; send order or shuffled --
parsed once and regrouped once by rfec_wire_regroup_shapes into sections of
cap = min(groups, 2 counts[p]) rows.  The families: 1 x 3 is a compiled row
layout (2), (10, 3, 4) a compiled matrix (1), k = 40 a wide matrix (3), 1 x 10
and 1 x 30 wide rows (4).

    chain_counts    the best chain without the new call, on the same tables and into the same dense layout: one
                    rfec_recover_indexed_shapes_out for the family-1 and family-2 sections (groups 0 for the others),
                    one rfec_recover_indexed_rows_wide_out per wide row section and one
                    rfec_recover_indexed_matrix_wide_out for the wide matrix, their outputs at first[p] -- four
                    launches, over counts[p] rows
    chain_cap       the same over cap rows (a receiver that did not read the counts back)
    window_counts   one rfec_recover_indexed_window_out with groups = counts
    window_cap      one rfec_recover_indexed_window_out with groups = NULL (cap)

Every variant's outputs are compared with chain_counts' before anything is timed (exit status 1 where they differ).
All calls go through prebuilt ctypes arguments.  The variants alternate step by step, each bracketed by stream
events around its calls, over enough steps for --min-ms (default 250) of timed work each; mean / std / p05 / p95 per
variant.  One JSON object per arrival order on stdout.

    python tools/recover_window_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--steps 0]
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

from razor_amd.fec import RFEC_LAYER_COLS, RFEC_LAYER_ROWS, as_plan, native, rfec_plan, rfec_regroup_section  # noqa: E402
from regroup_shapes_bench import DECODE_IN, E, S, SECTION, STRIDE, build_stream, decode_out, tables  # noqa: E402

FAMILY = (2, 1, 4, 4, 3)  # (the compiled families first: the chain's one shapes call covers a prefix of the rows)


def mix(lib):
    return [lib.plan_matrix(3, 1, 3, RFEC_LAYER_ROWS), lib.plan_matrix(10, 3, 4, RFEC_LAYER_ROWS | RFEC_LAYER_COLS),
            lib.plan_matrix(10, 1, 10, RFEC_LAYER_ROWS), lib.plan_matrix(30, 1, 30, RFEC_LAYER_ROWS),
            lib.plan_from_fraction(40, 80)]


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
        raise SystemExit("recover_window_bench.py: needs a GPU")
    if not 5 <= args.groups <= 65535:
        raise SystemExit("recover_window_bench.py: one window holds 5 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    raw = lib.lib
    raw.rfec_recover_window_family.restype, raw.rfec_recover_window_family.argtypes = C.c_int, [C.c_void_p]
    plans = mix(lib)
    assert tuple(int(raw.rfec_recover_window_family(C.byref(as_plan(p)))) for p in plans) == FAMILY
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
        rows_of = {"counts": counts, "cap": caps}
        first = {s: np.concatenate([[0], np.cumsum(r)]).astype(int) for s, r in rows_of.items()}
        dense = {f"{v}_{s}": decode_out(int(first[s][P]), dev) for v in ("chain", "window") for s in rows_of}
        pa = (rfec_plan * P)(*(as_plan(p) for p in plans))
        sa = (rfec_regroup_section * P)(*(rfec_regroup_section(**s) for s in sections))
        ga = {"counts": (C.c_uint32 * P)(*counts), "cap": None}
        # the chain's shapes call: the compiled families' sections alone, the others left out (groups 0)
        compiled = {s: (C.c_uint32 * P)(*(r if FAMILY[p] <= 2 else 0 for p, r in enumerate(rows_of[s])))
                    for s in rows_of}

        def ptrs(d, o=0):
            return (d["recovered"].data_ptr() + 16 * o, E, d["out_shards"].data_ptr() + o * E * STRIDE,
                    d["out_hdr"].data_ptr() + o * E * 20, d["out_index"].data_ptr() + o * E)

        def chain(s, d):
            def run():
                # (the compiled sections come first in the mix, so the rows the shapes call numbers densely over
                # them are first[p] of the window's numbering too)
                r = raw.rfec_recover_indexed_shapes_out(pa, P, sa, compiled[s], STRIDE, S, payload.data_ptr(), N,
                                                        *ptrs(d), st)
                assert r == 0, raw.rfec_last_error()
                for p in range(P):
                    if FAMILY[p] <= 2:
                        continue
                    a = (C.byref(pa[p]), rows_of[s][p], STRIDE, S, payload.data_ptr(), N,
                         *(sec[p][name].data_ptr() for name in DECODE_IN), *ptrs(d, int(first[s][p])))
                    r = raw.rfec_recover_indexed_matrix_wide_out(*a, st) if FAMILY[p] == 3 else \
                        raw.rfec_recover_indexed_rows_wide_out(*a, st)
                    assert r == 0, raw.rfec_last_error()
            return run

        def window(s, d):
            def run():
                r = raw.rfec_recover_indexed_window_out(pa, P, sa, ga[s], STRIDE, S, payload.data_ptr(), N, *ptrs(d),
                                                        st)
                assert r == 0, raw.rfec_last_error()
            return run

        variants = {"chain_counts": chain("counts", dense["chain_counts"]),
                    "window_counts": window("counts", dense["window_counts"]),
                    "chain_cap": chain("cap", dense["chain_cap"]),
                    "window_cap": window("cap", dense["window_cap"])}
        for f in variants.values():
            f()
        torch.cuda.synchronize(dev)
        # the outputs, before anything is timed: every variant's rows [0, counts[p]) of section p against
        # chain_counts', and the rows past counts[p] of the cap variants hold nothing
        equal, recovered = True, 0
        for p in range(P):
            c = counts[p]
            lo = int(first["counts"][p])
            a = {name: t[lo:lo + c] for name, t in dense["chain_counts"].items()}
            ok = a["out_index"] != 0xFF
            recovered += int(ok.sum())
            for v in ("window_counts", "chain_cap", "window_cap"):
                s = v.split("_")[1]
                lo, n = int(first[s][p]), rows_of[s][p]
                b = {name: t[lo:lo + n] for name, t in dense[v].items()}
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

        line = {"groups": G, "shapes": [[p.k, p.n_lines, f] for p, f in zip(plans, FAMILY)],
                "counts": counts, "caps": caps, "S": S, "stride": STRIDE, "records": N, "per_group": E,
                "arrival": order, "steps": steps, "chain_launches": 1 + sum(f > 2 for f in FAMILY),
                "timing": "stream events around each variant's calls, variants alternating",
                "outputs_equal": bool(equal), "recovered_segments": recovered,
                **{v: stat(t) for v, t in us.items()}}
        for s in ("counts", "cap"):
            new, old = us[f"window_{s}"], us[f"chain_{s}"]
            line[f"window_over_chain_{s}"] = round(float(new.mean() / old.mean()), 4)
            line[f"window_p95_below_chain_p05_{s}"] = bool(np.percentile(new, 95) < np.percentile(old, 5))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec, dense, win
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
