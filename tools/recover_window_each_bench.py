#!/usr/bin/env python3
"""rfec_recover_indexed_window_each_out and rfec_recover_deliver_each on one GPU:
what the per-section out-slot counts cost at a uniform per_group, and one launch
at mixed per_group against what the entries before it offer for the same slots.

Stream: tools/recover_window_bench.py's -- the video-like mix, shape p = g mod 5
of rows 1 x 3, the (10, 3, 4) rows + columns plan, rows 1 x 10 and 1 x 30 and the
planner's k = 40 matrix; 1,200-B segments in 1,216-B rows; two segments of every
group lost; send order or shuffled -- parsed once and regrouped once by
rfec_wire_regroup_shapes; groups = counts[p] everywhere.

    window_uniform   one rfec_recover_indexed_window_out at per_group 2
    each_uniform     one rfec_recover_indexed_window_each_out at per_group (2, 2, 2, 2, 2): the same tables, the same
                     bytes out -- what the per-section fields cost
    each_mixed       one rfec_recover_indexed_window_each_out at per_group min(k, 10) = (3, 10, 10, 10, 10)
    singles_mixed    what the entries before it offer for those slots: one single-shape call per section with its own
                     per_group into arrays of its own -- five launches
    deliver          rfec_recover_deliver over window_uniform's outputs
    deliver_each     rfec_recover_deliver_each over each_uniform's outputs at per_group (2, 2, 2, 2, 2)

Before anything is timed each_uniform's four arrays are compared with window_uniform's byte for byte, each_mixed's
sections with singles_mixed's arrays byte for byte, and deliver_each's outputs with deliver's (exit status 1 where
they differ).  All calls go through prebuilt ctypes arguments.  The variants alternate step by step, each bracketed
by stream events around its calls, over enough steps for --min-ms (default 250) of timed work each; mean / std /
p05 / p95 per variant.  One JSON object per arrival order on stdout.

    python tools/recover_window_each_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--steps 0]
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

from razor_amd.fec import as_plan, native, rfec_plan, rfec_regroup_section, window_first_slots  # noqa: E402
from recover_window_bench import FAMILY, mix  # noqa: E402
from regroup_shapes_bench import DECODE_IN, E, S, SECTION, STRIDE, build_stream, tables  # noqa: E402

PAIRS = (("each_uniform", "window_uniform"), ("each_mixed", "singles_mixed"), ("deliver_each", "deliver"))


def ragged_out(rows, slots, dev):
    return dict(recovered=torch.zeros((rows, 2), dtype=torch.int64, device=dev),
                out_shards=torch.zeros((slots, STRIDE), dtype=torch.uint8, device=dev),
                out_hdr=torch.zeros((slots, 20), dtype=torch.uint8, device=dev),
                out_index=torch.full((slots,), 0x3C, dtype=torch.uint8, device=dev))


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
        raise SystemExit("recover_window_each_bench.py: needs a GPU")
    if not 5 <= args.groups <= 65535:
        raise SystemExit("recover_window_each_bench.py: one window holds 5 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    raw = lib.lib
    plans = mix(lib)
    P, G = len(plans), args.groups
    cd = (S + 15) // 16
    mixed = [min(p.k, 10) for p in plans]
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
        pa = (rfec_plan * P)(*(as_plan(p) for p in plans))
        sa = (rfec_regroup_section * P)(*(rfec_regroup_section(**s) for s in sections))
        ga = (C.c_uint32 * P)(*counts)
        e_uni, e_mix = (C.c_uint32 * P)(*[E] * P), (C.c_uint32 * P)(*mixed)
        first, slots_uni = window_first_slots(counts, [E] * P)
        _, slots_mix = window_first_slots(counts, mixed)
        R = first[P]
        assert lib.recover_window_slots(sections, counts, mixed) == slots_mix[P] and slots_uni[P] == R * E
        out = {"window_uniform": ragged_out(R, R * E, dev), "each_uniform": ragged_out(R, R * E, dev),
               "each_mixed": ragged_out(R, slots_mix[P], dev)}
        single = [ragged_out(counts[p], counts[p] * mixed[p], dev) for p in range(P)]
        ws = [torch.zeros(max(16, lib.workspace_size(plans[p], counts[p])), dtype=torch.uint8, device=dev)
              if FAMILY[p] == 2 else None for p in range(P)]

        def ptrs(d, per_group):
            return (d["recovered"].data_ptr(), per_group, d["out_shards"].data_ptr(), d["out_hdr"].data_ptr(),
                    d["out_index"].data_ptr())

        def window_uniform():
            r = raw.rfec_recover_indexed_window_out(pa, P, sa, ga, STRIDE, S, payload.data_ptr(), N,
                                                    *ptrs(out["window_uniform"], E), st)
            assert r == 0, raw.rfec_last_error()

        def each(name, ea):
            def run():
                r = raw.rfec_recover_indexed_window_each_out(pa, P, sa, ga, STRIDE, S, payload.data_ptr(), N,
                                                             *ptrs(out[name], ea), st)
                assert r == 0, raw.rfec_last_error()
            return run

        def singles_mixed():
            for p in range(P):
                a = (C.byref(pa[p]), counts[p], STRIDE, S, payload.data_ptr(), N,
                     *(sec[p][name].data_ptr() for name in DECODE_IN), *ptrs(single[p], mixed[p]))
                f = FAMILY[p]
                r = raw.rfec_recover_indexed_matrix_out(*a, st) if f == 1 else \
                    raw.rfec_recover_indexed_out(*a, ws[p].data_ptr(), st) if f == 2 else \
                    raw.rfec_recover_indexed_matrix_wide_out(*a, st) if f == 3 else \
                    raw.rfec_recover_indexed_rows_wide_out(*a, st)
                assert r == 0, raw.rfec_last_error()

        max_out = 2 * G
        dl = {v: dict(seg=torch.full((max_out, 24), 0x5A, dtype=torch.uint8, device=dev),
                      pay=torch.full((max_out, STRIDE), 0x5A, dtype=torch.uint8, device=dev),
                      first_of=torch.zeros(G + 1, dtype=torch.int32, device=dev),
                      n_out=torch.zeros(1, dtype=torch.int32, device=dev),
                      ws=torch.zeros(lib.recover_deliver_workspace_size(G), dtype=torch.uint8, device=dev))
              for v in ("deliver", "deliver_each")}

        def deliver(name, fn, src, per_group):
            d, o = dl[name], out[src]

            def run():
                r = fn(pa, P, sa, ga, G, 1, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(), STRIDE, S,
                       per_group, o["out_shards"].data_ptr(), o["out_hdr"].data_ptr(), o["out_index"].data_ptr(),
                       max_out, d["seg"].data_ptr(), d["pay"].data_ptr(), d["first_of"].data_ptr(),
                       d["n_out"].data_ptr(), d["ws"].data_ptr(), st)
                assert r == 0, raw.rfec_last_error()
            return run

        variants = {"window_uniform": window_uniform, "each_uniform": each("each_uniform", e_uni),
                    "each_mixed": each("each_mixed", e_mix), "singles_mixed": singles_mixed,
                    "deliver": deliver("deliver", raw.rfec_recover_deliver, "window_uniform", E),
                    "deliver_each": deliver("deliver_each", raw.rfec_recover_deliver_each, "each_uniform", e_uni)}
        for f in variants.values():
            f()
        torch.cuda.synchronize(dev)
        # the outputs, before anything is timed
        a, b = out["window_uniform"], out["each_uniform"]
        equal = all(torch.equal(a[name], b[name]) for name in a)
        recovered = int((a["out_index"] != 0xFF).sum())
        mixed_recovered = 0
        for p in range(P):
            lo, hi = slots_mix[p], slots_mix[p + 1]
            s, m = single[p], out["each_mixed"]
            ok = s["out_index"] != 0xFF
            mixed_recovered += int(ok.sum())
            equal &= bool(torch.equal(s["recovered"], m["recovered"][first[p]:first[p + 1]]) and
                          torch.equal(s["out_index"], m["out_index"][lo:hi]) and
                          torch.equal(s["out_hdr"][ok], m["out_hdr"][lo:hi][ok]) and
                          torch.equal(s["out_shards"][ok][:, :16 * cd], m["out_shards"][lo:hi][ok][:, :16 * cd]))
        equal &= all(torch.equal(dl["deliver"][name], dl["deliver_each"][name])
                     for name in ("seg", "pay", "first_of", "n_out"))
        delivered = int(dl["deliver_each"]["n_out"].cpu().numpy().view(np.uint32)[0])
        rc |= 0 if equal and recovered and delivered == recovered and mixed_recovered >= recovered else 1

        def run(steps, keep):
            ev = {v: [] for v in variants}
            names = list(variants)
            for step in range(steps):
                for v in names[step % len(names):] + names[:step % len(names)]:
                    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    x.record(stream)
                    variants[v]()
                    y.record(stream)
                    ev[v].append((x, y))
            torch.cuda.synchronize(dev)
            return {v: np.array([x.elapsed_time(y) for x, y in e][-keep:]) * 1e3 for v, e in ev.items()}

        est = run(args.warmup + 3, 3)
        steps = args.steps or max(10, int(math.ceil(args.min_ms * 1e3 / min(float(t.mean()) for t in est.values()))))
        us = run(steps, steps)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "std_us": round(float(t.std()), 2),
                    "p05_us": round(float(np.percentile(t, 5)), 2), "p95_us": round(float(np.percentile(t, 95)), 2),
                    "median_us": round(float(np.median(t)), 2), "min_us": round(float(t.min()), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        line = {"groups": G, "shapes": [[p.k, p.n_lines, f] for p, f in zip(plans, FAMILY)], "counts": counts,
                "S": S, "stride": STRIDE, "records": N, "uniform_per_group": E, "mixed_per_group": mixed,
                "uniform_slots": R * E, "mixed_slots": slots_mix[P], "arrival": order, "steps": steps,
                "timing": "stream events around each variant's calls, variants alternating",
                "outputs_equal": bool(equal), "recovered_segments": recovered, "delivered": delivered,
                **{v: stat(t) for v, t in us.items()}}
        for new, old in PAIRS:
            line[f"{new}_over_{old}"] = round(float(us[new].mean() / us[old].mean()), 4)
            line[f"{new}_p95_below_{old}_p05"] = bool(np.percentile(us[new], 95) < np.percentile(us[old], 5))
            line[f"{old}_p95_below_{new}_p05"] = bool(np.percentile(us[old], 95) < np.percentile(us[new], 5))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec, out, single, dl, win
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
