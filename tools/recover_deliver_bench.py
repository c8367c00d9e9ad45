#!/usr/bin/env python3
"""rfec_recover_deliver on one GPU: the last stage of a closed window's receive
chain, the decode's dense outputs as a list of delivered segments in window
order, against the streaming floor and against the host round trip it replaces.

Stream: tools/recover_shapes_bench.py's (a window of --groups groups of four
shapes, 1,200-B segments in 1,216-B rows, two segments of every group lost; send
order or shuffled), parsed once, regrouped once by rfec_wire_regroup_shapes and
decoded by rfec_recover_indexed_shapes_out with groups = counts.

Stream events around each (the device's time):
    deliver        rfec_recover_deliver with max_out = the delivered segments T
    decode         the rfec_recover_indexed_shapes_out in front of it
    copy           rfec_probe_copy of T x 16 CD bytes, non-temporal: the streaming floor
Wall clock from a drained stream to a drained stream (host work is part of these):
    host_runs      what a caller did without the call: D2H of out_index, out_hdr, shape_of and rank_of into pinned
                   memory, a synchronise, a host-built slot list (numpy), then one D2H per run of adjacent delivered
                   slots
    host_whole     the same with one D2H of the whole out_shards in place of the runs
    deliver_d2h    rfec_recover_deliver, then one D2H of seg and seg_payload (max_out entries) and n_out

deliver's list is compared with the host route's before anything is timed (exit status 1 where they differ).  The
variants alternate step by step, each over enough steps of its own for --min-ms (default 250) of timed work; mean /
p05 / p95 per variant.  One JSON object per arrival order on stdout.

    python tools/recover_deliver_bench.py [--groups 65535] [--orders send,shuffled] [--min-ms 250] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from razor_amd.fec import as_plan, native, rfec_plan, rfec_regroup_section  # noqa: E402
from regroup_shapes_bench import E, S, SECTION, SHAPES, STRIDE, build_stream, decode_out, tables  # noqa: E402


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
        raise SystemExit("recover_deliver_bench.py: needs a GPU")
    if not 4 <= args.groups <= 65535:
        raise SystemExit("recover_deliver_bench.py: one window holds 4 .. 65,535 groups")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    raw = lib.lib
    plans = [lib.plan_matrix(*s) for s in SHAPES]
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
        R = sum(counts)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        d = decode_out(R, dev)
        pa = (rfec_plan * P)(*(as_plan(p) for p in plans))
        sa = (rfec_regroup_section * P)(*(rfec_regroup_section(**s) for s in sections))
        ga = (C.c_uint32 * P)(*counts)

        def decode():
            r = raw.rfec_recover_indexed_shapes_out(pa, P, sa, ga, STRIDE, S, payload.data_ptr(), N,
                                                    d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                                    d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), st)
            assert r == 0, raw.rfec_last_error()

        decode()
        torch.cuda.synchronize(dev)
        T = int((d["out_index"] != 0xFF).sum())
        max_out = T
        seg = torch.zeros((max_out, 24), dtype=torch.uint8, device=dev)
        segp = torch.zeros((max_out, STRIDE), dtype=torch.uint8, device=dev)
        first_of = torch.zeros(G + 1, dtype=torch.int32, device=dev)
        n_out = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(16, lib.recover_deliver_workspace_size(G)), dtype=torch.uint8, device=dev)

        def deliver():
            r = raw.rfec_recover_deliver(pa, P, sa, ga, G, 1, win["shape_of"].data_ptr(), win["rank_of"].data_ptr(),
                                         STRIDE, S, E, d["out_shards"].data_ptr(), d["out_hdr"].data_ptr(),
                                         d["out_index"].data_ptr(), max_out, seg.data_ptr(), segp.data_ptr(),
                                         first_of.data_ptr(), n_out.data_ptr(), ws.data_ptr(), st)
            assert r == 0, raw.rfec_last_error()

        row_bytes = max(16, T * 16 * cd)
        cp_src = torch.empty(row_bytes, dtype=torch.uint8, device=dev)
        cp_dst = torch.empty_like(cp_src)

        def copy():
            if raw.rfec_probe_copy(cp_src.data_ptr(), cp_dst.data_ptr(), row_bytes, 1, st):
                raise RuntimeError("rfec_probe_copy failed")

        pin = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt).pin_memory()  # noqa: E731
        h_ix, h_hd = pin(R, E), pin(R, E, 20)
        h_shape, h_rank = pin(G), pin(G, dt=torch.int32)
        h_rows, h_all = pin(max(T, 1), STRIDE), pin(R, E, STRIDE)
        h_seg, h_segp, h_n = pin(max_out, 24), pin(max_out, STRIDE), pin(1, dt=torch.int32)
        flat = d["out_shards"].view(R * E, STRIDE)
        first_t = first

        def slot_list():
            """The delivered out slots in window order, from the tables on the host."""
            p = h_shape.numpy().astype(np.int64)
            c = h_rank.numpy().view(np.uint32).astype(np.int64)
            ok = p < P
            pp = np.where(ok, p, 0)
            rows = np.array(counts, np.int64)
            dec = ok & (c < rows[pp])
            o = (first_t[pp] + c)[dec]
            hit = h_ix.numpy()[o] != 0xFF
            return (o[:, None] * E + np.arange(E)[None, :])[hit]

        def host(whole):
            def run():
                h_ix.copy_(d["out_index"], non_blocking=True)
                h_hd.copy_(d["out_hdr"], non_blocking=True)
                h_shape.copy_(win["shape_of"], non_blocking=True)
                h_rank.copy_(win["rank_of"], non_blocking=True)
                stream.synchronize()
                slots = slot_list()
                if whole:
                    h_all.copy_(d["out_shards"], non_blocking=True)
                elif len(slots):
                    cut = np.nonzero(np.diff(slots) != 1)[0] + 1
                    a = np.concatenate([[0], cut])
                    b = np.concatenate([cut, [len(slots)]])
                    for j0, j1 in zip(a.tolist(), b.tolist()):
                        s0 = int(slots[j0])
                        h_rows[j0:j1].copy_(flat[s0:s0 + (j1 - j0)], non_blocking=True)
                stream.synchronize()
                return slots
            return run

        def deliver_d2h():
            deliver()
            h_seg.copy_(seg, non_blocking=True)
            h_segp.copy_(segp, non_blocking=True)
            h_n.copy_(n_out, non_blocking=True)
            stream.synchronize()

        # the outputs, before anything is timed
        deliver()
        slots = host(False)()
        deliver_d2h()
        equal = int(h_n[0]) == T == len(slots)
        if equal and T:
            sl = torch.from_numpy(slots).to(dev)
            equal &= bool(torch.equal(segp[:, :16 * cd], flat[sl][:, :16 * cd]))
            equal &= bool(torch.equal(seg[:, :20], d["out_hdr"].view(R * E, 20)[sl]))
            equal &= bool(torch.equal(h_rows[:T, :16 * cd], h_segp[:, :16 * cd]))
            runs = int((np.diff(slots) != 1).sum()) + 1
        else:
            runs = 0
        rc |= 0 if equal and T else 1

        events = {"deliver": deliver, "decode": decode, "copy": copy}
        walls = {"host_runs": host(False), "host_whole": host(True), "deliver_d2h": deliver_d2h}
        names = list(events) + list(walls)

        def run(steps):
            """steps: per variant; a variant that has had its steps sits the later ones out."""
            ev = {v: [] for v in events}
            wall = {v: [] for v in walls}
            for step in range(max(steps.values())):
                for v in names[step % len(names):] + names[:step % len(names)]:
                    if step >= steps[v]:
                        continue
                    if v in events:
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        events[v]()
                        b.record(stream)
                        ev[v].append((a, b))
                    else:
                        stream.synchronize()
                        t0 = time.perf_counter()
                        walls[v]()
                        wall[v].append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize(dev)
            out = {v: np.array([a.elapsed_time(b) for a, b in e]) * 1e3 for v, e in ev.items()}
            out.update({v: np.array(t) for v, t in wall.items()})
            return out

        est = {v: t[-3:] for v, t in run({v: args.warmup + 3 for v in names}).items()}
        steps = {v: args.steps or min(20000, max(10, int(math.ceil(args.min_ms * 1e3 / float(est[v].mean())))))
                 for v in names}
        us = run(steps)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "p05_us": round(float(np.percentile(t, 5)), 2),
                    "p95_us": round(float(np.percentile(t, 95)), 2), "median_us": round(float(np.median(t)), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        best = "host_runs" if us["host_runs"].mean() <= us["host_whole"].mean() else "host_whole"
        faster = bool(np.percentile(us["deliver_d2h"], 95) < np.percentile(us[best], 5))
        line = {"groups": G, "counts": counts, "S": S, "stride": STRIDE, "records": N, "per_group": E, "arrival": order,
                "steps": steps, "delivered": T, "delivered_bytes": T * 16 * cd, "runs_of_adjacent_slots": runs,
                "launches": 2 if G <= 256 else 3, "outputs_equal": bool(equal),
                "timing": "deliver, decode, copy: stream events; host_*, deliver_d2h: wall clock between drained "
                          "streams; variants alternating",
                **{v: stat(t) for v, t in us.items()},
                "deliver_over_copy": round(float(us["deliver"].mean() / us["copy"].mean()), 3),
                "deliver_over_decode": round(float(us["deliver"].mean() / us["decode"].mean()), 3),
                "host_route_used": best,
                "deliver_d2h_over_host_route": round(float(us["deliver_d2h"].mean() / us[best].mean()), 4),
                "deliver_d2h_p95_below_host_route_p05": faster,
                "verdict": "faster" if faster else "not faster"}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del recs, payload, sec, d, win, ws, seg, segp, cp_src, cp_dst, h_all, h_rows, h_segp
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
