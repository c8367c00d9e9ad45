#!/usr/bin/env python3
"""A/B on one GPU: a batch of device-resident groups into SIM_FEC datagrams by
the two calls (rfec_encode_batch, then rfec_wire_frame_fec: the parities go
through HBM) against the fused call (rfec_wire_encode_fec,
k_encode_frame_fec_q), alternating step by step on the same inputs.  Shapes:
c3 (65,536 groups, k = 10, 3 row lines, 1,200 B in 1,216-B payload slots,
1,280-B datagram slots), c3full (the sender's 3 x 4 plan, 7 lines), c5 (k = 32,
8 rows of 4, 256 B, 320-B datagram slots).  The outputs are compared first;
times are the kernels' own start / stop (HIP events bound to the launch,
rfec_timing_events), the two kernels summed against the one.  Bytes are from
the shapes: the fused kernel reads every member once per line it sits on and
writes the datagram slots; the two calls also write and re-read the parity
slots.  One JSON object per shape and pass on stdout.

    python tools/wire_encode_ab.py [--passes 3] [--steps 1500] [--warmup 20] [--groups 65536] [--shapes c3,c3full,c5]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from razor_amd.fec import Native, native  # noqa: E402

SHAPES = {  # k, S, payload stride, datagram stride, plan
    "c3": dict(k=10, S=1200, stride=1216, dstride=1280, plan=lambda lib: lib.plan_from_fraction(10, 80, 1), cfg=2),
    "c3full": dict(k=10, S=1200, stride=1216, dstride=1280, plan=lambda lib: lib.plan_from_fraction(10, 80, 3),
                   cfg=3),
    "c5": dict(k=32, S=256, stride=256, dstride=320, plan=lambda lib: lib.plan_matrix(32, 8, 4, 1), cfg=5),
}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--shapes", default="c3,c3full,c5")
    ap.add_argument("--lib", default=None, help="another build of librazor_fec_v1200.so (kernel variants)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wire_encode_ab.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = Native(1200, path=args.lib) if args.lib else native(1200)
    G = args.groups
    rc = 0
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        k, S, P, D = sh["k"], sh["S"], sh["stride"], sh["dstride"]
        plan = sh["plan"](lib)
        n = plan.n_lines
        NF = G * n
        members = sum(plan.line[l].count for l in range(n))
        shards = torch.empty((G, k, P), dtype=torch.uint8, device=dev)
        lib.fill_xorshift(shards.data_ptr(), sh["cfg"], 0, G, k, S, P, st)
        hdr_np = bench.make_headers(G, k, S, 0)
        hdr = torch.from_numpy(hdr_np.view(np.uint8).reshape(G, k, 20).copy()).to(dev)
        fst, _ = bench.wire_stamps(hdr_np, plan, n)
        stamps = torch.from_numpy(fst.view(np.uint8).copy()).to(dev)
        parity = torch.empty((NF, P), dtype=torch.uint8, device=dev)
        meta = torch.empty((NF, 20), dtype=torch.uint8, device=dev)
        fsize = torch.empty((NF,), dtype=torch.int16, device=dev)
        status = torch.empty((NF,), dtype=torch.int8, device=dev)
        out = {v: (torch.full((NF, D), 0xEE, dtype=torch.uint8, device=dev),
                   torch.full((NF,), 0x7777, dtype=torch.int16, device=dev)) for v in ("two", "fused")}

        def encode():
            lib.encode_batch(plan, G, P, S, shards.data_ptr(), hdr.data_ptr(), parity.data_ptr(), meta.data_ptr(),
                             fsize.data_ptr(), status.data_ptr(), st)

        def frame():
            lib.wire_frame_fec(NF, P, S, parity.data_ptr(), meta.data_ptr(), fsize.data_ptr(), status.data_ptr(),
                               stamps.data_ptr(), D, out["two"][0].data_ptr(), out["two"][1].data_ptr(), st)

        def fused():
            lib.wire_encode_fec(plan, G, P, S, shards.data_ptr(), hdr.data_ptr(), stamps.data_ptr(), D,
                                out["fused"][0].data_ptr(), out["fused"][1].data_ptr(), st)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            b.record(stream)
            lib.timing_events(a.cuda_event, b.cuda_event)
            fn()
            assert lib.timing_launches() == 1
            return a, b

        encode(), frame(), fused()
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(out["two"][0], out["fused"][0]) and torch.equal(out["two"][1], out["fused"][1]))
        live = int((out["fused"][1] != 0).sum())
        rc |= 0 if same and live == NF else 1
        b_fused = G * members * S + NF * D
        b_two = G * (members + n) * S + NF * S + NF * D
        for p in range(args.passes):
            ev = {"encode": [], "frame": [], "fused": []}
            for step in range(args.warmup + args.steps):
                for v in (("two", "fused") if step & 1 else ("fused", "two")):
                    es = [("encode", timed(encode)), ("frame", timed(frame))] if v == "two" else \
                        [("fused", timed(fused))]
                    if step >= args.warmup:
                        for key, e in es:
                            ev[key].append(e)
            torch.cuda.synchronize(dev)
            us = {key: np.array([a.elapsed_time(b) for a, b in v]) * 1e3 for key, v in ev.items()}
            two = us["encode"] + us["frame"]

            def stat(t):
                return {"mean_us": round(float(t.mean()), 2), "median_us": round(float(np.median(t)), 2),
                        "min_us": round(float(t.min()), 2)}

            print(json.dumps({
                "shape": name, "pass": p, "groups": G, "k": k, "lines": n, "members_per_group": members, "S": S,
                "stride": P, "dstride": D, "steps": args.steps,
                "timing": "the kernels' own start / stop (rfec_timing_events)",
                "encode": stat(us["encode"]), "frame_fec": stat(us["frame"]), "two_calls": stat(two),
                "fused": dict(stat(us["fused"]), bytes=b_fused,
                              frac_of_8TBps=round(b_fused / (float(us["fused"].mean()) * 1e-6) / 1e9
                                                  / bench.HBM_PEAK_GBPS, 4)),
                "timed_ms": {"two_calls": round(float(two.sum()) * 1e-3, 1),
                             "fused": round(float(us["fused"].sum()) * 1e-3, 1)},
                "fused_over_two_calls": round(float(us["fused"].mean() / two.mean()), 4),
                "traffic_ratio_from_shapes": round(b_fused / b_two, 4),
                "outputs_equal": same, "datagrams_emitted": live}), flush=True)
        del shards, parity, out
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
