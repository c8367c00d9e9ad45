#!/usr/bin/env python3
"""A/B on one GPU: every datagram of a batch of device-resident groups -- the
G k SIM_SEG and the G n SIM_FEC -- by the two calls (rfec_wire_frame_seg, then
rfec_wire_encode_fec: the members stream out of HBM twice) against the fused
call (rfec_wire_encode_send, k_encode_send_q), alternating step by step on the
same inputs.  Shapes as tools/wire_encode_ab.py: c3 (65,536 groups, k = 10, 3
row lines, 1,200 B in 1,216-B payload slots, 1,280-B datagram slots), c3full
(the sender's 3 x 4 plan, 7 lines), c5 (k = 32, 8 rows of 4, 256 B, 320-B
datagram slots).  The outputs are compared first; times are the kernels' own
start / stop (HIP events bound to the launch, rfec_timing_events), the two
kernels summed against the one.  Bytes are from the shapes, in slots: the fused
kernel reads every member's payload slot once per line it sits on (at least
once) and writes the G (k + n) datagram slots; the two calls read every member
once more.  One JSON object per shape and pass on stdout.

    python tools/wire_send_ab.py [--passes 3] [--steps 1200] [--warmup 20] [--groups 65536] [--shapes c3,c3full,c5]
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
from wire_encode_ab import SHAPES  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--shapes", default="c3,c3full,c5")
    ap.add_argument("--lib", default=None, help="another build of librazor_fec_v1200.so (kernel variants)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wire_send_ab.py: needs a GPU")
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
        NS, NF = G * k, G * n
        members = sum(plan.line[l].count for l in range(n))
        on_a_line = len({m for l in range(n) for m in plan.members(l)})
        shards = torch.empty((G, k, P), dtype=torch.uint8, device=dev)
        lib.fill_xorshift(shards.data_ptr(), sh["cfg"], 0, G, k, S, P, st)
        hdr_np = bench.make_headers(G, k, S, 0)
        hdr = torch.from_numpy(hdr_np.view(np.uint8).reshape(G, k, 20).copy()).to(dev)
        fst, sst = bench.wire_stamps(hdr_np, plan, n)
        fstamps = torch.from_numpy(fst.view(np.uint8).copy()).to(dev)
        sstamps = torch.from_numpy(sst.view(np.uint8).copy()).to(dev)
        out = {v: (torch.full((NS, D), 0xEE, dtype=torch.uint8, device=dev),
                   torch.full((NS,), 0x7777, dtype=torch.int16, device=dev),
                   torch.full((NF, D), 0xEE, dtype=torch.uint8, device=dev),
                   torch.full((NF,), 0x7777, dtype=torch.int16, device=dev)) for v in ("two", "fused")}

        def seg():
            lib.wire_frame_seg(NS, P, S, shards.data_ptr(), hdr.data_ptr(), sstamps.data_ptr(), D,
                               out["two"][0].data_ptr(), out["two"][1].data_ptr(), st)

        def fec():
            lib.wire_encode_fec(plan, G, P, S, shards.data_ptr(), hdr.data_ptr(), fstamps.data_ptr(), D,
                                out["two"][2].data_ptr(), out["two"][3].data_ptr(), st)

        def fused():
            o = out["fused"]
            lib.wire_encode_send(plan, G, P, S, shards.data_ptr(), hdr.data_ptr(), sstamps.data_ptr(),
                                 o[0].data_ptr(), o[1].data_ptr(), fstamps.data_ptr(), o[2].data_ptr(),
                                 o[3].data_ptr(), D, st)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            b.record(stream)
            lib.timing_events(a.cuda_event, b.cuda_event)
            fn()
            assert lib.timing_launches() == 1
            return a, b

        seg(), fec(), fused()
        torch.cuda.synchronize(dev)
        same = all(bool(torch.equal(a, b)) for a, b in zip(out["two"], out["fused"]))
        live = int((out["fused"][1] != 0).sum()) + int((out["fused"][3] != 0).sum())
        rc |= 0 if same and live == NS + NF else 1
        # slots moved: members read (a member on no line still once), datagram slots written
        reads_fused = G * (members + k - on_a_line)
        b_fused = reads_fused * P + (NS + NF) * D
        b_two = G * k * P + NS * D + G * members * P + NF * D
        for p in range(args.passes):
            ev = {"seg": [], "fec": [], "fused": []}
            for step in range(args.warmup + args.steps):
                for v in (("two", "fused") if step & 1 else ("fused", "two")):
                    es = [("seg", timed(seg)), ("fec", timed(fec))] if v == "two" else [("fused", timed(fused))]
                    if step >= args.warmup:
                        for key, e in es:
                            ev[key].append(e)
            torch.cuda.synchronize(dev)
            us = {key: np.array([a.elapsed_time(b) for a, b in v]) * 1e3 for key, v in ev.items()}
            two = us["seg"] + us["fec"]

            def stat(t):
                return {"mean_us": round(float(t.mean()), 2), "median_us": round(float(np.median(t)), 2),
                        "min_us": round(float(t.min()), 2)}

            print(json.dumps({
                "shape": name, "pass": p, "groups": G, "k": k, "lines": n, "members_per_group": members, "S": S,
                "stride": P, "dstride": D, "steps": args.steps,
                "timing": "the kernels' own start / stop (rfec_timing_events)",
                "frame_seg": stat(us["seg"]), "encode_fec": stat(us["fec"]), "two_calls": stat(two),
                "fused": dict(stat(us["fused"]), bytes=b_fused,
                              frac_of_8TBps=round(b_fused / (float(us["fused"].mean()) * 1e-6) / 1e9
                                                  / bench.HBM_PEAK_GBPS, 4)),
                "timed_ms": {"two_calls": round(float(two.sum()) * 1e-3, 1),
                             "fused": round(float(us["fused"].sum()) * 1e-3, 1)},
                "fused_over_two_calls": round(float(us["fused"].mean() / two.mean()), 4),
                "traffic_ratio_from_shapes": round(b_fused / b_two, 4),
                "outputs_equal": same, "datagrams_emitted": live}), flush=True)
        del shards, out
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
