#!/usr/bin/env python3
"""A/B on one GPU: the c3full decode (65,536 groups, k = 10, the sender's full
3 x 4 plan, 1,200 B, bench.py's erasure pairs, per_group 2) from the batch
layout (rfec_recover_batch_out, k_decode_matrix_dense<10,4>) against the same
decode from packed matrix records (rfec_recover_packed_matrix_out,
k_decode_matrix_packed<10,4>), interleaved step by step, each decode cold (an
encode of the other buffer set runs before it, as in bench.py's steps).  Times
are the kernels' own start / stop (HIP events bound to the launch,
rfec_timing_events); k_pack_matrix, the records' producer, is timed the same
way and reported apart.  One JSON object per pass on stdout.

    python tools/packed_matrix_ab.py [--passes 3] [--steps 40] [--warmup 5] [--groups 65536]
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
from razor_amd.fec import native  # noqa: E402


def poison(w):
    for t in (w.out_shards, w.out_hdr, w.out_index, w.recovered):
        t.view(torch.uint8).fill_(0xEE)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=bench.CONFIGS["c3full"]["groups"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_matrix_ab.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    cfg = bench.CONFIGS["c3full"]
    k, S, G = cfg["k"], cfg["S"], args.groups
    sets = [bench.Workload(lib, G, k, S, 80, dev, 0, seed=2000, full_plan=True, config_id=cfg["config_id"])
            for _ in range(2)]
    pks = lib.packed_matrix_stride(sets[0].plan, 2)
    recs = [torch.full((G, pks), 0x77, dtype=torch.uint8, device=dev) for _ in sets]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        b.record(stream)
        lib.timing_events(a.cuda_event, b.cuda_event)
        fn()
        return a, b

    def pack(i):
        w = sets[i]
        lib.pack_erasures_matrix(w.plan, G, w.rx_hdr.data_ptr(), w.present.data_ptr(), w.meta.data_ptr(),
                                 w.fsize.data_ptr(), w.parity_present.data_ptr(), 2, recs[i].data_ptr(), st)

    def dec_packed(i):
        w = sets[i]
        lib.recover_packed_matrix_out(w.plan, G, w.stride, S, w.rx.data_ptr(), w.parity.data_ptr(),
                                      recs[i].data_ptr(), w.recovered.data_ptr(), 2, w.out_shards.data_ptr(),
                                      w.out_hdr.data_ptr(), w.out_index.data_ptr(), st)

    for w in sets:
        w.encode(st)
    torch.cuda.synchronize(dev)
    # both forms give the expected segments (checked once per form, on poisoned outputs)
    ok = {}
    for name in ("batch", "packed"):
        for i, w in enumerate(sets):
            poison(w)
            if name == "packed":
                pack(i)
                dec_packed(i)
            else:
                w.decode(st)
        torch.cuda.synchronize(dev)
        ok[name] = all(w.verify() for w in sets)
    dec_bytes = sets[0].dec_bytes
    for p in range(args.passes):
        ev = {"batch": [], "packed": [], "pack": []}
        for step in range(args.warmup + args.steps):
            i = step & 1
            order = ("batch", "packed") if (step >> 1) & 1 else ("packed", "batch")
            for name in order:
                sets[1 - i].encode(st)  # the decode below runs cold
                e = timed((lambda: sets[i].decode(st)) if name == "batch" else (lambda: dec_packed(i)))
                if step >= args.warmup:
                    ev[name].append(e)
            e = timed(lambda: pack(i))
            if step >= args.warmup:
                ev["pack"].append(e)
        torch.cuda.synchronize(dev)
        us = {n: np.array([a.elapsed_time(b) for a, b in v]) * 1e3 for n, v in ev.items()}
        frac = {n: dec_bytes / (float(us[n].mean()) * 1e-6) / 1e9 / bench.HBM_PEAK_GBPS for n in ("batch", "packed")}
        print(json.dumps({
            "pass": p, "groups": G, "k": k, "S": S, "per_group": 2, "steps": args.steps, "record_bytes": pks,
            "decode_bytes": dec_bytes, "timing": "the kernels' own start / stop (rfec_timing_events)",
            "batch": {"call": "rfec_recover_batch_out", "mean_us": round(float(us["batch"].mean()), 2),
                      "median_us": round(float(np.median(us["batch"])), 2),
                      "min_us": round(float(us["batch"].min()), 2), "frac_of_8TBps": round(frac["batch"], 4)},
            "packed": {"call": "rfec_recover_packed_matrix_out", "mean_us": round(float(us["packed"].mean()), 2),
                       "median_us": round(float(np.median(us["packed"])), 2),
                       "min_us": round(float(us["packed"].min()), 2), "frac_of_8TBps": round(frac["packed"], 4)},
            "packed_over_batch": round(float(us["packed"].mean() / us["batch"].mean()), 4),
            "producer": {"call": "rfec_pack_erasures_matrix (k_pack_matrix)",
                         "mean_us": round(float(us["pack"].mean()), 2),
                         "median_us": round(float(np.median(us["pack"])), 2)},
            "verified": ok}), flush=True)
    return 0 if all(ok.values()) else 1


if __name__ == "__main__":
    raise SystemExit(main())
