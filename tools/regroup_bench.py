#!/usr/bin/env python3
"""rfec_wire_regroup on one GPU: parsed datagrams (arrival order) into recover's
batch layout, timed as a whole call against two same-run yardsticks.

Shapes as tools/wire_encode_ab.py: c3 (k = 10, 3 row lines, 1,200 B in 1,216-B
rows), c3full (the sender's 3 x 4 plan, 7 lines), c5 (k = 32, 8 rows of 4,
256 B).  A window holds at most 65,535 fec_ids, so the 65,536 groups are two
windows of 32,768 and a "call" below is the two rfec_wire_regroup calls, one
after the other on the stream.  Records come from the product's own
rfec_wire_encode_send + rfec_wire_parse with 2 segments of every group lost
(length 0), in send order (every SIM_SEG of the window, then every SIM_FEC) or,
with --shuffle, in a random arrival order.

Variants, alternating step by step, each bracketed by stream events over enough
steps for --min-ms (default 250) of timed work:
    regroup   the whole call: fill, two record passes, the row pass (four launches per window)
    copy      rfec_probe_copy over the bytes of the filled rows (filled rows x 16 CD), non-temporal loads + stores
    copy_l2   the same with the default cache policy
    gather    k_gather_rows (rfec_launch_gather_rows) moving the same rows, whole `stride` bytes of each, by a
              map already on the device: the parent commit's way, the host's map build not counted
Bytes of the call: 2 x filled rows x 16 CD (rows read and written), 2 x 64 n (both record passes read every
record), 84 per filled slot (the winner's record read, its header record written), 12 per slot (src_of filled,
contended, read), 8 per record (slot_of written, read), 28 per group (masks, base_id).  One JSON object per shape
on stdout.  The kernels' separate times need a profiler run of few steps (--steps), e.g.
    rocprofv3 --kernel-trace --stats -d out -- python tools/regroup_bench.py --shapes c3 --steps 20

    python tools/regroup_bench.py [--groups 65536] [--shapes c3,c3full,c5] [--shuffle] [--min-ms 250] [--steps 0]
                                  [--lib other/librazor_fec_v1200.so]
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

import bench  # noqa: E402
from razor_amd.fec import Native, native  # noqa: E402
from wire_encode_ab import SHAPES  # noqa: E402

MAX_WINDOW = 65535


class Window:
    """One window of groups: its parsed records and rows, and the batch layout regroup fills."""

    def __init__(self, lib, sh, plan, G, g0, dev, st, shuffle, seed):
        k, S, P, D = sh["k"], sh["S"], sh["stride"], sh["dstride"]
        n = plan.n_lines
        self.G, self.k, self.n, self.N = G, k, n, G * (k + n)
        N, ns = self.N, G * k
        u8 = torch.uint8
        shards = torch.empty((G, k, P), dtype=u8, device=dev)
        lib.fill_xorshift(shards.data_ptr(), sh["cfg"], g0, G, k, S, P, st)
        hdr_np = bench.make_headers(G, k, S, g0)
        hdr = torch.from_numpy(hdr_np.view(np.uint8).reshape(G, k, 20).copy()).to(dev)
        fst, sst = bench.wire_stamps(hdr_np, plan, n)  # fec_id 1 .. G: fec_id0 = 1
        fstamps = torch.from_numpy(fst.view(np.uint8).copy()).to(dev)
        sstamps = torch.from_numpy(sst.view(np.uint8).copy()).to(dev)
        dgram = torch.empty((N, D), dtype=u8, device=dev)
        dlen = torch.empty((N,), dtype=torch.int16, device=dev)
        lib.wire_encode_send(plan, G, P, S, shards.data_ptr(), hdr.data_ptr(), sstamps.data_ptr(), dgram.data_ptr(),
                             dlen.data_ptr(), fstamps.data_ptr(), dgram.data_ptr() + ns * D, dlen.data_ptr() + ns * 2,
                             D, st)
        rng = np.random.default_rng(seed)
        lost = np.argsort(rng.random((G, k)), axis=1)[:, :2]  # 2 segments of every group
        self.lost = lost
        dlen[torch.from_numpy((np.arange(G)[:, None] * k + lost).reshape(-1)).to(dev)] = 0
        if shuffle:
            perm = torch.from_numpy(rng.permutation(N)).to(dev)
            dgram, dlen = dgram[perm].contiguous(), dlen[perm].contiguous()
        self.recs = torch.empty((N, 64), dtype=u8, device=dev)
        self.payload = torch.empty((N, P), dtype=u8, device=dev)
        lib.wire_parse(N, D, dgram.data_ptr(), dlen.data_ptr(), P, S, self.recs.data_ptr(), self.payload.data_ptr(),
                       st)
        torch.cuda.synchronize(dev)
        del dgram, dlen, shards
        z = lambda *shape, dt=u8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.out = dict(shards=z(G, k, P), hdr=z(G, k, 20), present=z(G, 2, dt=torch.int64), parity=z(G, n, P),
                        meta=z(G, n, 20), fec_size=z(G, n, dt=torch.int16), parity_present=z(G, dt=torch.int64),
                        base_id=z(G, dt=torch.int32), src_of=z(G * (k + n), dt=torch.int32),
                        slot_of=z(N, dt=torch.int32))
        self.filled = G * (k - 2 + n)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--shapes", default="c3,c3full,c5")
    ap.add_argument("--shuffle", action="store_true", help="random arrival order instead of send order")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of librazor_fec_v1200.so (kernel variants)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regroup_bench.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = Native(1200, path=args.lib) if args.lib else native(1200)
    gather = lib.lib.rfec_launch_gather_rows
    gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    gather.restype = C.c_int
    rc = 0
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        k, S, P = sh["k"], sh["S"], sh["stride"]
        plan = sh["plan"](lib)
        n = plan.n_lines
        nw = math.ceil(args.groups / MAX_WINDOW)
        per = math.ceil(args.groups / nw)
        wins = [Window(lib, sh, plan, min(per, args.groups - w * per), w * per, dev, st, args.shuffle, 7 + w)
                for w in range(nw)]
        cd = (S + 15) // 16 if S else 1

        def regroup():
            for w in wins:
                o = w.out
                lib.wire_regroup(plan, w.G, 1, w.N, w.recs.data_ptr(), w.payload.data_ptr(), P, S,
                                 *(o[key].data_ptr() for key in ("shards", "hdr", "present", "parity", "meta",
                                                                 "fec_size", "parity_present", "base_id", "src_of",
                                                                 "slot_of")), st)

        regroup()
        torch.cuda.synchronize(dev)
        # the call placed what was sent: the masks, the lost segments' slots empty, every live record in a slot
        ok = True
        for w in wins:
            want = np.full(w.G, (1 << k) - 1, np.uint64)
            for j in range(2):
                want &= ~(np.uint64(1) << w.lost[:, j].astype(np.uint64))
            pres = w.out["present"].cpu().numpy().view(np.uint64)
            pp = w.out["parity_present"].cpu().numpy().view(np.uint64)
            so = w.out["slot_of"].cpu().numpy()
            ok &= bool((pres[:, 0] == want).all() and (pres[:, 1] == 0).all() and (pp == (1 << n) - 1).all())
            ok &= int((so >= 0).sum()) == w.filled and int((so == -1).sum()) == 2 * w.G
            # the parent's way: the same rows by a host-built map (here: from src_of, empty slots zero-filled)
            src = w.out["src_of"].cpu().numpy().view(np.uint32).astype(np.int64).reshape(w.G, k + n)
            src[src == 0xFFFFFFFF] = -1
            w.map_s = torch.from_numpy(np.ascontiguousarray(src[:, :k]).astype(np.int32).reshape(-1)).to(dev)
            w.map_p = torch.from_numpy(np.ascontiguousarray(src[:, k:]).astype(np.int32).reshape(-1)).to(dev)
        rc |= 0 if ok else 1
        filled = sum(w.filled for w in wins)
        n_rec = sum(w.N for w in wins)
        row_bytes = filled * 16 * cd
        cp_src = torch.empty(row_bytes, dtype=torch.uint8, device=dev)
        cp_dst = torch.empty_like(cp_src)

        def copy(flags):
            def f():
                if lib.lib.rfec_probe_copy(cp_src.data_ptr(), cp_dst.data_ptr(), row_bytes, flags, st):
                    raise RuntimeError("rfec_probe_copy failed")
            return f

        def gather_rows():
            for w in wins:
                o = w.out
                if gather(o["shards"].data_ptr(), w.payload.data_ptr(), w.map_s.data_ptr(), w.G * k, P, st) or \
                        gather(o["parity"].data_ptr(), w.payload.data_ptr(), w.map_p.data_ptr(), w.G * n, P, st):
                    raise RuntimeError("rfec_launch_gather_rows failed")

        variants = {"regroup": regroup, "copy": copy(1), "copy_l2": copy(0), "gather": gather_rows}

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
        bytes_call = (2 * row_bytes + 2 * 64 * n_rec + 84 * filled + 12 * args.groups * (k + n) + 8 * n_rec
                      + 28 * args.groups)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "median_us": round(float(np.median(t)), 2),
                    "min_us": round(float(t.min()), 2), "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        rg, cp = float(us["regroup"].mean()), float(us["copy"].mean())
        print(json.dumps({
            "shape": name, "groups": args.groups, "windows": [w.G for w in wins], "k": k, "lines": n, "S": S,
            "stride": P, "records": n_rec, "filled_rows": filled, "arrival": "shuffled" if args.shuffle else "send order",
            "steps": steps, "timing": "stream events around the whole call (all windows)",
            "regroup": dict(stat(us["regroup"]), bytes=bytes_call, row_bytes_read_plus_written=2 * row_bytes,
                            GBps=round(bytes_call / (rg * 1e-6) / 1e9, 1),
                            frac_of_8TBps=round(bytes_call / (rg * 1e-6) / 1e9 / bench.HBM_PEAK_GBPS, 4)),
            "copy_probe": dict(stat(us["copy"]), bytes=2 * row_bytes, GBps=round(2 * row_bytes / (cp * 1e-6) / 1e9, 1)),
            "copy_probe_l2": stat(us["copy_l2"]),
            "gather_rows": dict(stat(us["gather"]), bytes=2 * filled * P),
            "copy_over_regroup": round(cp / rg, 4),
            "regroup_over_gather": round(rg / float(us["gather"].mean()), 4),
            "placement_verified": ok}), flush=True)
        del wins, cp_src, cp_dst
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
