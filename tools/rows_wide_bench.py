#!/usr/bin/env python3
"""rfec_recover_indexed_rows_wide_out (one launch of k_decode_rows_wide, no
workspace) against rfec_recover_indexed_out on one GPU, on the same tables and
the same row pool in the same run.  For a row layout with rows above 4 segments
(every strip-mode plan of 6 or more segments) rfec_recover_indexed_out takes
k_peel_lds + k_recover_indexed with a workspace -- the only other route; for
rows of <= 4 with k <= 64 (10x4, 32x4) it takes one launch of
k_decode_rows_indexed, so those shapes put the cost of the run-time shape on
record.

Record sets as tools/matrix_wide_bench.py (regroup_bench.Window's steps): the
product's own rfec_wire_encode_send + rfec_wire_parse over 1,200-byte segments
in 1,216-byte rows, the row layout k x col of each shape, in send order or, with
--shuffle, in a random arrival order; rfec_wire_regroup_index writes the tables
once.  Loss: a one-row shape loses one segment of every group (per_group 1); a
shape of several rows loses two segments in different rows (per_group 2).  Group
counts: --rows R gives each shape floor(R / (k + lines)) groups (default
1,114,112 rows: c3full's pool), in windows of at most 65,535 groups;
--segments S gives one window of max(1, S // k) groups (a session-sized window:
512).

Before anything is timed the four outputs of the new call are compared with
rfec_recover_indexed_out's ("outputs_equal"; exit status 1 where they differ or
nothing was recovered).  Then the variants alternate step by step, each a whole
call (all windows) between stream events, over enough steps for --min-ms of
timed work each.  Reported per variant: mean, median, p05, p95; wide / generic
of the means; the verdict by the project's criterion -- "faster" only where the
new call's p95 lies below the other's p05, else "not faster" (and the other way
round); and the algorithmic bytes (per out slot: the row's parity and other
members read and one slot written, 16 CD bytes each) over the mean time as a
fraction of 8 TB/s.

One JSON object per shape on stdout, and appended to --out when given.

    python tools/rows_wide_bench.py [--shapes 10x10,30x30,100x100,100x25,10x4,32x4]
                                    [--rows 1114112 | --segments 512] [--shuffle] [--min-ms 250]
                                    [--out profiles/r19/rows_wide/large_send_run1.jsonl]
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
from razor_amd.fec import RFEC_LAYER_ROWS, Native, native  # noqa: E402
from regroup_bench import MAX_WINDOW  # noqa: E402

S, STRIDE, DSTRIDE = 1200, 1216, 1280
TABLES = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")
PEAK = 8e12  # bytes / s


def lose(rng, G, k, col, n):
    """[G][E] lost segments: one per group of a one-row shape, two in different rows (rows with a line) otherwise."""
    if n == 1:
        return rng.integers(0, k, (G, 1))
    rows = np.argsort(rng.random((G, n)), axis=1)[:, :2]
    width = np.minimum(col, k - rows * col)
    return rows * col + (rng.random((G, 2)) * width).astype(np.int64)


class Window:
    """One window of groups (regroup_bench.Window's steps with the loss given): its parsed records and rows, and
    the tables rfec_wire_regroup_index fills."""

    def __init__(self, lib, plan, col, G, g0, dev, st, shuffle, seed):
        k, n = plan.k, plan.n_lines
        self.G, self.k, self.n, self.N = G, k, n, G * (k + n)
        N, ns = self.N, G * k
        u8 = torch.uint8
        shards = torch.empty((G, k, STRIDE), dtype=u8, device=dev)
        lib.fill_xorshift(shards.data_ptr(), 3, g0, G, k, S, STRIDE, st)
        hdr_np = bench.make_headers(G, k, S, g0)
        hdr = torch.from_numpy(hdr_np.view(np.uint8).reshape(G, k, 20).copy()).to(dev)
        fst, sst = bench.wire_stamps(hdr_np, plan, n)  # fec_id 1 .. G: fec_id0 = 1
        fstamps = torch.from_numpy(fst.view(np.uint8).copy()).to(dev)
        sstamps = torch.from_numpy(sst.view(np.uint8).copy()).to(dev)
        dgram = torch.empty((N, DSTRIDE), dtype=u8, device=dev)
        dlen = torch.empty((N,), dtype=torch.int16, device=dev)
        lib.wire_encode_send(plan, G, STRIDE, S, shards.data_ptr(), hdr.data_ptr(), sstamps.data_ptr(),
                             dgram.data_ptr(), dlen.data_ptr(), fstamps.data_ptr(), dgram.data_ptr() + ns * DSTRIDE,
                             dlen.data_ptr() + ns * 2, DSTRIDE, st)
        rng = np.random.default_rng(seed)
        self.lost = lose(rng, G, k, col, n)
        dlen[torch.from_numpy((np.arange(G)[:, None] * k + self.lost).reshape(-1)).to(dev)] = 0
        if shuffle:
            perm = torch.from_numpy(rng.permutation(N)).to(dev)
            dgram, dlen = dgram[perm].contiguous(), dlen[perm].contiguous()
        self.recs = torch.empty((N, 64), dtype=u8, device=dev)
        self.payload = torch.empty((N, STRIDE), dtype=u8, device=dev)
        lib.wire_parse(N, DSTRIDE, dgram.data_ptr(), dlen.data_ptr(), STRIDE, S, self.recs.data_ptr(),
                       self.payload.data_ptr(), st)
        torch.cuda.synchronize(dev)
        del dgram, dlen, shards
        z = lambda *shape, dt=u8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.tab = dict(hdr=z(G, k, 20), present=z(G, 2, dt=torch.int64), meta=z(G, n, 20),
                        fec_size=z(G, n, dt=torch.int16), parity_present=z(G, dt=torch.int64),
                        base_id=z(G, dt=torch.int32), src_of=z(G * (k + n), dt=torch.int32),
                        slot_of=z(N, dt=torch.int32))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10x10,30x30,100x100,100x25,10x4,32x4", help="k x col, comma separated")
    ap.add_argument("--rows", type=int, default=65536 * 17, help="pool rows per shape (c3full's)")
    ap.add_argument("--segments", type=int, default=0, help="one window of this many segments instead")
    ap.add_argument("--shuffle", action="store_true", help="random arrival order instead of send order")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of librazor_fec_v1200.so")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_wide_bench.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = Native(1200, path=args.lib) if args.lib else native(1200)
    path = lib.lib.rfec_indexed_last_path
    path.restype, path.argtypes = C.c_uint32, []
    cd = (S + 15) // 16
    u8 = torch.uint8
    rc = 0
    for k, col in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        plan = lib.plan_matrix(k, -(-k // col), col, RFEC_LAYER_ROWS)
        n = plan.n_lines
        E = 1 if n == 1 else 2
        groups = max(1, args.segments // k) if args.segments else args.rows // (k + n)
        nw = math.ceil(groups / MAX_WINDOW)
        per = math.ceil(groups / nw)
        wins = [Window(lib, plan, col, min(per, groups - w * per), w * per, dev, st, args.shuffle, 7 + w)
                for w in range(nw)]
        for w in wins:
            w.ws = torch.empty(max(16, lib.workspace_size(plan, w.G)), dtype=u8, device=dev)
            w.dec = dict(recovered=torch.zeros((w.G, 2), dtype=torch.int64, device=dev),
                         out_shards=torch.zeros((w.G, E, STRIDE), dtype=u8, device=dev),
                         out_hdr=torch.zeros((w.G, E, 20), dtype=u8, device=dev),
                         out_index=torch.zeros((w.G, E), dtype=u8, device=dev))
            lib.wire_regroup_index(plan, w.G, 1, w.N, w.recs.data_ptr(), S, *(w.tab[key].data_ptr() for key in TABLES),
                                   st)
        torch.cuda.synchronize(dev)

        def call(fn, workspace):
            for w in wins:
                d, t = w.dec, w.tab
                fn(plan, w.G, STRIDE, S, w.payload.data_ptr(), w.N, t["src_of"].data_ptr(),
                   *(t[key].data_ptr() for key in ("hdr", "present", "meta", "fec_size", "parity_present")),
                   d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(), d["out_hdr"].data_ptr(),
                   d["out_index"].data_ptr(), *((w.ws.data_ptr(),) if workspace else ()), st)

        variants = {"generic": lambda: call(lib.recover_indexed_out, True),
                    "wide": lambda: call(lib.recover_indexed_rows_wide_out, False)}
        # the new call's outputs against rfec_recover_indexed_out's, before anything is timed
        ref, paths, equal = None, {}, True
        for v, fn in variants.items():
            for w in wins:
                for t in w.dec.values():
                    t.fill_(0x3C)
            fn()
            paths[v] = hex(int(path()))
            torch.cuda.synchronize(dev)
            if ref is None:
                ref = [{key: t.clone() for key, t in w.dec.items()} for w in wins]
                continue
            for w, a in zip(wins, ref):
                b = w.dec
                ok = a["out_index"] != 0xFF
                equal &= bool(torch.equal(a["recovered"], b["recovered"]) and
                              torch.equal(a["out_index"], b["out_index"]) and
                              torch.equal(a["out_hdr"][ok], b["out_hdr"][ok]) and
                              torch.equal(a["out_shards"][ok][:, :16 * cd], b["out_shards"][ok][:, :16 * cd]) and
                              bool((b["out_shards"][:, :, 16 * cd:] == 0x3C).all()))
        recovered = sum(int((a["out_index"] != 0xFF).sum()) for a in ref)
        del ref
        rc |= 0 if equal and recovered == groups * E else 1

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
        steps = args.steps or min(20000, max(10, int(math.ceil(args.min_ms * 1e3 /
                                                               min(float(t.mean()) for t in est.values())))))
        us = run(steps, steps)

        def stat(t):
            return {"mean_us": round(float(t.mean()), 2), "median_us": round(float(np.median(t)), 2),
                    "p05_us": round(float(np.percentile(t, 5)), 2), "p95_us": round(float(np.percentile(t, 95)), 2),
                    "min_us": round(float(t.min()), 2), "max_us": round(float(t.max()), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        def verdict(x, y):  # faster only where x's 95th percentile lies below y's 5th
            return "faster" if np.percentile(x, 95) < np.percentile(y, 5) else "not faster"

        # per out slot: the row's parity and its other members read, one slot written = the row's width + 1 rows
        alg = int(sum(int((np.minimum(col, k - (w.lost // col) * col) + 1).sum()) for w in wins)) * 16 * cd
        line = {
            "k": k, "col": col, "lines": n, "groups": groups, "windows": [w.G for w in wins], "S": S,
            "stride": STRIDE, "pool_rows": sum(w.N for w in wins), "pool_bytes": sum(w.N for w in wins) * STRIDE,
            "per_group": E, "lost_per_group": E, "arrival": "shuffled" if args.shuffle else "send order",
            "steps": steps, "timing": "stream events around the whole call (all windows), variants alternating",
            "outputs_equal": equal, "recovered_segments": recovered, "indexed_path": paths,
            **{v: stat(t) for v, t in us.items()},
            "algorithmic_bytes": alg,
            "wide_fraction_of_8TBps": round(alg / (float(us["wide"].mean()) * 1e-6) / PEAK, 4),
            "generic_fraction_of_8TBps": round(alg / (float(us["generic"].mean()) * 1e-6) / PEAK, 4),
            "wide_over_generic": round(float(us["wide"].mean() / us["generic"].mean()), 4),
            "wide_against_generic": verdict(us["wide"], us["generic"]),
            "generic_against_wide": verdict(us["generic"], us["wide"]),
        }
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del wins
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
