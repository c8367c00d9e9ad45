#!/usr/bin/env python3
"""rfec_recover_indexed_matrix_wide_out (one launch of k_decode_matrix_wide, no
workspace) against rfec_recover_indexed_out (k_peel_lds + k_recover_indexed: the
only other route for a full matrix plan above k = 16) on one GPU, on the same
tables and the same row pool in the same run; at k <= 16 also against
rfec_recover_indexed_matrix_out, whose shape is compiled in -- what the run-time
shape costs.

Record sets as tools/indexed_recover_bench.py (regroup_bench.Window): the
product's own rfec_wire_encode_send + rfec_wire_parse over 1,200-byte segments in
1,216-byte rows, the sender's full row + column plan of each k, 2 segments of
every group lost, in send order or, with --shuffle, in a random arrival order;
rfec_wire_regroup_index writes the tables once.  per_group = 2.  Group counts:
--rows R gives each shape floor(R / (k + lines)) groups (default 1,114,112 rows:
c3full's 65,536 groups of 17), in windows of at most 32,768 groups; --segments S
gives one window of max(1, S // k) groups (a session-sized window: 512).

Before anything is timed the four outputs of every variant are compared with
rfec_recover_indexed_out's ("outputs_equal"; exit status 1 where they differ or
nothing was recovered).  Then the variants alternate step by step, each a whole
call (all windows) between stream events, over enough steps for --min-ms of
timed work each.  Reported per variant: mean, median, p05, p95; wide / generic
(and wide / matrix at k <= 16) of the means; the verdict by the project's
criterion -- "faster" only where the new call's p95 lies below the other's p05,
else "not faster"; and the algorithmic bytes (per out slot: the fired line's
parity and other members read and one slot written, 16 CD bytes each, rows
first as the decode takes them) over the mean time as a fraction of 8 TB/s.

One JSON object per shape on stdout, and appended to --out when given.

    python tools/matrix_wide_bench.py [--ks 17,40,100,10] [--rows 1114112 | --segments 512] [--shuffle]
                                      [--min-ms 250] [--out profiles/r18/matrix_wide/large_send_run1.jsonl]
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

from razor_amd.fec import Native, native  # noqa: E402
from regroup_bench import MAX_WINDOW, Window  # noqa: E402

E = 2  # dense out slots per group: the two lost segments
S, STRIDE, DSTRIDE = 1200, 1216, 1280
TABLES = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")
PEAK = 8e12  # bytes / s


def slot_rows(k, col, n_row_lines, lost):
    """Rows moved per group, [G]: for each of the two lost segments the line the decode takes -- its row when the
    row has a line and holds no other loss, else its column; where both are blocked (the target's row has no line and
    the other loss shares its column) the other loss's row first, then the column -- counted as the line's parity and
    other members read and one slot written."""
    t = np.sort(lost, axis=1).astype(np.int64)
    r, c = t // col, t % col
    row_n = np.minimum(col, k - r * col)           # members of the target's row
    col_n = (k - c + col - 1) // col               # and of its column
    rows = np.zeros(len(t), np.int64)
    for a, b in ((0, 1), (1, 0)):
        row_ok = (r[:, a] < n_row_lines) & (r[:, a] != r[:, b])
        col_ok = c[:, a] != c[:, b]
        rows += np.where(row_ok, row_n[:, a], np.where(col_ok, col_n[:, a], col_n[:, a] + row_n[:, b])) + 1
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,40,100,10")
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
        raise SystemExit("matrix_wide_bench.py: needs a GPU")
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
    for k in (int(v) for v in args.ks.split(",")):
        plan = lib.plan_from_fraction(k, 80, 3)
        n, col = plan.n_lines, plan.col
        sh = dict(k=k, S=S, stride=STRIDE, dstride=DSTRIDE, cfg=3)
        groups = max(1, args.segments // k) if args.segments else args.rows // (k + n)
        nw = math.ceil(groups / MAX_WINDOW)
        per = math.ceil(groups / nw)
        wins = [Window(lib, sh, plan, min(per, groups - w * per), w * per, dev, st, args.shuffle, 7 + w)
                for w in range(nw)]
        for w in wins:
            del w.out["shards"], w.out["parity"]  # the batch layout's rows: not used here
            w.tab = {key: w.out[key] for key in TABLES}
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
                    "wide": lambda: call(lib.recover_indexed_matrix_wide_out, False)}
        if lib.packed_matrix_stride(plan, 1) != 0:
            variants["matrix"] = lambda: call(lib.recover_indexed_matrix_out, False)
        # every variant's outputs against rfec_recover_indexed_out's, before anything is timed
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

        alg = int(sum(int(slot_rows(k, col, plan.n_row_lines, w.lost).sum()) for w in wins)) * 16 * cd
        line = {
            "k": k, "row": plan.row, "col": col, "lines": n, "groups": groups, "windows": [w.G for w in wins], "S": S,
            "stride": STRIDE, "pool_rows": sum(w.N for w in wins), "pool_bytes": sum(w.N for w in wins) * STRIDE,
            "per_group": E, "arrival": "shuffled" if args.shuffle else "send order", "steps": steps,
            "timing": "stream events around the whole call (all windows), variants alternating",
            "outputs_equal": equal, "recovered_segments": recovered, "indexed_path": paths,
            **{v: stat(t) for v, t in us.items()},
            "algorithmic_bytes": alg,
            "wide_fraction_of_8TBps": round(alg / (float(us["wide"].mean()) * 1e-6) / PEAK, 4),
            "generic_fraction_of_8TBps": round(alg / (float(us["generic"].mean()) * 1e-6) / PEAK, 4),
            "wide_over_generic": round(float(us["wide"].mean() / us["generic"].mean()), 4),
            "wide_against_generic": verdict(us["wide"], us["generic"]),
        }
        if "matrix" in us:
            line["wide_over_matrix"] = round(float(us["wide"].mean() / us["matrix"].mean()), 4)
            line["wide_against_matrix"] = verdict(us["wide"], us["matrix"])
            line["matrix_against_wide"] = verdict(us["matrix"], us["wide"])
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
