#!/usr/bin/env python3
"""rfec_wire_encode_send_shapes on one GPU: a send window whose groups have four
shapes into its SIM_SEG and SIM_FEC datagrams, in send order, with one launch
for the window against one rfec_wire_encode_send call per shape.

Window: 65,535 groups of the shapes of regroup_shapes_bench.py,
    (10, 3, 4) rows + columns, (32, 8, 4) rows, (16, 4, 4) rows + columns, (6, 2, 3) rows + columns,
1,200-B segments in 1,216-B rows, 1,280-B datagram slots.  Send order: SIM_SEG
slot = the member's row in window order, SIM_FEC slot = the line in window order.

    random window (a shape drawn uniformly per group):
      a   today's way: the rows sorted by shape, one rfec_wire_encode_send per shape.  An order of that call is a
          permutation of the call's own slots, so the datagrams come out grouped by shape: the sender walks an
          index to send them in order
      a_gather   a, then one gather of the slots and one of the lengths per kind into send order
      b   the new call on a's rows, the descriptors sorted by shape too, the orders back to send order
      c   the rows in window order, the descriptors sorted by shape (no orders)
      d   the rows and the descriptors in window order: mixed waves throughout
    video window (runs of 30 groups of one shape, one group of another between them):
      a, a_gather   as above
      e   the rows and the descriptors in window order
    one window (every group (10, 3, 4) rows + columns):
      f_old   rfec_wire_encode_send
      f_new   the new call, rows and descriptors in window order
      f_prev  rfec_wire_encode_send of another build of the library (--prev-lib: the parent commit's)

Every variant's four outputs are compared with the window's baseline before anything is timed (a's after its
gather; exit status 1 where they differ).  The variants of a window alternate step by step, each bracketed by
stream events around its calls, over enough steps for --min-ms (default 250) of timed work each; p05 / median /
p95 per variant, each variant's mean over each baseline's (a and a_gather, or f_old) and whether its p95 lies
below that baseline's p05.  One JSON object per window on stdout.

    python tools/wire_send_shapes_bench.py [--groups 65535] [--windows random,video,one] [--min-ms 250] [--steps 0]
                                           [--prev-lib FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from razor_amd.fec import (FEC_STAMP_DTYPE, HDR_DTYPE, RFEC_LAYER_COLS, RFEC_LAYER_ROWS, SEG_STAMP_DTYPE,  # noqa: E402
                           SEND_GROUP_DTYPE, Native, native)

S, STRIDE, DSTRIDE = 1200, 1216, 1280
SHAPES = ((10, 3, 4, RFEC_LAYER_ROWS | RFEC_LAYER_COLS), (32, 8, 4, RFEC_LAYER_ROWS),
          (16, 4, 4, RFEC_LAYER_ROWS | RFEC_LAYER_COLS), (6, 2, 3, RFEC_LAYER_ROWS | RFEC_LAYER_COLS))


def sequence(window, G, rng):
    if window == "random":
        return rng.integers(0, len(SHAPES), G)
    if window == "video":  # runs of 30 groups of one shape, one group of the next shape between them
        run = np.arange(G) // 31
        return np.where(np.arange(G) % 31 == 30, (run + 1) % len(SHAPES), run % len(SHAPES))
    return np.zeros(G, np.int64)


def window_inputs(plans, seq):
    """The window's rows in window order (headers and stamps as bench.py's: contiguous packet ids, a fec_id per
    group) and, per group, its first row and line."""
    G = len(seq)
    ks = np.array([p.k for p in plans])[seq]
    ns = np.array([p.n_lines for p in plans])[seq]
    row0, line0 = np.concatenate([[0], np.cumsum(ks)]), np.concatenate([[0], np.cumsum(ns)])
    n_rows, n_fec = int(row0[-1]), int(line0[-1])
    gr, gl = np.repeat(np.arange(G), ks), np.repeat(np.arange(G), ns)
    ir, il = np.arange(n_rows) - row0[gr], np.arange(n_fec) - line0[gl]
    hdr = np.zeros(n_rows, HDR_DTYPE)
    hdr["seq"], hdr["fid"], hdr["ts"] = 1 + np.arange(n_rows), 1 + gr, 33 * gr
    hdr["index"], hdr["total"], hdr["ftype"], hdr["size"] = ir, ks[gr], gr % 60 == 0, S
    ss = np.zeros(n_rows, SEG_STAMP_DTYPE)
    ss["uid"], ss["fec_id"], ss["send_ts"] = 0x52415A4F, gr % 65535 + 1, (33 * gr) & 0xFFFF
    ss["transport_seq"], ss["remb"] = np.arange(n_rows) & 0xFFFF, 0xFF
    fs = np.zeros(n_fec, FEC_STAMP_DTYPE)
    fs["uid"], fs["fec_id"], fs["base_id"] = 0x52415A4F, gl % 65535 + 1, 1 + row0[gl]
    fs["count"], fs["send_ts"], fs["transport_seq"] = ks[gl], 33 * gl, np.arange(n_fec) & 0xFFFF
    index = [np.array([p.line[l].index for l in range(p.n_lines)], np.int64) for p in plans]
    for p, plan in enumerate(plans):
        m = seq[gl] == p
        fs["row"][m], fs["col"][m], fs["index"][m] = plan.row, plan.col, index[p][il[m]]
    return hdr, ss, fs, row0[:-1], line0[:-1], ks, ns, n_rows, n_fec


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65535)
    ap.add_argument("--windows", default="random,video,one")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prev-lib", default=None, help="another build of librazor_fec_v1200.so for f_prev")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wire_send_shapes_bench.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = native(1200)
    prev = Native(1200, args.prev_lib) if args.prev_lib else None
    plans = [lib.plan_matrix(*s) for s in SHAPES]
    G = args.groups
    rc = 0

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).to(dev)

    for window in args.windows.split(","):
        rng = np.random.default_rng(11)
        seq = sequence(window, G, rng)
        hdr, ss, fs, row0, line0, ks, ns, n_rows, n_fec = window_inputs(plans, seq)
        shards = torch.randint(0, 256, (n_rows, STRIDE), dtype=torch.uint8, device=dev,
                               generator=torch.Generator(device=dev).manual_seed(11))
        shards[:, S:] = 0
        win = dict(shards=shards, hdr=up(hdr), ss=up(ss), fs=up(fs))
        # the rows sorted by shape (a stable sort of the groups), and the orders back to send order
        by_shape = np.argsort(seq, kind="stable")
        counts = np.bincount(seq, minlength=len(plans))
        srow = np.concatenate([row0[g] + np.arange(ks[g]) for g in by_shape]) if window != "one" else np.arange(n_rows)
        sline = np.concatenate([line0[g] + np.arange(ns[g]) for g in by_shape]) if window != "one" else np.arange(n_fec)
        if window != "one":
            t_row, t_line = torch.from_numpy(srow).to(dev), torch.from_numpy(sline).to(dev)
            srt = dict(shards=shards[t_row].contiguous(), hdr=win["hdr"][t_row].contiguous(),
                       ss=win["ss"][t_row].contiguous(), fs=win["fs"][t_line].contiguous(),
                       so=up(srow.astype(np.uint32)), fo=up(sline.astype(np.uint32)))

        def outputs():
            return dict(sd=torch.empty((n_rows, DSTRIDE), dtype=torch.uint8, device=dev),
                        sl=torch.empty(n_rows, dtype=torch.int16, device=dev),
                        fd=torch.empty((n_fec, DSTRIDE), dtype=torch.uint8, device=dev),
                        fl=torch.empty(n_fec, dtype=torch.int16, device=dev))

        out = outputs()
        if window != "one":
            stage = outputs()
            inv = np.empty(n_rows, np.int64)
            inv[srow] = np.arange(n_rows)
            inv_row = torch.from_numpy(inv).to(dev)
            inv = np.empty(n_fec, np.int64)
            inv[sline] = np.arange(n_fec)
            inv_line = torch.from_numpy(inv).to(dev)

        def desc(r0, l0, order):
            d = np.zeros(G, SEND_GROUP_DTYPE)
            d["row0"], d["line0"], d["shape"] = r0, l0, seq
            return up(d[order])

        # the sorted layout: group by_shape[j] has the j-th block of rows and lines
        sr0, sl0 = np.zeros(G, np.int64), np.zeros(G, np.int64)
        sr0[by_shape] = np.concatenate([[0], np.cumsum(ks[by_shape])])[:-1]
        sl0[by_shape] = np.concatenate([[0], np.cumsum(ns[by_shape])])[:-1]
        d_sorted_rows = desc(sr0, sl0, by_shape)
        d_byshape = desc(row0, line0, by_shape)
        d_window = desc(row0, line0, np.arange(G))

        def per_shape(L, src, dst):
            """One rfec_wire_encode_send per shape over src's rows (a shape's groups contiguous), into the same
            slots of dst."""
            r = l = 0
            for p, plan in enumerate(plans):
                Gp = int(counts[p])
                if Gp:
                    L.wire_encode_send(plan, Gp, STRIDE, S, src["shards"].data_ptr() + r * STRIDE,
                                       src["hdr"].data_ptr() + r * 20, src["ss"].data_ptr() + r * 12,
                                       dst["sd"].data_ptr() + r * DSTRIDE, dst["sl"].data_ptr() + r * 2,
                                       src["fs"].data_ptr() + l * 24, dst["fd"].data_ptr() + l * DSTRIDE,
                                       dst["fl"].data_ptr() + l * 2, DSTRIDE, st)
                r, l = r + Gp * plan.k, l + Gp * plan.n_lines

        def gather():
            """The staged slots into send order: slot r of the window is the sorted layout's slot inv[r]."""
            torch.index_select(stage["sd"], 0, inv_row, out=out["sd"])
            torch.index_select(stage["sl"], 0, inv_row, out=out["sl"])
            torch.index_select(stage["fd"], 0, inv_line, out=out["fd"])
            torch.index_select(stage["fl"], 0, inv_line, out=out["fl"])

        def a_gather():
            per_shape(lib, srt, stage)
            gather()

        def shapes(src, d, orders):
            lib.wire_encode_send_shapes(plans, G, d.data_ptr(), n_rows, n_fec, STRIDE, S, src["shards"].data_ptr(),
                                        src["hdr"].data_ptr(), src["ss"].data_ptr(), out["sd"].data_ptr(),
                                        out["sl"].data_ptr(), src["fs"].data_ptr(), out["fd"].data_ptr(),
                                        out["fl"].data_ptr(), DSTRIDE, st,
                                        seg_order=src["so"].data_ptr() if orders else None,
                                        fec_order=src["fo"].data_ptr() if orders else None)

        if window == "random":
            variants = {"a": lambda: per_shape(lib, srt, stage), "a_gather": a_gather,
                        "b": lambda: shapes(srt, d_sorted_rows, True), "c": lambda: shapes(win, d_byshape, False),
                        "d": lambda: shapes(win, d_window, False)}
            bases = ["a_gather", "a"]
        elif window == "video":
            variants = {"a": lambda: per_shape(lib, srt, stage), "a_gather": a_gather,
                        "e": lambda: shapes(win, d_window, False)}
            bases = ["a_gather", "a"]
        else:
            variants = {"f_old": lambda: per_shape(lib, win, out), "f_new": lambda: shapes(win, d_window, False)}
            if prev:
                variants["f_prev"] = lambda: per_shape(prev, win, out)
            bases = ["f_old"]
        base = bases[0]

        # the outputs, before anything is timed: every variant writes what the baseline writes
        ref, equal = None, True
        for v in [base] + [v for v in variants if v != base]:
            for t in out.values():
                t.fill_(0x5A)
            variants[v]()
            if v == "a":
                gather()
            torch.cuda.synchronize(dev)
            if ref is None:
                ref = {k: t.clone() for k, t in out.items()}
                equal &= bool((ref["sl"] >= 26 + S + 4).all()) and bool((ref["fl"] == S + 49).all())  # every datagram live
            else:
                equal &= all(bool(torch.equal(ref[k], out[k])) for k in out)
        del ref
        rc |= 0 if equal else 1

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
                    "p05_us": round(float(np.percentile(t, 5)), 2), "median_us": round(float(np.median(t)), 2),
                    "p95_us": round(float(np.percentile(t, 95)), 2), "min_us": round(float(t.min()), 2),
                    "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        quads = [len(set(seq[q:q + 4].tolist())) for q in range(0, G, 4)]
        line = {"window": window, "groups": G, "shapes": [list(s[:3]) + [plans[p].n_lines] for p, s in enumerate(SHAPES)],
                "counts": counts.tolist(), "S": S, "stride": STRIDE, "dstride": DSTRIDE, "rows": n_rows, "lines": n_fec,
                "passes_per_wave_in_window_order": round(float(np.mean(quads)), 3), "steps": steps,
                "timing": "stream events around each variant's calls, variants alternating",
                "outputs_equal": bool(equal), "baselines": bases, **{v: stat(t) for v, t in us.items()}}
        for b in bases:
            others = {v: t for v, t in us.items() if v not in bases}
            line[f"over_{b}"] = {v: round(float(t.mean() / us[b].mean()), 4) for v, t in others.items()}
            line[f"p95_below_p05_of_{b}"] = {v: bool(np.percentile(t, 95) < np.percentile(us[b], 5))
                                             for v, t in others.items()}
            line[f"{b}_p95_below_p05_of"] = {v: bool(np.percentile(us[b], 95) < np.percentile(t, 5))
                                             for v, t in others.items()}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del win, out, shards
        if window != "one":
            del srt, stage
        torch.cuda.empty_cache()
    return rc


if __name__ == "__main__":
    raise SystemExit(main())
