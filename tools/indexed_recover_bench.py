#!/usr/bin/env python3
"""The device receive chain after rfec_wire_parse, with and without the row
copy, on one GPU and on the same records in the same run:

    A   rfec_wire_regroup + rfec_recover_batch_out        (rows copied into the batch layout, then decoded)
    B   rfec_wire_regroup_index + rfec_recover_indexed_out (tables only, the decode reads the rows where they lie)

Record sets as tools/regroup_bench.py (its Window): shapes c3 (k = 10, 3 row
lines, 1,200 B in 1,216-B rows), c3full (the sender's 3 x 4 plan, 7 lines), c5
(k = 32, 8 rows of 4, 256 B); 65,536 groups as two windows of 32,768; records
from the product's own rfec_wire_encode_send + rfec_wire_parse with 2 segments
of every group lost, in send order or, with --shuffle, in a random arrival
order.  per_group = 2.

Before anything is timed, B's recovered, out_index, out_hdr and out_shards (over
[0, 16 CD) of the recovered slots) are compared with A's; "outputs_equal" says
so and the exit status is 1 where they differ.

Variants, alternating step by step, each bracketed by stream events around the
whole chain (both windows) over enough steps for --min-ms (default 250) of
timed work each:
    chain_a          A
    chain_b          B
    decode_a         rfec_recover_batch_out alone, on the regrouped layout
    decode_b         rfec_recover_indexed_out alone, on regroup_index's tables: what the gather costs the decode
    decode_b_generic the same under RFEC_TUNE_GENERIC (k_peel_lds + k_recover_indexed); row layouts only, where
                     the default is the fused k_decode_rows_indexed
    decode_b_matrix  rfec_recover_indexed_matrix_out alone (one launch of k_decode_matrix_indexed, no workspace), on
                     the same tables; the sender's full matrix plans only (c3full), where decode_b is the peel + replay
    chain_b_matrix   rfec_wire_regroup_index + rfec_recover_indexed_matrix_out
decode_b_matrix's four outputs are compared with decode_b's before anything is timed ("matrix_outputs_equal").
Each variant reports mean / median / min / max / std over its repetitions: the
spread the comparison is read against.  Payload bytes moved per chain (derived):
A copies filled rows x 16 CD twice (read + write), then the decode reads its
lines' rows and writes 2 slots per group; B moves the decode's rows only.

One JSON object per shape on stdout, and appended to --out when given.

    python tools/indexed_recover_bench.py [--groups 65536] [--shapes c3,c3full,c5] [--shuffle] [--min-ms 250]
                                          [--steps 0] [--out profiles/r10/indexed/send_order.jsonl]
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

from razor_amd.fec import RFEC_TUNE_GENERIC, Native, native  # noqa: E402
from regroup_bench import MAX_WINDOW, Window  # noqa: E402
from wire_encode_ab import SHAPES  # noqa: E402

E = 2  # dense out slots per group: the two lost segments
TABLES = ("hdr", "present", "meta", "fec_size", "parity_present", "base_id", "src_of", "slot_of")
BATCH_IN = ("shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--shapes", default="c3,c3full,c5")
    ap.add_argument("--shuffle", action="store_true", help="random arrival order instead of send order")
    ap.add_argument("--min-ms", type=float, default=250.0, help="timed work per variant")
    ap.add_argument("--steps", type=int, default=0, help="fixed step count (0: from --min-ms)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of librazor_fec_v1200.so")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("indexed_recover_bench.py: needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    lib = Native(1200, path=args.lib) if args.lib else native(1200)
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
        u8 = torch.uint8
        for w in wins:
            # chain B's own tables (chain A keeps Window.out), and one set of decode outputs per chain
            w.tab = {key: torch.zeros_like(w.out[key]) for key in TABLES}
            w.ws = torch.empty(max(16, lib.workspace_size(plan, w.G)), dtype=u8, device=dev)
            for c in "ab":
                setattr(w, "dec_" + c, dict(recovered=torch.zeros((w.G, 2), dtype=torch.int64, device=dev),
                                            out_shards=torch.zeros((w.G, E, P), dtype=u8, device=dev),
                                            out_hdr=torch.zeros((w.G, E, 20), dtype=u8, device=dev),
                                            out_index=torch.zeros((w.G, E), dtype=u8, device=dev)))

        def regroup_a():
            for w in wins:
                o = w.out
                lib.wire_regroup(plan, w.G, 1, w.N, w.recs.data_ptr(), w.payload.data_ptr(), P, S,
                                 *(o[key].data_ptr() for key in ("shards", "hdr", "present", "parity", "meta",
                                                                 "fec_size", "parity_present", "base_id", "src_of",
                                                                 "slot_of")), st)

        def decode_a():
            for w in wins:
                d = w.dec_a
                lib.recover_batch_out(plan, w.G, P, S, *(w.out[key].data_ptr() for key in BATCH_IN),
                                      d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                      d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), w.ws.data_ptr(), st)

        def regroup_b():
            for w in wins:
                lib.wire_regroup_index(plan, w.G, 1, w.N, w.recs.data_ptr(), S,
                                       *(w.tab[key].data_ptr() for key in TABLES), st)

        def decode_b():
            for w in wins:
                d, t = w.dec_b, w.tab
                lib.recover_indexed_out(plan, w.G, P, S, w.payload.data_ptr(), w.N, t["src_of"].data_ptr(),
                                        *(t[key].data_ptr() for key in ("hdr", "present", "meta", "fec_size",
                                                                        "parity_present")),
                                        d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                        d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), w.ws.data_ptr(), st)

        def decode_b_generic():
            lib.set_tuning(RFEC_TUNE_GENERIC)
            try:
                decode_b()
            finally:
                lib.set_tuning(0)

        def decode_b_matrix():
            for w in wins:
                d, t = w.dec_b, w.tab
                lib.recover_indexed_matrix_out(plan, w.G, P, S, w.payload.data_ptr(), w.N, t["src_of"].data_ptr(),
                                               *(t[key].data_ptr() for key in ("hdr", "present", "meta", "fec_size",
                                                                               "parity_present")),
                                               d["recovered"].data_ptr(), E, d["out_shards"].data_ptr(),
                                               d["out_hdr"].data_ptr(), d["out_index"].data_ptr(), st)

        def chain_b_matrix():
            regroup_b()
            decode_b_matrix()

        def chain_a():
            regroup_a()
            decode_a()

        def chain_b():
            regroup_b()
            decode_b()

        path = lib.lib.rfec_indexed_last_path
        path.restype, path.argtypes = C.c_uint32, []
        # B's outputs against A's, under both kernel selections of B, before anything is timed
        chain_a()
        torch.cuda.synchronize(dev)
        recovered = sum(int((w.dec_a["out_index"] != 0xFF).sum()) for w in wins)
        equal, paths = True, {}
        for label, dec in (("default", decode_b), ("generic", decode_b_generic)):
            for w in wins:
                for t in w.dec_b.values():
                    t.fill_(0x3C)
            regroup_b()
            dec()
            paths[label] = hex(int(path()))
            torch.cuda.synchronize(dev)
            for w in wins:
                a, b = w.dec_a, w.dec_b
                ok = a["out_index"] != 0xFF
                equal &= bool(torch.equal(a["recovered"], b["recovered"]) and
                              torch.equal(a["out_index"], b["out_index"]) and
                              torch.equal(a["out_hdr"][ok], b["out_hdr"][ok]) and
                              torch.equal(a["out_shards"][ok][:, :16 * cd], b["out_shards"][ok][:, :16 * cd]))
                equal &= all(torch.equal(w.out[key], w.tab[key]) for key in TABLES)
        rc |= 0 if equal and recovered else 1
        variants = {"chain_a": chain_a, "chain_b": chain_b, "decode_a": decode_a, "decode_b": decode_b}
        if paths["default"] != paths["generic"]:
            variants["decode_b_generic"] = decode_b_generic
        matrix = lib.packed_matrix_stride(plan, 1) != 0  # the plans rfec_recover_indexed_matrix_out takes
        matrix_equal = None
        if matrix:  # its four outputs against decode_b's (rfec_recover_indexed_out, default selection)
            regroup_b()
            decode_b()
            torch.cuda.synchronize(dev)
            ref = [{key: t.clone() for key, t in w.dec_b.items()} for w in wins]
            for w in wins:
                for t in w.dec_b.values():
                    t.fill_(0x3C)
            decode_b_matrix()
            paths["matrix"] = hex(int(path()))
            torch.cuda.synchronize(dev)
            matrix_equal = True
            for w, a in zip(wins, ref):
                b = w.dec_b
                ok = a["out_index"] != 0xFF
                matrix_equal &= bool(torch.equal(a["recovered"], b["recovered"]) and
                                     torch.equal(a["out_index"], b["out_index"]) and
                                     torch.equal(a["out_hdr"][ok], b["out_hdr"][ok]) and
                                     torch.equal(a["out_shards"][ok][:, :16 * cd], b["out_shards"][ok][:, :16 * cd]) and
                                     bool((b["out_shards"][:, :, 16 * cd:] == 0x3C).all()))
            del ref
            assert matrix_equal, "rfec_recover_indexed_matrix_out differs from rfec_recover_indexed_out"
            variants["decode_b_matrix"] = decode_b_matrix
            variants["chain_b_matrix"] = chain_b_matrix

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
            return {"mean_us": round(float(t.mean()), 2), "median_us": round(float(np.median(t)), 2),
                    "min_us": round(float(t.min()), 2), "p05_us": round(float(np.percentile(t, 5)), 2),
                    "p95_us": round(float(np.percentile(t, 95)), 2), "max_us": round(float(t.max()), 2),
                    "std_us": round(float(t.std()), 2), "timed_ms": round(float(t.sum()) * 1e-3, 1)}

        def below(x, y):  # x's repetitions lie below y's: the 95th percentile of x under the 5th of y
            return bool(np.percentile(x, 95) < np.percentile(y, 5))

        filled = sum(w.filled for w in wins)
        # the decode's payload rows: per out slot its line's parity and other members read, one slot written
        # (c3 / c5: rows of 4, so at most 4 reads; c3full: bounded the same way per step)
        dec_rows = args.groups * E * 5
        a_us, b_us = us["chain_a"], us["chain_b"]
        line = {
            "shape": name, "groups": args.groups, "windows": [w.G for w in wins], "k": k, "lines": n, "S": S,
            "stride": P, "records": sum(w.N for w in wins), "filled_rows": filled, "per_group": E,
            "arrival": "shuffled" if args.shuffle else "send order", "steps": steps,
            "timing": "stream events around the whole chain (all windows), variants alternating",
            "outputs_equal": equal, "recovered_segments": recovered, "indexed_path": paths,
            **{v: stat(t) for v, t in us.items()},
            "payload_bytes": {"chain_a_copy": 2 * filled * 16 * cd, "decode_at_most": dec_rows * 16 * cd},
            "b_over_a": round(float(b_us.mean() / a_us.mean()), 4),
            "b_over_a_median": round(float(np.median(b_us) / np.median(a_us)), 4),
            "b_max_below_a_min": bool(b_us.max() < a_us.min()), "b_p95_below_a_p05": below(b_us, a_us),
            "decode_b_over_decode_a": round(float(us["decode_b"].mean() / us["decode_a"].mean()), 4),
        }
        if "decode_b_generic" in us:
            g_us = us["decode_b_generic"]
            line["fused_over_generic"] = round(float(us["decode_b"].mean() / g_us.mean()), 4)
            line["fused_max_below_generic_min"] = bool(us["decode_b"].max() < g_us.min())
            line["fused_p95_below_generic_p05"] = below(us["decode_b"], g_us)
        if matrix:  # the bar: the new decode's 95th percentile below decode_b's 5th
            m_us = us["decode_b_matrix"]
            line["matrix_outputs_equal"] = matrix_equal
            line["matrix_over_decode_b"] = round(float(m_us.mean() / us["decode_b"].mean()), 4)
            line["matrix_over_decode_a"] = round(float(m_us.mean() / us["decode_a"].mean()), 4)
            line["matrix_p95_below_decode_b_p05"] = below(m_us, us["decode_b"])
            line["chain_matrix_over_chain_b"] = round(float(us["chain_b_matrix"].mean() / b_us.mean()), 4)
            line["chain_matrix_p95_below_chain_b_p05"] = below(us["chain_b_matrix"], b_us)
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
