"""Sorted per-row top-k against what a caller does without it, on one GPU.

    python tools/bench_sort_rows.py [--steps 50] [--rounds 3] > profiles/sort_rows_bench.jsonl

Shapes: 65536 x 4096 at k = 64 and 1048576 x 256 at k = 8 (topk_rows /
topk_rows16), wide rows 64 x 131072 and 512 x 131072 at k = 50, 1024 and 4096
(topk_rows_wide / topk_rows_wide16); float32 and bfloat16 randn keys, largest.
Four legs alternate in one process:
  (s) the call with sorted=True,
  (u) the same call unsorted,
  (c) what a caller does today: (u), then torch.sort(stable=True) over d_vals
      and a gather of d_idx by its permutation,
  (b) torch.topk(sorted=True) on the matrix.
`rounds` windows of `steps` (>= 20) calls after a warm-up, wall clock around a
window that ends with a synchronise; then one more window a leg in the reverse
order, so that no leg always follows the same neighbour.

Every (s) result is certified on the device against (c): the values bit for
bit, the indices exactly (randn keys hold no NaN and no zero of either sign, so
torch's stable descending sort and the library's order agree on every tie).

One JSON line per leg and window; a summary line per shape and kind with the
medians, (s) - (u) against (c) - (u) (the sort's own cost either way), s / b and
each leg's window spread (max - min over the median).  Nothing is asserted about
the times: lines where (s) loses are reported as they fall.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

SHAPES = ([("rows", 65536, 4096, 64), ("rows", 1048576, 256, 8)] +
          [("wide", rows, 131072, k) for rows in (64, 512) for k in (50, 1024, 4096)])
ROW_CHUNK = 8192


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x50F7)
    ap.add_argument("--kinds", default="f32,bf16")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("windows of at least 20 calls")
    dev = torch.device("cuda", 0)
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: (c)'s torch.sort is ordered after its top-k call
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)

    def emit(rec):
        print(json.dumps(rec), flush=True)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        sel.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    summary = []
    for form, rows, cols, k in SHAPES:
        for kind in args.kinds.split(","):
            f32 = kind == "f32"
            keys = torch.empty((rows, cols), dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
            for part in torch.split(keys, ROW_CHUNK):
                part.copy_(torch.randn(part.shape, generator=g, device=dev, dtype=torch.float32))
            vals_s, vals_u = (torch.zeros(rows * k, dtype=keys.dtype, device=dev) for _ in range(2))
            idx_s, idx_u = (torch.zeros(rows * k, dtype=torch.int32, device=dev) for _ in range(2))

            def call(vals, idx, srt):
                if form == "rows" and f32:
                    sel.topk_rows(keys, rows, cols, k, vals, idx, largest=True, f32=True, sorted=srt)
                elif form == "rows":
                    sel.topk_rows16(keys, rows, cols, k, vals, idx, largest=True, sorted=srt)
                elif f32:
                    sel.topk_rows_wide(keys, rows, cols, k, vals, idx, largest=True, f32=True, sorted=srt)
                else:
                    sel.topk_rows_wide16(keys, rows, cols, k, vals, idx, largest=True, sorted=srt)

            def leg_s():
                call(vals_s, idx_s, True)

            def leg_u():
                call(vals_u, idx_u, False)

            def leg_c():
                call(vals_u, idx_u, False)
                v, perm = torch.sort(vals_u.view(rows, k), dim=1, descending=True, stable=True)
                return v, torch.gather(idx_u.view(rows, k), 1, perm)

            def leg_b():
                return torch.topk(keys, k, dim=1, largest=True, sorted=True)

            legs = (("s_sorted", leg_s), ("u_unsorted", leg_u), ("c_unsorted_then_torch_sort", leg_c),
                    ("b_torch_topk_sorted", leg_b))
            for _, fn in legs:
                for _ in range(args.warmup):
                    fn()
            sel.sync()
            leg_s()
            cv, ci = leg_c()
            sel.sync()
            torch.cuda.synchronize()
            bits = torch.int32 if f32 else torch.int16
            ok = bool((vals_s.view(bits) == cv.reshape(-1).view(bits)).all()) and bool((idx_s == ci.reshape(-1)).all())
            del cv, ci
            ts = {name: [] for name, _ in legs}
            base = {"form": form, "kind": kind, "rows": rows, "cols": cols, "k": k, "steps": args.steps}
            for r in range(args.rounds):
                for name, fn in legs:
                    dt_ = window(fn)
                    ts[name].append(dt_)
                    emit({"leg": name, **base, "round": r, "ms": round(dt_ * 1e3, 4), "verified": ok})
            for name, fn in reversed(legs):
                dt_ = window(fn)
                ts[name].append(dt_)
                emit({"leg": name, **base, "round": args.rounds, "ms": round(dt_ * 1e3, 4), "verified": ok})
            med = {name: statistics.median(v) for name, v in ts.items()}
            s, u, c, b = (med[name] for name, _ in legs)
            summary.append({"leg": "summary", **base,
                            **{f"{name}_median_ms": round(v * 1e3, 4) for name, v in med.items()},
                            **{f"{name}_spread": round((max(v) - min(v)) / med[name], 3) for name, v in ts.items()},
                            "s_minus_u_ms": round((s - u) * 1e3, 4), "c_minus_u_ms": round((c - u) * 1e3, 4),
                            "s_over_b": round(s / b, 3), "s_faster_than_c": bool(s < c), "s_faster_than_b": bool(s < b),
                            "verified": ok})
            del keys, vals_s, vals_u, idx_s, idx_u
            torch.cuda.empty_cache()
    for rec in summary:
        emit(rec)
    emit({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode()})
    sel.close()


if __name__ == "__main__":
    main()
