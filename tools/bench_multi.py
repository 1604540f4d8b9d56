"""Several ranks of one array: one multi call against the same ranks as single selects.

    python tools/bench_multi.py [--log2n 30] [--steps 10] [--rounds 3] > profiles/multi_bench.jsonl

n = 2^log2n keys of the flagship family (uniform_half), as int32 and as the
same values in float32.  For m in 1, 2, 4, 8 the ranks are the m quantiles
i n / (m + 1).  Two legs alternate in one process, `rounds` windows of `steps`
calls each (wall clock around the window, as bench.py times), after both are
warmed up:
  multi    one kth_select_multi_*_async call for the m ranks
  singles  the same m ranks as m kth_select_*_async calls (the path a caller
           had before the multi call; its kernels are unchanged)
After the windows, one more window of multi calls runs with the ctx's timing
events on: main_ms is the streaming launch alone (kth_ctx_take_timing).

Every answer of every window is rank-certified on the device with integer
operations, as tools/bench_f32.py does: v is the k-th smallest iff
#(key < v) < k <= #(key <= v), float keys compared as ordered int32 words.

One JSON line per leg and window (ms per call of m ranks, verified), then one
summary line per key kind and m: the medians, their ratio, and whether the
multi call is faster.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

from bench_f32 import certify, ordered_i32  # noqa: E402  (tools/ is this script's directory)


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ranks", type=int, nargs="*", default=[1, 2, 4, 8])
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    sel = kselect.Selector(0)
    sel.reserve(n)
    sel.reserve_multi(n, max(args.ranks))

    ikeys = torch.empty(n, dtype=torch.int32, device=dev)
    sel.fill(ikeys, n, "uniform_half")
    sel.sync()
    fkeys = torch.empty(n, dtype=torch.float32, device=dev)
    fwords = torch.empty(n, dtype=torch.int32, device=dev)  # the certificates' view: ordered int32 words
    for f, w, i in zip(torch.split(fkeys, 1 << 28), torch.split(fwords, 1 << 28), torch.split(ikeys, 1 << 28)):
        f.copy_(i)
        w.copy_(ordered_i32(f))
    kinds = {"i32": (ikeys, ikeys, False, torch.int32), "f32": (fkeys, fwords, True, torch.float32)}

    def emit(rec):
        print(json.dumps(rec), flush=True)

    for name, (keys, words, f32, dt) in kinds.items():
        for m in args.ranks:
            ks = [(i + 1) * n // (m + 1) for i in range(m)]
            out = torch.zeros(m, dtype=dt, device=dev)

            def window(leg, steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    if leg == "multi":
                        sel.select_multi_async(keys, n, ks, out, f32=f32)
                    else:
                        for i, k in enumerate(ks):
                            sel.select_async(keys, n, k, out[i:i + 1], f32=f32)
                sel.sync()
                return (time.perf_counter() - t0) / steps

            def verified(leg):
                got = (ordered_i32(out) if f32 else out).cpu().tolist()
                if leg == "multi":
                    clean = all(sel.multi_stats(i)["error"] == 0 for i in range(m))
                else:
                    clean = sel.stats()["error"] == 0
                return clean and all(certify(words, v, k) for v, k in zip(got, ks))

            for leg in ("multi", "singles"):
                window(leg, args.warmup)
            ms = {"multi": [], "singles": []}
            for r in range(args.rounds):
                for leg in ("singles", "multi"):
                    out.zero_()
                    t = window(leg, args.steps)
                    ms[leg].append(t * 1e3)
                    emit({"leg": f"{leg}_{name}", "m": m, "round": r, "log2n": args.log2n, "steps": args.steps,
                          "ms": round(t * 1e3, 4), "verified": bool(verified(leg))})
            sel.enable_timing(True)
            sel.take_timing()
            window("multi", args.steps)
            nsel, main_ms, total_ms = sel.take_timing()
            sel.enable_timing(False)
            paths = [sel.multi_stats(i)["path"] for i in range(m)]
            mm, sm = statistics.median(ms["multi"]), statistics.median(ms["singles"])
            emit({"leg": f"summary_{name}", "m": m, "log2n": args.log2n, "multi_median_ms": round(mm, 4),
                  "singles_median_ms": round(sm, 4), "multi_over_singles": round(mm / sm, 3),
                  "multi_faster": bool(mm < sm), "timed_selects_per_call": nsel / args.steps,
                  "main_ms": round(main_ms / args.steps, 4), "device_total_ms": round(total_ms / args.steps, 4),
                  "paths": paths, "build_id": kselect.LIB.kth_build_id().decode()})
    sel.close()


if __name__ == "__main__":
    main()
