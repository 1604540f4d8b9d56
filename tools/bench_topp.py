"""Top-p rows (kth_topp_wide_rows_*) against the var top-k alone and against
torch's sort -> softmax -> cumsum -> mask, on one GPU.

    python tools/bench_topp.py [--steps 50] [--rounds 3] >> profiles/topp_bench.jsonl
    python tools/bench_topp.py --sweep >> profiles/topp_bench.jsonl

Shapes: bfloat16 and float32 randn * 4 rows, rows in {1, 8, 64, 512} x cols in
{32768, 131072}, p in {0.5, 0.9, 0.99}, T = 1, cap k = 1024.  The legs
alternate in one process:
  (t) the topp call: nucleus and cap jointly, values, columns and d_cnt,
  (n) the nucleus call alone (d_n and d_thr),
  (a) the var top-k largest alone with the same cap (d_ks[r] = k): what a
      caller of the library pays today before any top-p filter,
  (b) torch: sort descending, softmax, cumsum, mask (mass before a key < p).
`rounds` rounds of one window per leg in turn; a window is `steps` calls (fewer
for a leg whose single call is long: about --window-s seconds a window) behind
a warm-up, wall clock around a window that ends with a synchronise.  One JSON
line per shape, kind and p: every leg's windows (ms per call), their medians,
each leg's spread (max - min over its windows, relative to the median) and the
ratios (t)/(a), the cost of the filter on top of a call users already make,
and (t)/(b).  t_above_a: (t)'s median is above (a)'s by more than twice the
larger of the two spreads; a difference inside the spread decides nothing.

Every row is certified on the device in float64 with the header's band,
eps = 2^-16 + cols * 2^-39: S(n) >= p Z (1 - eps) and (n == 1 or S(n - 1) <
p Z (1 + eps)) for the n of the nucleus call, d_thr equal to the n-th largest
key, the topp call's d_cnt equal to min(n, k), and its values and columns
certified as the top d_cnt of the row by tools/bench_rows_var.py's integer
certificate.

--sweep: the (t) and (n) legs under forced plans (slices 1 .. 256) per shape,
for the plan rule's thresholds; lines with "leg": "sweep".
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROWS = (1, 8, 64, 512)
COLS = (32768, 131072)
PS = (0.5, 0.9, 0.99)
K = 1024
SWEEP = (1, 4, 8, 16, 32, 64, 128, 256)
CERT_ELEMS = 1 << 23  # keys per certification chunk (float64 weights and their sort)


def certify_band(keys, p, temp, n, thr):
    """The band of every row, in float64 on the device (rows without NaN or +inf); chunked over rows."""
    import torch
    rows, cols = keys.shape
    eps = 2.0 ** -16 + cols * 2.0 ** -39
    step = max(1, CERT_ELEMS // cols)
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        x = torch.sort(keys[sl].double(), dim=1, descending=True).values
        s = torch.exp((x - x[:, :1]) / temp).cumsum(dim=1)
        pz = p * s[:, -1:]
        nn = n[sl].long().unsqueeze(1)
        if not bool(((nn >= 1) & (nn <= cols)).all()):
            return False
        at = torch.gather(s, 1, nn - 1)
        before = torch.gather(s, 1, (nn - 2).clamp(min=0))
        if not bool(((at >= pz * (1 - eps)) & ((nn == 1) | (before < pz * (1 + eps)))).all()):
            return False
        if not bool((torch.gather(x, 1, nn - 1).squeeze(1) == thr[sl].double()).all()):
            return False
    return True


def main():
    import torch

    import kselect
    from bench_rows_var import certify
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x70BB)
    ap.add_argument("--kinds", default="bf16,f32")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--cols", default=",".join(map(str, COLS)))
    ap.add_argument("--ps", default=",".join(map(str, PS)))
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: the legs and the certification are ordered
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    k, temp = K, 1.0

    def window(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sel.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def steps_for(fn):
        for _ in range(args.warmup):
            fn()
        t1 = window(fn, 1)
        return max(1, min(args.steps, int(args.window_s / max(t1, 1e-7))))

    def measure(legs):
        steps = {name: steps_for(fn) for name, fn in legs}
        ts = {name: [] for name, _ in legs}
        for _ in range(args.rounds):
            for name, fn in legs:
                ts[name].append(window(fn, steps[name]))
        med = {n: statistics.median(v) for n, v in ts.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in ts.items()}
        return ts, med, spread

    for rows in map(int, args.rows.split(",")):
        for cols in map(int, args.cols.split(",")):
            for kind in args.kinds.split(","):
                f32 = kind == "f32"
                keys = torch.randn((rows, cols), generator=g, device=dev, dtype=torch.float32) * 4
                if not f32:
                    keys = keys.to(torch.bfloat16)
                sel.reserve_topp_rows(rows, cols)
                full_l = torch.full((rows,), cols, dtype=torch.int32, device=dev)
                full_k = torch.full((rows,), k, dtype=torch.int32, device=dev)
                vals = torch.zeros(rows * k, dtype=keys.dtype, device=dev)
                idx = torch.zeros(rows * k, dtype=torch.int32, device=dev)
                cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
                d_n = torch.zeros(rows, dtype=torch.int32, device=dev)
                d_thr = torch.zeros(rows, dtype=keys.dtype, device=dev)
                plan = kselect.wide_rows_plan(rows, cols, num_cu) if f32 else kselect.wide_rows_plan16(rows, cols, num_cu)
                for p in map(float, args.ps.split(",")):
                    def leg_t():
                        if f32:
                            sel.topp_rows_wide(keys, rows, cols, k, vals, idx, p=p, temp=temp, d_cnt=cnt)
                        else:
                            sel.topp_rows_wide16(keys, rows, cols, k, vals, idx, p=p, temp=temp, d_cnt=cnt)

                    def leg_n():
                        if f32:
                            sel.nucleus_rows_wide(keys, rows, cols, d_n, d_thr, p=p, temp=temp)
                        else:
                            sel.nucleus_rows_wide16(keys, rows, cols, d_n, d_thr, p=p, temp=temp)

                    def leg_a():
                        if f32:
                            sel.topk_rows_wide_var(keys, rows, cols, k, vals, idx, largest=True, f32=True, d_ks=full_k,
                                                   d_cnt=cnt)
                        else:
                            sel.topk_rows_wide16_var(keys, rows, cols, k, vals, idx, largest=True, d_ks=full_k, d_cnt=cnt)

                    def leg_b():
                        s, i = torch.sort(keys.float(), dim=1, descending=True)
                        pr = torch.softmax(s / temp, dim=1)
                        return i, (pr.cumsum(dim=1) - pr) < p

                    cnt.fill_(-1), d_n.fill_(-1)
                    leg_n(), leg_t()
                    sel.sync()
                    kr = torch.minimum(d_n, full_k)
                    ok = {"band": certify_band(keys, p, temp, d_n, d_thr),
                          "topp": bool((kr >= 1).all()) and certify(keys, kind, full_l, kr.long(), k, vals.view(rows, k),
                                                                     idx.view(rows, k), cnt)}
                    common = {"kind": kind, "rows": rows, "cols": cols, "k": k, "p": p, "temp": temp,
                              "mean_n": round(float(d_n.float().mean()), 1), "capped_rows": int((d_n > k).sum())}
                    if args.sweep:
                        for slices in SWEEP:
                            sel.wide_rows_force(slices, 0)
                            ts, med, spread = measure((("t", leg_t), ("n", leg_n)))
                            sel.wide_rows_force(0, 0)
                            print(json.dumps({"leg": "sweep", **common, "slices": slices, "auto_slices": plan[0],
                                              "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                                              "spread": {n: round(v, 3) for n, v in spread.items()}}), flush=True)
                        continue
                    ts, med, spread = measure((("t", leg_t), ("n", leg_n), ("a", leg_a), ("b", leg_b)))
                    print(json.dumps({
                        "leg": "shape", "what": "topp", **common, "form": "fused" if plan[0] == 1 else "split",
                        "slices": plan[0],
                        "window_ms": {n: [round(t * 1e3, 4) for t in v] for n, v in ts.items()},
                        "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                        "spread": {n: round(v, 3) for n, v in spread.items()},
                        "t_over_a": round(med["t"] / med["a"], 3), "t_over_b": round(med["t"] / med["b"], 3),
                        "n_over_a": round(med["n"] / med["a"], 3),
                        "t_above_a": bool(med["t"] - med["a"] > 2 * max(spread["a"], spread["t"]) * med["a"]),
                        "verified": ok}), flush=True)
                del keys, vals, idx
                torch.cuda.empty_cache()
    print(json.dumps({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "num_cu": num_cu}), flush=True)
    sel.close()


if __name__ == "__main__":
    main()
