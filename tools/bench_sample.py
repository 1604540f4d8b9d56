"""Sampling rows (kth_sample_wide_rows_*) against what a caller of the library
does today and against torch alone, on one GPU.

    python tools/bench_sample.py [--steps 50] [--rounds 3] >> profiles/sample_bench.jsonl

Shapes and inputs of tools/bench_topp.py: bfloat16 and float32 randn * 4 rows,
rows in {1, 8, 64, 512} x cols in {32768, 131072}, p in {0.5, 0.9, 0.99}, T = 1,
a cap of 1024 and no cap.  One uniform number a row, drawn once per shape.  The
legs alternate in one process:
  (s) the sample call: one token and d_cnt a row,
  (t) the topp call alone at cap 1024 (values, columns, d_cnt),
  (c) what a caller does today: (t), then torch over its output -- the padding
      masked, softmax, cumsum, compare with the same u, gather the column,
  (b) torch alone: sort descending, softmax, cumsum, the top-p mask and the cap,
      multinomial, gather.
Without a cap only (s) and (b) exist: the topp call's cap is its output stride.
`rounds` rounds of one window per leg in turn; a window is `steps` calls (fewer
for a leg whose single call is long: about --window-s seconds a window) behind
a warm-up, wall clock around a window that ends with a synchronise.  One JSON
line per shape, kind, p and cap: every leg's windows (ms per call), their
medians, each leg's spread (max - min over its windows, relative to the median)
and the ratios (s)/(c) and (s)/(b).  s_above_c: (s)'s median is above (c)'s by
more than twice the larger of the two spreads; a difference inside the spread
decides nothing.

Every row of every (s) line is certified on the device in float64 with the
header's bands, eps = 2^-16 + cols * 2^-39: d_cnt = min(n, cap) for an n in the
nucleus's band, and for j, the position of d_tok in the stable descending order,
1 <= j <= d_cnt, S(j) >= A (1 - 2 eps) and (j == 1 or S(j - 1) <= A (1 + 2 eps)),
A = u S(d_cnt).
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
CAPS = (1024, 0)
CERT_ELEMS = 1 << 23  # keys per certification chunk (float64 weights and their sort)


def certify_sample(keys, p, temp, cap, us, tok, cnt):
    """Both bands of every row, in float64 on the device (rows without NaN or +inf); chunked over rows."""
    import torch
    rows, cols = keys.shape
    eps = 2.0 ** -16 + cols * 2.0 ** -39
    step = max(1, CERT_ELEMS // cols)
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        x, order = torch.sort(keys[sl].double(), dim=1, descending=True, stable=True)
        s = torch.exp((x - x[:, :1]) / temp).cumsum(dim=1)
        pz = p * s[:, -1:]
        n = cnt[sl].long().unsqueeze(1)
        if not bool(((n >= 1) & (n <= cols)).all()):
            return False
        at = torch.gather(s, 1, n - 1)
        before = torch.gather(s, 1, (n - 2).clamp(min=0))
        upper = (n == 1) | (before < pz * (1 + eps))
        inside = (at >= pz * (1 - eps)) & upper if p < 1.0 else n == cols
        if cap > 0:  # the cap binds: some n of the band is at or above it
            inside = torch.where(n == cap, upper if p < 1.0 else torch.full_like(upper, cap <= cols), inside & (n < cap))
        if not bool(inside.all()):
            return False
        t = tok[sl].long().unsqueeze(1)
        if not bool(((t >= 0) & (t < cols)).all()):
            return False
        j = (order == t).int().argmax(dim=1, keepdim=True) + 1
        a = us[sl].double().clamp(0.0, 1.0).unsqueeze(1) * at
        sj = torch.gather(s, 1, j - 1)
        sb = torch.gather(s, 1, (j - 2).clamp(min=0))
        if not bool(((j <= n) & (sj >= a * (1 - 2 * eps)) & ((j == 1) | (sb <= a * (1 + 2 * eps)))).all()):
            return False
    return True


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5A3B)
    ap.add_argument("--kinds", default="bf16,f32")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--cols", default=",".join(map(str, COLS)))
    ap.add_argument("--ps", default=",".join(map(str, PS)))
    ap.add_argument("--caps", default=",".join(map(str, CAPS)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: the legs and the certification are ordered
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    temp = 1.0

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
                us = torch.rand(rows, generator=g, device=dev, dtype=torch.float32)
                sel.reserve_sample_rows(rows, cols)
                sel.reserve_topp_rows(rows, cols)
                tok = torch.zeros(rows, dtype=torch.int32, device=dev)
                cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
                plan = kselect.wide_rows_plan(rows, cols, num_cu) if f32 else kselect.wide_rows_plan16(rows, cols, num_cu)
                for cap in map(int, args.caps.split(",")):
                    k = max(cap, 1)
                    vals = torch.zeros(rows * k, dtype=keys.dtype, device=dev)
                    idx = torch.zeros(rows * k, dtype=torch.int32, device=dev)
                    tcnt = torch.zeros(rows, dtype=torch.int32, device=dev)
                    ranks = torch.arange(cols, device=dev).unsqueeze(0)
                    for p in map(float, args.ps.split(",")):
                        def leg_s():
                            if f32:
                                sel.sample_rows_wide(keys, rows, cols, us, tok, k=cap, p=p, temp=temp, d_cnt=cnt)
                            else:
                                sel.sample_rows_wide16(keys, rows, cols, us, tok, k=cap, p=p, temp=temp, d_cnt=cnt)

                        def leg_t():
                            if f32:
                                sel.topp_rows_wide(keys, rows, cols, k, vals, idx, p=p, temp=temp, d_cnt=tcnt)
                            else:
                                sel.topp_rows_wide16(keys, rows, cols, k, vals, idx, p=p, temp=temp, d_cnt=tcnt)

                        def leg_c():
                            leg_t()
                            i = idx.view(rows, k)
                            x = vals.view(rows, k).float().masked_fill(i < 0, float("-inf"))
                            cs = torch.softmax(x / temp, dim=1).cumsum(dim=1)
                            j = (cs <= us.unsqueeze(1)).sum(dim=1, keepdim=True).clamp(max=k - 1)
                            return torch.gather(i, 1, j)

                        def leg_b():
                            s, i = torch.sort(keys.float(), dim=1, descending=True)
                            pr = torch.softmax(s / temp, dim=1)
                            keep = (pr.cumsum(dim=1) - pr) < p
                            if cap > 0:
                                keep &= ranks < cap
                            j = torch.multinomial(pr * keep, 1)
                            return torch.gather(i, 1, j)

                        tok.fill_(-2), cnt.fill_(-1)
                        leg_s()
                        sel.sync()
                        ok = certify_sample(keys, p, temp, cap, us, tok, cnt)
                        legs = (("s", leg_s), ("t", leg_t), ("c", leg_c), ("b", leg_b)) if cap > 0 else \
                            (("s", leg_s), ("b", leg_b))
                        ts, med, spread = measure(legs)
                        line = {"leg": "shape", "what": "sample", "kind": kind, "rows": rows, "cols": cols, "cap": cap,
                                "p": p, "temp": temp, "mean_cnt": round(float(cnt.float().mean()), 1),
                                "form": "fused" if plan[0] == 1 else "split", "slices": plan[0],
                                "window_ms": {n: [round(t * 1e3, 4) for t in v] for n, v in ts.items()},
                                "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                                "spread": {n: round(v, 3) for n, v in spread.items()},
                                "s_over_b": round(med["s"] / med["b"], 3), "verified": ok}
                        if cap > 0:
                            line["s_over_c"] = round(med["s"] / med["c"], 3)
                            line["s_over_t"] = round(med["s"] / med["t"], 3)
                            line["s_above_c"] = bool(med["s"] - med["c"] > 2 * max(spread["c"], spread["s"]) * med["c"])
                        print(json.dumps(line), flush=True)
                    del vals, idx
                del keys
                torch.cuda.empty_cache()
    print(json.dumps({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "num_cu": num_cu}), flush=True)
    sel.close()


if __name__ == "__main__":
    main()
