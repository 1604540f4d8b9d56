"""Ragged wide rows (kth_topk_wide_rows_var_*) against the uniform call and
against what a caller does without them, on one GPU.

    python tools/bench_rows_var.py [--steps 50] [--rounds 3] > profiles/rows_var_bench.jsonl

Shapes: bfloat16 and float32 randn rows, rows in {8, 64, 512} x cols in
{32768, 131072}, top-k largest with k = 1024.  The legs alternate in one
process:
  (a) the uniform call (kth_topk_wide_rows_*) on the matrix,
  (b) the var call with d_lens[r] = cols and d_ks[r] = k: the feature's cost
      when nothing is ragged,
  (c) the var call with len_r uniform in [1, cols] and k_r uniform in [1, k],
  (d) what a caller does today for (c): a -inf fill of every row's columns at
      and past len_r into a copy, then the uniform call at k,
  (e) torch.topk(sorted=False) on that filled copy.
`rounds` rounds of one window per leg in turn; a window is `steps` calls (fewer
for a leg whose single call is long: about --window-s seconds a window) behind
a warm-up, wall clock around a window that ends with a synchronise.  One JSON
line per shape and key kind: every leg's windows (ms per call), their medians,
each leg's spread (max - min over its windows, relative to the median) and the
ratios (b)/(a), (c)/(a) and (c)/(d) of the medians.  b_above_a: (b)'s median is
above (a)'s by more than twice the larger of the two spreads.

Every result of the legs (a), (b) and (c) is certified on the device with
integer compares of order keys over each row's first len_r columns: ascending
columns below len_r, values equal to keys[idx], every better key kept, of the
keys equal to the k_r-th the first ones by column, #(key < v) < k_r <=
#(key <= v); entries at and past k_r are index -1 and the zero word, and d_cnt
is k_r.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

ROWS = (8, 64, 512)
COLS = (32768, 131072)
K = 1024
CERT_ELEMS = 1 << 24  # keys per certification chunk (int64 order keys)
WORST = 1 << 40       # the order key of a column at or past its row's end: after every real key


def order_key(t, kind):
    """int64 order keys of a float32 / bfloat16 tensor's elements; integer operations only."""
    import torch
    if kind == "f32":
        b = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        key = torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)
        return torch.where((b & 0x7FFFFFFF) > 0x7F800000, torch.full_like(b, 0xFFFFFFFF), key)
    b = t.view(torch.int16).to(torch.int64) & 0xFFFF
    key = torch.where(b >= 0x8000, b ^ 0xFFFF, b | 0x8000)
    return torch.where((b & 0x7FFF) > 0x7F80, torch.full_like(b, 0xFFFF), key)


def certify(keys, kind, lens, kr, k, vals, idx, cnt):
    """The ragged top-k largest certificate of every row (kr >= 1 everywhere); chunked over rows."""
    import torch
    rows, cols = keys.shape
    top = 0xFFFFFFFF if kind == "f32" else 0xFFFF
    if not bool((cnt.long() == kr).all()):
        return False
    step = max(1, CERT_ELEMS // cols)
    col = torch.arange(cols, device=keys.device).unsqueeze(0)
    slot = torch.arange(k, device=keys.device).unsqueeze(0)
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        n, q = lens[sl].long().unsqueeze(1), kr[sl].unsqueeze(1)
        o = torch.where(col < n, top - order_key(keys[sl], kind), torch.full((1, 1), WORST, device=keys.device))
        live = slot < q
        ix = idx[sl].long()
        raw = vals[sl].view(torch.int32 if kind == "f32" else torch.int16)
        if not bool(((ix == -1) & (raw == 0))[~live].all()):  # the padding
            return False
        if not bool(((ix >= 0) & (ix < n))[live].all()):
            return False
        if not bool(((ix[:, 1:] > ix[:, :-1]) | ~live[:, 1:]).all()):
            return False
        ixc = ix.clamp(min=0)
        ov = torch.where(live, top - order_key(vals[sl], kind), torch.full((1, 1), -1, device=keys.device))
        if not bool(((torch.gather(o, 1, ixc) == ov) | ~live).all()):
            return False
        v = ov.max(dim=1, keepdim=True).values
        if not bool((((ov < v) & live).sum(dim=1) == (o < v).sum(dim=1)).all()):  # every better key is kept
            return False
        kept_tie = (ov == v) & live
        last = torch.where(kept_tie, ix, torch.full_like(ix, -1)).max(dim=1, keepdim=True).values
        if not bool((((o == v) & (col <= last)).sum(dim=1) == kept_tie.sum(dim=1)).all()):  # the first ties
            return False
        lt, le = (o < v).sum(dim=1), (o <= v).sum(dim=1)
        if not bool(((lt < q.squeeze(1)) & (le >= q.squeeze(1))).all()):
            return False
    return True


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x7A66)
    ap.add_argument("--kinds", default="bf16,f32")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--cols", default=",".join(map(str, COLS)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: the legs and the certification are ordered
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    k = K

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

    for rows in map(int, args.rows.split(",")):
        for cols in map(int, args.cols.split(",")):
            for kind in args.kinds.split(","):
                f32 = kind == "f32"
                keys = torch.randn((rows, cols), generator=g, device=dev, dtype=torch.float32)
                if not f32:
                    keys = keys.to(torch.bfloat16)
                full_l = torch.full((rows,), cols, dtype=torch.int32, device=dev)
                full_k = torch.full((rows,), k, dtype=torch.int32, device=dev)
                rag_l = torch.randint(1, cols + 1, (rows,), generator=g, device=dev, dtype=torch.int32)
                rag_k = torch.randint(1, k + 1, (rows,), generator=g, device=dev, dtype=torch.int32)
                vals = torch.zeros(rows * k, dtype=keys.dtype, device=dev)
                idx = torch.zeros(rows * k, dtype=torch.int32, device=dev)
                cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
                filled = torch.empty_like(keys)
                past = torch.arange(cols, device=dev).unsqueeze(0) >= rag_l.unsqueeze(1)
                ninf = torch.full((1, 1), float("-inf"), dtype=keys.dtype, device=dev)

                def uniform(src):
                    if f32:
                        sel.topk_rows_wide(src, rows, cols, k, vals, idx, largest=True, f32=True)
                    else:
                        sel.topk_rows_wide16(src, rows, cols, k, vals, idx, largest=True)

                def var(lens, ks):
                    if f32:
                        sel.topk_rows_wide_var(keys, rows, cols, k, vals, idx, largest=True, f32=True, d_lens=lens,
                                               d_ks=ks, d_cnt=cnt)
                    else:
                        sel.topk_rows_wide16_var(keys, rows, cols, k, vals, idx, largest=True, d_lens=lens, d_ks=ks,
                                                 d_cnt=cnt)

                def leg_d():
                    torch.where(past, ninf, keys, out=filled)
                    uniform(filled)

                legs = (("a", lambda: uniform(keys)), ("b", lambda: var(full_l, full_k)),
                        ("c", lambda: var(rag_l, rag_k)), ("d", leg_d),
                        ("e", lambda: torch.topk(filled, k, dim=1, largest=True, sorted=False)))

                def certified(name, lens, kr):
                    cnt.fill_(k if name == "a" else -1)
                    dict(legs)[name]()
                    sel.sync()
                    return certify(keys, kind, lens, kr, k, vals.view(rows, k), idx.view(rows, k), cnt)

                ok = {"a": certified("a", full_l, full_k.long()), "b": certified("b", full_l, full_k.long()),
                      "c": certified("c", rag_l, torch.minimum(rag_k, rag_l).long())}
                leg_d()  # `filled` for (e)
                steps = {name: steps_for(fn) for name, fn in legs}
                ts = {name: [] for name, _ in legs}
                for _ in range(args.rounds):
                    for name, fn in legs:
                        ts[name].append(window(fn, steps[name]))
                med = {n: statistics.median(v) for n, v in ts.items()}
                spread = {n: (max(v) - min(v)) / med[n] for n, v in ts.items()}
                plan = kselect.wide_rows_plan(rows, cols, num_cu) if f32 else kselect.wide_rows_plan16(rows, cols, num_cu)
                print(json.dumps({
                    "leg": "shape", "what": "topk_largest", "kind": kind, "rows": rows, "cols": cols, "k": k,
                    "form": "fused" if plan[0] == 1 else "split", "slices": plan[0],
                    "mean_len": round(float(rag_l.float().mean()), 1), "mean_k": round(float(rag_k.float().mean()), 1),
                    "window_ms": {n: [round(t * 1e3, 4) for t in v] for n, v in ts.items()},
                    "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                    "spread": {n: round(v, 3) for n, v in spread.items()},
                    "b_over_a": round(med["b"] / med["a"], 3), "c_over_a": round(med["c"] / med["a"], 3),
                    "c_over_d": round(med["c"] / med["d"], 3), "c_over_e": round(med["c"] / med["e"], 3),
                    "b_above_a": bool(med["b"] - med["a"] > 2 * max(spread["a"], spread["b"]) * med["a"]),
                    "verified": ok}), flush=True)
                del keys, filled, past, vals, idx
                torch.cuda.empty_cache()
    print(json.dumps({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "num_cu": num_cu}), flush=True)
    sel.close()


if __name__ == "__main__":
    main()
