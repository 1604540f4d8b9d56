"""float32 against int32 keys on one GPU: the one-array select and top-k.

    python tools/bench_f32.py [--log2n 30] [--steps 20] [--rounds 3] > profiles/f32_bench.jsonl

Select: n = 2^log2n, k = n / 2; float32 keys from a seeded torch.randn, int32
keys of the flagship family (uniform_half).  The two alternate in one process,
`rounds` windows of `steps` asynchronous selects each (wall clock around the
window, as bench.py times), after both are warmed up.  Top-k (smallest, values
and indices) of the same arrays at k = 1024, 2^20, 2^24, the same way.

Every answer of a window is rank-certified on the device with integer
operations: v is the k-th smallest iff #(key < v) < k <= #(key <= v), the float
keys compared as their ordered int32 words (b ^ 0x7FFFFFFF for negative b, NaN
-> INT32_MAX), never as floats, which would merge +-0 and drop NaNs.  A top-k
window is certified through its k-th value the same way, with strictly
increasing indices and vals == keys[idx].

One JSON line per leg and window: ms (per call), gkeys_per_s, path, verified.
The last line compares the select medians: the float32 select counts as slower
when it is behind the int32 median by more than the spread (max - min) of the
int32 windows of this run.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))


def ordered_i32(t):
    import torch
    b = t.view(torch.int32)
    s = torch.where(b < 0, b ^ 0x7FFFFFFF, b)
    return torch.where((b & 0x7FFFFFFF) > 0x7F800000, torch.full_like(b, 0x7FFFFFFF), s)


def certify(words, v, k):
    """words: int32 tensor in key order (chunks bound the temporaries); v: int"""
    import torch
    lt = le = 0
    for c in torch.split(words, 1 << 28):
        lt += int((c < v).sum())
        le += int((c <= v).sum())
    return lt < k <= le


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xF32)
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    sel = kselect.Selector(0)
    sel.reserve(n)

    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    fkeys = torch.randn(n, generator=g, device=dev, dtype=torch.float32)
    ikeys = torch.empty(n, dtype=torch.int32, device=dev)
    sel.fill(ikeys, n, "uniform_half")
    sel.sync()
    # the certificates' views of the keys: ordered int32 words, built chunk-wise
    fwords = torch.empty(n, dtype=torch.int32, device=dev)
    for a, b in zip(torch.split(fwords, 1 << 28), torch.split(fkeys, 1 << 28)):
        a.copy_(ordered_i32(b))
    kinds = {"f32": (fkeys, fwords, True, torch.float32), "i32": (ikeys, ikeys, False, torch.int32)}

    def to_word(x, f32):  # a result tensor -> python ints in key order
        return (ordered_i32(x) if f32 else x).cpu().tolist()

    def emit(rec):
        print(json.dumps(rec), flush=True)

    # ---- select
    k = n // 2
    outs = {name: torch.zeros(args.steps, dtype=dt, device=dev) for name, (_, _, _, dt) in kinds.items()}

    def window_select(name, steps):
        keys, _, f32, _ = kinds[name]
        out = outs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            sel.select_async(keys, n, k, out[i:i + 1], f32=f32)
        sel.sync()
        return (time.perf_counter() - t0) / steps

    for name in kinds:
        window_select(name, args.warmup)
    sel_gk = {"f32": [], "i32": []}
    for r in range(args.rounds):
        for name in ("i32", "f32"):
            _, words, f32, _ = kinds[name]
            outs[name].zero_()
            dt = window_select(name, args.steps)
            st = sel.stats()
            answers = set(to_word(outs[name], f32))
            ok = st["error"] == 0 and all(certify(words, v, k) for v in answers)
            sel_gk[name].append(n / dt / 1e9)
            emit({"leg": f"select_{name}", "round": r, "log2n": args.log2n, "k": k, "steps": args.steps,
                  "ms": round(dt * 1e3, 4), "gkeys_per_s": round(n / dt / 1e9, 1), "path": st["path"],
                  "verified": bool(ok)})

    # ---- top-k (smallest; values + indices)
    for kk in (1 << 10, 1 << 20, 1 << 24):
        if kk > n:
            continue
        idx = torch.empty(kk, dtype=torch.int64, device=dev)
        vals = {name: torch.empty(kk, dtype=dt, device=dev) for name, (_, _, _, dt) in kinds.items()}

        def window_topk(name, steps):
            keys, _, f32, _ = kinds[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                sel.topk(keys, n, kk, vals[name], idx, f32=f32)
            sel.sync()
            return (time.perf_counter() - t0) / steps

        for name in kinds:
            window_topk(name, 2)
        for r in range(args.rounds):
            for name in ("i32", "f32"):
                keys, words, f32, _ = kinds[name]
                dt = window_topk(name, args.steps)
                st = sel.stats()
                vw = ordered_i32(vals[name]) if f32 else vals[name]
                ok = (st["error"] == 0 and bool((idx[1:] > idx[:-1]).all()) and torch.equal(vw, words[idx])
                      and certify(words, int(vw.max()), kk))
                emit({"leg": f"topk_{name}", "round": r, "log2n": args.log2n, "k": kk, "steps": args.steps,
                      "ms": round(dt * 1e3, 4), "gkeys_per_s": round(n / dt / 1e9, 1), "path": st["path"],
                      "verified": bool(ok)})
        del idx, vals

    i_med, f_med = statistics.median(sel_gk["i32"]), statistics.median(sel_gk["f32"])
    spread = max(sel_gk["i32"]) - min(sel_gk["i32"])
    emit({"leg": "select_summary", "i32_median_gkeys_per_s": round(i_med, 1), "f32_median_gkeys_per_s": round(f_med, 1),
          "i32_spread_gkeys_per_s": round(spread, 1), "f32_slower_than_i32_spread": bool(i_med - f_med > spread),
          "build_id": kselect.LIB.kth_build_id().decode()})
    sel.close()


if __name__ == "__main__":
    main()
