"""The 16-bit one-array top-k against the 32-bit top-k on one GPU.

    python tools/bench_topk16.py [--log2n 30] [--steps 20] [--rounds 3] > profiles/topk16_bench.jsonl

n = 2^30 keys: bfloat16 randn, float16 randn, int16 uniform; k in {1024, 2^20,
2^24, 2^27}, largest, values and indices.  Each kth_topk_k16 leg alternates in
one process with
  (a) kth_topk_f32 / kth_topk_i32 on an already widened copy of the keys,
  (b) widening plus that call: what a caller without the 16-bit call does.
`rounds` windows of `steps` calls after a warm-up, wall clock around a window
that ends with a synchronise, then one more window per leg in the other order;
the summary lines give the window medians.

Every 16-bit result is certified on the device with integer compares of order
keys: indices strictly ascending and in range, values = keys[idx] (a NaN
canonical), the k-th kept key v, every key better than v kept, and the kept
ties the first k - #better by index.  Each line also carries tiles_read /
tiles of the count pass and the embedded select's path.  Where the count pass
skipped tiles, a fourth leg runs the same call with KTH_HOOK_K16_TOPK_NOSKIP.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

CHUNK = 1 << 26


def order_key16(t, kind):
    """int32 order keys (0..65535) of a 2-byte tensor's elements; integer operations only."""
    import torch
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    if kind == "i16":
        return b ^ 0x8000
    inf = 0x7C00 if kind == "f16" else 0x7F80
    key = torch.where(b >= 0x8000, b ^ 0xFFFF, b | 0x8000)
    return torch.where((b & 0x7FFF) > inf, torch.full_like(b, 0xFFFF), key)


def certify(keys, kind, k, vals, idx):
    """The properties that pin the exact top-k (largest), chunked over the input."""
    import torch
    n = keys.numel()
    if int(idx[0]) < 0 or int(idx[-1]) >= n or not bool((idx[1:] > idx[:-1]).all()):
        return False
    ov = 0xFFFF - order_key16(vals, kind)
    if not bool((0xFFFF - order_key16(keys[idx], kind) == ov).all()):
        return False
    inf = 0x7C00 if kind == "f16" else 0x7F80
    bits, kept = vals.view(torch.int16), keys[idx].view(torch.int16)
    nan = (kept.to(torch.int32) & 0x7FFF) > inf if kind != "i16" else torch.zeros_like(kept, dtype=torch.bool)
    canon = 0x7E00 if kind == "f16" else 0x7FC0
    if not bool((bits == torch.where(nan, torch.full_like(kept, canon), kept)).all()):
        return False
    v = int(ov.max())
    n_better, ties, need = 0, [], None
    for c0 in range(0, n, CHUNK):
        o = 0xFFFF - order_key16(keys[c0:c0 + CHUNK], kind)
        n_better += int((o < v).sum())
        ties.append(torch.nonzero(o == v).flatten() + c0)
    if int((ov < v).sum()) != n_better or n_better >= k:
        return False
    need = k - n_better
    first = torch.cat(ties)[:need]
    return bool(torch.equal(idx[ov == v], first))


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x1616)
    ap.add_argument("--kinds", default="bf16,f16,i16")
    ap.add_argument("--ks", default="1024,1048576,16777216,134217728")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: (b)'s widening copy is ordered before its call
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    build = kselect.LIB.kth_build_id().decode()

    def emit(rec):
        print(json.dumps(rec), flush=True)

    def window(fn, noskip=False):
        sel.test_hook(kselect.KTH_HOOK_K16_TOPK_NOSKIP, 1 if noskip else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        sel.sync()
        torch.cuda.synchronize()
        sel.test_hook(kselect.KTH_HOOK_K16_TOPK_NOSKIP, 0)
        return (time.perf_counter() - t0) / args.steps

    summary = []
    for kind in args.kinds.split(","):
        if kind == "i16":
            keys = torch.randint(-32768, 32768, (n,), generator=g, device=dev, dtype=torch.int16)
            wide_dt = torch.int32
        else:
            keys = torch.empty(n, dtype=torch.bfloat16 if kind == "bf16" else torch.float16, device=dev)
            for part in torch.split(keys, CHUNK):
                part.copy_(torch.randn(part.shape, generator=g, device=dev, dtype=torch.float32))
            wide_dt = torch.float32
        f32 = wide_dt == torch.float32
        wide = keys.to(wide_dt)          # (a)'s input, widened once outside every window
        wide_b = torch.empty_like(wide)  # (b) widens into this every call
        for k in (int(x) for x in args.ks.split(",")):
            if k > n:
                continue
            v16 = torch.zeros(k, dtype=keys.dtype, device=dev)
            i16 = torch.zeros(k, dtype=torch.int64, device=dev)
            v32 = torch.zeros(k, dtype=wide_dt, device=dev)
            i32 = torch.zeros(k, dtype=torch.int64, device=dev)

            def call16():
                sel.topk16(keys, n, k, v16, i16, largest=True)

            def call32(src=wide):
                sel.topk(src, n, k, v32, i32, largest=True, f32=f32)

            def call_widen():
                wide_b.copy_(keys)
                call32(wide_b)

            for fn in (call16, call32, call_widen):
                for _ in range(args.warmup):
                    fn()
            sel.sync()
            call16()
            sel.sync()
            tiles, read = sel.topk16_tiles()
            path = sel.stats()["path"]
            ok = certify(keys, kind, k, v16, i16)
            call32()
            sel.sync()
            agree = bool(torch.equal(i16, i32))
            common = {"kind": kind, "n": n, "k": k, "steps": args.steps, "verified": bool(ok), "agrees_with_32bit": agree,
                      "tiles": tiles, "tiles_read": read, "select_path": path, "build_id": build}
            med = {}
            for name, fn in (("k16", call16), ("a_prewidened", call32), ("b_widen_then_call", call_widen)):
                ts = []
                for r in range(args.rounds):
                    ts.append(window(fn))
                    emit({"leg": name, "round": r, "ms": round(ts[-1] * 1e3, 4), **common})
                med[name] = ts
            # a last window in the other order, so that no leg always follows the same neighbour
            for name, fn in (("b_widen_then_call", call_widen), ("a_prewidened", call32), ("k16", call16)):
                med[name].append(window(fn))
                emit({"leg": name, "round": args.rounds, "ms": round(med[name][-1] * 1e3, 4), **common})
            if read < tiles:  # what the skipped tiles buy: the same call with the flags ignored
                med["k16_noskip"] = []
                for r in range(args.rounds):
                    med["k16_noskip"].append(window(call16, noskip=True))
                    emit({"leg": "k16_noskip", "round": r, "ms": round(med["k16_noskip"][-1] * 1e3, 4), **common})
            med = {name: statistics.median(ts) for name, ts in med.items()}
            summary.append({"leg": "summary", **common,
                            **{f"{name}_median_ms": round(v * 1e3, 4) for name, v in med.items()},
                            "faster_than_a": bool(med["k16"] < med["a_prewidened"]),
                            "faster_than_b": bool(med["k16"] < med["b_widen_then_call"])})
            del v16, i16, v32, i32
        del keys, wide, wide_b
        torch.cuda.empty_cache()
    for rec in summary:
        emit(rec)
    sel.close()


if __name__ == "__main__":
    main()
