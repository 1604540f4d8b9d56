"""16-bit keys against int32 keys on one GPU: the one-array select.

    python tools/bench_k16.py [--log2n 30] [--steps 20] [--rounds 3] > profiles/k16_bench.jsonl

Headline legs, n = 2^log2n, k = n / 2, all in one process: bfloat16 and float16
keys of a seeded randn, int16 keys uniform over the full range, each
alternating with the int32 select of n uniform_half keys; `rounds` windows of
`steps` asynchronous selects (wall clock around the window, as bench.py
times), after a warm-up.  Then a 4-rank call (quartiles and p99) of the
bfloat16 keys against four single selects, and the adversarial families
(all-equal, two values differing in the lowest bit, a few distinct values,
sorted ascending and descending) at k in {1, n/2, n}, int16 keys beside the
int32 select of the same family and n.

Every answer is rank-certified on the device with integer compares of order
keys: v is the k-th smallest iff #(key < v) < k <= #(key <= v).

One JSON line per leg and window: ms (per call), main_ms (the streaming
launch, from the ctx's events in a separate timed call), path, verified.  The
last line compares the medians.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

CHUNK = 1 << 27


def order_key16(t, kind):
    """int32 order keys (0..65535) of a 2-byte tensor's elements; integer operations only."""
    import torch
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    if kind == "i16":
        return b ^ 0x8000
    if kind == "u16":
        return b
    inf = 0x7C00 if kind == "f16" else 0x7F80
    key = torch.where(b >= 0x8000, b ^ 0xFFFF, b | 0x8000)
    return torch.where((b & 0x7FFF) > inf, torch.full_like(b, 0xFFFF), key)


def certify16(keys, kind, bits, k):
    import torch
    v = int(order_key16(torch.tensor([bits], dtype=torch.int32).to(torch.int16), kind)[0])
    lt = le = 0
    for c in torch.split(keys, CHUNK):
        w = order_key16(c, kind)
        lt += int((w < v).sum())
        le += int((w <= v).sum())
    return lt < k <= le


def certify32(keys, v, k):
    import torch
    lt = le = 0
    for c in torch.split(keys, CHUNK):
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
    ap.add_argument("--adv-steps", type=int, default=5)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x16)
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    sel = kselect.Selector(0)
    sel.reserve(n)
    sel.reserve16(n, 4)

    def emit(rec):
        print(json.dumps(rec), flush=True)

    def bits_of(t):
        return [int(x) & 0xFFFF for x in t.view(torch.int16).cpu().tolist()]

    def run16(keys, kind, ks, out, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if len(ks) == 1:
                sel.select16_async(keys, n, ks[0], out, kind=kind)
            else:
                sel.select16_multi_async(keys, n, ks, out, kind=kind)
        sel.sync()
        return (time.perf_counter() - t0) / steps

    def run32(keys, k, out, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sel.select_async(keys, n, k, out)
        sel.sync()
        return (time.perf_counter() - t0) / steps

    def main_ms(fn):
        sel.enable_timing(True)
        fn()
        cnt, m, _ = sel.take_timing()
        sel.enable_timing(False)
        return round(m / max(cnt, 1), 4)

    def leg16(name, keys, kind, ks, steps, extra=None):
        out = torch.zeros(len(ks), dtype=torch.int16, device=dev)
        dt = run16(keys, kind, ks, out, steps)
        paths = [sel.multi_stats(i)["path"] for i in range(len(ks))]
        err = [sel.multi_stats(i)["error"] for i in range(len(ks))]
        ok = not any(err) and all(certify16(keys, kind, b, k) for b, k in zip(bits_of(out), ks))
        rec = {"leg": name, "kind": kind, "log2n": args.log2n, "k": ks if len(ks) > 1 else ks[0], "steps": steps,
               "ms": round(dt * 1e3, 4), "main_ms": main_ms(lambda: run16(keys, kind, ks, out, 1)),
               "gkeys_per_s": round(n / dt / 1e9, 1), "path": paths if len(ks) > 1 else paths[0], "verified": bool(ok)}
        rec.update(extra or {})
        emit(rec)
        return dt

    def leg32(name, keys, k, steps, extra=None):
        out = torch.zeros(1, dtype=torch.int32, device=dev)
        dt = run32(keys, k, out, steps)
        st = sel.stats()
        ok = st["error"] == 0 and certify32(keys, int(out.cpu()[0]), k)
        rec = {"leg": name, "kind": "i32", "log2n": args.log2n, "k": k, "steps": steps, "ms": round(dt * 1e3, 4),
               "main_ms": main_ms(lambda: run32(keys, k, out, 1)), "gkeys_per_s": round(n / dt / 1e9, 1),
               "path": st["path"], "verified": bool(ok)}
        rec.update(extra or {})
        emit(rec)
        return dt

    ikeys = torch.empty(n, dtype=torch.int32, device=dev)
    sel.fill(ikeys, n, "uniform_half")
    sel.sync()
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    k = n // 2
    k16 = torch.empty(n, dtype=torch.int16, device=dev)  # one 2-byte buffer, refilled per leg
    med = {}
    for kind in ("bf16", "f16", "i16"):
        for a in torch.split(k16, CHUNK):
            if kind == "i16":
                a.copy_(torch.randint(-32768, 32768, (a.numel(),), generator=g, device=dev, dtype=torch.int16))
            else:
                dt_ = torch.bfloat16 if kind == "bf16" else torch.float16
                a.view(dt_).copy_(torch.randn(a.numel(), generator=g, device=dev, dtype=torch.float32).to(dt_))
        out16 = torch.zeros(1, dtype=torch.int16, device=dev)
        out32 = torch.zeros(1, dtype=torch.int32, device=dev)
        run16(k16, kind, [k], out16, args.warmup)
        run32(ikeys, k, out32, args.warmup)
        t16, t32 = [], []
        for r in range(args.rounds):
            t32.append(leg32(f"select_i32_vs_{kind}", ikeys, k, args.steps, {"round": r}))
            t16.append(leg16(f"select_{kind}", k16, kind, [k], args.steps, {"round": r}))
        med[kind] = (statistics.median(t16), statistics.median(t32))
        if kind == "bf16":  # quartiles and p99 in one call against four single selects
            ks = [n // 4, n // 2, 3 * n // 4, n - n // 100]
            for r in range(args.rounds):
                four = leg16("multi4_bf16", k16, kind, ks, args.steps, {"round": r})
                singles = sum(leg16("single_of_multi4_bf16", k16, kind, [kk], args.steps, {"round": r}) for kk in ks)
                emit({"leg": "multi4_vs_singles", "round": r, "multi_ms": round(four * 1e3, 4),
                      "four_singles_ms": round(singles * 1e3, 4), "multi_faster": bool(four < singles)})

    # ---- adversarial families: int16 keys beside the int32 select of the same family
    idx = torch.arange(CHUNK, device=dev, dtype=torch.int64)
    fams = {
        "all_equal": lambda i: torch.full_like(i, 1234),
        "two_values_bit0": lambda i: 1234 + ((i * 2654435761 >> 13) & 1),
        "few_distinct": lambda i: ((i * 2654435761 >> 11) & 7) * 4099 - 16000,
        "sorted_asc": lambda i: (i >> (args.log2n - 16)) - 32768 if args.log2n >= 16 else i - 32768,
        "sorted_desc": lambda i: 32767 - ((i >> (args.log2n - 16)) if args.log2n >= 16 else i),
    }
    for fam, fn in fams.items():
        for at, (a16, a32) in enumerate(zip(torch.split(k16, CHUNK), torch.split(ikeys, CHUNK))):
            v = fn(idx[:a16.numel()] + at * CHUNK)
            a16.copy_(v.to(torch.int16))
            a32.copy_(v.to(torch.int32))
        for kk in (1, n // 2, n):
            leg32(f"adv_{fam}_i32", ikeys, kk, args.adv_steps, {"family": fam})
            leg16(f"adv_{fam}_i16", k16, "i16", [kk], args.adv_steps, {"family": fam})

    emit({"leg": "summary", "log2n": args.log2n,
          **{f"{kind}_median_ms": round(m16 * 1e3, 4) for kind, (m16, _) in med.items()},
          **{f"i32_beside_{kind}_median_ms": round(m32 * 1e3, 4) for kind, (_, m32) in med.items()},
          **{f"{kind}_faster_than_i32": bool(m16 < m32) for kind, (m16, m32) in med.items()},
          "build_id": kselect.LIB.kth_build_id().decode()})
    sel.close()


if __name__ == "__main__":
    main()
