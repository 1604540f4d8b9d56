"""16-bit rows against the 32-bit rows calls on one GPU.

    python tools/bench_rows16.py [--steps 200] [--rounds 3] > profiles/rows16_bench.jsonl

Shapes: 65536 x 4096 select at k = 64 and k = 2048, 65536 x 4096 top-k largest
at k = 64, 1048576 x 256 top-k largest at k = 8 (the MoE-routing shape).  Keys:
bfloat16 randn, float16 randn, int16 uniform.  Each 16-bit call alternates in
one process with
  (a) the float32 / int32 rows call on an already widened copy of the keys,
  (b) widening plus that call: what a caller without the 16-bit calls does.
`rounds` windows of `steps` (>= 20) calls after a warm-up, wall clock around a
window that ends with a synchronise.

Every row's answer is rank-certified on the device with integer compares of
order keys: #(key < v) < k <= #(key <= v); for top-k, v is the k-th kept key,
the kept values are the keys at the kept columns, and the columns ascend.

One JSON line per leg and window: ms per call, Gkeys/s, and floor_share, the
2-bytes-per-key HBM time at the streaming rate the README records (6.71 TB/s)
over the measured time.  The last lines compare the medians per shape and kind.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

STREAM_TBPS = 6.71  # README: the streaming pass of the 2^30-key select
SHAPES = (("select", 65536, 4096, 64), ("select", 65536, 4096, 2048), ("topk_largest", 65536, 4096, 64),
          ("topk_largest", 1048576, 256, 8))
ROW_CHUNK = 8192


def order_key16(t, kind):
    """int32 order keys (0..65535) of a 2-byte tensor's elements; integer operations only."""
    import torch
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    if kind == "i16":
        return b ^ 0x8000
    inf = 0x7C00 if kind == "f16" else 0x7F80
    key = torch.where(b >= 0x8000, b ^ 0xFFFF, b | 0x8000)
    return torch.where((b & 0x7FFF) > inf, torch.full_like(b, 0xFFFF), key)


def certify(keys, kind, k, largest, out=None, vals=None, idx=None):
    """Every row's rank certificate (and, for top-k, the kept set's shape), chunked over rows."""
    import torch
    rows = keys.shape[0]
    for r0 in range(0, rows, ROW_CHUNK):
        sl = slice(r0, min(rows, r0 + ROW_CHUNK))
        o = order_key16(keys[sl], kind)
        if largest:
            o = 0xFFFF - o
        if out is not None:
            v = order_key16(out[sl], kind)  # (out: rows x 1)
        else:
            ov = order_key16(vals[sl], kind)
            if largest:
                ov = 0xFFFF - ov
            ix = idx[sl].long()
            if int(ix.min()) < 0 or int(ix.max()) >= keys.shape[1] or not bool((ix[:, 1:] > ix[:, :-1]).all()):
                return False
            if not bool((torch.gather(o, 1, ix) == ov).all()):
                return False
            v = ov.max(dim=1, keepdim=True).values
            if not bool(((ov < v).sum(dim=1) == (o < v).sum(dim=1)).all()):  # every key below the k-th is kept
                return False
        lt, le = (o < v).sum(dim=1), (o <= v).sum(dim=1)
        if not bool(((lt < k) & (le >= k)).all()):
            return False
    return True


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x1616)
    ap.add_argument("--kinds", default="bf16,f16,i16")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("windows of at least 20 calls")
    dev = torch.device("cuda", 0)
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: (b)'s widening copy is ordered before its rows call
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
    for what, rows, cols, k in SHAPES:
        topk = what != "select"
        for kind in args.kinds.split(","):
            if kind == "i16":
                keys = torch.randint(-32768, 32768, (rows, cols), generator=g, device=dev, dtype=torch.int16)
                wide_dt = torch.int32
            else:
                dt = torch.bfloat16 if kind == "bf16" else torch.float16
                keys = torch.empty((rows, cols), dtype=dt, device=dev)
                for part in torch.split(keys, ROW_CHUNK):
                    part.copy_(torch.randn(part.shape, generator=g, device=dev, dtype=torch.float32))
                wide_dt = torch.float32
            f32 = wide_dt == torch.float32
            wide = keys.to(wide_dt)   # (a)'s input, widened once outside every window
            wide_b = torch.empty_like(wide)  # (b) widens into this every call
            nout = rows * k if topk else rows
            out16 = torch.zeros(nout, dtype=keys.dtype, device=dev)
            out32 = torch.zeros(nout, dtype=wide_dt, device=dev)
            idx16 = torch.zeros(nout, dtype=torch.int32, device=dev) if topk else None
            idx32 = torch.zeros(nout, dtype=torch.int32, device=dev) if topk else None

            def call16():
                if topk:
                    sel.topk_rows16(keys, rows, cols, k, out16, idx16, largest=True)
                else:
                    sel.rows16(keys, rows, cols, k, out16)

            def call32(src=wide):
                if topk:
                    sel.topk_rows(src, rows, cols, k, out32, idx32, largest=True, f32=f32)
                else:
                    sel.rows(src, rows, cols, k, out32, f32=f32)

            def call_widen():
                wide_b.copy_(keys)
                call32(wide_b)

            for fn in (call16, call32, call_widen):
                for _ in range(args.warmup):
                    fn()
            sel.sync()
            # certify: the 16-bit answers by their own order keys; the 32-bit ones agree with them in value
            call16()
            call32()
            sel.sync()
            if topk:
                ok = certify(keys, kind, k, True, vals=out16.view(rows, k), idx=idx16.view(rows, k))
                agree = bool((idx16 == idx32).all())
            else:
                ok = certify(keys, kind, k, False, out=out16.view(rows, 1))
                agree = bool((order_key16(out16, kind) == order_key16(out32.to(keys.dtype), kind)).all())
            floor_ms = rows * cols * 2 / (STREAM_TBPS * 1e12) * 1e3
            med = {}
            for name, fn in (("k16", call16), ("a_prewidened", call32), ("b_widen_then_call", call_widen)):
                ts = []
                for r in range(args.rounds):
                    dt_ = window(fn)
                    ts.append(dt_)
                    emit({"leg": name, "what": what, "kind": kind, "rows": rows, "cols": cols, "k": k, "round": r,
                          "steps": args.steps, "ms": round(dt_ * 1e3, 4), "gkeys_per_s": round(rows * cols / dt_ / 1e9, 1),
                          "floor_share": round(floor_ms / (dt_ * 1e3), 3), "verified": bool(ok),
                          "agrees_with_32bit": agree})
                med[name] = statistics.median(ts)
            # a second pass in the other order, so that no leg always follows the same neighbour
            for name, fn in (("b_widen_then_call", call_widen), ("a_prewidened", call32), ("k16", call16)):
                dt_ = window(fn)
                emit({"leg": name, "what": what, "kind": kind, "rows": rows, "cols": cols, "k": k, "round": args.rounds,
                      "steps": args.steps, "ms": round(dt_ * 1e3, 4), "gkeys_per_s": round(rows * cols / dt_ / 1e9, 1),
                      "floor_share": round(floor_ms / (dt_ * 1e3), 3), "verified": bool(ok), "agrees_with_32bit": agree})
            summary.append({"leg": "summary", "what": what, "kind": kind, "rows": rows, "cols": cols, "k": k,
                            **{f"{n}_median_ms": round(v * 1e3, 4) for n, v in med.items()},
                            "k16_floor_share": round(floor_ms / (med["k16"] * 1e3), 3),
                            "faster_than_b": bool(med["k16"] < med["b_widen_then_call"]),
                            "faster_than_a": bool(med["k16"] < med["a_prewidened"]), "verified": bool(ok)})
            del keys, wide, wide_b, out16, out32, idx16, idx32
            torch.cuda.empty_cache()
    for rec in summary:
        emit(rec)
    emit({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "stream_tbps": STREAM_TBPS})
    sel.close()


if __name__ == "__main__":
    main()
