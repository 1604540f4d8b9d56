"""Wide rows (kth_select_wide_rows_*, kth_topk_wide_rows_*) against what a
caller has without them, on one GPU.

    python tools/bench_rows_wide.py [--steps 50] [--rounds 3] > profiles/rows_wide_bench.jsonl
    python tools/bench_rows_wide.py --sweep > profiles/rows_wide_plan_sweep.jsonl

Shapes: rows in {1, 8, 64, 512, 4096} x cols in {32768, 131072, 262144}
(matrices above 2 GiB are skipped), float32 randn and int32 uniform keys;
select at k = cols / 2, top-k largest at k = 50 and k = 1024.  The new call
alternates in one process with
  (a) the loop over rows of kth_select_*_async / kth_topk_* on one ctx: what a
      user does today,
  (b) torch.kthvalue / torch.topk(sorted=False) on the same tensor.
`rounds` rounds of one window per leg, new / a / b in turn; a window is `steps`
calls (fewer for a leg whose single call is long: about --window-s seconds a
window) behind a warm-up, wall clock around a window that ends with a
synchronise.  One JSON line per shape, key kind and operation: every leg's
windows (ms per call), their medians and each leg's spread (max - min over its
windows, relative to the median).

Every result of the new call is certified on the device with integer compares
of order keys: select by #(key < v) < k <= #(key <= v); top-k by ascending
columns, values equal to keys[idx], every better key kept, and of the keys
equal to the k-th the first ones by column.

A line also reports Gkeys/s, the form and slices of the plan, and hbm_share: the
time of ONE read of the matrix at the 8 TB/s spec over the measured time (the
select reads the row two or three times).  in_infinity_cache marks matrices of
at most 256 MiB, which may be served from the Infinity Cache after the first
call of a window and so not from HBM at all.

--sweep: the new call alone under forced plans (slices 1, 2, 4, ... 256; 1 is
the fused form), one line per shape with the median us per call by slices: the
data the automatic plan's thresholds come from.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd"))

SPEC_TBPS = 8.0
ROWS = (1, 8, 64, 512, 4096)
COLS = (32768, 131072, 262144)
OPS = (("select", None), ("topk_largest", 50), ("topk_largest", 1024))
MAX_BYTES = 2 << 30
CACHE_BYTES = 256 << 20
CERT_ELEMS = 1 << 24  # keys per certification chunk (int64 order keys)


def order_key(t, f32):
    """int64 order keys (0 .. 2^32 - 1) of a 4-byte tensor's elements; integer operations only."""
    import torch
    b = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if not f32:
        return b ^ 0x80000000
    key = torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)
    return torch.where((b & 0x7FFFFFFF) > 0x7F800000, torch.full_like(b, 0xFFFFFFFF), key)


def certify(keys, f32, k, largest, out=None, vals=None, idx=None):
    """Every row's rank certificate and, for top-k, the kept set's shape and tie rule; chunked over rows."""
    import torch
    rows, cols = keys.shape
    step = max(1, CERT_ELEMS // cols)
    col = torch.arange(cols, device=keys.device).unsqueeze(0)
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        o = order_key(keys[sl], f32)
        if largest:
            o = 0xFFFFFFFF - o
        if out is not None:
            v = order_key(out[sl], f32)  # (out: rows x 1)
        else:
            ov = order_key(vals[sl], f32)
            if largest:
                ov = 0xFFFFFFFF - ov
            ix = idx[sl].long()
            if int(ix.min()) < 0 or int(ix.max()) >= cols or not bool((ix[:, 1:] > ix[:, :-1]).all()):
                return False
            if not bool((torch.gather(o, 1, ix) == ov).all()):
                return False
            v = ov.max(dim=1, keepdim=True).values
            if not bool(((ov < v).sum(dim=1) == (o < v).sum(dim=1)).all()):  # every better key is kept
                return False
            kept_tie = ov == v
            last = torch.where(kept_tie, ix, torch.full_like(ix, -1)).max(dim=1, keepdim=True).values
            if not bool((((o == v) & (col <= last)).sum(dim=1) == kept_tie.sum(dim=1)).all()):  # the first ties
                return False
        lt, le = (o < v).sum(dim=1), (o <= v).sum(dim=1)
        if not bool(((lt < k) & (le >= k)).all()):
            return False
    return True


def effective_slices(cols, want):
    slice_keys = (-(-cols // want) + 3) // 4 * 4
    return -(-cols // slice_keys)


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x31DE)
    ap.add_argument("--kinds", default="f32,i32")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--cols", default=",".join(map(str, COLS)))
    ap.add_argument("--ops", default="select,topk50,topk1024")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sel = kselect.Selector(0)
    sel.set_stream(None)  # the null stream, torch's default: the legs and the certification are ordered
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    ops = [(w, k) for w, k in OPS if (w if k is None else f"topk{k}") in args.ops.split(",")]

    def emit(rec):
        print(json.dumps(rec), flush=True)

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
            nbytes = rows * cols * 4
            if nbytes > MAX_BYTES:
                continue
            for kind in args.kinds.split(","):
                f32 = kind == "f32"
                if f32:
                    keys = torch.randn((rows, cols), generator=g, device=dev, dtype=torch.float32)
                else:
                    keys = torch.randint(-2 ** 31, 2 ** 31, (rows, cols), generator=g, device=dev, dtype=torch.int32)
                for what, ktop in ops:
                    topk = ktop is not None
                    k = ktop if topk else cols // 2
                    nout = rows * k if topk else rows
                    out = torch.zeros(nout, dtype=keys.dtype, device=dev)
                    idx = torch.zeros(nout, dtype=torch.int32, device=dev) if topk else None
                    out_a = torch.zeros(nout, dtype=keys.dtype, device=dev)
                    idx_a = torch.zeros(nout, dtype=torch.int64, device=dev) if topk else None

                    def new():
                        if topk:
                            sel.topk_rows_wide(keys, rows, cols, k, out, idx, largest=True, f32=f32)
                        else:
                            sel.rows_wide(keys, rows, cols, k, out, f32=f32)

                    def loop_a():
                        for r in range(rows):
                            if topk:
                                sel.topk(keys[r], cols, k, out_a[r * k:], idx_a[r * k:], largest=True, f32=f32)
                            else:
                                sel.select_async(keys[r], cols, k, out_a[r:], f32=f32)

                    def torch_b():
                        if topk:
                            torch.topk(keys, k, dim=1, largest=True, sorted=False)
                        else:
                            torch.kthvalue(keys, k, dim=1)

                    def certified():
                        new()
                        sel.sync()
                        if topk:
                            return certify(keys, f32, k, True, vals=out.view(rows, k), idx=idx.view(rows, k))
                        return certify(keys, f32, k, False, out=out.view(rows, 1))

                    base = {"what": what, "kind": kind, "rows": rows, "cols": cols, "k": k}

                    if args.sweep:
                        us, ok = {}, True
                        for want in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                            if effective_slices(cols, want) != want:
                                continue
                            sel.wide_rows_force(want, 0)
                            ok = certified() and ok
                            steps = steps_for(new)
                            ts = [window(new, steps) for _ in range(args.rounds)]
                            us[want] = round(statistics.median(ts) * 1e6, 1)
                        sel.wide_rows_force(0, 0)
                        emit({"leg": "sweep", **base, "us_by_slices": us, "verified": bool(ok)})
                        continue
                    slices = kselect.wide_rows_plan(rows, cols, num_cu)[0]
                    ok = certified()
                    legs = (("new", new), ("a", loop_a), ("b", torch_b))
                    steps = {name: steps_for(fn) for name, fn in legs}
                    ts = {name: [] for name, _ in legs}
                    for r in range(args.rounds):
                        for name, fn in legs:
                            ts[name].append(window(fn, steps[name]))
                    med = {n: statistics.median(v) for n, v in ts.items()}
                    emit({"leg": "shape", **base, "form": "fused" if slices == 1 else "split", "slices": slices,
                          "in_infinity_cache": nbytes <= CACHE_BYTES,
                          "window_ms": {n: [round(t * 1e3, 4) for t in v] for n, v in ts.items()},
                          "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                          "spread": {n: round((max(v) - min(v)) / med[n], 3) for n, v in ts.items()},
                          "gkeys_per_s": round(rows * cols / med["new"] / 1e9, 2),
                          "hbm_share": round(nbytes / (SPEC_TBPS * 1e12) / med["new"], 4),
                          "faster_than_a": bool(med["new"] < med["a"]),
                          "faster_than_b": bool(med["new"] < med["b"]), "verified": bool(ok)})
                    del out, idx, out_a, idx_a
                del keys
                torch.cuda.empty_cache()
    emit({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "num_cu": num_cu, "spec_tbps": SPEC_TBPS})
    sel.close()


if __name__ == "__main__":
    main()
