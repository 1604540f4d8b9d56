"""16-bit wide rows (kth_select_wide_rows_k16, kth_topk_wide_rows_k16) against
what a caller with a bfloat16 / float16 / int16 matrix has without them, on one
GPU.

    python tools/bench_rows_wide16.py [--steps 50] [--rounds 3] > profiles/rows_wide16_bench.jsonl
    python tools/bench_rows_wide16.py --sweep > profiles/rows_wide16_plan_sweep.jsonl

Shapes: rows in {1, 8, 64, 512, 4096} x cols in {32768, 131072, 262144}
(matrices above 1 GiB of keys are skipped); bfloat16 randn, float16 randn and
int16 uniform rows, and one few-valued bfloat16 input of five values per row
("bf16five"); select at k = cols / 2, top-k largest at k = 50 and k = 1024.
The new call alternates in one process with
  (a) the float32 / int32 wide-rows call on a copy widened beforehand,
  (b) widening (tensor.to(float32 / int32)) plus that call: what a caller does
      today, and the yardstick,
  (c) torch.kthvalue / torch.topk(sorted=False) on the 16-bit tensor itself,
      "unsupported" where torch refuses the dtype.
`rounds` rounds of one window per leg in turn; a window is `steps` calls (fewer
for a leg whose single call is long: about --window-s seconds a window) behind
a warm-up, wall clock around a window that ends with a synchronise.  One JSON
line per shape, input and operation: every leg's windows (ms per call), their
medians and each leg's spread (max - min over its windows, relative to the
median).  below_b: the new call's median is below (b)'s by more than the larger
of the two spreads.

Every result of the new call is certified on the device with integer compares
of order keys: select by #(key < v) < k <= #(key <= v); top-k by ascending
columns, values equal to keys[idx], every better key kept, and of the keys
equal to the k-th the first ones by column.

A line also reports the form and slices of the plan and hbm_share: the time of
ONE read of the matrix (2 bytes a key) at the 8 TB/s spec over the measured
time (the select reads a row twice, the top-k three times).

--sweep: the new call alone under forced plans (slices 1, 2, 4, ... 256; 1 is
the fused form), one line per shape with the median us per call by slices, the
automatic rule's choice and the best: the data the plan's thresholds are
judged by.
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
INPUTS = ("bf16", "f16", "i16", "bf16five")
MAX_BYTES = 1 << 30
CERT_ELEMS = 1 << 24  # keys per certification chunk (int64 order keys)
INF = {"f16": 0x7C00, "bf16": 0x7F80}


def order_key(t, kind):
    """int64 order keys (0 .. 65535) of a 2-byte tensor's elements; integer operations only."""
    import torch
    b = t.view(torch.int16).to(torch.int64) & 0xFFFF
    if kind == "i16":
        return b ^ 0x8000
    if kind == "u16":
        return b
    key = torch.where(b >= 0x8000, b ^ 0xFFFF, b | 0x8000)
    return torch.where((b & 0x7FFF) > INF[kind], torch.full_like(b, 0xFFFF), key)


def certify(keys, kind, k, largest, out=None, vals=None, idx=None):
    """Every row's rank certificate and, for top-k, the kept set's shape and tie rule; chunked over rows."""
    import torch
    rows, cols = keys.shape
    step = max(1, CERT_ELEMS // cols)
    col = torch.arange(cols, device=keys.device).unsqueeze(0)
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        o = order_key(keys[sl], kind)
        if largest:
            o = 0xFFFF - o
        if out is not None:
            v = order_key(out[sl], kind)  # (out: rows x 1)
        else:
            ov = order_key(vals[sl], kind)
            if largest:
                ov = 0xFFFF - ov
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
    slice_keys = (-(-cols // want) + 7) // 8 * 8
    return -(-cols // slice_keys)


def make_keys(torch, name, rows, cols, g, dev):
    if name == "i16":
        return torch.randint(-2 ** 15, 2 ** 15, (rows, cols), generator=g, device=dev, dtype=torch.int16)
    dt = torch.float16 if name == "f16" else torch.bfloat16
    x = torch.randn((rows, cols), generator=g, device=dev, dtype=torch.float32)
    if name == "bf16five":  # five values per row: column j holds the row's x[j % 5], shuffled by a fixed stride
        pick = (torch.arange(cols, device=dev) * 7919) % 5
        x = torch.gather(x[:, :5], 1, pick.unsqueeze(0).expand(rows, cols))
    return x.to(dt)


def main():
    import torch

    import kselect
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x31DE)
    ap.add_argument("--inputs", default=",".join(INPUTS))
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
            nbytes = rows * cols * 2
            if nbytes > MAX_BYTES:
                continue
            for name in args.inputs.split(","):
                kind = "bf16" if name == "bf16five" else name
                f32 = kind != "i16"
                wide_dt = torch.float32 if f32 else torch.int32
                keys = make_keys(torch, name, rows, cols, g, dev)
                wide = None if args.sweep else keys.to(wide_dt)
                for what, ktop in ops:
                    topk = ktop is not None
                    k = ktop if topk else cols // 2
                    nout = rows * k if topk else rows
                    out = torch.zeros(nout, dtype=keys.dtype, device=dev)
                    idx = torch.zeros(nout, dtype=torch.int32, device=dev) if topk else None
                    out_w = torch.zeros(nout, dtype=wide_dt, device=dev)
                    idx_w = torch.zeros(nout, dtype=torch.int32, device=dev) if topk else None

                    def new():
                        if topk:
                            sel.topk_rows_wide16(keys, rows, cols, k, out, idx, largest=True)
                        else:
                            sel.rows_wide16(keys, rows, cols, k, out)

                    def wide_call(w):
                        if topk:
                            sel.topk_rows_wide(w, rows, cols, k, out_w, idx_w, largest=True, f32=f32)
                        else:
                            sel.rows_wide(w, rows, cols, k, out_w, f32=f32)

                    def leg_a():
                        wide_call(wide)

                    def leg_b():
                        wide_call(keys.to(wide_dt))

                    def leg_c():
                        if topk:
                            torch.topk(keys, k, dim=1, largest=True, sorted=False)
                        else:
                            torch.kthvalue(keys, k, dim=1)

                    def certified():
                        new()
                        sel.sync()
                        if topk:
                            return certify(keys, kind, k, True, vals=out.view(rows, k), idx=idx.view(rows, k))
                        return certify(keys, kind, k, False, out=out.view(rows, 1))

                    base = {"what": what, "input": name, "rows": rows, "cols": cols, "k": k}
                    rule = kselect.wide_rows_plan16(rows, cols, num_cu)[0]

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
                        best = min(us, key=us.get)
                        emit({"leg": "sweep", **base, "us_by_slices": us, "rule_slices": rule, "best_slices": best,
                              "rule_over_best": round(us[rule] / us[best], 3) if rule in us else None,
                              "verified": bool(ok)})
                        continue
                    ok = certified()
                    legs = [("new", new), ("a", leg_a), ("b", leg_b)]
                    try:
                        leg_c()
                        torch.cuda.synchronize()
                        legs.append(("c", leg_c))
                    except (RuntimeError, TypeError, NotImplementedError):
                        pass
                    steps = {n: steps_for(fn) for n, fn in legs}
                    ts = {n: [] for n, _ in legs}
                    for r in range(args.rounds):
                        for n, fn in legs:
                            ts[n].append(window(fn, steps[n]))
                    med = {n: statistics.median(v) for n, v in ts.items()}
                    spread = {n: (max(v) - min(v)) / med[n] for n, v in ts.items()}
                    margin_b = 1.0 - med["new"] / med["b"]
                    emit({"leg": "shape", **base, "form": "fused" if rule == 1 else "split", "slices": rule,
                          "window_ms": {n: [round(t * 1e3, 4) for t in v] for n, v in ts.items()},
                          "median_ms": {n: round(v * 1e3, 4) for n, v in med.items()},
                          "spread": {n: round(v, 3) for n, v in spread.items()},
                          "c": "measured" if "c" in med else "unsupported",
                          "gkeys_per_s": round(rows * cols / med["new"] / 1e9, 2),
                          "hbm_share": round(nbytes / (SPEC_TBPS * 1e12) / med["new"], 4),
                          "margin_vs_b": round(margin_b, 3),
                          "below_b": bool(margin_b > max(spread["new"], spread["b"])),
                          "faster_than_a": bool(med["new"] < med["a"]), "verified": bool(ok)})
                    del out, idx, out_w, idx_w
                del keys, wide
                torch.cuda.empty_cache()
    emit({"leg": "build", "build_id": kselect.LIB.kth_build_id().decode(), "num_cu": num_cu, "spec_tbps": SPEC_TBPS})
    sel.close()


if __name__ == "__main__":
    main()
