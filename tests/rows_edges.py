"""Inputs and the path model for the narrow 32-bit rows edge tests
(tests/test_gpu_rows_edges.py; proved on the CPU by tests/test_rows_edges_inputs.py).
numpy only, no library call.

The model restates, for one row and one rank, which branch of k_rows_reg
(csrc/kth_rows.hpp) the row takes: the first-pass map and its bins, the picked bin,
the keys below it and in it, how the bin is finished, and how a top-k row is stored.
It is exact because the rows are built so that no float rounding is left to emulate:

  int rows    FULL: the top byte of x ^ 0x80000000 (of its complement for largest);
              ragged: min(255, (key - kmin) >> sh), the padding counted as the kernel
              counts it.
  float rows  on the unit grid: 0.0 and 256.0 (or a subnormal in place of 0.0) on
              columns = 0 (mod 4), the only ones the FULL path samples, every other
              sampled value inside, so the scale 256 / range is exactly 1 and a bin
              is one float32 add: trunc(v - vmin) for smallest, trunc(256 - v) for
              largest, clamped to [0, 255].  numpy's float32 add is that one rounding.
              A row whose scale is not +-1 is reported as map "value", exact False,
              and no claim is made about its bins.

The model only chooses rows and ranks and names them.  Expected values come from
Ref: one stable argsort of test_gpu_parity's documented order keys, the same
result as its _topk_ref at every k, a NaN expected as 0x7FC00000.
"""
import collections

import numpy as np

import test_gpu_parity as P

WAVE = 64
R0, RW_STRIDE = 4, 260                          # KTH_ROWS_R0, kth::RW_STRIDE
LIST_MAX = WAVE                                 # a picked bin of more keys is "dense"
STAGE_CAP = (R0 * RW_STRIDE - WAVE) // 2        # 488: pairs the filter pass can stage
LDS_OUT_MAX = R0 * RW_STRIDE // 2               # 520: largest k the general compaction stages in LDS
REG_MAX_COLS = 4096
CANON_NAN = 0x7FC00000
DTYPES = ("i32", "f32")
CALLS = ("select", "smallest", "largest")
ROWS = 67                                       # not a multiple of the 4 rows of a workgroup
WIDTHS = (1, 3, 4, 7, 8, 63, 64, 65, 256, 1000, 1021, 1024, 1028, 1500, 2045, 2048, 2052, 4092, 4093, 4096)
WIDE_WIDTHS = (4097, 4099, 5000, 16383, 16384)
WIDE_ROWS = 5
FULL_WIDTHS = (1024, 2048, 4096)
RAGGED_WIDTHS = (1000, 1500, 4092, 4093)
OFFS = (0, 1)                                   # elements past a 16-byte boundary
PICK_BINS = (0, 3, 4, 127, 128, 251, 252, 255)  # ends of lane 0, 31 / 32, 62 / 63 and of the histogram


# ------------------------------------------------------------------ keys and the reference
def order_key(dtype, bits):
    """The documented order keys as uint64 (test_gpu_parity's for float rows)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    if dtype == "f32":
        return np.asarray(P._f32_order_key(bits.view(np.float32)), dtype=np.uint64)
    return (P._i32_order_key(bits.view(np.int32)) + (1 << 31)).astype(np.uint64)


class Ref:
    """The stable argsorts of a matrix, computed once: column of the k-th key, and the
    column-ordered top-k with ties by column (P._topk_ref sliced at k)."""

    def __init__(self, dtype, bits):
        self.dtype = dtype
        self.bits = np.ascontiguousarray(bits, dtype=np.uint32)
        self.bits.setflags(write=False)
        self.keys = order_key(dtype, self.bits).astype(np.int64)
        self.asc = np.argsort(self.keys, axis=1, kind="stable")
        self.desc = np.argsort(-self.keys, axis=1, kind="stable")

    def canon(self, vals, idx):
        if self.dtype != "f32":
            return vals
        return np.where(np.take_along_axis(self.keys, idx, 1) == 0xFFFFFFFF, np.uint32(CANON_NAN), vals)

    def select(self, k):
        col = self.asc[:, k - 1:k]
        return self.canon(np.take_along_axis(self.bits, col, 1), col)[:, 0]

    def topk(self, k, largest):
        idx = np.sort((self.desc if largest else self.asc)[:, :k], axis=1)
        return self.canon(np.take_along_axis(self.bits, idx, 1), idx), idx.astype(np.int32)


# ------------------------------------------------------------------ the form of a call
Form = collections.namedtuple("Form", "kernel dtype kpl load topk")


def form_of(dtype, cols, off, topk):
    """The kernel form a call lands in (launch_rows / launch_rows_reg): `off` is the base's
    distance from a 16-byte boundary in elements."""
    if cols > REG_MAX_COLS:
        assert not topk
        return Form("k_rows", dtype, 0, None, False)
    kpl = 16 if cols <= 1024 else 32 if cols <= 2048 else 64
    vec = off % 4 == 0 and cols % 4 == 0
    load = "full" if vec and cols == kpl * WAVE else "vec" if vec else "scalar"
    return Form("k_rows_reg", dtype, kpl, load, bool(topk))


def all_forms():
    return {Form("k_rows_reg", d, kpl, load, topk) for d in DTYPES for kpl in (16, 32, 64)
            for load in ("full", "vec", "scalar") for topk in (False, True)}


def wide_row_load(cols, off, r):
    """k_rows decides per row: 16-byte loads when the row starts on a 16-byte boundary and cols % 4 == 0."""
    return "vec" if (off + r * cols) % 4 == 0 and cols % 4 == 0 else "scalar"


# ------------------------------------------------------------------ the model
def _sel_value(key, flip):
    """kth::sel_value: the float an order key stands for, negated under flip."""
    k = int(key) ^ flip
    raw = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    v = np.array([raw], dtype=np.uint32).view(np.float32)[0]
    return -v if flip else v


def _clamp_bins(t):
    with np.errstate(invalid="ignore"):
        return np.clip(t, np.float32(0), np.float32(255)).astype(np.int64)


def _pick(bins, k, pad=0, pad_bin=255):
    hist = np.bincount(bins, minlength=256)
    hist[pad_bin] += pad
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, k))
    return b, int(cum[b] - hist[b]), int(hist[b])


def order_raw(keys):
    """The raw float bits of (non-NaN) order keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    raw = np.where(keys & np.uint64(0x80000000), keys & np.uint64(0x7FFFFFFF), ~keys & np.uint64(0xFFFFFFFF))
    return raw.astype(np.uint32)


def first_pass(dtype, bits, largest, topk, off=0):
    """(map, exact, bins, pad_bin): the first-pass map of the row under the call, the bin of every
    column (None when the row takes no histogram, or its float scale is not +-1) and the bin the
    padding of a ragged row is counted in."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    cols = bits.size
    f = form_of(dtype, cols, off, topk)
    flip = 0xFFFFFFFF if topk and largest else 0
    keys = order_key(dtype, bits) ^ np.uint64(flip)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        if f.load == "full":
            if dtype == "f32":
                x = bits.view(np.float32)
                if not np.isnan(x).any():
                    vmin, vmax = x[0::4].min(), x[0::4].max()
                    rng = np.float32(vmax - vmin)
                    scale = np.float32(256) / rng
                    if np.isfinite(rng) and rng > 0 and np.isfinite(scale) and scale > 0:
                        if scale != one:
                            return "value", False, None, None
                        t = (-x + vmax * scale) if flip else (x + -vmin * scale)
                        return "value", True, _clamp_bins(t.astype(np.float32)), None
            else:
                slot = keys[0:4 * WAVE:4] >> np.uint64(24)
                if np.unique(slot).size <= 2 and int(keys.max() - keys.min()) < 8:
                    return "few", True, None, None
            return "byte", True, (keys >> np.uint64(24)).astype(np.int64), None
        kmin, kmax = int(keys.min()), int(keys.max())
        if kmin == kmax:
            return "equal", True, None, None
        if dtype == "f32":
            vmin, vmax = _sel_value(kmin, flip), _sel_value(kmax, flip)
            rng = np.float32(vmax - vmin)
            scale = np.float32(256) / rng
            if (np.isfinite(vmin) and np.isfinite(vmax) and np.isfinite(rng) and rng > 0 and np.isfinite(scale)
                    and scale > 0):
                if scale != one:
                    return "range-value", False, None, None
                # sel_value of every key: the value of x ^ flip, negated under flip
                v = order_raw(keys ^ np.uint64(flip)).view(np.float32)
                v = -v if flip else v
                return "range-value", True, _clamp_bins((v - vmin).astype(np.float32)), 255
        w0 = (kmax - kmin).bit_length()
        sh = max(w0 - 8, 0)
        return ("range-int", True, np.minimum(255, (keys - np.uint64(kmin)) >> np.uint64(sh)).astype(np.int64),
                min(255, (0xFFFFFFFF - kmin) >> sh))


def trace(dtype, bits, k, call, off=0):
    """What k_rows_reg does with this row at rank k under `call` (one of CALLS): a dict of
    map, exact, bin, below, cnt, finish, span, and for top-k staged / store / out."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    cols = bits.size
    topk, largest = call != "select", call == "largest"
    f = form_of(dtype, cols, off, topk)
    flip = 0xFFFFFFFF if topk and largest else 0
    keys = order_key(dtype, bits) ^ np.uint64(flip)
    skeys = np.sort(keys)
    answer = skeys[k - 1]
    eqn = int((keys == answer).sum())
    kk_eq = k - int((keys < answer).sum())
    mp, exact, bins, pad_bin = first_pass(dtype, bits, largest, topk, off)
    t = {"form": f, "map": mp, "exact": exact, "eqn": eqn, "kk": kk_eq, "finish": None, "staged": False}
    if f.load == "full":
        if mp == "few":
            t["finish"] = "count8"
            t["slot_bytes"] = int(np.unique(keys[0:4 * WAVE:4] >> np.uint64(24)).size)
        elif bins is not None:
            if dtype == "i32":
                t["slot_bytes"] = int(np.unique(keys[0:4 * WAVE:4] >> np.uint64(24)).size)
            b, below, cnt = _pick(bins, k)
            inb = keys[bins == b]
            t.update(bin=b, below=below, cnt=cnt, span=int(inb.max() - inb.min()))
            zeros = (bits << np.uint32(1)) == 0
            only_zeros = mp == "value" and zeros.any() and bool((bins[zeros] == b).all()) and int(zeros.sum()) == cnt
            if cnt > LIST_MAX:
                if only_zeros and not topk:
                    t["finish"] = "zero-bin"
                elif only_zeros and np.unique(bits[zeros]).size == 2:
                    t["finish"] = "two-zeros"
                else:
                    t["finish"] = "span0" if t["span"] == 0 else "count8" if t["span"] < 8 else "radix"
            else:
                t["finish"] = "list"
                if topk and below + cnt <= STAGE_CAP:
                    low = (bins <= b).reshape(-1, WAVE, 4).sum(axis=2)  # [group of 256 columns, lane]
                    t.update(staged=True, n_staged=below + cnt,
                             fast_groups=int(((low.max(axis=1) == 1)).sum()),
                             coll_groups=int((low.max(axis=1) > 1).sum()))
    else:
        if mp == "equal":
            t["finish"] = "equal"
        elif bins is not None:
            pad = f.kpl * WAVE - cols
            b, below, cnt = _pick(bins, k, pad, pad_bin)
            inb = keys[bins == b]
            t.update(bin=b, below=below, cnt=cnt)
            if mp == "range-value":
                hi = 0xFFFFFFFF if b == pad_bin and pad else int(inb.max())
                t["span"] = hi - int(inb.min())
                t["finish"] = "interval-one" if t["span"] == 0 else "digits"
                t["interval_keys"] = cnt
            else:
                t["width"] = (int(keys.max()) - int(keys.min())).bit_length()
                t["finish"] = "digits" if t["width"] > 8 and cnt > 1 else "single" if t["width"] > 8 else "one-pass"
    if topk:
        t["out"] = "lds" if k <= LDS_OUT_MAX else "direct"
        if t["staged"]:
            t["store"], t["out"] = "staged", "direct"
        elif f.load != "full":
            t["store"] = "ragged"
        elif dtype == "i32":
            t["store"] = "regs"
        else:
            t["store"] = "all-ties" if kk_eq == eqn else "reread"
    return t


# ------------------------------------------------------------------ ranks
def select_ranks(cols):
    return sorted({k for k in (1, 2, min(64, cols), (cols + 1) // 2, cols - 1, cols) if 1 <= k <= cols})


def topk_ranks(cols):
    return sorted(set(select_ranks(cols)) | {k for k in (LDS_OUT_MAX, LDS_OUT_MAX + 1) if k <= cols})


def group_ranks(dtype, bits, largest, mask, limit=4):
    """The first and last rank (and, in a group of three or more, the second) of the tie groups
    of the row's keys under `mask`: every group of several keys, and the `limit` first and last
    groups."""
    keys = order_key(dtype, bits)
    allk = np.sort(keys)
    vals, counts = np.unique(keys[mask], return_counts=True)
    pick = set(range(min(limit, vals.size))) | set(range(max(0, vals.size - limit), vals.size))
    pick |= {i for i in range(vals.size) if counts[i] > 1}
    out = set()
    for i in sorted(pick):
        lo = int(np.searchsorted(allk, vals[i], "left"))
        hi = int(np.searchsorted(allk, vals[i], "right"))
        ranks = {lo + 1, hi} | ({lo + 2} if hi - lo >= 3 else set())
        out |= {bits.size + 1 - r for r in ranks} if largest else ranks
    return sorted(out)


def bin_end_ranks(dtype, bits, largest, off=0, want=PICK_BINS):
    """k = cum and cum + 1 for the cumulative count at the end of every populated bin of `want`."""
    _, _, bins, _ = first_pass(dtype, bits, largest, largest, off)
    assert bins is not None
    cum = np.cumsum(np.bincount(bins, minlength=256))
    out = set()
    for b in want:
        if cum[b] > (cum[b - 1] if b else 0):
            out |= {int(cum[b]), int(cum[b]) + 1}
    return sorted(k for k in out if 1 <= k <= bits.size)


# ------------------------------------------------------------------ bits of values
def fv(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def grid(b, j=64):
    """The unit-grid float b + j / 128 (bin b for smallest, 255 - b for largest; j = 64: b + 0.5)."""
    assert 0 <= b < 256 and 0 < j < 128
    return fv(b + j / 128.0)


def iw(b, low):
    """The int32 word whose order key has top byte b and low bits `low`."""
    assert 0 <= b < 256 and 0 <= low < (1 << 24)
    return ((b << 24) | low) ^ 0x80000000


def in_bin(dtype, b, n, ties=True):
    """n keys of value-space bin b: distinct but for one pair (n >= 3) when `ties`."""
    if dtype == "f32":
        assert n <= 120
        out = [grid(b, 1 + i) for i in range(n)]
    else:
        out = [iw(b, 0x010000 + 0x3331 * i) for i in range(n)]
    if ties and n >= 3:
        out[n // 2] = out[0]
    return out


NEG0, POS0 = 0x80000000, 0x00000000
SUB40 = fv(1e-40)
F_PINS = ((0, POS0), (4, fv(256.0)))                       # the sampled range of a unit-grid row
I_PINS = ((0, iw(40, 1)), (4, iw(90, 1)), (8, iw(200, 1)))  # three top bytes in the first key slot
PIN_BINS = {"f32": (0, 255), "i32": (40, 90, 200)}


def filler(dtype, n, avoid):
    """n keys spread over the value-space bins outside `avoid`, distinct, at most a few a bin."""
    free = [b for b in range(5, 251) if b not in avoid and b not in PIN_BINS[dtype]]
    out = []
    for i in range(n):
        b, r = free[i % len(free)], i // len(free)
        assert r < 60
        out.append(grid(b, 3 + 2 * r) if dtype == "f32" else iw(b, 0x200000 + 0x1235 * r))
    return out


def arrange(dtype, cols, vals, seed, pins=None, outside=(), placed=(), avoid=()):
    """A row of `cols` words: `pins` (column, word) and `placed` (columns, words) as given,
    `outside` at random columns != 0 (mod 4), `vals` and filler (avoiding the bins `avoid`)
    at the rest in a fixed-seed order."""
    pins = (F_PINS if dtype == "f32" else I_PINS) if pins is None else pins
    row = np.zeros(cols, dtype=np.uint32)
    taken = np.zeros(cols, dtype=bool)
    for c, w in pins:
        row[c], taken[c] = w, True
    for cs, ws in placed:
        assert not taken[cs].any()
        row[cs], taken[cs] = ws, True
    rng = np.random.default_rng(seed)
    if len(outside):
        cand = np.nonzero(~taken & (np.arange(cols) % 4 != 0))[0]
        cs = rng.choice(cand, len(outside), replace=False)
        row[cs], taken[cs] = outside, True
    rest = np.nonzero(~taken)[0]
    body = list(vals) + filler(dtype, rest.size - len(vals), avoid)
    assert len(body) == rest.size, (len(vals), rest.size)
    row[rest[rng.permutation(rest.size)]] = body
    return row


def mask_of(row, words):
    return np.isin(row, np.array(sorted(set(words)), dtype=np.uint32))


# ------------------------------------------------------------------ edge rows
class Edge:
    """A named row, the ranks it is probed at per direction, and the claims the CPU test proves:
    `claims[call][k]` is a dict of trace fields the row must show at rank k; `every[call]`
    (None: every call) one it must show at each of its `focus` ranks (all its ranks if None)."""

    def __init__(self, name, row, ranks, claims=None, every=None, focus=None):
        self.name, self.row = name, row
        self.ranks = ranks                      # {largest: [k, ...]}
        self.claims = claims or {}
        self.every = every or {}
        self.focus = focus or ranks

    def probes(self, call):
        return self.ranks[call == "largest"]

    def claimed(self, call):
        """[(k, fields)] for the call."""
        want = dict(self.every.get(None, {}), **self.every.get(call, {}))
        out = [(k, want) for k in self.focus[call == "largest"]] if want else []
        return out + sorted(self.claims.get(call, {}).items())


def _both(fn):
    return {False: fn(False), True: fn(True)}


def _pick_claims(dtype, row, off=0):
    """At k = cum(b) the k-th is the last key of kernel bin b; at cum + 1 the first of the next bin."""
    claims = {}
    for call in CALLS:
        largest = call == "largest"
        _, _, bins, _ = first_pass(dtype, row, largest, call != "select", off)
        hist = np.bincount(bins, minlength=256)
        cum = np.cumsum(hist)
        c = claims.setdefault(call, {})
        for b in PICK_BINS:
            if hist[b] == 0:
                continue
            c[int(cum[b])] = {"bin": b, "below": int(cum[b] - hist[b]), "cnt": int(hist[b])}
            if cum[b] < row.size:
                nb = int(np.nonzero(hist[b + 1:])[0][0]) + b + 1
                c[int(cum[b]) + 1] = {"bin": nb, "below": int(cum[b])}
    return claims


def full_edges(dtype, cols):
    """The edge rows of a FULL width, in a fixed order."""
    f32 = dtype == "f32"
    out = []
    seed = iter(range(1000 * cols + (7 if f32 else 0), 1000 * cols + 900))

    def add(name, row, masks=None, extra=(), claims=None, every=None, limit=4):
        """masks: the columns whose tie groups are probed (one mask, or one per direction); the
        claims of `every` hold at those probes (at every probe when there is no mask)."""
        def focus(largest):
            m = masks[largest] if isinstance(masks, dict) else masks
            return [] if m is None else group_ranks(dtype, row, largest, m, limit)

        def ranks(largest):
            ks = set(extra) | ({cols + 1 - k for k in extra} if largest else set()) | set(focus(largest))
            return sorted(k for k in ks if 1 <= k <= cols)
        out.append(Edge(name, row, _both(ranks), claims, every, _both(focus) if masks is not None else None))
        return out[-1]

    # the pick: cumulative counts ending at the bins of PICK_BINS (both directions: the set is symmetric)
    words = []
    for b in PICK_BINS:
        n = 5 - sum(1 for pb in PIN_BINS[dtype] if pb == b)
        words += in_bin(dtype, b, n)
    row = arrange(dtype, cols, words, next(seed), avoid=PICK_BINS)
    e = add("pick", row, claims=_pick_claims(dtype, row))
    for lg in (False, True):
        e.ranks[lg] = bin_end_ranks(dtype, row, lg)

    # list versus dense: 1, 63, 64, 65 keys in bin 100
    for n in (1, 63, 64, 65):
        words = in_bin(dtype, 100, n)
        row = arrange(dtype, cols, words, next(seed), avoid=(100, 155))
        add("list%d" % n, row, mask_of(row, words), every={None: {"cnt": n, "finish": "list" if n <= 64 else "radix"}})

    # dense bins: one value, 8 adjacent keys, 9 adjacent keys
    base = grid(100) if f32 else iw(100, 5000)
    for name, nv, fin in (("span0", 1, "span0"), ("span7", 8, "count8"), ("span8", 9, "radix")):
        words = [base + (i % nv) for i in range(100)]
        row = arrange(dtype, cols, words, next(seed), avoid=(100, 155))
        add(name, row, mask_of(row, words), every={None: {"cnt": 100, "finish": fin, "span": nv - 1}}, limit=9)

    # dense bin 0 and dense bin 255, float keys clamped in from outside the sampled range
    if f32:
        lo = [fv(x) for x in (-1e30, -3.5, 0.25, 0.75)]
        hi = [fv(x) for x in (255.25, 255.75, 300.0, 1e30)]
        outside = [lo[i % 2] for i in range(50)] + [hi[2 + i % 2] for i in range(50)]
        words = [lo[2 + i % 2] for i in range(49)] + [hi[i % 2] for i in range(49)]
        row = arrange(dtype, cols, words, next(seed), outside=outside, avoid=(0, 255))
        add("dense0_255", row, mask_of(row, lo + hi + [POS0, fv(256.0)]), every={None: {"cnt": 100, "finish": "radix"}})
    else:
        lo = [iw(0, 0), iw(0, 1), iw(0, 0x800000), iw(0, 0xFFFFFF)]
        hi = [iw(255, 0), iw(255, 0x7FFFFF), iw(255, 0xFFFFFE), iw(255, 0xFFFFFF)]
        words = [lo[i % 4] for i in range(100)] + [hi[i % 4] for i in range(100)]
        row = arrange(dtype, cols, words, next(seed), avoid=(0, 255))
        add("dense0_255", row, mask_of(row, lo + hi), every={None: {"cnt": 100, "finish": "radix"}})

    # top-k staging: below + cnt = 488 and 489, mirrored so that both directions meet it
    for total in (STAGE_CAP, STAGE_CAP + 1):
        words, focus = [], {0: [], 1: []}
        for side in (0, 1):
            n_low = total - 8 - (1 if f32 else 0)  # (the pinned 0.0 / 256.0 is one of the keys below)
            for i in range(n_low):
                b, r = i % 8, i // 8
                b = 255 - b if side else b
                words.append(grid(b, 2 + r) if f32 else iw(b, 0x4000 + 0x0101 * r))
            b = 247 if side else 8
            tie = grid(b, 50) if f32 else iw(b, 0x5000)
            f = [tie] * 4 + ([grid(b, 10 + 9 * i) for i in range(4)] if f32 else [iw(b, 0x100 + 0x2000 * i) for i in range(4)])
            words += f
            focus[side] = f
        row = arrange(dtype, cols, words, next(seed), avoid=tuple(range(0, 9)) + tuple(range(247, 256)))
        ev = {c: {"bin": 8, "below": total - 8, "cnt": 8, "finish": "list", "staged": total <= STAGE_CAP}
              for c in ("smallest", "largest")}
        add("stage%d" % total, row, {False: mask_of(row, focus[0]), True: mask_of(row, focus[1])}, every=ev)

    # staged keys never two to a lane's four columns, versus on adjacent columns; more than 64 staged
    for name in ("stage_sparse", "stage_adjacent"):
        lows, highs = [], []
        for side, dst in ((0, lows), (1, highs)):
            for i in range(100 - (1 if f32 else 0)):
                b, r = i % 5, i // 5
                b = 255 - b if side else b
                dst.append(grid(b, 2 + r) if f32 else iw(b, 0x4000 + 0x0101 * r))
            b = 250 if side else 5
            tie = grid(b, 50) if f32 else iw(b, 0x5000)
            dst += [tie] * 3 + ([grid(b, 10 + 9 * i) for i in range(3)] if f32 else [iw(b, 0x100 + 0x2000 * i) for i in range(3)])
        n = len(lows)
        if name == "stage_sparse":
            g = 3 + np.arange(2 * n)  # one key to a group of four columns, the column within it rotating
            cs = 4 * g + g % 4
            lo_cols, hi_cols = cs[0::2], cs[1::2]
        else:
            lo_cols, hi_cols = 16 + np.arange(n), 16 + n + np.arange(n)
        perm = np.random.default_rng(next(seed)).permutation(n)
        placed = ((lo_cols, np.array(lows, dtype=np.uint32)[perm]), (hi_cols, np.array(highs, dtype=np.uint32)[perm]))
        row = arrange(dtype, cols, [], next(seed), placed=placed, avoid=tuple(range(0, 6)) + tuple(range(250, 256)))
        ev = {c: {"bin": 5, "below": 100, "cnt": 6, "finish": "list", "staged": True, "n_staged": 106}
              for c in ("smallest", "largest")}
        for c in ev:
            ev[c]["coll_groups" if name == "stage_sparse" else "fast_groups"] = 0
        add(name, row, {False: mask_of(row, lows[-6:]), True: mask_of(row, highs[-6:])}, every=ev)

    if f32:
        _f32_zero_edges(cols, seed, add)
        _f32_range_edges(cols, seed, add)
    else:
        _i32_few_edges(cols, seed, add)
    return out


def _f32_zero_edges(cols, seed, add):
    """Dense bins at zero (value-space bin 0: kernel bin 0 for smallest, 255 for largest)."""
    half, sub1 = fv(0.5), 0x00000001
    specs = (("zeros_neg", [NEG0] * 99, ((0, NEG0), (4, fv(256.0)))),
             ("zeros_pos", [POS0] * 99, None),
             ("zeros_mixed", [NEG0, POS0] * 49 + [NEG0], None),
             ("zeros_subnormal", [NEG0] * 45 + [POS0] * 44 + [SUB40] * 10, None),
             ("zeros_half", [NEG0] * 45 + [POS0] * 44 + [half] * 10, None),
             ("end_min_subnormal", [sub1 + i % 8 for i in range(99)], ((0, sub1), (4, fv(256.0)))),
             ("end_1e-40", [SUB40] * 69 + [fv(0.25)] * 30, ((0, SUB40), (4, fv(256.0)))))
    fins = {"zeros_neg": ("zero-bin", "span0"), "zeros_pos": ("zero-bin", "span0"), "zeros_mixed": ("zero-bin", "two-zeros"),
            "zeros_subnormal": ("radix", "radix"), "zeros_half": ("radix", "radix"),
            "end_min_subnormal": ("count8", "count8"), "end_1e-40": ("radix", "radix")}
    for name, words, pins in specs:
        row = arrange("f32", cols, words, next(seed), pins=pins, avoid=(0, 255))
        sel, tk = fins[name]
        ev = {"select": {"bin": 0, "cnt": 100, "finish": sel}, "smallest": {"bin": 0, "cnt": 100, "finish": tk},
              "largest": {"bin": 255, "cnt": 100, "finish": tk}}
        add(name, row, mask_of(row, words + [w for _, w in (pins or F_PINS)][:1]), every=ev, limit=8)


def _f32_range_edges(cols, seed, add):
    """Rows that decide the FULL path's sampled range and its map."""
    generic = (1, 2, 64, 65, cols // 2)
    body = [w for b in (3, 4, 100, 127, 128, 252) for w in in_bin("f32", b, 4)]
    for r in (1, 2, 3):  # the row's extremes on columns = r (mod 4): outside the sampled range
        ext = [fv(-1000.0), fv(1000.0), fv(-2.0), fv(257.0)]
        cs = np.array([400 + r, 404 + r, 600 + r, 608 + r])
        row = arrange("f32", cols, body, next(seed), placed=((cs, np.array(ext, dtype=np.uint32)),))
        add("extremes_col%d" % r, row, mask_of(row, ext), extra=generic, every={None: {"map": "value", "exact": True}})
    uns = np.arange(cols) % 4 != 0
    rng = np.random.default_rng(next(seed))

    def sampled(svals, rest):
        row = np.zeros(cols, dtype=np.uint32)
        row[~uns] = np.array(svals, dtype=np.uint32)[np.arange((~uns).sum()) % len(svals)]
        row[uns] = rest
        return row

    varied = np.array([grid(b, 64) for b in range(256)], dtype=np.uint32)[rng.integers(0, 256, int(uns.sum()))]
    add("sampled_equal", sampled([fv(7.0)], varied), extra=generic, every={None: {"map": "byte"}})
    add("sampled_subnormal", sampled([POS0, SUB40], varied), extra=generic, every={None: {"map": "byte"}})
    big = rng.uniform(-3e38, 3e38, int(uns.sum())).astype(np.float32).view(np.uint32)
    add("sampled_3e38", sampled([fv(-3e38), fv(3e38), fv(1.0)], big), extra=generic, every={None: {"map": "byte"}})
    for name, col, w, mp in (("pinf_sampled", 8, fv(np.inf), "byte"), ("ninf_sampled", 8, fv(-np.inf), "byte"),
                             ("pinf_unsampled", 9, fv(np.inf), "value"), ("ninf_unsampled", 9, fv(-np.inf), "value")):
        row = arrange("f32", cols, body, next(seed), placed=((np.array([col]), np.array([w], dtype=np.uint32)),))
        add(name, row, mask_of(row, [w]), extra=generic, every={None: {"map": mp}})
    row = arrange("f32", cols, body, next(seed), placed=((np.array([cols - 1]), np.array([0xFFC00001], dtype=np.uint32)),))
    add("nan_last_column", row, mask_of(row, [0xFFC00001]), extra=generic, every={None: {"map": "byte"}})


def _i32_few_edges(cols, seed, add):
    """Few-valued int rows: the shortcut (at most two top bytes in the first key slot and a
    range below 8) and its neighbours."""
    rng = np.random.default_rng(next(seed))
    every_col = np.ones(cols, dtype=bool)

    def few(lo_key, n):
        keys = (lo_key + rng.permutation(cols) % n).astype(np.uint64)  # every value, as often as the others
        return (keys ^ np.uint64(0x80000000)).astype(np.uint32)

    cnt8 = {None: {"map": "few", "finish": "count8"}}
    add("few_range7", few(0x80000000 + 1000, 8), every_col, every=cnt8, limit=9)
    add("few_range8", few(0x80000000 + 1000, 9), every_col, every={None: {"map": "byte", "finish": "radix", "span": 8}},
        limit=9)
    add("few_across_top_byte", few(0x65000000 - 4, 8), every_col, every=dict(cnt8, **{"select": {"slot_bytes": 2}}), limit=9)
    add("few_across_minus1", few(0x80000000 - 4, 8), every_col, every=cnt8, limit=9)
    add("few_int_min", few(0, 8), every_col, every=cnt8, limit=9)
    add("few_int_max", few(0xFFFFFFFF - 7, 8), every_col, every=cnt8, limit=9)
    row = few(0x80000000 + 1000, 8)
    row[[0, 4]] = [iw(3, 7), iw(254, 7)]  # with the row's own: three
    add("few_three_top_bytes", row, every_col, every={None: {"map": "byte", "slot_bytes": 3}}, limit=12)
    row = few(0x80000000 + 1000, 8)
    row[1::4] = iw(130, 7)  # a second value far away, never in the first key slot's columns
    add("few_one_byte_wide_range", row, every_col, every={None: {"map": "byte", "slot_bytes": 1}}, limit=12)
    row = few(0x80000000 + 1000, 8)
    lane = 5
    row[(np.arange(cols) // 4) % WAVE == lane] = np.uint32((0x80000000 + 1003) ^ 0x80000000)
    add("few_one_valued_lane", row, every_col, every=cnt8, limit=9)


# ragged widths ------------------------------------------------------
INT_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32)


def ragged_edges(dtype, cols):
    """The edge rows of a ragged width (the same rows serve an aligned base and one an element off)."""
    out = []
    seed = iter(range(5000 * cols + (7 if dtype == "f32" else 0), 5000 * cols + 900))
    generic = {1, 2, (cols + 1) // 2, cols - 1, cols}

    def add(name, row, ks_fn, every=None, focus_only=False):
        focus = _both(lambda lg: sorted(k for k in set(ks_fn(lg)) if 1 <= k <= cols))
        ranks = {lg: sorted(set(ks) | generic) for lg, ks in focus.items()}
        out.append(Edge(name, row, ranks, None, every, focus if focus_only else None))

    if dtype == "i32":
        for w in INT_WIDTHS:
            rng = np.random.default_rng(next(seed))
            lo = 0 if w == 32 else 0x80000000 - (1 << w) // 2  # (widths above 1 straddle -1 / 0)
            keys = lo + rng.integers(0, 1 << w, cols).astype(np.uint64)
            ends = rng.permutation(cols)[:6]
            keys[ends[:3]], keys[ends[3:]] = lo, lo + (1 << w) - 1  # both ends present, three times each
            row = (keys ^ np.uint64(0x80000000)).astype(np.uint32)
            ends_mask = np.zeros(cols, dtype=bool)
            ends_mask[ends] = True
            mask = np.ones(cols, dtype=bool) if w <= 3 else ends_mask
            add("width%d" % w, row,
                lambda lg, row=row, mask=mask: set(bin_end_ranks("i32", row, lg)) | set(group_ranks("i32", row, lg, mask, 8)),
                every={None: {"map": "range-int", "width": w}})
    else:
        words = [w for b in PICK_BINS for w in in_bin("f32", b, 3)] + [POS0, fv(256.0)]
        row = arrange("f32", cols, words, next(seed), pins=(), avoid=PICK_BINS)
        add("pick", row, lambda lg, row=row, words=words: set(bin_end_ranks("f32", row, lg)) |
            set(group_ranks("f32", row, lg, mask_of(row, words), 30)), every={None: {"map": "range-value", "exact": True}})
        for name, n in (("interval_one_value", 6), ("interval_single_key", 1)):
            words = [grid(100, 64)] * n
            row = arrange("f32", cols, words + [POS0, fv(256.0)], next(seed), pins=(), avoid=(100, 155))
            add(name, row, lambda lg, row=row, words=words: group_ranks("f32", row, lg, mask_of(row, words)),
                every={None: {"map": "range-value", "finish": "interval-one", "interval_keys": n}}, focus_only=True)
        rng = np.random.default_rng(next(seed))
        body = rng.standard_normal(cols).astype(np.float32).view(np.uint32)
        row = body.copy()
        row[[3, cols - 2, cols // 2]] = [fv(np.inf), fv(-np.inf), fv(np.inf)]
        add("non_finite", row, lambda lg, row=row: group_ranks("f32", row, lg, mask_of(row, [fv(np.inf), fv(-np.inf)])),
            every={None: {"map": "range-int"}})
        row = body.copy()
        row[[5, cols - 1, cols // 3]] = [0x7FC00001, 0xFFC00000, 0xFF800001]
        add("nan", row, lambda lg, row=row: group_ranks("f32", row, lg, (order_key("f32", row) == 0xFFFFFFFF)),
            every={None: {"map": "range-int"}})
    return out


# ------------------------------------------------------------------ the form matrix
def matrix_bits(cols, rows=ROWS, seed=0):
    """`rows` rows of `cols` bit patterns, shared by both types: the fixed special rows, then
    random patterns over all 2^32 values."""
    rng = np.random.default_rng(977 * cols + seed)
    rnd = lambda: rng.integers(0, 1 << 32, cols, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    out = [np.full(cols, v, dtype=np.uint32) for v in (0x80000000, 0x7FFFFFFF, 0x00000000, 0xFFFFFFFF, 0xFF7FFFFF,
                                                        0x7F7FFFFF)]               # all equal, the types' extremes
    out.append(np.where(np.arange(cols) % 2 == 0, NEG0, POS0).astype(np.uint32))  # -0.0 / +0.0 alternating
    out.append(np.where(rng.integers(0, 2, cols) != 0, 0x7F800000, 0xFF800000).astype(np.uint32))  # +-inf
    out.append((rnd() & np.uint32(0x807FFFFF)))                                    # subnormals and zeros, both signs
    nan = np.uint32(0x7F800001) + rnd() % np.uint32(0x007FFFFF)                    # every payload ...
    out.append(nan | (rnd() & np.uint32(0x80000000)))                              # ... of either sign
    mixed = rnd()
    mixed[::5] = nan[::5] | (mixed[::5] & np.uint32(0x80000000))                   # NaNs among ordinary keys
    out.append(mixed)
    r = rnd()
    for dtype in DTYPES:
        asc = r[np.argsort(order_key(dtype, r), kind="stable")]
        out += [asc, asc[::-1].copy()]                                             # sorted in the type's order
    out.append(np.where(rng.integers(0, 2, cols) != 0, 0x3F800001, 0x3F800000).astype(np.uint32))  # two values
    out.append(np.where(rng.integers(0, 2, cols) != 0, 0xBF800000, 0x3F800000).astype(np.uint32))
    while len(out) < max(rows, 18):
        out.append(rnd())
    if rows < 18:  # the wide selects: NaNs among keys, a sorted row, two values, random rows
        out = [out[i] for i in (10, 11, 15, 16, 17)][:rows]
    return np.ascontiguousarray(np.stack(out[:rows]), dtype=np.uint32)


# ------------------------------------------------------------------ built once
_BUILT = {}


def once(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


def matrix(dtype, cols):
    rows = ROWS if cols <= REG_MAX_COLS else WIDE_ROWS
    return once(("matrix", dtype, cols), lambda: Ref(dtype, matrix_bits(cols, rows)))


def edges(dtype, cols):
    return once(("edges", dtype, cols), lambda: (full_edges if cols in FULL_WIDTHS else ragged_edges)(dtype, cols))


def edge_case(dtype, cols):
    """(Ref of the stacked edge rows, {call: sorted ranks probed}): every row meets every rank."""
    def make():
        es = edges(dtype, cols)
        ranks = {call: sorted({k for e in es for k in e.probes(call)}) for call in CALLS}
        return Ref(dtype, np.stack([e.row for e in es])), ranks
    return once(("edge case", dtype, cols), make)
