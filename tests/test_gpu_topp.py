"""GPU: top-p (nucleus) selection per row (include/kth.h "wide rows, top-p";
csrc/kth_rows_topp.hpp, csrc/kth_rows_topp16.hpp) for float32, bfloat16 and
float16 rows, in both forms, under forced plans and on both load paths.

Reference: numpy float64 over the documented order -- the stable argsort of
the order key, largest first -- and the header's weight rule.  The device
weighs in float32 and sums fixed point, so a call may return any n inside the
header's band, eps = 2^-16 + cols * 2^-39:
    S(n) >= p Z (1 - eps)  and  (n == 1 or S(n - 1) < p Z (1 + eps));
p < 0 counts as 0, p >= 1 or NaN gives len exactly, an empty row 0.  d_thr must
be the bits of the n-th key of the order for the n returned (a NaN canonical,
the zero word for an empty row).  The matrices, order keys, poisoned outputs
and helpers are those of tests/test_gpu_rows_wide.py, tests/test_gpu_rows_wide16.py
and tests/test_gpu_rows_var.py; every column at and past len_r, the row padding
and the elements before a shifted base hold a NaN, which would be the maximum,
so a read past the length changes n.
"""
import math

import numpy as np
import pytest

import test_gpu_rows_var as V
import test_gpu_rows_wide as W
import test_gpu_rows_wide16 as W16

pytestmark = pytest.mark.gpu

NAMES = ("f32", "bf16", "f16")
ROWS = V.ROWS
NAN = float("nan")
PS = (-1.0, 0.0, 0.3, 0.9, 0.999, 1.0, 2.0, NAN)
TEMPS = (0.5, 1.0, 2.0, 0.0, NAN)
# (slices, group_rows): fused, three split plans, groups of 3 rows under the automatic plan and,
# split in 4, with every per-row array advanced and the scratch reused from group to group
PLANS = ((1, 0), (4, 0), (7, 0), (256, 0), (0, 3), (4, 3))


def eps_of(cols):
    return 2.0 ** -16 + cols * 2.0 ** -39


# ------------------------------------------------------------------ the reference
def values(fl, words):
    """The keys as float64."""
    with np.errstate(invalid="ignore"):  # (a signalling NaN among the keys)
        if fl.name == "f32":
            return words.astype(np.uint32).view(np.float32).astype(np.float64)
        if fl.name == "f16":
            return words.astype(np.uint16).view(np.float16).astype(np.float64)
        return (words.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


class RowRef:
    """One row's order, cumulative weights and band."""

    def __init__(self, fl, words, p, temp, cols):
        self.len = words.size
        self.eps = eps_of(cols)
        p32 = np.float32(p)
        self.p = 1.0 if (math.isnan(p) or p32 >= 1) else max(float(p32), 0.0)
        t32 = np.float32(temp)
        t = float(t32) if (np.isfinite(t32) and t32 > 0) else 1.0
        if self.len == 0:
            return
        key = fl.keys(words)
        self.order = np.argsort(~key, kind="stable")
        self.bits = fl.canon(words[self.order])
        x = values(fl, words)
        m = x[self.order[0]]
        top = key == key[self.order[0]]
        with np.errstate(invalid="ignore", over="ignore"):
            if math.isnan(m) or m == math.inf:
                w = np.where(top, 1.0, 0.0)
            else:
                w = np.where(top, 1.0, np.where(x == -math.inf, 0.0, np.exp((x - m) / t)))
        self.s = np.concatenate([[0.0], np.cumsum(w[self.order])])  # s[j] = S(j)
        self.z = self.s[-1]

    def admits(self, n):
        if self.len == 0:
            return n == 0
        if self.p >= 1.0:
            return n == self.len
        if not 1 <= n <= self.len:
            return False
        pz = self.p * self.z
        return self.s[n] >= pz * (1 - self.eps) and (n == 1 or self.s[n - 1] < pz * (1 + self.eps))

    def band(self):
        """Every n the contract admits (the contract value among them)."""
        if self.len == 0:
            return [0]
        if self.p >= 1.0:
            return [self.len]
        pz = self.p * self.z
        lo = max(1, int(np.searchsorted(self.s, pz * (1 - self.eps), side="left")))
        out = [n for n in range(max(1, lo - 2), min(self.len, lo + 66) + 1) if self.admits(n)]
        assert out and out[-1] < lo + 66, "the band search window is too narrow"
        return out

    def thr(self, n):
        return self.bits[n - 1] if n >= 1 else 0


def per_row(a, r, default):
    return default if a is None else a[r]


def refs_of(fl, words, lens, ps, temps, p=1.0, temp=1.0):
    rows, cols = words.shape
    return [RowRef(fl, words[r, :n], per_row(ps, r, p), per_row(temps, r, temp), cols)
            for r, n in enumerate(V.row_lens(lens, rows, cols))]


def dev_f32(a):
    import torch
    return None if a is None else torch.tensor([float(x) for x in a], dtype=torch.float32, device="cuda")


def nucleus(sel, fl, d, rows, cols, d_n, d_thr, p=1.0, temp=1.0, lens=None, ps=None, temps=None, ld=None):
    if fl.w16:
        sel.nucleus_rows_wide16(d, rows, cols, d_n, d_thr, p=p, temp=temp, kind=fl.name, d_lens=lens, d_ps=ps,
                                d_temps=temps, ld=ld)
    else:
        sel.nucleus_rows_wide(d, rows, cols, d_n, d_thr, p=p, temp=temp, d_lens=lens, d_ps=ps, d_temps=temps, ld=ld)


def topp(sel, fl, d, rows, cols, k, vals, idx, p=1.0, temp=1.0, lens=None, ks=None, ps=None, temps=None, cnt=None,
         ld=None):
    if fl.w16:
        sel.topp_rows_wide16(d, rows, cols, k, vals, idx, p=p, temp=temp, kind=fl.name, d_lens=lens, d_ks=ks, d_ps=ps,
                             d_temps=temps, d_cnt=cnt, ld=ld)
    else:
        sel.topp_rows_wide(d, rows, cols, k, vals, idx, p=p, temp=temp, d_lens=lens, d_ks=ks, d_ps=ps, d_temps=temps,
                           d_cnt=cnt, ld=ld)


def run_nucleus(sel, fl, d, rows, cols, lens, ps, temps, p=1.0, temp=1.0, ld=None):
    """(n, thr) of one call, from poisoned outputs with guards."""
    o_n, o_t = W.Out(rows), fl.out_vals(rows)
    W.run(sel, lambda: nucleus(sel, fl, d, rows, cols, o_n.t, o_t.t, p, temp, V.dev_i32(lens), dev_f32(ps),
                               dev_f32(temps), ld))
    return o_n.get().view(np.int32).copy(), o_t.get().copy()


def check_band(refs, n, thr, tag):
    for r, ref in enumerate(refs):
        assert ref.admits(int(n[r])), (tag, "row", r, "n", int(n[r]), "band", ref.band(), "len", ref.len, "p", ref.p)
        assert int(thr[r]) == int(ref.thr(int(n[r]))), (tag, "row", r, "thr", hex(int(thr[r])), hex(int(ref.thr(int(n[r])))))


# ------------------------------------------------------------------ inputs
def logits(fl, cols, seed=0):
    """ROWS rows a sampler meets: randn logits of three spreads, sorted both ways, a few equal
    maxima, -inf masked columns, one dominant key."""
    rng = np.random.default_rng(7000 + cols + seed)
    x = rng.standard_normal((ROWS, cols)).astype(np.float32) * np.array([4, 1, 12, 4, 4, 0.25, 4, 4, 4, 30],
                                                                        dtype=np.float32)[:, None]
    x[3] = np.sort(x[3])
    x[4] = np.sort(x[4])[::-1]
    x[6, rng.integers(0, cols, max(1, cols // 3))] = -np.inf
    x[7, rng.integers(0, cols, min(cols, 5))] = x[7].max()
    x[8, rng.integers(0, cols)] = x[8].max() + 9
    if fl.name == "f32":
        return x.view(np.uint32).copy()
    return W16.to_kind_bits(x.ravel(), fl.name).reshape(ROWS, cols)


_CASES = {}


def case(name, cols, which):
    """(flavor, words, lens, ps, temps, refs): built and referenced once, shared by every plan and path."""
    key = (name, cols, which)
    if key not in _CASES:
        fl = V.Flavor(name)
        words = fl.words(cols) if which == 0 else logits(fl, cols)
        pool = [cols, 0, 1, cols - 1, cols // 2 + 1, min(5, cols), cols + 5, -3, (3 * cols) // 4, 2]
        rot = 3 * which
        lens = [pool[(r + rot) % len(pool)] for r in range(ROWS)]
        ps = [PS[(r + 5 * which + 2) % len(PS)] for r in range(ROWS)]
        temps = [TEMPS[(2 * r + which) % len(TEMPS)] for r in range(ROWS)]
        _CASES[key] = (fl, words, lens, ps, temps, refs_of(fl, words, lens, ps, temps))
    return _CASES[key]


def paths(fl, cols):
    """(ld, shift): the aligned base with ld = cols rounded up, and a shifted base with an odd ld."""
    return ((-(-cols // fl.align) * fl.align, 0), (cols + 1 if cols % 2 == 0 else cols + 2, 1))


# ------------------------------------------------------------------ the band
@pytest.mark.parametrize("cols", (1, 3, 5, 1023, 4099, 8191, 8193, 33001))
@pytest.mark.parametrize("name", NAMES)
def test_band(gpu, name, cols):
    """Every row of every case returns an n inside the band and the n-th key's bits: two matrices
    (the mixed row kinds of the wide-rows tests, and logits), ragged lengths with 0, 1 and cols
    among them, the device p and T lists, under every plan and on both load paths."""
    plans = PLANS + (((0, 0),) if cols == 33001 else ())
    for which in (0, 1):
        fl, words, lens, ps, temps, refs = case(name, cols, which)
        for ld, shift in paths(fl, cols):
            d = fl.device(words, lens, True, ld=ld, shift=shift)
            for slices, group in plans:
                with W.forced(gpu, slices, group):
                    n, thr = run_nucleus(gpu, fl, d, ROWS, cols, lens, ps, temps, ld=ld)
                check_band(refs, n, thr, (name, cols, which, ld, shift, slices, group))
    # the host scalars: no device array at all
    fl, words = V.Flavor(name), logits(V.Flavor(name), cols)
    for p, temp in ((0.9, 1.0), (0.5, 0.7), (-2.0, 1.0), (1.0, 3.0)):
        refs = refs_of(fl, words, None, None, None, p, temp)
        n, thr = run_nucleus(gpu, fl, fl.device(words, None, True), ROWS, cols, None, None, None, p, temp)
        check_band(refs, n, thr, (name, cols, "scalars", p, temp))


# ------------------------------------------------------------------ exact rows
EXACT_COLS = 1023


def exact_rows(fl):
    """Rows whose band admits one n: (values, len, p, T)."""
    c = EXACT_COLS
    inf = np.float32(np.inf)
    eq = np.full(c, 1.5, dtype=np.float32)
    peak = np.full(c, -3.0, dtype=np.float32)
    peak[c // 3] = 17.0  # one key 20 above the rest
    two = np.where(np.arange(c) % 10 == 3, 1.0, 0.0).astype(np.float32)  # 102 keys at 1.0, the rest at 0.0
    infs = np.linspace(-4, 4, c).astype(np.float32)
    infs[[7, 600]] = inf
    nans = np.linspace(-4, 4, c).astype(np.float32)
    ninf = np.full(c, -inf, dtype=np.float32)
    zeros = np.where(np.arange(c) % 2 == 0, -0.0, 0.0).astype(np.float32)
    rows = [(eq, c, 0.5, 1.0), (eq, 701, 0.3, 2.0), (peak, c, 0.9, 1.0), (peak, c, 0.999, 0.5), (two, c, 0.5, 1.0),
            (two, c, 0.1, 1.0), (infs, c, 0.3, 1.0), (infs, c, 0.9, 1.0), (nans, c, 0.5, 1.0), (ninf, c, 0.5, 1.0),
            (zeros, c, 0.25, 1.0), (zeros, c, 0.75, 1.0)]
    x = np.stack([r[0] for r in rows])
    words = x.view(np.uint32).copy() if fl.name == "f32" else W16.to_kind_bits(x.ravel(), fl.name).reshape(x.shape)
    nan_row = 8  # three NaNs of different payloads and signs
    if fl.name == "f32":
        words[nan_row, [5, 300, 900]] = [0x7FC00000, 0xFFC12345, 0x7F800001]
    else:
        q = W16.INF[fl.name]
        words[nan_row, [5, 300, 900]] = [q + 1, 0x8000 | (q + 3), W16.CANON[fl.name]]
    return words, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]


@pytest.mark.parametrize("name", NAMES)
def test_exact_rows(gpu, name):
    """c equal values, one key 20 above the rest, two levels, +inf twice, NaNs, all -inf, -0.0 / +0.0:
    the band is one n wide (asserted on the CPU first), so n and the threshold are compared for equality."""
    fl = V.Flavor(name)
    words, lens, ps, temps = exact_rows(fl)
    refs = refs_of(fl, words, lens, ps, temps)
    want = []
    for r, ref in enumerate(refs):
        band = ref.band()
        assert len(band) == 1, ("the band of exact row", r, "is", band)
        want.append(band[0])
    # what the rows are built to give: ceil(p c) for equal keys, the peak alone, both infinities, two NaNs
    assert want[0] == 512 and want[1] == 211 and want[2] == 1 and want[3] == 1
    assert want[6] == 1 and want[7] == 2 and want[8] == 2 and want[9] == 512 and want[10] == 256 and want[11] == 768
    rows, cols = words.shape
    for ld, shift in paths(fl, cols):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        for slices, group in ((1, 0), (4, 0), (0, 5)):
            with W.forced(gpu, slices, group):
                n, thr = run_nucleus(gpu, fl, d, rows, cols, lens, ps, temps, ld=ld)
            assert n.tolist() == want, (name, slices, group, n.tolist(), want)
            assert [int(t) for t in thr] == [int(ref.thr(w)) for ref, w in zip(refs, want)], (name, slices, group)


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", NAMES)
def test_deterministic_across_plans_paths_and_runs(gpu, name):
    """One 10 x 33001 matrix under every plan and both load paths, twice each: d_n and d_thr are
    bit-identical throughout."""
    cols = 33001
    fl, words, lens, ps, temps, refs = case(name, cols, 1)
    lens = [cols, cols - 1, cols, 20000, cols, cols, 8193, cols, cols, cols]
    ps = [0.9, 0.5, 0.99, 0.3, 0.999, 0.9, 0.7, 0.95, 0.9, 0.6]
    temps = [1.0, 0.7, 2.0, 1.0, 1.3, 0.5, 1.0, 1.0, 3.0, 1.0]
    first = None
    for ld, shift in paths(fl, cols):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        for slices, group in PLANS + ((0, 0),):
            for again in range(2):
                with W.forced(gpu, slices, group):
                    got = run_nucleus(gpu, fl, d, ROWS, cols, lens, ps, temps, ld=ld)
                if first is None:
                    first = got
                    check_band(refs_of(fl, words, lens, ps, temps), got[0], got[1], (name, "determinism"))
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), \
                    (name, ld, shift, slices, group, again, got[0], first[0])


# ------------------------------------------------------------------ composition
@pytest.mark.parametrize("cols", (4099, 33001))
@pytest.mark.parametrize("name", NAMES)
def test_topp_is_nucleus_then_var_topk(gpu, name, cols):
    """topp_* against the caller-side composition -- nucleus_*, a min with the caps, then the var
    top-k with largest -- bit for bit: values, columns, padding and d_cnt; d_ks given and NULL;
    d_vals-only and d_idx-only; poisoned outputs with guards."""
    import torch
    k = 64
    fl, words, lens, ps, temps, _ = case(name, cols, 1)
    caps = [64, 0, 1, 7, 64, 100, -2, 33, 64, 2]
    for (ld, shift), (slices, group) in zip(paths(fl, cols) + paths(fl, cols)[:1], ((1, 0), (4, 0), (0, 3))):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        dl, dp, dt = V.dev_i32(lens), dev_f32(ps), dev_f32(temps)
        with W.forced(gpu, slices, group):
            o_n = W.Out(ROWS)
            W.run(gpu, lambda: nucleus(gpu, fl, d, ROWS, cols, o_n.t, None, lens=dl, ps=dp, temps=dt, ld=ld))
            n = o_n.get().view(np.int32)
            for ks in (caps, None):
                cap = [k] * ROWS if ks is None else [V.clamp(q, 0, k) for q in ks]
                ranks = torch.tensor([min(int(a), b) for a, b in zip(n, cap)], dtype=torch.int32, device="cuda")
                w_v, w_i, w_c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
                W.run(gpu, lambda: fl.topk(gpu, d, ROWS, cols, k, w_v.t, w_i.t, True, dl, ranks, w_c.t, ld))
                for mode in ("both", "vals", "idx"):
                    g_v = fl.out_vals(ROWS * k) if mode != "idx" else None
                    g_i = fl.out_idx(ROWS * k) if mode != "vals" else None
                    g_c = W.Out(ROWS) if mode == "both" else None
                    W.run(gpu, lambda: topp(gpu, fl, d, ROWS, cols, k, g_v.t if g_v else None, g_i.t if g_i else None,
                                            lens=dl, ks=V.dev_i32(ks), ps=dp, temps=dt, cnt=g_c.t if g_c else None,
                                            ld=ld))
                    tag = (name, cols, slices, group, ks is None, mode)
                    if g_v:
                        assert np.array_equal(g_v.get(), w_v.get()), tag
                    if g_i:
                        assert np.array_equal(g_i.get(), w_i.get()), tag
                    if g_c:
                        assert np.array_equal(g_c.get(), w_c.get()), (tag, g_c.get(), w_c.get())


# ------------------------------------------------------------------ scratch left as found
@pytest.mark.parametrize("slices", (1, 5))
@pytest.mark.parametrize("name", NAMES)
def test_scratch_left_as_found(gpu, name, slices):
    """A top-p call (and two in a row) between two uniform wide selects and between two var top-k
    calls on one ctx changes none of their outputs, nor its own."""
    cols, k = 8193, 32
    fl, words, lens, ps, temps, refs = case(name, cols, 1)
    d = fl.device(words, lens, True)
    dfull = fl.device(words, None, True)
    dl, dp, dt = V.dev_i32(lens), dev_f32(ps), dev_f32(temps)

    def select():
        o = fl.out_vals(ROWS)
        W.run(gpu, lambda: fl.uniform_select(gpu, dfull, ROWS, cols, cols // 3, o.t))
        return o.get().copy()

    def var_topk():
        v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        W.run(gpu, lambda: fl.topk(gpu, d, ROWS, cols, k, v.t, i.t, True, dl, None, c.t))
        return v.get().copy(), i.get().copy(), c.get().copy()

    def top_p():
        v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        W.run(gpu, lambda: topp(gpu, fl, d, ROWS, cols, k, v.t, i.t, lens=dl, ps=dp, temps=dt, cnt=c.t))
        n, thr = run_nucleus(gpu, fl, d, ROWS, cols, lens, ps, temps)
        check_band(refs, n, thr, (name, slices, "scratch"))
        return v.get().copy(), i.get().copy(), c.get().copy(), n, thr

    with W.forced(gpu, slices, 0):
        s0, t0 = select(), var_topk()
        p0 = top_p()
        s1 = select()
        p1 = top_p()
        p2 = top_p()
        t1 = var_topk()
        s2 = select()
    assert np.array_equal(s0, s1) and np.array_equal(s0, s2)
    assert all(np.array_equal(a, b) for a, b in zip(t0, t1))
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1)) and all(np.array_equal(a, b) for a, b in zip(p0, p2))
    assert np.array_equal(s0, V.expect_select(fl, words, None, None, cols // 3))


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("name", ("f32", "bf16"))
def test_graph_replay(gpu, name):
    """After reserve_topp_rows and reserve_wide_rows: one topp call captured at forced slices = 3;
    a replay, then d_ps and d_lens rewritten in place and a second replay; each matches an eager
    call with those arrays."""
    import torch
    cols, k = 20001, 48
    fl = V.Flavor(name)
    words = logits(fl, cols)
    batches = [([cols] * ROWS, [0.9] * ROWS),
               ([cols, 0, 1, 9000, cols - 1, 5, cols, 12000, 2, cols], [0.5, 0.9, 0.3, 2.0, 0.0, 0.99, NAN, 0.7, 0.9, 0.1])]
    b = W.Bench()
    g = None
    try:
        d = fl.device(words, None, True)
        dl, dp = V.dev_i32([0] * ROWS), dev_f32([0.0] * ROWS)
        dk = V.dev_i32([48, 3, 48, 48, 1, 48, 48, 20, 48, 48])
        o_v, o_i, o_c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        b.sel.reserve_topp_rows(ROWS, cols)
        b.sel.reserve_wide_rows(ROWS, cols)
        b.sel.wide_rows_force(3, 0)
        g = b.capture(lambda: topp(b.sel, fl, d, ROWS, cols, k, o_v.t, o_i.t, temp=0.8, lens=dl, ks=dk, ps=dp, cnt=o_c.t))
        for n, (lens, ps) in enumerate(batches):
            dl.copy_(V.dev_i32(lens)), dp.copy_(dev_f32(ps))
            for o in (o_v, o_i, o_c):
                o.buf.fill_(o.poison if hasattr(o, "poison") else W.POISON)
            b.replay(g)
            e_v, e_i, e_c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
            b.eager(lambda: topp(b.sel, fl, d, ROWS, cols, k, e_v.t, e_i.t, temp=0.8, lens=dl, ks=dk, ps=dp, cnt=e_c.t))
            assert np.array_equal(o_c.get(), e_c.get()), (n, o_c.get(), e_c.get())
            assert np.array_equal(o_i.get(), e_i.get()) and np.array_equal(o_v.get(), e_v.get()), n
            # and the eager call is the documented one: its counts are min(n_r, cap_r) for an n_r in the band
            refs = refs_of(fl, words, lens, ps, None, temp=0.8)
            caps = [V.clamp(q, 0, k) for q in dk.cpu().tolist()]
            for r, ref in enumerate(refs):
                c = int(e_c.get().view(np.int32)[r])
                assert c == caps[r] or ref.admits(c), (n, r, c, caps[r], ref.band())
    finally:
        del g
        b.close()
    torch.cuda.synchronize()
