"""GPU: one token per row drawn from the top-k / top-p filtered distribution
(include/kth.h "wide rows, sampling"; csrc/kth_rows_sample.hpp) for float32,
bfloat16 and float16 rows, in both forms, under forced plans and on both load
paths.

Reference: tests/test_gpu_topp.py's RowRef -- the documented order and its
float64 cumulative weights s.  A returned (tok, cnt) passes if
    cnt = min(n, cap) for an n that RowRef.admits (cap <= 0: no cap),
    j, the position of tok in RowRef.order, lies in [1, cnt], and
    S(j) >= A (1 - e) and (j == 1 or S(j - 1) <= A (1 + e)),
with A = u S(cnt), e = 2 * eps, eps = 2^-16 + cols * 2^-39 (the header's band);
u is the float32 the device reads, NaN or negative counting as 0 and a value
above 1 as 1.  The matrices, lengths, p and T lists, load paths, plans and the
poisoned outputs with guards are those of the top-p tests.
"""
import math

import numpy as np
import pytest

import test_gpu_rows_var as V
import test_gpu_rows_wide as W
import test_gpu_rows_wide16 as W16
import test_gpu_topp as T

pytestmark = pytest.mark.gpu

NAMES = T.NAMES
ROWS = V.ROWS
NAN = float("nan")
PLANS = T.PLANS
US = (0.0, 2.0 ** -24, 0.25, 0.5, 0.999999, 1.0, 2.0, -0.1, NAN)


def caps_of(cols):
    return (0, -1, 1, 2, 50, cols, cols + 5)


def u_of(u):
    """The number the device uses for the float32 it reads."""
    u = float(np.float32(u))
    return 0.0 if (math.isnan(u) or u < 0) else min(u, 1.0)


# ------------------------------------------------------------------ the reference
def cnt_ok(ref, cnt, cap):
    """cnt == min(n, cap) for an n inside the nucleus's band."""
    if cap <= 0 or cnt < cap:
        return ref.admits(cnt)
    if ref.p >= 1.0:
        return cnt == cap <= ref.len
    # the largest n the band admits: the largest with S(n - 1) < p Z (1 + eps), or 1
    top = max(1, min(ref.len, int(np.searchsorted(ref.s, ref.p * ref.z * (1 + ref.eps), side="left"))))
    return cnt == cap <= top


def j_ok(ref, cnt, u, j):
    e = 2.0 * ref.eps
    a = u_of(u) * ref.s[cnt]
    return 1 <= j <= cnt and ref.s[j] >= a * (1 - e) and (j == 1 or ref.s[j - 1] <= a * (1 + e))


def j_band(ref, cnt, u):
    return [j for j in range(1, cnt + 1) if j_ok(ref, cnt, u, j)]


def check(refs, caps, us, tok, cnt, tag):
    for r, ref in enumerate(refs):
        t, c, cap = int(tok[r]), int(cnt[r]), int(caps[r])
        if ref.len == 0:
            assert (t, c) == (-1, 0), (tag, "row", r, "empty", t, c)
            continue
        assert cnt_ok(ref, c, cap), (tag, "row", r, "cnt", c, "cap", cap, "len", ref.len, "p", ref.p)
        assert 0 <= t < ref.len, (tag, "row", r, "tok", t, "len", ref.len)
        j = int(np.nonzero(ref.order == t)[0][0]) + 1
        assert j_ok(ref, c, us[r], j), (tag, "row", r, "tok", t, "j", j, "cnt", c, "u", us[r], "S(j-1), S(j), A",
                                        ref.s[j - 1], ref.s[j], u_of(us[r]) * ref.s[c])


def sample(sel, fl, d, rows, cols, us, tok, k=0, p=1.0, temp=1.0, lens=None, ks=None, ps=None, temps=None, cnt=None,
           ld=None):
    if fl.w16:
        sel.sample_rows_wide16(d, rows, cols, us, tok, k=k, p=p, temp=temp, kind=fl.name, d_lens=lens, d_ks=ks, d_ps=ps,
                               d_temps=temps, d_cnt=cnt, ld=ld)
    else:
        sel.sample_rows_wide(d, rows, cols, us, tok, k=k, p=p, temp=temp, d_lens=lens, d_ks=ks, d_ps=ps, d_temps=temps,
                             d_cnt=cnt, ld=ld)


def run_sample(sel, fl, d, rows, cols, us, lens=None, ks=None, ps=None, temps=None, k=0, p=1.0, temp=1.0, ld=None):
    """(tok, cnt) of one call, from poisoned outputs with guards."""
    o_t, o_c = W.Out(rows), W.Out(rows)
    W.run(sel, lambda: sample(sel, fl, d, rows, cols, T.dev_f32(us), o_t.t, k, p, temp, V.dev_i32(lens), V.dev_i32(ks),
                              T.dev_f32(ps), T.dev_f32(temps), o_c.t, ld))
    return o_t.get().view(np.int32).copy(), o_c.get().view(np.int32).copy()


def rot(pool, step, off, rows=ROWS):
    return [pool[(step * r + off) % len(pool)] for r in range(rows)]


# ------------------------------------------------------------------ the band
@pytest.mark.parametrize("cols", (1, 3, 5, 1023, 4099, 8191, 8193, 33001))
@pytest.mark.parametrize("name", NAMES)
def test_band(gpu, name, cols):
    """Every row of every case returns a (tok, cnt) inside the band: both matrices of the top-p
    tests with their ragged lengths and device p and T lists, a cap list with 0, -1, 1, 2, 50, cols
    and cols + 5, a u list with 0, 2^-24, 1, 2, a negative and a NaN, under every plan and on both
    load paths; then the host scalars with every device array but d_us NULL."""
    plans = PLANS + (((0, 0),) if cols == 33001 else ())
    n = 0
    for which in (0, 1):
        fl, words, lens, ps, temps, refs = T.case(name, cols, which)
        for ld, shift in T.paths(fl, cols):
            d = fl.device(words, lens, True, ld=ld, shift=shift)
            for slices, group in plans:
                caps, us = rot(caps_of(cols), 1, n), rot(US, 4, n)  # another pairing of cap, u and row each time
                n += 1
                with W.forced(gpu, slices, group):
                    tok, cnt = run_sample(gpu, fl, d, ROWS, cols, us, lens, caps, ps, temps, ld=ld)
                check(refs, caps, us, tok, cnt, (name, cols, which, ld, shift, slices, group))
    fl = V.Flavor(name)
    words = T.logits(fl, cols)
    d = fl.device(words, None, True)
    for i, (p, temp, k) in enumerate(((0.9, 1.0, 0), (0.5, 0.7, 50), (-2.0, 1.0, -1), (1.0, 3.0, 0), (1.0, 1.0, 2))):
        refs = T.refs_of(fl, words, None, None, None, p, temp)
        us = rot(US, 1, i)
        tok, cnt = run_sample(gpu, fl, d, ROWS, cols, us, k=k, p=p, temp=temp)
        check(refs, [k] * ROWS, us, tok, cnt, (name, cols, "scalars", p, temp, k))


# ------------------------------------------------------------------ exact rows
EXACT_COLS = 1023


def exact_us(n, count=3):
    """Multiples of 2^-12 at which u * n lies mid-way between two integers: the band is one j wide."""
    out = [k / 4096.0 for k in range(1, 4096, 37) if 0.3 <= (k * n / 4096.0) % 1.0 <= 0.7]
    return out[::max(1, len(out) // count)][:count]


def exact_rows(fl):
    """(values, len, p, T, cap, u, the token the row is built to give or None) a row."""
    c = EXACT_COLS
    inf = np.float32(np.inf)
    eq = np.full(c, 1.5, dtype=np.float32)
    peak = np.full(c, -3.0, dtype=np.float32)
    peak[c // 3] = 17.0
    two = np.where(np.arange(c) % 10 == 3, 1.0, 0.0).astype(np.float32)
    infs = np.linspace(-4, 4, c).astype(np.float32)
    infs[[7, 600]] = inf
    nans = np.linspace(-4, 4, c).astype(np.float32)
    ninf = np.full(c, -inf, dtype=np.float32)
    zeros = np.where(np.arange(c) % 2 == 0, -0.0, 0.0).astype(np.float32)
    rows = [(eq, c, 1.0, 1.0, 0, 0.0, 0), (eq, 0, 1.0, 1.0, 0, 0.5, -1), (eq, 1, 0.5, 1.0, 0, 0.75, 0),
            (eq, 0, 0.5, 1.0, 3, 0.5, -1), (eq, 1, 1.0, 2.0, 5, 0.999, 0)]
    rows += [(eq, c, 1.0, 1.0, 0, u, math.floor(u * c)) for u in exact_us(c)]
    rows += [(eq, 701, 2.0, 2.0, -1, u, math.floor(u * 701)) for u in exact_us(701)]
    rows += [(eq, c, 1.0, 1.0, 100, u, math.floor(u * 100)) for u in exact_us(100)]
    rows += [(eq, c, 0.5, 1.0, 100, u, math.floor(u * 100)) for u in exact_us(100)]
    rows += [(ninf, c, 1.0, 1.0, 0, u, math.floor(u * c)) for u in exact_us(c, 2)]
    rows += [(peak, c, 0.0, 1.0, 0, 0.9, c // 3), (peak, c, -1.0, 0.5, 50, 0.3, c // 3), (peak, c, 0.9, 1.0, 1, 0.999, c // 3),
             (two, c, 0.0, 1.0, 0, 0.7, 3), (two, c, 1.0, 1.0, 1, 0.7, 3)]
    rows += [(infs, c, 1.0, 1.0, 0, 0.25, 7), (infs, c, 1.0, 1.0, 0, 0.4375, 7), (infs, c, 1.0, 1.0, 0, 0.75, 600),
             (infs, c, 0.9, 1.0, 0, 0.75, 600), (infs, c, 0.3, 1.0, 0, 0.75, 7), (infs, c, 1.0, 1.0, 1, 0.75, 7)]
    rows += [(nans, c, 1.0, 1.0, 0, 0.25, None), (nans, c, 1.0, 1.0, 0, 0.75, None), (nans, c, 0.5, 1.0, 0, 0.75, None)]
    rows += [(zeros, c, 1.0, 1.0, 0, u, 2 * math.floor(u * c) + 1) for u in exact_us(c, 2) if u < 0.49]
    x = np.stack([r[0] for r in rows])
    words = x.view(np.uint32).copy() if fl.name == "f32" else W16.to_kind_bits(x.ravel(), fl.name).reshape(x.shape)
    for r, row in enumerate(rows):
        if row[0] is nans:  # three NaNs of different payloads and signs
            if fl.name == "f32":
                words[r, [5, 300, 900]] = [0x7FC00000, 0xFFC12345, 0x7F800001]
            else:
                q = W16.INF[fl.name]
                words[r, [5, 300, 900]] = [q + 1, 0x8000 | (q + 3), W16.CANON[fl.name]]
    return words, rows


@pytest.mark.parametrize("name", NAMES)
def test_exact_rows(gpu, name):
    """Equal keys with and without a cap (tok = floor(u * len), floor(u * c)), greedy rows, +inf twice,
    NaNs, all -inf, -0.0 / +0.0, len 0 and 1: the bands of n and of j are one wide (asserted on
    the CPU first), so tok and cnt are compared for equality.  And u = 0.5 on the two +inf keys,
    exact by the integer arithmetic alone (Z = 2^40, t = 2^39 + 1): the second."""
    fl = V.Flavor(name)
    words, rows = exact_rows(fl)
    lens, ps, temps, caps, us = ([r[i] for r in rows] for i in (1, 2, 3, 4, 5))
    refs = T.refs_of(fl, words, lens, ps, temps)
    want_tok, want_cnt = [], []
    for r, ref in enumerate(refs):
        band = ref.band()
        assert len(band) == 1, ("the n band of exact row", r, "is", band)
        n = min(band[0], caps[r]) if caps[r] > 0 else band[0]
        js = j_band(ref, n, us[r]) if n else [0]
        assert len(js) == 1, ("the j band of exact row", r, "is", js)
        tok = int(ref.order[js[0] - 1]) if n else -1
        assert rows[r][6] is None or rows[r][6] == tok, ("exact row", r, "is built to give", rows[r][6], "not", tok)
        want_tok.append(tok), want_cnt.append(n)
    nrows, cols = words.shape
    half = [r for r, row in enumerate(rows) if row[6] == 600][:1]
    for ld, shift in T.paths(fl, cols):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        for slices, group in ((1, 0), (4, 0), (0, 5)):
            with W.forced(gpu, slices, group):
                tok, cnt = run_sample(gpu, fl, d, nrows, cols, us, lens, caps, ps, temps, ld=ld)
                u2 = list(us)
                u2[half[0]] = 0.5
                tok2, _ = run_sample(gpu, fl, d, nrows, cols, u2, lens, caps, ps, temps, ld=ld)
            assert tok.tolist() == want_tok, (name, slices, group, [(r, a, b) for r, (a, b) in
                                                                    enumerate(zip(tok.tolist(), want_tok)) if a != b])
            assert cnt.tolist() == want_cnt, (name, slices, group, cnt.tolist(), want_cnt)
            assert tok2[half[0]] == 600, (name, slices, group, tok2[half[0]])


# ------------------------------------------------------------------ the distribution
def strat_case(which):
    """(flavor name, one row's values, p, T, cap, R, plan)."""
    if which == 0:
        rng = np.random.default_rng(97)
        x = rng.choice(np.array([0.0, -0.25, -0.5, -0.75, -1.0, -1.5, -2.0], dtype=np.float32), 97)
        return "bf16", x, 0.9, 1.3, 40, 2048, (0, 0)
    rng = np.random.default_rng(8193)
    x = (rng.standard_normal(8193) * 0.3).astype(np.float32)
    x[rng.choice(8193, 24, replace=False)] += 6.0
    return "f32", x, 0.9, 0.8, 32, 512, (4, 0)


@pytest.mark.parametrize("which", (0, 1))
def test_stratified_u_gives_the_distribution(gpu, which):
    """R identical rows with u_r = (r + 0.5) / R and no randomness: the per-column counts of d_tok
    differ from the float64 reference's by at most 2 (one sample at each end of a key's interval),
    no column outside the kept set appears, the counts sum to R."""
    name, x, p, temp, cap, R, plan = strat_case(which)
    fl = V.Flavor(name)
    cols = x.size
    row = x.view(np.uint32).copy() if name == "f32" else W16.to_kind_bits(x, name)
    ref = T.RowRef(fl, row, p, temp, cols)
    band = ref.band()
    assert len(band) == 1 or min(band) >= cap, band  # (n is one number either way)
    n = min(band[0], cap)
    us = ((np.arange(R) + 0.5) / R).astype(np.float32)
    j = np.searchsorted(ref.s[1:n + 1], us.astype(np.float64) * ref.s[n], side="right") + 1  # least j with S(j) > u S(n)
    want = np.bincount(ref.order[j - 1], minlength=cols)
    assert (want >= 8).sum() >= 16, ("the row is too peaked for this test", int((want >= 8).sum()))
    words = np.tile(row, (R, 1))
    d = fl.device(words, None, True)
    with W.forced(gpu, *plan):
        tok, cnt = run_sample(gpu, fl, d, R, cols, us.tolist(), k=cap, p=p, temp=temp)
    assert (cnt == n).all(), (np.unique(cnt), n)
    assert tok.min() >= 0 and tok.max() < cols
    got = np.bincount(tok, minlength=cols)
    kept = np.zeros(cols, dtype=bool)
    kept[ref.order[:n]] = True
    assert not got[~kept].any(), np.nonzero(got[~kept])
    assert got.sum() == R
    assert np.abs(got - want).max() <= 2, (np.nonzero(np.abs(got - want) > 2)[0], got[np.abs(got - want) > 2])


# ------------------------------------------------------------------ d_cnt against the nucleus
@pytest.mark.parametrize("cols", (4099, 33001))
@pytest.mark.parametrize("name", NAMES)
def test_cnt_is_the_nucleus_under_the_cap(gpu, name, cols):
    """d_cnt equals min(d_n of nucleus_rows_wide*, cap) bit for bit, with caps given and with d_ks
    NULL and k = 0."""
    fl, words, lens, ps, temps, _ = T.case(name, cols, 1)
    us = rot(US, 2, 1)
    for (ld, shift), (slices, group) in zip(T.paths(fl, cols) + T.paths(fl, cols)[:1], ((1, 0), (4, 0), (0, 3))):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        with W.forced(gpu, slices, group):
            n, _ = T.run_nucleus(gpu, fl, d, ROWS, cols, lens, ps, temps, ld=ld)
            for caps in ([64, 0, 1, 7, cols, 100, -2, 33, cols + 5, 2], None):
                _, cnt = run_sample(gpu, fl, d, ROWS, cols, us, lens, caps, ps, temps, ld=ld)
                want = [int(a) if caps is None or caps[r] <= 0 else min(int(a), caps[r]) for r, a in enumerate(n)]
                assert cnt.tolist() == want, (name, cols, slices, group, caps, cnt.tolist(), want)


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", NAMES)
def test_deterministic_across_plans_paths_and_runs(gpu, name):
    """One 10 x 33001 matrix under every plan and both load paths, twice each: d_tok and d_cnt are
    bit-identical throughout."""
    cols = 33001
    fl, words, _, _, _, _ = T.case(name, cols, 1)
    lens = [cols, cols - 1, cols, 20000, cols, cols, 8193, cols, cols, cols]
    ps = [0.9, 0.5, 0.99, 0.3, 0.999, 1.0, 0.7, 0.95, 0.9, 0.6]
    temps = [1.0, 0.7, 2.0, 1.0, 1.3, 0.5, 1.0, 1.0, 3.0, 1.0]
    caps = [0, 50, 1000, 0, 3, 0, 20000, -1, 1, 64]
    us = [0.1, 0.5, 0.9, 0.33, 0.999999, 0.77, 0.25, 0.6, 0.05, 0.45]
    first = None
    for ld, shift in T.paths(fl, cols):
        d = fl.device(words, lens, True, ld=ld, shift=shift)
        for slices, group in PLANS + ((0, 0),):
            for again in range(2):
                with W.forced(gpu, slices, group):
                    got = run_sample(gpu, fl, d, ROWS, cols, us, lens, caps, ps, temps, ld=ld)
                if first is None:
                    first = got
                    check(T.refs_of(fl, words, lens, ps, temps), caps, us, got[0], got[1], (name, "determinism"))
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), \
                    (name, ld, shift, slices, group, again, got, first)


# ------------------------------------------------------------------ scratch left as found
@pytest.mark.parametrize("slices", (1, 5))
@pytest.mark.parametrize("name", NAMES)
def test_scratch_left_as_found(gpu, name, slices):
    """A sample call (and two in a row) between uniform wide selects, var top-k calls and top-p
    calls on one ctx changes none of their outputs, nor its own."""
    cols, k = 8193, 32
    fl, words, lens, ps, temps, refs = T.case(name, cols, 1)
    d = fl.device(words, lens, True)
    dfull = fl.device(words, None, True)
    dl, dp, dt = V.dev_i32(lens), T.dev_f32(ps), T.dev_f32(temps)
    caps, us = rot(caps_of(cols), 3, 0), rot(US, 2, 0)

    def select():
        o = fl.out_vals(ROWS)
        W.run(gpu, lambda: fl.uniform_select(gpu, dfull, ROWS, cols, cols // 3, o.t))
        return (o.get().copy(),)

    def var_topk():
        v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        W.run(gpu, lambda: fl.topk(gpu, d, ROWS, cols, k, v.t, i.t, True, dl, None, c.t))
        return v.get().copy(), i.get().copy(), c.get().copy()

    def top_p():
        v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        W.run(gpu, lambda: T.topp(gpu, fl, d, ROWS, cols, k, v.t, i.t, lens=dl, ps=dp, temps=dt, cnt=c.t))
        return (v.get().copy(), i.get().copy(), c.get().copy()) + T.run_nucleus(gpu, fl, d, ROWS, cols, lens, ps, temps)

    def draw():
        got = run_sample(gpu, fl, d, ROWS, cols, us, lens, caps, ps, temps)
        check(refs, caps, us, got[0], got[1], (name, slices, "scratch"))
        return got

    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    with W.forced(gpu, slices, 0):
        s0, t0, p0 = select(), var_topk(), top_p()
        d0 = draw()
        s1, p1 = select(), top_p()
        d1 = draw()
        d2 = draw()
        t1, p2, s2 = var_topk(), top_p(), select()
        d3 = draw()
    assert same(s0, s1) and same(s0, s2) and same(t0, t1) and same(p0, p1) and same(p0, p2)
    assert same(d0, d1) and same(d0, d2) and same(d0, d3)
    assert np.array_equal(s0[0], V.expect_select(fl, words, None, None, cols // 3))


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("name", ("f32", "bf16"))
def test_graph_replay(gpu, name):
    """After reserve_sample_rows: one call captured at forced slices = 3; a replay, then d_us, d_ps,
    d_ks and d_lens rewritten in place and a second replay; each equals an eager call with those
    arrays and passes the band."""
    import torch
    cols = 20001
    fl = V.Flavor(name)
    words = T.logits(fl, cols)
    batches = [([cols] * ROWS, [0.9] * ROWS, [0] * ROWS, [0.5] * ROWS),
               ([cols, 0, 1, 9000, cols - 1, 5, cols, 12000, 2, cols], [0.5, 0.9, 0.3, 2.0, 0.0, 0.99, NAN, 0.7, 0.9, 0.1],
                [48, 3, 0, -1, 1, 48, 20000, 20, 0, 2], [0.1, 0.7, 0.3, 0.999999, 0.5, 0.0, 0.42, 1.0, 0.9, 0.77])]
    b = W.Bench()
    g = None
    try:
        d = fl.device(words, None, True)
        dl, dp, dk, du = V.dev_i32([0] * ROWS), T.dev_f32([0.0] * ROWS), V.dev_i32([0] * ROWS), T.dev_f32([0.0] * ROWS)
        o_t, o_c = W.Out(ROWS), W.Out(ROWS)
        b.sel.reserve_sample_rows(ROWS, cols)
        b.sel.wide_rows_force(3, 0)
        g = b.capture(lambda: sample(b.sel, fl, d, ROWS, cols, du, o_t.t, temp=0.8, lens=dl, ks=dk, ps=dp, cnt=o_c.t))
        for n, (lens, ps, caps, us) in enumerate(batches):
            dl.copy_(V.dev_i32(lens)), dp.copy_(T.dev_f32(ps)), dk.copy_(V.dev_i32(caps)), du.copy_(T.dev_f32(us))
            for o in (o_t, o_c):
                o.buf.fill_(W.POISON)
            b.replay(g)
            e_t, e_c = W.Out(ROWS), W.Out(ROWS)
            b.eager(lambda: sample(b.sel, fl, d, ROWS, cols, du, e_t.t, temp=0.8, lens=dl, ks=dk, ps=dp, cnt=e_c.t))
            assert np.array_equal(o_t.get(), e_t.get()) and np.array_equal(o_c.get(), e_c.get()), \
                (n, o_t.get(), e_t.get(), o_c.get(), e_c.get())
            check(T.refs_of(fl, words, lens, ps, None, temp=0.8), caps, us, o_t.get().view(np.int32),
                  o_c.get().view(np.int32), (name, "replay", n))
    finally:
        del g
        b.close()
    torch.cuda.synchronize()
