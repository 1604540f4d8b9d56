"""GPU: the wide-rows calls at digit, tie-quota and mass edges.

The inputs, their probes and the reasoning are in tests/wide_edges.py;
tests/test_wide_edges_inputs.py proves on the CPU that every probe is the boundary it
is named for and that every top-p / sampling probe admits exactly one answer (margin
>= 4 eps), so every comparison here is for equality, bit for bit:

  staircase  every rank at which the answer moves from the last key of a digit bin to
             the first key of the next (k_wide_pick's bin pick and its early end,
             k16_ord2 at ords 0x0000 / 0x7FFF / 0x8000 / 0xFFFF);
  fence      every k at which the tie quota runs out on, before and after a slice or
             tile boundary (k_wide_tk_write's taken / quota / want == 0, the store
             guard of wd_write_range / w16_write_range);
  mass       every p and u that put the target half a key's weight before S(j), for j
             the first and last key of each tie group (tp_pick_digit, tp_ties,
             sm_pick_digit, sm_locate).

Expected values are numpy's: V.expect_select / V.expect_topk (a stable argsort of the
documented order key) and test_gpu_topp.RowRef (float64 cumulative weights).  Outputs
are poisoned and guarded (W.Out, W16.Out); the device matrix holds winners past each
row's end and before a shifted base; both load paths (T.paths) and the forced plans
fused, 3 slices, 7 slices and 7 slices in groups of 5 rows.  What each case aims at is
tabulated in DESIGN.md "Wide-row edges".
"""
import numpy as np
import pytest

import test_gpu_rows_var as V
import test_gpu_rows_wide as W
import test_gpu_sample as S
import test_gpu_topp as T
import wide_edges as E

pytestmark = pytest.mark.gpu

PLAN_IDS = ["fused", "s3", "s7", "s7g5"]


# ------------------------------------------------------------------ inputs, expected once
def var_case(name, largest):
    """(words, ks): the staircase's probes, its all-equal row and the three fences' probes, one row each."""
    def make():
        parts = [E.staircase(name).case(largest)] + [f.case(largest) for f in E.fences(name)]
        return np.vstack([w for w, _ in parts]), [k for _, ks in parts for k in ks]
    return E.expected(("var", name, largest), make)


def want_var_topk(name, largest):
    words, ks = var_case(name, largest)
    return E.expected(("var topk", name, largest), lambda: V.expect_topk(V.Flavor(name), words, None, ks, max(ks), largest))


def want_var_select(name):
    words, ks = var_case(name, False)
    return E.expected(("var select", name), lambda: V.expect_select(V.Flavor(name), words, None, ks, max(ks)))


def uniform_inputs(name, largest):
    """[(label, 2 x cols words, probe ranks)]: the staircase and the three fences."""
    st = E.staircase(name)
    out = [("staircase", st.pair_words(), [k for k, _, _ in st.probes(largest)])]
    return out + [(f"fence{f.slices}", f.pair_words(largest), list(f.ks)) for f in E.fences(name)]


def same_rows(got, want, tag):
    bad = np.nonzero((got != want).any(axis=1))[0] if got.ndim == 2 else np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, "rows", bad[:6], "got", got[bad[0]].ravel()[:8], "want", want[bad[0]].ravel()[:8])


def check_var_topk(sel, fl, words, ks, d, largest, ld, want, tag):
    rows, cols = words.shape
    k = max(ks)
    v, i, c = fl.out_vals(rows * k), fl.out_idx(rows * k), W.Out(rows)
    dk = V.dev_i32(ks)
    W.run(sel, lambda: fl.topk(sel, d, rows, cols, k, v.t, i.t, largest, None, dk, c.t, ld))
    want_v, want_i, want_c = want
    same_rows(c.get().view(np.int32), want_c, (tag, "cnt"))
    same_rows(i.get().view(np.int32).reshape(rows, k), want_i, (tag, "idx", ks))
    same_rows(v.get().reshape(rows, k), want_v, (tag, "vals", ks))
    return v.get().copy(), i.get().copy(), c.get().copy()


def check_var_select(sel, fl, words, ks, d, ld, want, tag):
    rows, cols = words.shape
    o = fl.out_vals(rows)
    dk = V.dev_i32(ks)
    W.run(sel, lambda: fl.select(sel, d, rows, cols, max(ks), o.t, None, dk, ld))
    same_rows(o.get(), want, (tag, "select", ks))
    return (o.get().copy(),)


# ------------------------------------------------------------------ (a), (b): the var calls
@pytest.mark.parametrize("plan", E.PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", E.FLAVORS)
def test_var_calls_at_every_edge(gpu, name, plan):
    """One var select and one var top-k (smallest, largest) per load path: a row per probe, d_ks
    the probes, k the largest probe.  Values, columns, padding and d_cnt."""
    fl = V.Flavor(name)
    for largest in (False, True):
        words, ks = var_case(name, largest)
        for ld, shift in T.paths(fl, words.shape[1]):
            d = fl.device(words, None, largest, ld=ld, shift=shift)
            tag = (name, plan, "largest" if largest else "smallest", "ld", ld, "shift", shift)
            with W.forced(gpu, *plan):
                check_var_topk(gpu, fl, words, ks, d, largest, ld, want_var_topk(name, largest), tag)
                if not largest:
                    check_var_select(gpu, fl, words, ks, d, ld, want_var_select(name), tag)


# ------------------------------------------------------------------ (a), (b): the uniform calls
@pytest.mark.parametrize("plan", ((1, 0), (7, 0)), ids=["fused", "s7"])
@pytest.mark.parametrize("name", E.FLAVORS)
def test_uniform_select_at_every_edge(gpu, name, plan):
    """rows_wide / rows_wide16 (the kernels compiled without the var arrays), rows = 2, once per
    probe rank of the staircase and of every fence; the load path alternates with the probe."""
    fl = V.Flavor(name)
    with W.forced(gpu, *plan):
        for label, words, ks in uniform_inputs(name, False):
            cols = words.shape[1]
            ds = [(fl.device(words, None, False, ld=ld, shift=shift), ld) for ld, shift in T.paths(fl, cols)]
            for n, k in enumerate(ks):
                d, ld = ds[n % 2]
                want = E.expected(("uni select", name, label, k), lambda: V.expect_select(fl, words, None, None, k))
                o = fl.out_vals(2)
                W.run(gpu, lambda: fl.uniform_select(gpu, d, 2, cols, k, o.t, ld))
                same_rows(o.get(), want, (name, plan, label, "k", k, "ld", ld))


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("plan", ((1, 0), (7, 0)), ids=["fused", "s7"])
@pytest.mark.parametrize("name", E.FLAVORS)
def test_uniform_topk_at_every_edge(gpu, name, plan, largest):
    """topk_rows_wide / topk_rows_wide16, rows = 2, once per probe of every fence and per fourth
    probe of the staircase."""
    fl = V.Flavor(name)
    with W.forced(gpu, *plan):
        for label, words, ks in uniform_inputs(name, largest):
            cols = words.shape[1]
            ds = [(fl.device(words, None, largest, ld=ld, shift=shift), ld) for ld, shift in T.paths(fl, cols)]
            for n, k in enumerate(ks[::4] if label == "staircase" else ks):
                d, ld = ds[n % 2]
                want_v, want_i, _ = E.expected(("uni topk", name, label, largest, k),
                                               lambda: V.expect_topk(fl, words, None, None, k, largest))
                v, i = fl.out_vals(2 * k), fl.out_idx(2 * k)
                W.run(gpu, lambda: fl.uniform_topk(gpu, d, 2, cols, k, v.t, i.t, largest, ld))
                tag = (name, plan, label, "k", k, "ld", ld)
                same_rows(i.get().view(np.int32).reshape(2, k), want_i, (tag, "idx"))
                same_rows(v.get().reshape(2, k), want_v, (tag, "vals"))


# ------------------------------------------------------------------ (c): the weighted descent
def nucleus_call(sel, m, d, ld):
    rows = len(m.nuc)
    n, thr = T.run_nucleus(sel, m.fl, d, rows, m.cols, None, [p for _, p in m.nuc], None, temp=m.temp, ld=ld)
    return n, thr


def check_nucleus(m, got, tag):
    n, thr = got
    want_n = np.array([j for j, _ in m.nuc], dtype=np.int32)
    want_t = np.array([int(m.ref.thr(j)) for j, _ in m.nuc], dtype=m.fl.np_t)
    same_rows(n, want_n, (tag, "d_n", [round(p, 6) for _, p in m.nuc][:4]))
    same_rows(thr, want_t, (tag, "d_thr"))


def sample_call(sel, m, d, ld):
    rows = len(m.draws)
    return S.run_sample(sel, m.fl, d, rows, m.cols, [u for *_, u in m.draws], None, [cap for _, cap, *_ in m.draws],
                        [p for p, *_ in m.draws], None, temp=m.temp, ld=ld)


def check_sample(m, got, tag):
    tok, cnt = got
    want_tok = np.array([m.ref.order[j - 1] for _, _, _, j, _ in m.draws], dtype=np.int32)
    want_cnt = np.array([c for _, _, c, _, _ in m.draws], dtype=np.int32)
    same_rows(cnt, want_cnt, (tag, "d_cnt"))
    bad = np.nonzero(tok != want_tok)[0]
    assert bad.size == 0, (tag, "d_tok rows", bad[:6], "got", tok[bad[:6]], "want", want_tok[bad[:6]],
                           "(p, cap, cnt, j, u)", [m.draws[b] for b in bad[:3]])


@pytest.mark.parametrize("temp", (1.0, 0.5))
@pytest.mark.parametrize("name", E.FLOATS)
def test_nucleus_at_every_mass_edge(gpu, name, temp):
    """d_n == j and d_thr == the bits of the j-th key, for p Z half a key's weight before S(j), j
    the first and last rank of every tie group; every plan, both load paths."""
    m = E.mass(name, temp)
    words = m.words(len(m.nuc))
    for ld, shift in T.paths(m.fl, m.cols):
        d = m.fl.device(words, None, True, ld=ld, shift=shift)
        for plan in E.PLANS:
            with W.forced(gpu, *plan):
                check_nucleus(m, nucleus_call(gpu, m, d, ld), (name, temp, plan, "ld", ld))


@pytest.mark.parametrize("temp", (1.0, 0.5))
@pytest.mark.parametrize("name", E.FLOATS)
def test_topp_at_every_mass_edge(gpu, name, temp):
    """topp_rows_wide* under the caps j - 1, j, j + 1 equals numpy's var top-k at rank min(j, cap):
    values, columns, padding and d_cnt."""
    m = E.mass(name, temp)
    fl = m.fl
    rows = len(m.capped)
    words = m.words(rows)
    caps = [cap for _, _, cap in m.capped]
    ranks = [min(j, cap) for j, _, cap in m.capped]
    k = max(caps)
    want_v, want_i, want_c = E.expected(("topp", name, temp), lambda: V.expect_topk(fl, words, None, ranks, k, True))
    assert want_c.tolist() == ranks
    for ld, shift in T.paths(fl, m.cols):
        d = fl.device(words, None, True, ld=ld, shift=shift)
        for plan in E.PLANS:
            v, i, c = fl.out_vals(rows * k), fl.out_idx(rows * k), W.Out(rows)
            with W.forced(gpu, *plan):
                W.run(gpu, lambda: T.topp(gpu, fl, d, rows, m.cols, k, v.t, i.t, temp=temp, ks=V.dev_i32(caps),
                                          ps=T.dev_f32([p for _, p, _ in m.capped]), cnt=c.t, ld=ld))
            tag = (name, temp, plan, "ld", ld)
            same_rows(c.get().view(np.int32), want_c, (tag, "d_cnt", caps))
            same_rows(i.get().view(np.int32).reshape(rows, k), want_i, (tag, "idx"))
            same_rows(v.get().reshape(rows, k), want_v, (tag, "vals"))


@pytest.mark.parametrize("temp", (1.0, 0.5))
@pytest.mark.parametrize("name", E.FLOATS)
def test_sample_at_every_mass_edge(gpu, name, temp):
    """d_tok == the column of the j-th key and d_cnt == min(n, cap), for u S(cnt) half a key's
    weight before S(j): p = 1 without a cap and with a binding one, two p < 1, and the caps
    n - 1, n, n + 1 around a nucleus of n keys."""
    m = E.mass(name, temp)
    words = m.words(len(m.draws))
    for ld, shift in T.paths(m.fl, m.cols):
        d = m.fl.device(words, None, True, ld=ld, shift=shift)
        for plan in E.PLANS:
            with W.forced(gpu, *plan):
                check_sample(m, sample_call(gpu, m, d, ld), (name, temp, plan, "ld", ld))


# ------------------------------------------------------------------ scratch left as found
def test_alternating_calls_on_one_ctx(gpu):
    """A staircase select, a fence top-k, a mass nucleus and a sample call alternate on one ctx
    of its own under the 7-slice plan, in two orders; every result is the reference's, and the first call
    repeated at the end gives identical bits."""
    import torch
    import kselect
    fa, fb = V.Flavor("f32"), V.Flavor("bf16")
    wa, ka = var_case("f32", False)
    wb, kb = var_case("bf16", True)
    mc, md = E.mass("f32", 1.0), E.mass("bf16", 0.5)
    da = fa.device(wa, None, False)
    db = fb.device(wb, None, True)
    dc = mc.fl.device(mc.words(len(mc.nuc)), None, True)
    dd = md.fl.device(md.words(len(md.draws)), None, True)

    def nucleus(sel):
        got = nucleus_call(sel, mc, dc, None)
        check_nucleus(mc, got, "alternating")
        return got

    def sample(sel):
        got = sample_call(sel, md, dd, None)
        check_sample(md, got, "alternating")
        return got

    with kselect.Selector(0) as sel:
        sel.wide_rows_force(7, 0)
        calls = [lambda: check_var_select(sel, fa, wa, ka, da, None, want_var_select("f32"), "alternating"),
                 lambda: check_var_topk(sel, fb, wb, kb, db, True, None, want_var_topk("bf16", True), "alternating"),
                 lambda: nucleus(sel), lambda: sample(sel)]
        for order in ((0, 1, 2, 3, 0), (3, 1, 0, 2, 1, 3)):
            first = None
            for n, c in enumerate(order):
                got = calls[c]()
                if n == 0:
                    first = got
            assert order[-1] == order[0] and all(np.array_equal(a, b) for a, b in zip(first, got)), order
    torch.cuda.synchronize()
