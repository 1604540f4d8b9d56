"""GPU: the ragged wide-rows calls (include/kth.h "wide rows, ragged";
csrc/kth_rows_wide_kernels.hpp, csrc/kth_rows_wide16_kernels.hpp): a length
and a rank per row, read from device memory, for int32, float32, int16,
uint16, float16 and bfloat16 keys, in both forms and on both load paths.

Expected values come from numpy on the host, with the matrices, the order-key
rules, the poisoned outputs and the helpers of tests/test_gpu_rows_wide.py and
tests/test_gpu_rows_wide16.py: per row, the stable argsort of the documented
order key over the row's first len_r columns; the first k_r of it sorted by
column, a NaN written canonical; entries [k_r, k) are padding (index -1, the
zero word) and d_cnt[r] = k_r.  len_r and k_r follow the header's clamps.
Bits are compared, not floats.  Every output is poisoned and carries two guard
elements past each end.  The columns at and past len_r of the device matrix,
its row padding and the elements before a shifted base hold a key that would
win (the minimum for smallest, the maximum for largest, NaNs for float
largest), so a read past len_r changes the answer.
"""
import numpy as np
import pytest

import test_gpu_rows_wide as W
import test_gpu_rows_wide16 as W16

pytestmark = pytest.mark.gpu

FLAVORS = ("i32", "f32") + W16.KINDS
ROWS = 10
# (minimum, maximum) bit patterns in the documented order; for the float kinds the maximum is a NaN
WINNERS = {"i32": (0x80000000, 0x7FFFFFFF), "f32": (0xFF800000, 0xFFC00001), "i16": (0x8000, 0x7FFF),
           "u16": (0x0000, 0xFFFF), "f16": (0xFC00, 0xFE01), "bf16": (0xFF80, 0x7FC1)}


class Flavor:
    """One key kind: its words, order keys, outputs and calls."""

    def __init__(self, name):
        self.name, self.w16, self.f32 = name, name in W16.KINDS, name == "f32"
        self.np_t = np.uint16 if self.w16 else np.uint32
        self.align = 8 if self.w16 else 4

    def words(self, cols):
        """ROWS rows of mixed kinds (tie, equal, specials / NaN rows among them)."""
        if not self.w16:
            return W.matrix(self.f32, ROWS, cols, tie=True).words
        return np.vstack([W16.matrix(self.name, cols, 0).words, W16.matrix(self.name, cols, 1).words[:ROWS - 8]])

    def keys(self, words):
        return W16.rule_key(words, self.name) if self.w16 else W.order_keys(words, self.f32)

    def canon(self, words):
        if self.name == "f32":
            return np.where((words & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(W.QNAN), words)
        if self.name in W16.CANON:
            return np.where(self.keys(words) == np.uint16(0xFFFF), np.uint16(W16.CANON[self.name]), words)
        return words

    def slice_keys(self, cols, slices):
        """The columns of a slice under a forced plan: the plan's arithmetic, its rounding taken from the library."""
        import kselect
        plan = kselect.wide_rows_plan16 if self.w16 else kselect.wide_rows_plan
        auto_slices, auto_sk, _, _ = plan(1, 1 << 20, 256)  # a split-form plan: slice_keys is rounded up to the alignment
        assert auto_slices > 1 and auto_sk % self.align == 0 and auto_sk == -(-(-(-(1 << 20) // auto_slices)) // self.align) * self.align
        return -(-(-(-cols // max(slices, 1))) // self.align) * self.align

    def device(self, words, lens, largest, ld=None, shift=0):
        """The matrix on the device; everything that is not one of a row's first len_r columns would win."""
        import torch
        rows, cols = words.shape
        ld = cols if ld is None else ld
        win = self.np_t(WINNERS[self.name][1 if largest else 0])
        host = np.full(shift + rows * ld + 8, win, dtype=self.np_t)
        view = host[shift:shift + rows * ld].reshape(rows, ld)
        for r in range(rows):
            n = cols if lens is None else min(max(int(lens[r]), 0), cols)
            view[r, :n] = words[r, :n]
        if self.w16:
            return torch.from_numpy(host.view(np.int16)).cuda()[shift:]
        t = torch.from_numpy(host.view(np.int32)).cuda()[shift:]
        return t.view(torch.float32) if self.f32 else t

    def out_vals(self, n):
        return W16.Out(n) if self.w16 else W.Out(n, self.f32)

    def out_idx(self, n):
        return W16.Out(n, idx=True) if self.w16 else W.Out(n)

    def select(self, sel, d, rows, cols, k, out, lens=None, ks=None, ld=None):
        if self.w16:
            sel.rows_wide16_var(d, rows, cols, k, out, kind=self.name, d_lens=lens, d_ks=ks, ld=ld)
        else:
            sel.rows_wide_var(d, rows, cols, k, out, f32=self.f32, d_lens=lens, d_ks=ks, ld=ld)

    def topk(self, sel, d, rows, cols, k, vals, idx, largest, lens=None, ks=None, cnt=None, ld=None):
        if self.w16:
            sel.topk_rows_wide16_var(d, rows, cols, k, vals, idx, largest=largest, kind=self.name, d_lens=lens,
                                     d_ks=ks, d_cnt=cnt, ld=ld)
        else:
            sel.topk_rows_wide_var(d, rows, cols, k, vals, idx, largest=largest, f32=self.f32, d_lens=lens, d_ks=ks,
                                   d_cnt=cnt, ld=ld)

    def uniform_select(self, sel, d, rows, cols, k, out, ld=None):
        if self.w16:
            sel.rows_wide16(d, rows, cols, k, out, kind=self.name, ld=ld)
        else:
            sel.rows_wide(d, rows, cols, k, out, f32=self.f32, ld=ld)

    def uniform_topk(self, sel, d, rows, cols, k, vals, idx, largest, ld=None):
        if self.w16:
            sel.topk_rows_wide16(d, rows, cols, k, vals, idx, largest=largest, kind=self.name, ld=ld)
        else:
            sel.topk_rows_wide(d, rows, cols, k, vals, idx, largest=largest, f32=self.f32, ld=ld)


# ------------------------------------------------------------------ the reference
def clamp(x, lo, hi):
    return max(lo, min(int(x), hi))


def row_lens(lens, rows, cols):
    return [cols if lens is None else clamp(lens[r], 0, cols) for r in range(rows)]


def expect_topk(fl, words, lens, ks, k, largest):
    """(vals rows x k, idx rows x k, cnt rows) by the header's rule."""
    rows, cols = words.shape
    vals = np.zeros((rows, k), dtype=fl.np_t)
    idx = np.full((rows, k), -1, dtype=np.int32)
    cnt = np.zeros(rows, dtype=np.int32)
    for r, n in enumerate(row_lens(lens, rows, cols)):
        kr = min(k if ks is None else clamp(ks[r], 0, k), n)
        key = fl.keys(words[r, :n])
        keep = np.sort(np.argsort(~key if largest else key, kind="stable")[:kr])
        vals[r, :kr], idx[r, :kr], cnt[r] = fl.canon(words[r, keep]), keep, kr
    return vals, idx, cnt


def expect_select(fl, words, lens, ks, k):
    rows, cols = words.shape
    out = np.zeros(rows, dtype=fl.np_t)
    for r, n in enumerate(row_lens(lens, rows, cols)):
        if n:
            kr = clamp(k if ks is None else ks[r], 1, n)
            out[r] = fl.canon(words[r, np.argsort(fl.keys(words[r, :n]), kind="stable")[kr - 1]][None])[0]
    return out


def dev_i32(a):
    import torch
    return None if a is None else torch.tensor([int(x) for x in a], dtype=torch.int32, device="cuda")


def check_topk(sel, fl, words, d, k, largest, lens, ks, mode="both", with_cnt=True, ld=None, what=""):
    rows, cols = words.shape
    want_v, want_i, want_c = expect_topk(fl, words, lens, ks, k, largest)
    v = fl.out_vals(rows * k) if mode != "idx" else None
    i = fl.out_idx(rows * k) if mode != "vals" else None
    c = W.Out(rows) if with_cnt else None
    dl, dk = dev_i32(lens), dev_i32(ks)
    W.run(sel, lambda: fl.topk(sel, d, rows, cols, k, v.t if v else None, i.t if i else None, largest, dl, dk,
                               c.t if c else None, ld))
    tag = (what, fl.name, cols, k, largest, mode, with_cnt)
    if c:
        got = c.get().view(np.int32)
        assert np.array_equal(got, want_c), (tag, "cnt", got, want_c)
    if i:
        got = i.get().view(np.int32).reshape(rows, k)
        bad = np.nonzero((got != want_i).any(axis=1))[0]
        assert bad.size == 0, (tag, "idx rows", bad[:4], want_c[bad[0]], got[bad[0]][:8], want_i[bad[0]][:8])
    if v:
        got = v.get().reshape(rows, k)
        bad = np.nonzero((got != want_v).any(axis=1))[0]
        assert bad.size == 0, (tag, "vals rows", bad[:4], want_c[bad[0]], got[bad[0]][:8], want_v[bad[0]][:8])


def check_select(sel, fl, words, d, k, lens, ks, ld=None, what=""):
    rows, cols = words.shape
    o = fl.out_vals(rows)
    dl, dk = dev_i32(lens), dev_i32(ks)
    W.run(sel, lambda: fl.select(sel, d, rows, cols, k, o.t, dl, dk, ld))
    got, want = o.get(), expect_select(fl, words, lens, ks, k)
    assert np.array_equal(got, want), (what, fl.name, cols, k, np.nonzero(got != want)[0][:4], got, want)


# ------------------------------------------------------------------ lengths and ranks
def len_pool(fl, cols, slices):
    """The lengths to cover: short ones around the load widths, the slice boundaries of the
    (forced, else 3-slice) plan, the row's end, and values the kernels must clamp."""
    sk = fl.slice_keys(cols, slices if slices > 1 else 3)
    return [0, 1, 3, 4, 5, 7, 8, 9, sk - 1, sk, sk + 1, 2 * sk, cols - 1, cols, cols + 5, -3]


def lens_at(pool, rot, rows=ROWS):
    """Row r takes pool[(7 r + rot) % 16]: consecutive rows alternate short and boundary lengths,
    and `rot` moves every row kind through the pool."""
    return [pool[(7 * r + rot) % len(pool)] for r in range(rows)]


def topk_ks_at(lens, cols, k, rot):
    """Row r's rank from 0, 1, len - 1, len, len + 1, k, k + 9, -1: ranks above the length and
    rank 0 on rows that have keys among them."""
    out = []
    for r, ln in enumerate(lens):
        n = clamp(ln, 0, cols)
        out.append([0, 1, n - 1, n, n + 1, k, k + 9, -1][(3 * r + rot) % 8])
    return out


def select_ks_at(lens, cols, rot):
    out = []
    for r, ln in enumerate(lens):
        n = clamp(ln, 0, cols)
        out.append([-2, 0, 1, n // 2, n, n + 1][(r + rot) % 6])
    return out


def test_pools_cover_what_they_claim():
    """The reference's view of the inputs, so that the parity tests mean it (no device work)."""
    fl = Flavor("f32")
    assert fl.slice_keys(20001, 3) == 6668 and Flavor("bf16").slice_keys(20001, 3) == 6672
    pool = len_pool(fl, 20001, 3)
    seen_l, seen_k, zero_rank_on_keys, rank_above_len = set(), set(), False, False
    for rot in range(16):
        lens = lens_at(pool, rot)
        seen_l.update(lens)
        ks = topk_ks_at(lens, 20001, 64, rot)
        for ln, q in zip(lens, ks):
            n = clamp(ln, 0, 20001)
            zero_rank_on_keys |= n > 0 and clamp(q, 0, 64) == 0
            rank_above_len |= 0 < n < clamp(q, 0, 64)
        seen_k.update((3 * r + rot) % 8 for r in range(ROWS))
    assert seen_l == set(pool) and seen_k == set(range(8)) and zero_rank_on_keys and rank_above_len


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("slices", [0, 1, 3, 7])
@pytest.mark.parametrize("cols", [4099, 20001])
@pytest.mark.parametrize("name", FLAVORS)
def test_select_parity(gpu, name, cols, slices):
    fl = Flavor(name)
    words = fl.words(cols)
    pool = len_pool(fl, cols, slices)
    with W.forced(gpu, slices):
        for n, rot in enumerate((slices, slices + 5, slices + 11)):
            lens = lens_at(pool, rot)
            ks = select_ks_at(lens, cols, rot)
            d = fl.device(words, lens, False)
            check_select(gpu, fl, words, d, cols // 2, lens, ks, what=f"both rot={rot}")
            if n == 0:
                check_select(gpu, fl, words, d, cols // 3, lens, None, what="lens only")  # the host k, clamped to len_r
            if n == 1:
                full = fl.device(words, None, False)
                check_select(gpu, fl, words, full, 1, None, select_ks_at([cols] * ROWS, cols, rot), what="ks only")


@pytest.mark.parametrize("slices", [0, 1, 3, 7])
@pytest.mark.parametrize("cols", [4099, 20001])
@pytest.mark.parametrize("name", FLAVORS)
def test_topk_parity(gpu, name, cols, slices):
    """Smallest and largest; both outputs, values only, columns only; d_cnt present and absent;
    d_lens only, d_ks only and both.  Padding is index -1 and the zero word, d_cnt the expected k_r."""
    fl = Flavor(name)
    words = fl.words(cols)
    pool = len_pool(fl, cols, slices)
    k = 64
    with W.forced(gpu, slices):
        for largest in (False, True):
            rot = 2 * slices + (9 if largest else 0) + (4 if cols == 4099 else 0)
            lens = lens_at(pool, rot)
            ks = topk_ks_at(lens, cols, k, rot)
            d = fl.device(words, lens, largest)
            check_topk(gpu, fl, words, d, k, largest, lens, ks, "both", True, what="both arrays")
            check_topk(gpu, fl, words, d, k, largest, lens, ks, "vals", False, what="both arrays")
            check_topk(gpu, fl, words, d, k, largest, lens, ks, "idx", True, what="both arrays")
            check_topk(gpu, fl, words, d, k, largest, lens, None, "both", largest, what="lens only")
            full = fl.device(words, None, largest)
            check_topk(gpu, fl, words, full, k, largest, None, topk_ks_at([cols] * ROWS, cols, k, rot), "both",
                       not largest, what="ks only")


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("name", FLAVORS)
def test_topk_parity_large_k(gpu, name, slices):
    """k = cols / 2: padding longer than a workgroup's stride, ranks past a slice."""
    fl = Flavor(name)
    cols = 4099
    k = cols // 2
    words = fl.words(cols)
    lens = lens_at(len_pool(fl, cols, slices), 6)
    ks = topk_ks_at(lens, cols, k, 1)
    with W.forced(gpu, slices):
        for largest in (False, True):
            check_topk(gpu, fl, words, fl.device(words, lens, largest), k, largest, lens, ks, what="large k")


# ------------------------------------------------------------------ both arrays NULL
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("name", FLAVORS)
def test_null_arrays_equal_the_uniform_calls(gpu, name, slices):
    fl = Flavor(name)
    cols, k = 4099, 64
    words = fl.words(cols)
    d = fl.device(words, None, False)
    with W.forced(gpu, slices):
        for largest in (False, True):
            a_v, a_i, b_v, b_i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
            W.run(gpu, lambda: fl.uniform_topk(gpu, d, ROWS, cols, k, a_v.t, a_i.t, largest))
            W.run(gpu, lambda: fl.topk(gpu, d, ROWS, cols, k, b_v.t, b_i.t, largest, None, None, c.t))
            assert np.array_equal(a_v.get(), b_v.get()) and np.array_equal(a_i.get(), b_i.get()), largest
            assert (c.get().view(np.int32) == k).all()
            want_v, want_i, _ = expect_topk(fl, words, None, None, k, largest)
            assert np.array_equal(b_v.get(), want_v.ravel()) and np.array_equal(b_i.get().view(np.int32), want_i.ravel())
        for ksel in (1, cols // 2, cols):
            a, b = fl.out_vals(ROWS), fl.out_vals(ROWS)
            W.run(gpu, lambda: fl.uniform_select(gpu, d, ROWS, cols, ksel, a.t))
            W.run(gpu, lambda: fl.select(gpu, d, ROWS, cols, ksel, b.t))
            assert np.array_equal(a.get(), b.get()) and np.array_equal(b.get(), expect_select(fl, words, None, None, ksel))


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("name", FLAVORS)
def test_both_load_paths(gpu, name, slices):
    """An aligned base with ld % 8 == 0 and ld > cols (16-byte loads), and a base shifted by one
    element with an odd ld (guarded loads).  Everything outside a row's first len_r columns would win."""
    import torch
    fl = Flavor(name)
    cols, k = 4099, 64
    words = fl.words(cols)
    lens = lens_at(len_pool(fl, cols, slices), 3)
    with W.forced(gpu, slices):
        for ld, shift in ((cols + 13, 0), (cols + 4, 1)):
            assert (ld % 8 == 0) == (shift == 0)
            for largest in (False, True):
                d = fl.device(words, lens, largest, ld=ld, shift=shift)
                assert (d.data_ptr() % 16 == 0) == (shift == 0)
                ks = topk_ks_at(lens, cols, k, 5)
                check_topk(gpu, fl, words, d, k, largest, lens, ks, ld=ld, what=f"ld={ld} shift={shift}")
                if not largest:
                    check_select(gpu, fl, words, d, cols // 2, lens, select_ks_at(lens, cols, 2), ld=ld,
                                 what=f"ld={ld} shift={shift}")
    torch.cuda.synchronize()


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("name", ("i32", "f32", "bf16", "u16"))
def test_row_groups(gpu, name, slices):
    """10 rows in groups of 4: every group has its own lens, ks and counts."""
    fl = Flavor(name)
    cols, k = 4099, 64
    words = fl.words(cols)
    lens = [cols - 11 * r * r - r for r in range(ROWS)]
    lens[4], lens[9] = 0, 3
    ks = [(5 * r + 2) % (k + 3) for r in range(ROWS)]
    assert len(set(lens)) == ROWS and len(set(ks)) == ROWS
    with W.forced(gpu, slices, 4):
        for largest in (False, True):
            check_topk(gpu, fl, words, fl.device(words, lens, largest), k, largest, lens, ks, what="groups")
        check_select(gpu, fl, words, fl.device(words, lens, False), cols // 2, lens, [7 * r + 1 for r in range(ROWS)],
                     what="groups")


# ------------------------------------------------------------------ scratch
@pytest.mark.parametrize("name", ("f32", "bf16"))
def test_stale_counts_and_scratch(gpu, name):
    """slices = 7 on one ctx: full-length rows, then rows no longer than a slice (the other six
    slices' counts are stale unless rewritten), then empty rows, then an existing 32-bit wide
    select and a 16-bit wide top-k.  Each result equals numpy's and that of a fresh ctx."""
    import kselect
    fl = Flavor(name)
    cols, k = 20001, 64
    words = fl.words(cols)
    sk = fl.slice_keys(cols, 7)
    batches = [[cols] * ROWS, [sk - (r * 131) % sk for r in range(ROWS)], [0] * ROWS]
    assert all(0 < n <= sk for n in batches[1]) and sk in batches[1]
    ks = [k, k + 9, 1, 0, 33, k, 2, k - 1, 64, 17]
    m32 = W.matrix(True, 6, 20001)
    m16 = W16.matrix("bf16", 20001, 0)
    d32, d16 = m32.device(), m16.device()

    def sequence(sel):
        got = []
        for lens in batches:
            v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
            dl, dk = dev_i32(lens), dev_i32(ks)
            d = fl.device(words, lens, True)
            W.run(sel, lambda: fl.topk(sel, d, ROWS, cols, k, v.t, i.t, True, dl, dk, c.t))
            got.append((v.get().copy(), i.get().view(np.int32).copy(), c.get().view(np.int32).copy()))
        o = W.Out(6, True)
        W.run(sel, lambda: sel.rows_wide(d32, 6, 20001, 10000, o.t, f32=True))
        v16, i16 = W16.Out(m16.rows * k), W16.Out(m16.rows * k, idx=True)
        W.run(sel, lambda: sel.topk_rows_wide16(d16, m16.rows, 20001, k, v16.t, i16.t, largest=True, kind="bf16"))
        return got, o.get().copy(), v16.get().copy(), i16.get().view(np.int32).copy()

    def alone(index):
        """Call `index` of the sequence on a ctx of its own."""
        with kselect.Selector(0) as sel:
            sel.wide_rows_force(7, 0)
            if index < 3:
                lens = batches[index]
                v, i, c = fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
                dl, dk = dev_i32(lens), dev_i32(ks)
                d = fl.device(words, lens, True)
                W.run(sel, lambda: fl.topk(sel, d, ROWS, cols, k, v.t, i.t, True, dl, dk, c.t))
                return v.get().copy(), i.get().view(np.int32).copy(), c.get().view(np.int32).copy()
            if index == 3:
                o = W.Out(6, True)
                W.run(sel, lambda: sel.rows_wide(d32, 6, 20001, 10000, o.t, f32=True))
                return o.get().copy()
            v16, i16 = W16.Out(m16.rows * k), W16.Out(m16.rows * k, idx=True)
            W.run(sel, lambda: sel.topk_rows_wide16(d16, m16.rows, 20001, k, v16.t, i16.t, largest=True, kind="bf16"))
            return v16.get().copy(), i16.get().view(np.int32).copy()

    with kselect.Selector(0) as sel:
        sel.wide_rows_force(7, 0)
        got, sel32, v16, i16 = sequence(sel)
    for n, lens in enumerate(batches):
        want_v, want_i, want_c = expect_topk(fl, words, lens, ks, k, True)
        for g, w, f in zip(got[n], (want_v.ravel(), want_i.ravel(), want_c), alone(n)):
            assert np.array_equal(g, w) and np.array_equal(g, f), (n, g[:8], w[:8], f[:8])
    assert np.array_equal(sel32, m32.want_select(10000)) and np.array_equal(sel32, alone(3))
    want_v, want_i = m16.want_topk(k, True)
    f_v, f_i = alone(4)
    assert np.array_equal(v16, want_v.ravel()) and np.array_equal(i16, want_i.ravel())
    assert np.array_equal(v16, f_v) and np.array_equal(i16, f_i)


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("name", ("i32", "f32", "bf16", "i16"))
def test_graph_replay(gpu, name):
    """After reserve_wide_rows: one var select and one var top-k captured at a forced slices = 3,
    force back to automatic; three replays with d_lens, d_ks and the keys rewritten in place
    (full length, ragged, with empty rows); then an eager existing wide call on the ctx."""
    import torch
    fl = Flavor(name)
    cols, k, ksel = 20001, 64, 20001 // 3
    pool = len_pool(fl, cols, 3)
    wa, wb = fl.words(cols), fl.words(cols)[::-1].copy()
    ragged = lens_at(pool, 8)
    empties = [0 if r % 3 == 0 else n for r, n in enumerate(lens_at(pool, 13))]
    batches = [(wa, [cols] * ROWS, [k] * ROWS, [ksel] * ROWS),
               (wb, ragged, topk_ks_at(ragged, cols, k, 2), select_ks_at(ragged, cols, 4)),
               (wa, empties, topk_ks_at(empties, cols, k, 7), select_ks_at(empties, cols, 1))]
    b = W.Bench()
    g = None
    try:
        d = fl.device(wa, None, True)
        dl, dk, dks = dev_i32([0] * ROWS), dev_i32([0] * ROWS), dev_i32([0] * ROWS)
        o_s, o_v, o_i, o_c = fl.out_vals(ROWS), fl.out_vals(ROWS * k), fl.out_idx(ROWS * k), W.Out(ROWS)
        b.sel.reserve_wide_rows(ROWS, cols)
        b.sel.wide_rows_force(3, 0)
        g = b.capture(lambda: (fl.select(b.sel, d, ROWS, cols, ksel, o_s.t, dl, dks),
                               fl.topk(b.sel, d, ROWS, cols, k, o_v.t, o_i.t, True, dl, dk, o_c.t)))
        b.sel.wide_rows_force(0, 0)
        for n, (words, lens, ks, kss) in enumerate(batches):
            d.copy_(fl.device(words, lens, True))
            dl.copy_(dev_i32(lens)), dk.copy_(dev_i32(ks)), dks.copy_(dev_i32(kss))
            for o in (o_s, o_v, o_i, o_c):
                o.buf.fill_(o.poison if hasattr(o, "poison") else W.POISON)
            b.replay(g)
            want_v, want_i, want_c = expect_topk(fl, words, lens, ks, k, True)
            assert np.array_equal(o_c.get().view(np.int32), want_c), (n, o_c.get(), want_c)
            assert np.array_equal(o_i.get().view(np.int32), want_i.ravel()), n
            assert np.array_equal(o_v.get(), want_v.ravel()), n
            want_s = expect_select(fl, words, lens, kss, ksel)
            assert np.array_equal(o_s.get(), want_s), (n, o_s.get(), want_s)
        d.copy_(fl.device(wa, None, True))
        o_e = fl.out_vals(ROWS)
        b.eager(lambda: fl.uniform_select(b.sel, d, ROWS, cols, cols // 2, o_e.t))
        assert np.array_equal(o_e.get(), expect_select(fl, wa, None, None, cols // 2))
    finally:
        del g
        b.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("name", ("i32", "f32", "f16"))
def test_bad_arguments(gpu, name):
    import kselect
    fl = Flavor(name)
    cols = 4099
    words = fl.words(cols)
    d = fl.device(words, None, False)
    lens, ks = dev_i32([5] * ROWS), dev_i32([2] * ROWS)
    o, v, i, c = fl.out_vals(ROWS), fl.out_vals(ROWS * 4), fl.out_idx(ROWS * 4), W.Out(ROWS)
    bad = [dict(cols=0), dict(cols=(1 << 24) + 1, ld=(1 << 24) + 1), dict(ld=cols - 1), dict(k=0), dict(k=cols + 1),
           dict(rows=-1)]
    for kw in bad:
        a = dict(rows=ROWS, cols=cols, ld=cols, k=4)
        a.update(kw)
        with pytest.raises(kselect.KthError) as e:
            fl.select(gpu, d, a["rows"], a["cols"], a["k"], o.t, lens, ks, a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
        with pytest.raises(kselect.KthError) as e:
            fl.topk(gpu, d, a["rows"], a["cols"], a["k"], v.t, i.t, False, lens, ks, c.t, a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
    with pytest.raises(kselect.KthError) as e:
        fl.topk(gpu, d, ROWS, cols, 4, None, None, False, lens, ks, c.t)  # no output pointer (d_cnt alone is none)
    assert e.value.code == kselect.KTH_EINVAL
    lib, P = kselect.LIB, kselect._ptr
    if fl.w16:
        for kind in (-1, 4, 99):
            assert lib.kth_select_wide_rows_var_k16(gpu._ctx, P(d), ROWS, cols, cols, P(lens), P(ks), 4, kind,
                                                    P(o.t)) == kselect.KTH_EINVAL
            assert lib.kth_topk_wide_rows_var_k16(gpu._ctx, P(d), ROWS, cols, cols, P(lens), P(ks), 4, 0, kind, P(v.t),
                                                  P(i.t), P(c.t)) == kselect.KTH_EINVAL
        assert lib.kth_select_wide_rows_var_k16(gpu._ctx, None, ROWS, cols, cols, P(lens), P(ks), 4, kselect.KTH_K16_F16,
                                                P(o.t)) == kselect.KTH_EINVAL
        assert lib.kth_select_wide_rows_var_k16(gpu._ctx, P(d), ROWS, cols, cols, P(lens), P(ks), 4, kselect.KTH_K16_F16,
                                                None) == kselect.KTH_EINVAL
    else:
        fn = lib.kth_select_wide_rows_var_f32 if fl.f32 else lib.kth_select_wide_rows_var_i32
        assert fn(gpu._ctx, None, ROWS, cols, cols, P(lens), P(ks), 4, P(o.t)) == kselect.KTH_EINVAL
        assert fn(gpu._ctx, P(d), ROWS, cols, cols, P(lens), P(ks), 4, None) == kselect.KTH_EINVAL
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched() and c.untouched()
    # rows == 0 is fine and launches nothing
    fl.select(gpu, d, 0, cols, 4, o.t, lens, ks)
    fl.topk(gpu, d, 0, cols, 4, v.t, i.t, False, lens, ks, c.t)
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched() and c.untouched()
    check_select(gpu, fl, words, d, cols // 2, None, None, what="after errors")


# ------------------------------------------------------------------ the workload's shape
@pytest.mark.parametrize("name", ("bf16", "f32"))
def test_vocabulary_sized(gpu, name):
    """4 x 128256 randn logits under the automatic plan: top-50 largest, one k and one length a request."""
    fl = Flavor(name)
    rows, cols, k = 4, 128256, 50
    x = np.random.default_rng(17).standard_normal((rows, cols)).astype(np.float32)
    words = W16.to_kind_bits(x, "bf16").reshape(rows, cols) if fl.w16 else x.view(np.uint32)
    lens, ks = [128256, 100000, 50, 1], [50, 1, 50, 7]
    d = fl.device(words, lens, True)
    check_topk(gpu, fl, words, d, k, True, lens, ks, what="vocabulary")
    check_select(gpu, fl, words, fl.device(words, lens, False), cols // 2, lens, [cols // 2, 1, 50, 7], what="vocabulary")
