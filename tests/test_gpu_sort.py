"""GPU: the stable in-place sort of top-k rows (include/kth.h "rows, sorted
top-k"; csrc/kth_rows_sort.hpp), both forms -- 64 / k' rows a wavefront for k
<= 64, one workgroup a row above -- for int32, float32, int16, uint16, float16
and bfloat16 values, and sorted=True of the eight per-row top-k wrappers.

Expected values come from numpy on the host: per row, np.argsort(kind="stable")
of the documented order key (order_keys of tests/test_gpu_rows_wide.py, rule_key
of tests/test_gpu_rows_wide16.py; the bit-inverted key for largest) over the
row's first n_r = clamp(d_cnt[r], 0, k) entries, applied to the values and to
the indices.  Bits are compared, not floats.  Every buffer is poisoned, carries
two guard elements past each end, and is compared whole: entries [n_r, k) of a
row must still hold their poison.
"""
import numpy as np
import pytest

import test_gpu_rows_wide as W
import test_gpu_rows_wide16 as W16

pytestmark = pytest.mark.gpu

FLAVOURS = ("i32", "f32") + W16.KINDS
KS = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 255, 257, 1000, 2048, 2049, 4095, 4096)
ROWS = (1, 3, 67)
POISON_V = {4: W.POISON, 2: W16.POISON16}
POISON_I = W16.POISON32
# float specials as bits: NaNs of several payloads and both signs, +-0.0, +-inf, subnormals
SPECIALS16 = {"f16": np.array([0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7FFF, 0xFD23, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x0001,
                               0x8001, 0x03FF, 0x83FF, 0x0010], dtype=np.uint16),
              "bf16": np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFA5, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x0001,
                                0x8001, 0x007F, 0x807F, 0x0010], dtype=np.uint16)}


def np_t(fl):
    return np.uint16 if fl in W16.KINDS else np.uint32


def keys_of(fl, words):
    return W16.rule_key(words, fl) if fl in W16.KINDS else W.order_keys(words, fl == "f32")


def specials(fl):
    return SPECIALS16[fl] if fl in SPECIALS16 else W.SPECIALS if fl == "f32" else None


def clamp_cnt(cnt, rows, k):
    return [k if cnt is None else max(0, min(int(cnt[r]), k)) for r in range(rows)]


def expect(fl, vals, idx, cnt, largest):
    """The sorted rows: vals, idx (or None) as rows x k arrays; cnt a list or None."""
    rows, k = vals.shape
    ov, oi = vals.copy(), None if idx is None else idx.copy()
    for r, n in enumerate(clamp_cnt(cnt, rows, k)):
        key = keys_of(fl, vals[r, :n])
        o = np.argsort(~key if largest else key, kind="stable")
        ov[r, :n] = vals[r, :n][o]
        if idx is not None:
            oi[r, :n] = idx[r, :n][o]
    return ov, oi


def make_rows(fl, rows, k, seed, kinds=("five", "equal", "asc", "desc", "uniform", "specials")):
    """rows x k words; row r is of kind kinds[(r + seed) % len]: keys drawn from five values (long tie
    runs), all equal, sorted either way, distinct-ish random, and for the float kinds the specials."""
    rng = np.random.default_rng(7919 * k + 31 * rows + seed + 1000003 * FLAVOURS.index(fl))
    t = np_t(fl)
    out = np.empty((rows, k), dtype=t)
    sp = specials(fl)
    for r in range(rows):
        kind = kinds[(r + seed) % len(kinds)]
        if fl == "f32":
            u = (rng.standard_normal(k) * 3.0).astype(np.float32).view(np.uint32)
        elif fl in SPECIALS16:
            u = W16.to_kind_bits(rng.standard_normal(k).astype(np.float32), fl)
        else:
            u = rng.integers(0, 1 << (8 * t().itemsize), k, dtype=np.uint64).astype(t)
        if kind == "five":
            u = u[:5][rng.integers(0, min(5, k), k)]
        elif kind == "equal":
            u = np.full(k, u[0], dtype=t)
        elif kind in ("asc", "desc"):
            u = u[np.argsort(keys_of(fl, u), kind="stable")]
            u = u if kind == "asc" else u[::-1].copy()
        elif kind == "specials" and sp is not None:
            pos = rng.permutation(k)[:max(1, k // 2)]
            u[pos] = sp[rng.integers(0, len(sp), len(pos))]
        out[r] = u
    out[out == POISON_V[t().itemsize]] ^= t(1)
    return out


class Buf:
    """rows x k elements on the device, entries [n_r, k) of each row and two guard elements past
    each end poisoned; idx: an int32 payload buffer."""

    def __init__(self, fl, data, cnt, idx=False):
        import torch
        rows, k = data.shape
        self.t = np.uint32 if idx else np_t(fl)
        self.poison = POISON_I if idx else POISON_V[self.t().itemsize]
        host = np.full(rows * k + 4, self.poison, dtype=self.t)
        body = host[2:-2].reshape(rows, k)
        for r, n in enumerate(clamp_cnt(cnt, rows, k)):
            body[r, :n] = data[r, :n].astype(self.t)
        self.start = host.copy()
        self.shape = (rows, k)
        self.buf = torch.from_numpy(host.view(np.int16 if self.t == np.uint16 else np.int32)).cuda()
        self.d = self.buf[2:2 + rows * k]
        if fl == "f32" and not idx:
            self.d = self.d.view(torch.float32)

    def host(self):
        return self.buf.cpu().numpy().view(self.t)

    def want(self, sorted_rows, cnt):
        """The whole buffer after the call: guards and padding as they were."""
        rows, k = self.shape
        w = self.start.copy()
        body = w[2:-2].reshape(rows, k)
        for r, n in enumerate(clamp_cnt(cnt, rows, k)):
            body[r, :n] = sorted_rows[r, :n].astype(self.t)
        return w


def payload(mode, rows, k):
    if mode == "none":
        return None
    if mode == "cols":
        return np.tile(np.arange(k, dtype=np.int32), (rows, 1))
    return (1000 * np.arange(rows, dtype=np.int32)[:, None] + (k - np.arange(k, dtype=np.int32))[None, :]).astype(np.int32)


def counts(mode, rows, k, seed):
    if mode == "null":
        return None
    if mode == "mix":  # per row: in range, above k, below 0, the edges
        pool = [k, 0, 1, k + 5, -3, k // 2, max(k - 1, 0), 2, 1 << 30, -(1 << 31)]
        return [pool[(r + seed) % len(pool)] for r in range(rows)]
    return [{"all": k, "zero": 0, "one": 1}[mode]] * rows


def run_sort(sel, fl, vals, idx, cnt, largest):
    """One sort of rows x k host arrays on the device; returns nothing, asserts every element."""
    import torch
    rows, k = vals.shape
    bv = Buf(fl, vals, cnt)
    bi = None if idx is None else Buf(fl, idx.view(np.uint32), cnt, idx=True)
    dc = None if cnt is None else torch.tensor(cnt, dtype=torch.int64).to(torch.int32).cuda()
    torch.cuda.synchronize()
    sel.sort_topk_rows(bv.d, None if bi is None else bi.d, rows, k, largest=largest, f32=fl == "f32",
                       kind=fl if fl in W16.KINDS else None, d_cnt=dc)
    sel.sync()
    wv, wi = expect(fl, vals, idx, cnt, largest)
    got, want = bv.host(), bv.want(wv, cnt)
    tag = (fl, rows, k, largest, cnt if cnt is None else cnt[:6])
    assert np.array_equal(got, want), (tag, "vals", np.nonzero(got != want)[0][:6], got[:12], want[:12])
    if bi is not None:
        got, want = bi.host(), bi.want(wi.view(np.uint32), cnt)
        assert np.array_equal(got, want), (tag, "idx", np.nonzero(got != want)[0][:6], got[:12], want[:12])
    if dc is not None:
        assert np.array_equal(dc.cpu().numpy(), np.array(cnt, dtype=np.int64).astype(np.int32)), (tag, "d_cnt written")
    return bv, bi


CNT_MODES = ("all", "zero", "one", "mix", "null")
IDX_MODES = ("none", "cols", "desc")


# ------------------------------------------------------------------ the sort itself
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_sort_rows(gpu, fl, largest, k):
    """Every k at the edges of the forms and of the power-of-two padding, rows = 1, 3 and 67 (a
    packed wave form then has a full workgroup and a partial last wavefront), every d_cnt mode;
    the payload mode rotates with them (NULL, columns, descending numbers)."""
    for rows in ROWS:
        vals = make_rows(fl, rows, k, seed=rows + k)
        for ci, cmode in enumerate(CNT_MODES):
            idx = payload(IDX_MODES[(ci + rows + k) % 3], rows, k)
            run_sort(gpu, fl, vals, idx, counts(cmode, rows, k, ci + k), largest)


@pytest.mark.parametrize("fl", FLAVOURS)
def test_every_payload_mode_on_tie_runs(gpu, fl):
    """Keys drawn from five values, every payload mode and direction, in both forms: ties keep
    their input order whatever the payload is."""
    for k in (8, 33, 300):
        vals = make_rows(fl, 5, k, seed=0, kinds=("five",))
        for mode in IDX_MODES:
            for largest in (False, True):
                run_sort(gpu, fl, vals, payload(mode, 5, k), None, largest)


@pytest.mark.parametrize("fl", FLAVOURS)
def test_packed_thousand_rows(gpu, fl):
    """1000 rows at k = 8: eight rows a wavefront, 32 a workgroup, a partial last workgroup."""
    vals = make_rows(fl, 1000, 8, seed=3)
    run_sort(gpu, fl, vals, payload("desc", 1000, 8), counts("mix", 1000, 8, 1), True)
    run_sort(gpu, fl, vals, payload("cols", 1000, 8), None, False)


@pytest.mark.parametrize("k", [2, 8, 64, 65, 1000, 4096])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_all_equal_rows_come_back_as_they_went(gpu, fl, k):
    vals = make_rows(fl, 3, k, seed=1, kinds=("equal",))
    idx = payload("desc", 3, k)
    for largest in (False, True):
        bv, bi = run_sort(gpu, fl, vals, idx, None, largest)
        assert np.array_equal(bv.host(), bv.start) and np.array_equal(bi.host(), bi.start)


@pytest.mark.parametrize("k", [15, 64, 200])
@pytest.mark.parametrize("fl", ["f32", "f16", "bf16"])
def test_float_specials_keep_their_bits(gpu, fl, k):
    """Rows of -0.0, +0.0, subnormals, both infinities and NaNs of several payloads: -0.0 before
    +0.0, every NaN above +inf, the NaNs in their input order with their payloads."""
    sp = specials(fl)
    rng = np.random.default_rng(k)
    vals = sp[rng.integers(0, len(sp), (4, k))].astype(np_t(fl))
    idx = payload("cols", 4, k)
    inf = W16.INF[fl] if fl in W16.INF else 0x7F800000
    mag = np_t(fl)(0x7FFF if fl in W16.INF else 0x7FFFFFFF)
    for largest in (False, True):
        bv, bi = run_sort(gpu, fl, vals, idx, None, largest)
        got = bv.host()[2:-2].reshape(4, k)
        cols = bi.host()[2:-2].reshape(4, k).view(np.int32)
        for r in range(4):
            assert np.array_equal(np.sort(got[r]), np.sort(vals[r])), "the multiset of bit patterns changed"
            nan_in = vals[r][(vals[r] & mag) > inf]
            nan_out = got[r][(got[r] & mag) > inf]
            assert np.array_equal(nan_in, nan_out), "NaNs moved among themselves or lost a payload"
            assert np.array_equal(vals[r][cols[r]], got[r]), "a value left its index"
            at = slice(0, len(nan_out)) if largest else slice(k - len(nan_out), k)
            assert ((got[r][at] & mag) > inf).all(), "a NaN does not stand above +inf"


def test_two_runs_are_bit_equal(gpu):
    vals = make_rows("f32", 67, 129, seed=2)
    idx, cnt = payload("desc", 67, 129), counts("mix", 67, 129, 4)
    a = run_sort(gpu, "f32", vals, idx, cnt, True)
    b = run_sort(gpu, "f32", vals, idx, cnt, True)
    assert np.array_equal(a[0].host(), b[0].host()) and np.array_equal(a[1].host(), b[1].host())


# ------------------------------------------------------------------ sorted=True of the wrappers
def outs(fl, rows, k):
    """Poisoned vals and idx outputs with guards (the wide tests' helpers)."""
    if fl in W16.KINDS:
        return W16.Out(rows * k), W16.Out(rows * k, idx=True)
    return W.Out(rows * k, fl == "f32"), W.Out(rows * k)


def keys_on_device(fl, rows, cols):
    """(host words, device keys) of the wide tests' mixed matrices."""
    if fl in W16.KINDS:
        m = W16.matrix(fl, cols, 0, rows=rows)
        return m.words, m.device()
    m = W.matrix(fl == "f32", rows, cols)
    return m.words, m.device()


def end_to_end(sel, fl, rows, k, largest, call, with_cnt):
    """call(vals, idx, cnt, sorted) enqueues one wrapper; sorted=True must give the unsorted call's
    output put through the numpy stable sort, poison and padding included."""
    import torch
    res = []
    for srt in (False, True):
        v, i = outs(fl, rows, k)
        c = W.Out(rows) if with_cnt else None
        torch.cuda.synchronize()
        call(v.t, i.t, c.t if c else None, srt)
        sel.sync()
        res.append((v.get().copy(), i.get().view(np.int32).copy(), c.get().view(np.int32).copy() if c else None))
    (uv, ui, uc), (sv, si, sc) = res
    cnt = None if uc is None else [int(x) for x in uc]
    wv, wi = expect(fl, uv.reshape(rows, k), ui.reshape(rows, k), cnt, largest)
    tag = (fl, rows, k, largest, cnt)
    assert uc is None or np.array_equal(uc, sc), (tag, "d_cnt differs")
    assert np.array_equal(sv.reshape(rows, k), wv), (tag, "vals", sv[:16], wv.ravel()[:16])
    assert np.array_equal(si.reshape(rows, k), wi), (tag, "idx", si[:16], wi.ravel()[:16])
    return sv.reshape(rows, k), si.reshape(rows, k)


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_topk_rows_sorted(gpu, fl, largest):
    """topk_rows / topk_rows16 (narrow rows): k in the wave form and in the workgroup form."""
    rows, cols = 8, 1000
    words, d = keys_on_device(fl, rows, cols)
    for k in (7, 100):
        if fl in W16.KINDS:
            call = lambda v, i, c, s: gpu.topk_rows16(d, rows, cols, k, v, i, largest=largest, kind=fl, sorted=s)
        else:
            call = lambda v, i, c, s: gpu.topk_rows(d, rows, cols, k, v, i, largest=largest, f32=fl == "f32", sorted=s)
        end_to_end(gpu, fl, rows, k, largest, call, False)


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_topk_rows_wide_sorted(gpu, fl, largest):
    import torch
    rows, cols = 6, 4099
    words, d = keys_on_device(fl, rows, cols)
    for k in (33, 64, 500):
        if fl in W16.KINDS:
            call = lambda v, i, c, s: gpu.topk_rows_wide16(d, rows, cols, k, v, i, largest=largest, kind=fl, sorted=s)
        else:
            call = lambda v, i, c, s: gpu.topk_rows_wide(d, rows, cols, k, v, i, largest=largest, f32=fl == "f32",
                                                         sorted=s)
        sv, _ = end_to_end(gpu, fl, rows, k, largest, call, False)
        if fl == "f32" and largest:  # against torch.topk(sorted=True) on the rows without a NaN
            clean = [r for r in range(rows) if not np.isnan(words[r].view(np.float32)).any()]
            assert clean
            want = torch.topk(d[:rows * cols].view(rows, cols)[clean], k, dim=1, largest=True, sorted=True).values
            assert np.array_equal(sv[clean].view(np.float32), want.cpu().numpy())


def ragged(rows, cols, k):
    """A length and a k per row: a row with k_r = 0, an empty row, a row shorter than k (its padding
    follows sorted entries), rows at the bounds."""
    lens = [cols, k // 2, cols // 2, 0, cols, 1, cols - 1, 3][:rows]
    ks = [k, k, 0, k, 1, k, k - 1, 2][:rows]
    return lens, ks


@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_topk_rows_wide_var_sorted(gpu, fl, largest):
    import test_gpu_rows_var as V
    rows, cols = 8, 4099
    words, d = keys_on_device(fl, rows, cols)
    for k in (33, 200):
        lens, ks = ragged(rows, cols, k)
        dl, dk = V.dev_i32(lens), V.dev_i32(ks)
        if fl in W16.KINDS:
            call = lambda v, i, c, s: gpu.topk_rows_wide16_var(d, rows, cols, k, v, i, largest=largest, kind=fl,
                                                               d_lens=dl, d_ks=dk, d_cnt=c, sorted=s)
        else:
            call = lambda v, i, c, s: gpu.topk_rows_wide_var(d, rows, cols, k, v, i, largest=largest, f32=fl == "f32",
                                                             d_lens=dl, d_ks=dk, d_cnt=c, sorted=s)
        sv, si = end_to_end(gpu, fl, rows, k, largest, call, True)
        assert (si[2] == -1).all() and (si[1, k // 2:] == -1).all() and (si[1, :k // 2] >= 0).all()


@pytest.mark.parametrize("fl", ["f32", "f16", "bf16"])
def test_topp_rows_wide_sorted(gpu, fl):
    import torch
    rows, cols = 8, 4099
    words, d = keys_on_device(fl, rows, cols)
    for k in (33, 200):
        lens, ks = ragged(rows, cols, k)
        dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        dk = torch.tensor(ks, dtype=torch.int32, device="cuda")
        dp = torch.tensor([0.9, 0.5, 1.0, 0.3, 0.0, 1.0, 0.99, 0.7][:rows], dtype=torch.float32, device="cuda")
        if fl in W16.KINDS:
            call = lambda v, i, c, s: gpu.topp_rows_wide16(d, rows, cols, k, v, i, kind=fl, d_lens=dl, d_ks=dk,
                                                           d_ps=dp, d_cnt=c, sorted=s)
        else:
            call = lambda v, i, c, s: gpu.topp_rows_wide(d, rows, cols, k, v, i, d_lens=dl, d_ks=dk, d_ps=dp, d_cnt=c,
                                                         sorted=s)
        end_to_end(gpu, fl, rows, k, True, call, True)


# ------------------------------------------------------------------ graph capture
def test_graph_replay_sees_new_lengths_and_ks(gpu):
    """topk_rows_wide_var(sorted=True) captured once on 8 x 4096 at k = 33 (one linear chain on the
    ctx's stream, after reserve_wide_rows: nothing is allocated inside the capture); replayed
    after d_lens and d_ks were rewritten on the device, it gives the new answer."""
    import torch
    import test_gpu_rows_var as V
    rows, cols, k = 8, 4096, 33
    fl = V.Flavor("f32")
    words = W.matrix(True, rows, cols).words
    batches = [([cols] * rows, [k] * rows), ragged(rows, cols, k), ([5, cols, 0, 40, cols, 33, 34, 2], [k, 1, k, 20, 0, k, k, k])]
    b = W.Bench()
    g = None
    try:
        d = W.matrix(True, rows, cols).device()
        dl, dk = V.dev_i32([0] * rows), V.dev_i32([0] * rows)
        o_v, o_i, o_c = W.Out(rows * k, True), W.Out(rows * k), W.Out(rows)
        b.sel.reserve_wide_rows(rows, cols)
        g = b.capture(lambda: b.sel.topk_rows_wide_var(d, rows, cols, k, o_v.t, o_i.t, largest=True, f32=True, d_lens=dl,
                                                       d_ks=dk, d_cnt=o_c.t, sorted=True))
        for n, (lens, ks) in enumerate(batches):
            dl.copy_(V.dev_i32(lens)), dk.copy_(V.dev_i32(ks))
            for o in (o_v, o_i, o_c):
                o.buf.fill_(W.POISON)
            b.replay(g)
            uv, ui, uc = V.expect_topk(fl, words, lens, ks, k, True)
            wv, wi = expect("f32", uv, ui, [int(x) for x in uc], True)
            assert np.array_equal(o_c.get().view(np.int32), uc), n
            assert np.array_equal(o_v.get().reshape(rows, k), wv), n
            assert np.array_equal(o_i.get().view(np.int32).reshape(rows, k), wi), n
    finally:
        del g
        b.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ independence
def test_last_stats_stay_the_selects(gpu):
    """A top-k, a sort and a select alternating on one ctx: kth_ctx_last_stats stays as the
    select set it."""
    import torch
    n = 1 << 16
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int64, device="cuda").to(torch.int32)
    rows, cols, k = 6, 4099, 64
    words, d = keys_on_device("i32", rows, cols)
    for rank in (1, n // 2, n):
        got = gpu.select(keys, rank)
        assert got == int(np.sort(keys.cpu().numpy())[rank - 1])
        before = gpu.stats()
        v, i = outs("i32", rows, k)
        gpu.topk_rows_wide(d, rows, cols, k, v.t, i.t, largest=True, sorted=True)
        gpu.sort_topk_rows(v.t, i.t, rows, k, largest=False)
        gpu.sync()
        assert gpu.stats() == before
        wv, wi = expect("i32", v.get().reshape(rows, k), i.get().reshape(rows, k), None, False)
        assert np.array_equal(wv, v.get().reshape(rows, k)), "the second sort did not leave ascending rows"
