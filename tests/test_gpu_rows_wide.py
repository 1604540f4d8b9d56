"""GPU: per-row select and top-k for wide rows (include/kth.h "wide rows";
csrc/kth_rows_wide.hpp), both forms -- `slices` workgroups a row and the fused
one-workgroup-per-row kernel -- and both load paths.

Expected values come from numpy on the host: the words are mapped to uint32
order keys by the documented rule (int32: bits ^ 0x80000000; float32: negative
b -> ~b, any other b -> b | 0x80000000, every NaN -> 0xFFFFFFFF) and each row
takes one stable argsort.  Select is the element of rank k, written with a NaN
canonical; top-k is the first k of the stable order (for largest: of the
stable order of the reversed key), sorted by column.  Bits are compared, not
floats.  Every output is poisoned and carries two guard elements past each
end.  A matrix and its orders are built once a module run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A  # (no test content holds it as a key)
QNAN = 0x7FC00000
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345,  # NaNs, both signs
                     0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                            # +-0.0, +-inf
                     0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00000400], dtype=np.uint32)  # subnormals


def order_keys(words, f32):
    w = words.astype(np.uint32)
    if not f32:
        return w ^ np.uint32(0x80000000)
    key = np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000))
    return np.where((w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def _uniform(rng, cols, f32):
    if f32:
        return (rng.standard_normal(cols) * 3.0).astype(np.float32).view(np.uint32)
    return rng.integers(0, 1 << 32, cols, dtype=np.uint64).astype(np.uint32)


def _row(kind, rng, cols, f32):
    u = _uniform(rng, cols, f32)
    if kind == "uniform":
        return u
    if kind == "specials":  # float only: the specials scattered over a uniform row
        pos = rng.permutation(cols)[:max(1, cols // 8)]
        u[pos] = SPECIALS[rng.integers(0, len(SPECIALS), len(pos))]
        return u
    if kind == "five":
        return u[:5][rng.integers(0, min(5, cols), cols)]
    if kind == "equal":
        return np.full(cols, u[0], dtype=np.uint32)
    if kind in ("asc", "desc"):
        s = u[np.argsort(order_keys(u, f32), kind="stable")]
        return s if kind == "asc" else s[::-1].copy()
    if kind == "low10":  # keys that differ only in their low 10 bits: the third digit decides
        return np.uint32(0x3F800000 if f32 else 0x12345400) | rng.integers(0, 1 << 10, cols, dtype=np.uint32)
    if kind == "tie":  # by column % 4: below, T, T, above -- the k-th of k = cols / 2 is T, in every slice
        lo, t, hi = (np.float32([0.5, 1.0, 2.0]).view(np.uint32) if f32 else np.uint32([5, 9, 77]))
        return np.array([lo, t, t, hi], dtype=np.uint32)[np.arange(cols) % 4]
    raise ValueError(kind)


def kinds(f32, tie=False):
    base = (["specials"] if f32 else ["uniform"]) + ["five", "equal", "asc", "desc", "low10"]
    return base + (["tie"] if tie else []) + (["uniform"] if f32 else [])


class Matrix:
    """rows x cols words (uint32 bit patterns) of mixed row kinds, with the stable orders of its rows."""

    def __init__(self, f32, rows, cols, tie=False, words=None, seed=0):
        self.f32, self.rows, self.cols = f32, rows, cols
        if words is None:
            rng = np.random.default_rng(1000 * cols + 10 * rows + int(f32) + seed)
            ks = kinds(f32, tie)
            words = np.stack([_row(ks[r % len(ks)], rng, cols, f32) for r in range(rows)])
        self.words = np.ascontiguousarray(words, dtype=np.uint32)
        assert not (self.words == POISON).any()
        self._order = {}

    def order(self, largest):
        if largest not in self._order:
            key = order_keys(self.words, self.f32)
            self._order[largest] = np.argsort(~key if largest else key, axis=1, kind="stable")
        return self._order[largest]

    def canon(self, w):
        if not self.f32:
            return w
        return np.where((w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(QNAN), w)

    def want_select(self, k):
        col = self.order(False)[:, k - 1]
        return self.canon(self.words[np.arange(self.rows), col])

    def want_topk(self, k, largest):
        idx = np.sort(self.order(largest)[:, :k], axis=1)
        return self.canon(np.take_along_axis(self.words, idx, axis=1)), idx.astype(np.int32)

    def device(self, ld=None, shift=0):
        """The matrix on the device, rows ld elements apart, the base `shift` elements into its buffer."""
        import torch
        ld = self.cols if ld is None else ld
        host = np.full(shift + self.rows * ld + 4, 0x01010101, dtype=np.uint32)
        view = host[shift:shift + self.rows * ld].reshape(self.rows, ld)
        view[:, :self.cols] = self.words
        buf = torch.from_numpy(host.view(np.int32)).cuda()
        keys = buf[shift:]
        return keys.view(torch.float32) if self.f32 else keys


_MATS = {}


def matrix(f32, rows, cols, tie=False):
    key = (f32, rows, cols, tie)
    if key not in _MATS:
        _MATS[key] = Matrix(f32, rows, cols, tie)
    return _MATS[key]


class Out:
    """A poisoned output of n words with two guard words past each end."""

    def __init__(self, n, f32=False):
        import torch
        self.n = n
        self.buf = torch.full((n + 4,), POISON, dtype=torch.int32, device="cuda")
        self.t = self.buf[2:2 + n].view(torch.float32) if f32 else self.buf[2:2 + n]

    def get(self):
        host = self.buf.cpu().numpy().view(np.uint32)
        assert (host[:2] == POISON).all() and (host[-2:] == POISON).all(), "a guard word was written"
        return host[2:2 + self.n]

    def untouched(self):
        return (self.buf.cpu().numpy().view(np.uint32) == POISON).all()


def run(sel, fn):
    import torch
    torch.cuda.synchronize()
    fn()
    sel.sync()


def check_select(sel, m, d_keys, ks, ld=None, what=""):
    for k in ks:
        o = Out(m.rows, m.f32)
        run(sel, lambda: sel.rows_wide(d_keys, m.rows, m.cols, k, o.t, f32=m.f32, ld=ld))
        got, want = o.get(), m.want_select(k)
        assert np.array_equal(got, want), (what, m.cols, k, np.nonzero(got != want)[0][:4], got[:8], want[:8])


def check_topk(sel, m, d_keys, ks, largest, modes=("both", "vals", "idx"), ld=None, what=""):
    for k in ks:
        want_v, want_i = m.want_topk(k, largest)
        for mode in modes:
            v = Out(m.rows * k, m.f32) if mode != "idx" else None
            i = Out(m.rows * k) if mode != "vals" else None
            run(sel, lambda: sel.topk_rows_wide(d_keys, m.rows, m.cols, k, v.t if v else None, i.t if i else None,
                                                largest=largest, f32=m.f32, ld=ld))
            tag = (what, m.cols, k, largest, mode)
            if i:
                got = i.get().view(np.int32).reshape(m.rows, k)
                bad = np.nonzero((got != want_i).any(axis=1))[0]
                assert bad.size == 0, (tag, "idx rows", bad[:4], got[bad[0]][:8], want_i[bad[0]][:8])
            if v:
                got = v.get().reshape(m.rows, k)
                bad = np.nonzero((got != want_v).any(axis=1))[0]
                assert bad.size == 0, (tag, "vals rows", bad[:4], got[bad[0]][:8], want_v[bad[0]][:8])


def select_ks(cols):
    return sorted({k for k in (1, 2, cols // 2, cols - 1, cols) if 1 <= k <= cols})


def topk_ks(cols):
    return sorted({k for k in (1, 7, 64, cols // 2, cols) if 1 <= k <= cols})


class forced:
    """The ctx's plan forced inside the block, automatic again after it."""

    def __init__(self, sel, slices=0, group_rows=0):
        self.sel, self.args = sel, (slices, group_rows)

    def __enter__(self):
        self.sel.wide_rows_force(*self.args)

    def __exit__(self, *exc):
        self.sel.wide_rows_force(0, 0)


# ------------------------------------------------------------------ select
@pytest.mark.parametrize("cols", [1, 2, 63, 1000, 4099, 16384, 20001])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_select_automatic_plan(gpu, f32, cols):
    m = matrix(f32, 6, cols)
    check_select(gpu, m, m.device(), select_ks(cols), what="auto")


@pytest.mark.parametrize("slices", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("cols", [4099, 20001])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_select_forced_slices(gpu, f32, cols, slices):
    """slices = 1 is the fused form; 64 slices of 4099 columns are shorter than
    one load round and the last one is short."""
    m = matrix(f32, 6, cols)
    with forced(gpu, slices):
        check_select(gpu, m, m.device(), select_ks(cols), what=f"slices={slices}")


# ------------------------------------------------------------------ top-k
@pytest.mark.parametrize("slices", [1, 3, 7])
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_topk_forced_slices(gpu, f32, largest, slices):
    """Every row kind and the tie rows: an all-equal row keeps columns 0..k-1; the
    `tie` row's k-th value (k = cols / 2) occurs in every slice and its quota
    ends in the middle of one."""
    cols = 4099
    m = matrix(f32, 8, cols, tie=True)
    with forced(gpu, slices):
        check_topk(gpu, m, m.device(), topk_ks(cols), largest, what=f"slices={slices}")
    # what the reference says about the tie rows, so that the check above means it
    ks = kinds(f32, True)
    k = cols // 2
    _, idx = m.want_topk(k, largest)
    assert np.array_equal(idx[ks.index("equal")], np.arange(k))
    tie = idx[ks.index("tie")]
    kept_ties = tie[(tie % 4 == 1) | (tie % 4 == 2)]  # the kept keys equal to the k-th
    assert 0 < kept_ties.size < cols // 2 - 8
    if slices > 1:
        slice_keys = (-(-cols // slices) + 3) // 4 * 4
        assert kept_ties.max() // slice_keys < slices - 1 and 4 < kept_ties.max() % slice_keys < slice_keys - 4


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("slices", [0, 1, 3])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_padded_rows_unaligned_base(gpu, f32, slices):
    """ld = cols + 3 and the base moved by one element: the guarded loads.  The
    outputs stay dense rows x k (the guards past them are checked)."""
    cols = 4099
    m = matrix(f32, 6, cols)
    d = m.device(ld=cols + 3, shift=1)
    assert d.data_ptr() % 16 == 4
    with forced(gpu, slices):
        check_select(gpu, m, d, (1, cols // 2, cols), ld=cols + 3, what="guarded")
        for largest in (False, True):
            check_topk(gpu, m, d, (7, cols // 2), largest, modes=("both",), ld=cols + 3, what="guarded")


@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_padded_rows_aligned(gpu, f32):
    """ld = cols + 1 with cols % 4 == 3: 16-byte loads, each row's last vector partly past the row."""
    cols = 4099
    m = matrix(f32, 6, cols)
    d = m.device(ld=cols + 1)
    for slices in (1, 3):
        with forced(gpu, slices):
            check_select(gpu, m, d, (2, cols // 2, cols), ld=cols + 1, what="padded")
            check_topk(gpu, m, d, (64,), True, modes=("both",), ld=cols + 1, what="padded")


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_row_groups(gpu, f32, slices):
    """group_rows = 2 with rows = 5: three groups, the last one partial."""
    cols = 4099
    m = matrix(f32, 5, cols)
    d = m.device()
    with forced(gpu, slices, 2):
        check_select(gpu, m, d, (1, cols // 2, cols), what="groups")
        check_topk(gpu, m, d, (7, cols // 2), False, modes=("both",), what="groups")
        check_topk(gpu, m, d, (64,), True, modes=("both",), what="groups")


# ------------------------------------------------------------------ the existing calls
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_agrees_with_rows_calls(gpu, f32):
    """Bit for bit: cols = 4096 against kth_topk_rows_*, cols = 16384 against kth_select_rows_*."""
    m = matrix(f32, 8, 4096, tie=True)
    d = m.device()
    for largest in (False, True):
        for k in (1, 64, 2048, 4096):
            a_v, a_i, b_v, b_i = Out(8 * k, f32), Out(8 * k), Out(8 * k, f32), Out(8 * k)
            run(gpu, lambda: gpu.topk_rows(d, 8, 4096, k, a_v.t, a_i.t, largest=largest, f32=f32))
            run(gpu, lambda: gpu.topk_rows_wide(d, 8, 4096, k, b_v.t, b_i.t, largest=largest, f32=f32))
            assert np.array_equal(a_v.get(), b_v.get()) and np.array_equal(a_i.get(), b_i.get()), (k, largest)
    m = matrix(f32, 6, 16384)
    d = m.device()
    for k in select_ks(16384):
        a, b = Out(6, f32), Out(6, f32)
        run(gpu, lambda: gpu.rows(d, 6, 16384, k, a.t, f32=f32))
        run(gpu, lambda: gpu.rows_wide(d, 6, 16384, k, b.t, f32=f32))
        assert np.array_equal(a.get(), b.get()), k


# ------------------------------------------------------------------ the workload's shape
def test_logits_shape_f32(gpu):
    """4 x 128256 float32 randn: the median per row and the top-50 largest."""
    rows, cols = 4, 128256
    words = np.random.default_rng(7).standard_normal((rows, cols)).astype(np.float32).view(np.uint32)
    m = Matrix(True, rows, cols, words=words)
    d = m.device()
    check_select(gpu, m, d, (cols // 2,), what="logits")
    check_topk(gpu, m, d, (50,), True, modes=("both",), what="logits")


def test_many_rows_i32(gpu):
    """300 x 32768 int32, automatic plan: the median per row and the top-64 smallest."""
    rows, cols = 300, 32768
    words = np.random.default_rng(8).integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    m = Matrix(False, rows, cols, words=words)
    d = m.device()
    check_select(gpu, m, d, (cols // 2,), what="many rows")
    check_topk(gpu, m, d, (64,), False, modes=("both",), what="many rows")


# ------------------------------------------------------------------ neighbours
def test_neighbours_on_one_ctx(gpu):
    """An int32 select, a wide top-k, a topk16, a wide select and a rows call on
    one ctx: every result equals that of the call alone on a ctx of its own."""
    import torch
    import kselect
    n = (1 << 20) + 7
    rng = np.random.default_rng(11)
    arr = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)).cuda()
    arr16 = torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, n, dtype=np.int64).astype(np.int16)).cuda()
    m = matrix(True, 6, 20001)
    dw = m.device()
    mr = matrix(False, 6, 1000)
    dr = mr.device()
    kw = 20001 // 2

    def calls(sel):
        o_sel, o_tv, o_ti = Out(1), Out(6 * 64, True), Out(6 * 64)
        o16v = torch.full((100,), 0x5A5A, dtype=torch.int16, device="cuda")
        o16i = torch.full((100,), -1, dtype=torch.int64, device="cuda")
        o_ws, o_rows = Out(6, True), Out(6)
        return [
            (lambda: sel.select_async(arr, n, n // 2, o_sel.t), lambda: [o_sel.get()]),
            (lambda: sel.topk_rows_wide(dw, 6, 20001, 64, o_tv.t, o_ti.t, largest=True, f32=True),
             lambda: [o_tv.get(), o_ti.get()]),
            (lambda: sel.topk16(arr16, n, 100, o16v, o16i), lambda: [o16v.cpu().numpy(), o16i.cpu().numpy()]),
            (lambda: sel.rows_wide(dw, 6, 20001, kw, o_ws.t, f32=True), lambda: [o_ws.get()]),
            (lambda: sel.rows(dr, 6, 1000, 500, o_rows.t), lambda: [o_rows.get()]),
        ]

    alone = []
    for i in range(5):
        with kselect.Selector(0) as sel:
            call, read = calls(sel)[i]
            run(sel, call)
            alone.append(read())
    # the wide results are the reference's, so "alone" is not merely self-consistent
    want_v, want_i = m.want_topk(64, True)
    assert np.array_equal(alone[1][0], want_v.ravel()) and np.array_equal(alone[1][1].view(np.int32), want_i.ravel())
    assert np.array_equal(alone[3][0], m.want_select(kw))
    with kselect.Selector(0) as sel:
        for order in ((0, 1, 2, 3, 4), (3, 2, 1, 0, 4, 1, 3)):
            cs = calls(sel)
            select_last = False  # the int32 select is the last call that owns the stats
            for i in order:
                call, read = cs[i]
                run(sel, call)
                for got, want in zip(read(), alone[i]):
                    assert np.array_equal(got, want), (order, i)
                select_last = i == 0 or (select_last and i != 2)
                if select_last:  # its stats survive the wide calls
                    st = sel.stats()
                    assert st["n"] == n and st["k"] == n // 2, (order, i, st)


# ------------------------------------------------------------------ graph capture
class Bench:
    """One stream and one ctx bound to it (the helper of tests/test_gpu_graph.py)."""

    def __init__(self):
        import torch
        import kselect
        self.stream = torch.cuda.Stream()
        self.sel = kselect.Selector(0, stream=self.stream)
        torch.cuda.synchronize()

    def capture(self, enqueue):
        """A graph of what enqueue() sends to the ctx; an error inside the capture fails the test."""
        import torch
        import kselect
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=self.stream):
                enqueue()
        except (kselect.KthError, RuntimeError) as e:
            pytest.fail(f"the capture did not complete: {e!r}")
        torch.cuda.synchronize()
        return g

    def replay(self, g):
        import torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            g.replay()
        torch.cuda.synchronize()

    def eager(self, fn):
        import torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            fn()
        torch.cuda.synchronize()

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.sel.close()


@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_graph_replay(gpu, f32):
    """After reserve_wide_rows: one wide select and one wide top-k captured at a
    forced slices = 3 (frozen in the graph), force back to automatic, two
    replays with the key buffer refilled in between, then an eager select."""
    rows, cols, k, kt = 6, 20001, 20001 // 3, 64
    ma, mb = matrix(f32, rows, cols), Matrix(f32, rows, cols, seed=5)
    b = Bench()
    g = None
    try:
        d = ma.device()
        o_s, o_v, o_i = Out(rows, f32), Out(rows * kt, f32), Out(rows * kt)
        b.sel.reserve_wide_rows(rows, cols)
        b.sel.wide_rows_force(3, 0)
        g = b.capture(lambda: (b.sel.rows_wide(d, rows, cols, k, o_s.t, f32=f32),
                               b.sel.topk_rows_wide(d, rows, cols, kt, o_v.t, o_i.t, largest=True, f32=f32)))
        b.sel.wide_rows_force(0, 0)
        for m in (ma, mb):
            d.copy_(m.device())
            for o in (o_s, o_v, o_i):
                o.buf.fill_(POISON)
            b.replay(g)
            want_v, want_i = m.want_topk(kt, True)
            assert np.array_equal(o_s.get(), m.want_select(k))
            assert np.array_equal(o_v.get(), want_v.ravel()) and np.array_equal(o_i.get().view(np.int32), want_i.ravel())
        o_e = Out(rows, f32)
        b.eager(lambda: b.sel.rows_wide(d, rows, cols, cols // 2, o_e.t, f32=f32))
        assert np.array_equal(o_e.get(), mb.want_select(cols // 2))
    finally:
        del g
        b.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
def test_bad_arguments(gpu, f32):
    import kselect
    cols = 1000
    m = matrix(f32, 6, cols)
    d = m.device()
    o, v, i = Out(6, f32), Out(6 * 4, f32), Out(6 * 4)
    bad = [dict(cols=0), dict(cols=(1 << 24) + 1, ld=(1 << 24) + 1), dict(ld=cols - 1), dict(k=0), dict(k=cols + 1),
           dict(rows=-1)]
    for kw in bad:
        a = dict(rows=6, cols=cols, ld=cols, k=4)
        a.update(kw)
        with pytest.raises(kselect.KthError) as e:
            gpu.rows_wide(d, a["rows"], a["cols"], a["k"], o.t, f32=f32, ld=a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
        with pytest.raises(kselect.KthError) as e:
            gpu.topk_rows_wide(d, a["rows"], a["cols"], a["k"], v.t, i.t, f32=f32, ld=a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
    with pytest.raises(kselect.KthError) as e:
        gpu.topk_rows_wide(d, 6, cols, 4, None, None, f32=f32)
    assert e.value.code == kselect.KTH_EINVAL
    for args in ((-1, 0), (0, -1), (kselect.KTH_WIDE_MAX_SLICES + 1, 0)):
        with pytest.raises(kselect.KthError) as e:
            gpu.wide_rows_force(*args)
        assert e.value.code == kselect.KTH_EINVAL
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched()
    # rows == 0 is fine and launches nothing
    gpu.rows_wide(d, 0, cols, 4, o.t, f32=f32)
    gpu.topk_rows_wide(d, 0, cols, 4, v.t, i.t, f32=f32)
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched()
    # and the automatic plan still answers after the refused force calls
    check_select(gpu, m, d, (cols // 2,), what="after errors")
