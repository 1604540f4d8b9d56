"""GPU: per-row select and top-k for wide rows of 16-bit keys (include/kth.h
"wide rows, 16-bit keys"; csrc/kth_rows_wide16.hpp), both forms -- `slices`
workgroups a row and the fused one-workgroup-per-row kernel -- and both load
paths, for int16, uint16, float16 and bfloat16 keys.

Expected values come from numpy on the host: the 2-byte words are mapped to
uint16 order keys by the documented rule (rule_key, as in
tests/test_gpu_rows16.py) and each row takes one stable argsort.  Select is the
element of rank k, written with a NaN canonical; top-k is the first k of the
stable order (for largest: of the stable order of ~key), sorted by column.
Bits are compared, not floats.  Every output is poisoned (0x5A5A, and a
distinct int32 poison for the columns) and carries two guard elements past
each end.  A matrix and its orders are built once a module run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("i16", "u16", "f16", "bf16")
INF = {"f16": 0x7C00, "bf16": 0x7F80}
CANON = {"f16": 0x7E00, "bf16": 0x7FC0}
POISON16 = 0x5A5A
POISON32 = 0x6B6B6B6B
TIE_LO, TIE_T, TIE_HI = 0x3800, 0x3C00, 0x4000  # ascending in all four kinds


def rule_key(bits, kind):
    """The documented order as uint16 keys (tests/test_gpu_rows16.py's rule_key, restated)."""
    b = np.asarray(bits, dtype=np.uint16)
    if kind == "i16":
        return b ^ np.uint16(0x8000)
    if kind == "u16":
        return b.copy()
    key = np.where(b >> 15 != 0, ~b, b | np.uint16(0x8000)).astype(np.uint16)
    return np.where((b & np.uint16(0x7FFF)) > np.uint16(INF[kind]), np.uint16(0xFFFF), key)


def to_kind_bits(x, kind):
    """float32 values rounded to the kind, as bits (float kinds only)."""
    if kind == "f16":
        return x.astype(np.float16).view(np.uint16)
    w = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even


# the row kinds, in two sets of 8 and 7 rows
ROW_SETS = (("random", "randn", "equal", "bit0", "bit5", "low5", "nan", "tie"),
            ("asc", "desc", "zeros", "random", "equal", "tie", "randn"))


def _row(what, rng, cols, kind):
    rnd = rng.integers(0, 1 << 16, cols, dtype=np.uint32).astype(np.uint16)
    if what == "random":  # all 65536 bit patterns: NaNs of both signs, infinities, subnormals
        return rnd
    if what == "randn":  # float kinds: randn rounded to the kind; integer kinds: a thousand values
        if kind in INF:
            return to_kind_bits(rng.standard_normal(cols).astype(np.float32), kind)
        return (rnd % np.uint16(1000)).astype(np.uint16)
    if what == "equal":
        return np.full(cols, rnd[0], dtype=np.uint16)
    if what == "bit0":  # two values that differ only in bit 0: the second digit decides
        return np.where(rnd & 1, 0x3C01, 0x3C00).astype(np.uint16)
    if what == "bit5":  # two values that differ only in bit 5: adjacent first-digit bins
        return np.where(rnd & 1, 0x3C20, 0x3C00).astype(np.uint16)
    if what == "low5":  # constant high 11 bits, random low 5
        return (rnd & np.uint16(0x001F)) | np.uint16(0xBE00)
    if what in ("asc", "desc"):
        s = rnd[np.argsort(rule_key(rnd, kind), kind="stable")]
        return s if what == "asc" else s[::-1].copy()
    if what == "nan":  # NaNs only (float kinds), any payload, either sign
        inf = INF.get(kind, 0x7F80)
        pay = (rnd % np.uint16(0x7FFF - inf)) + np.uint16(inf + 1)
        sign = rng.integers(0, 2, cols, dtype=np.uint32).astype(np.uint16) << np.uint16(15)
        return (pay | sign).astype(np.uint16)
    if what == "zeros":  # -0.0 / +0.0 alternating
        return np.where(np.arange(cols) % 2 == 0, 0x8000, 0x0000).astype(np.uint16)
    if what == "tie":  # by column % 4: below, T, T, above -- the k-th of k = cols / 2 is T, in every slice
        return np.array([TIE_LO, TIE_T, TIE_T, TIE_HI], dtype=np.uint16)[np.arange(cols) % 4]
    raise ValueError(what)


class Matrix:
    """rows x cols 2-byte words (bit patterns) of one key kind, with the stable orders of its rows."""

    def __init__(self, kind, cols, rowset=0, words=None, seed=0, rows=None):
        self.kind, self.cols = kind, cols
        if words is None:
            rng = np.random.default_rng(1000 * cols + 10 * rowset + KINDS.index(kind) + 100003 * seed)
            names = ROW_SETS[rowset][:rows]
            words = np.stack([_row(w, rng, cols, kind) for w in names])
        self.words = np.ascontiguousarray(words, dtype=np.uint16)
        self.rows = self.words.shape[0]
        self.keys = rule_key(self.words, kind)
        self._order = {}

    def order(self, largest):
        if largest not in self._order:
            key = (~self.keys).astype(np.uint16) if largest else self.keys
            self._order[largest] = np.argsort(key, axis=1, kind="stable")
        return self._order[largest]

    def canon(self, bits, keys):
        if self.kind not in CANON:
            return bits
        return np.where(keys == np.uint16(0xFFFF), np.uint16(CANON[self.kind]), bits)

    def want_select(self, k):
        col = self.order(False)[:, k - 1]
        r = np.arange(self.rows)
        return self.canon(self.words[r, col], self.keys[r, col])

    def want_topk(self, k, largest):
        idx = np.sort(self.order(largest)[:, :k], axis=1)
        vals = self.canon(np.take_along_axis(self.words, idx, axis=1), np.take_along_axis(self.keys, idx, axis=1))
        return vals, idx.astype(np.int32)

    def device(self, ld=None, shift=0):
        """The matrix on the device as int16 words, rows ld elements apart, the base `shift` elements into its buffer."""
        import torch
        ld = self.cols if ld is None else ld
        host = np.full(shift + self.rows * ld + 8, 0x0101, dtype=np.uint16)
        view = host[shift:shift + self.rows * ld].reshape(self.rows, ld)
        view[:, :self.cols] = self.words
        return torch.from_numpy(host.view(np.int16)).cuda()[shift:]


_MATS = {}


def matrix(kind, cols, rowset=0, rows=None):
    key = (kind, cols, rowset, rows)
    if key not in _MATS:
        _MATS[key] = Matrix(kind, cols, rowset, rows=rows)
    return _MATS[key]


class Out:
    """A poisoned output of n elements (2-byte words, or int32 columns) with two guard elements past each end."""

    def __init__(self, n, idx=False):
        import torch
        self.n = n
        self.poison = POISON32 if idx else POISON16
        self.np_t = np.uint32 if idx else np.uint16
        self.buf = torch.full((n + 4,), self.poison, dtype=torch.int32 if idx else torch.int16, device="cuda")
        self.t = self.buf[2:2 + n]

    def get(self):
        host = self.buf.cpu().numpy().view(self.np_t)
        assert (host[:2] == self.poison).all() and (host[-2:] == self.poison).all(), "a guard element was written"
        return host[2:2 + self.n]

    def untouched(self):
        return (self.buf.cpu().numpy().view(self.np_t) == self.poison).all()


def run(sel, fn):
    import torch
    torch.cuda.synchronize()
    fn()
    sel.sync()


def check_select(sel, m, d_keys, ks, ld=None, what=""):
    for k in ks:
        o = Out(m.rows)
        run(sel, lambda: sel.rows_wide16(d_keys, m.rows, m.cols, k, o.t, kind=m.kind, ld=ld))
        got, want = o.get(), m.want_select(k)
        assert np.array_equal(got, want), (what, m.kind, m.cols, k, np.nonzero(got != want)[0][:4], got[:8], want[:8])


def check_topk(sel, m, d_keys, ks, largest, modes=("both", "vals", "idx"), ld=None, what=""):
    for k in ks:
        want_v, want_i = m.want_topk(k, largest)
        for mode in modes:
            v = Out(m.rows * k) if mode != "idx" else None
            i = Out(m.rows * k, idx=True) if mode != "vals" else None
            run(sel, lambda: sel.topk_rows_wide16(d_keys, m.rows, m.cols, k, v.t if v else None, i.t if i else None,
                                                  largest=largest, kind=m.kind, ld=ld))
            tag = (what, m.kind, m.cols, k, largest, mode)
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
@pytest.mark.parametrize("cols", [1, 2, 7, 8, 9, 63, 1000, 4099, 8192, 20001])
@pytest.mark.parametrize("kind", KINDS)
def test_select_automatic_plan(gpu, kind, cols):
    for rowset in (0, 1):
        m = matrix(kind, cols, rowset)
        check_select(gpu, m, m.device(), select_ks(cols), what=f"auto set {rowset}")


@pytest.mark.parametrize("slices", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("cols", [4099, 20001])
@pytest.mark.parametrize("kind", KINDS)
def test_select_forced_slices(gpu, kind, cols, slices):
    """slices = 1 is the fused form; 64 slices of 4099 columns are 72 columns
    each, shorter than one load round, and the last one is short."""
    for rowset in (0, 1):
        m = matrix(kind, cols, rowset)
        with forced(gpu, slices):
            check_select(gpu, m, m.device(), select_ks(cols), what=f"slices={slices} set {rowset}")


# ------------------------------------------------------------------ top-k
@pytest.mark.parametrize("slices", [1, 3, 7])
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("kind", KINDS)
def test_topk_forced_slices(gpu, kind, largest, slices):
    """Every row kind and the tie rows: an all-equal row keeps columns 0..k-1; the
    `tie` row's k-th value (k = cols / 2) occurs in every slice and its quota
    ends in the middle of one."""
    cols = 4099
    for rowset in (0, 1):
        m = matrix(kind, cols, rowset)
        with forced(gpu, slices):
            check_topk(gpu, m, m.device(), topk_ks(cols), largest, what=f"slices={slices} set {rowset}")
    # what the reference says about the tie rows, so that the check above means it
    m = matrix(kind, cols, 0)
    k = cols // 2
    _, idx = m.want_topk(k, largest)
    assert np.array_equal(idx[ROW_SETS[0].index("equal")], np.arange(k))
    tie = idx[ROW_SETS[0].index("tie")]
    kept_ties = tie[(tie % 4 == 1) | (tie % 4 == 2)]  # the kept keys equal to the k-th
    assert 0 < kept_ties.size < cols // 2 - 8
    if slices > 1:
        slice_keys = (-(-cols // slices) + 7) // 8 * 8
        assert kept_ties.max() // slice_keys < slices - 1 and 8 < kept_ties.max() % slice_keys < slice_keys - 8


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_more_than_65535_equal_keys(gpu, kind, slices):
    """cols = 65547: a row holds more than 65535 equal keys and the kept columns
    exceed 16 bits.  An all-equal row, a two-valued row, and a row whose largest
    keys sit at columns >= 65536."""
    cols = 65547
    key = ("big", kind)
    if key not in _MATS:
        rng = np.random.default_rng(65547 + KINDS.index(kind))
        late = (rng.integers(0, 1 << 12, cols, dtype=np.uint32) | 0x1000).astype(np.uint16)  # 0x1000 .. 0x1FFF
        late[65536:] = np.uint16(0x4000) + rng.permutation(cols - 65536).astype(np.uint16)  # the largest, distinct
        two = np.where(rng.integers(0, 2, cols) != 0, 0x3C01, 0x3C00).astype(np.uint16)
        _MATS[key] = Matrix(kind, cols, words=np.stack([np.full(cols, 0x3C00, dtype=np.uint16), two, late]))
    m = _MATS[key]
    d = m.device()
    with forced(gpu, slices):
        check_select(gpu, m, d, (cols // 2,), what="65547")
        check_topk(gpu, m, d, (65540,), False, modes=("both",), what="65547")
        check_topk(gpu, m, d, (64,), True, modes=("both",), what="65547")
    _, idx = m.want_topk(65540, False)
    assert np.array_equal(idx[0], np.arange(65540))  # the all-equal row keeps columns 0 .. k-1
    _, idx = m.want_topk(64, True)
    assert (idx[2] >= 65536).sum() == cols - 65536


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("slices", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_padded_rows_unaligned_base(gpu, kind, slices):
    """ld = cols + 3 and the base moved by one element: the guarded loads.  The
    outputs stay dense rows x k (the guards past them are checked)."""
    cols = 4099
    m = matrix(kind, cols, 0)
    d = m.device(ld=cols + 3, shift=1)
    assert d.data_ptr() % 16 == 2
    with forced(gpu, slices):
        check_select(gpu, m, d, (1, cols // 2, cols), ld=cols + 3, what="guarded")
        for largest in (False, True):
            check_topk(gpu, m, d, (7, cols // 2), largest, modes=("both",), ld=cols + 3, what="guarded")


@pytest.mark.parametrize("kind", KINDS)
def test_padded_rows_aligned(gpu, kind):
    """ld = cols + 5 with cols = 4099 (ld % 8 == 0): 16-byte loads, each row's last vector partly past the row."""
    cols = 4099
    m = matrix(kind, cols, 0)
    d = m.device(ld=cols + 5)
    assert d.data_ptr() % 16 == 0 and (cols + 5) % 8 == 0
    for slices in (1, 3):
        with forced(gpu, slices):
            check_select(gpu, m, d, (2, cols // 2, cols), ld=cols + 5, what="padded")
            check_topk(gpu, m, d, (64, cols // 2), True, modes=("both",), ld=cols + 5, what="padded")


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_row_groups(gpu, kind, slices):
    """group_rows = 2 with rows = 5: three groups, the last one partial."""
    cols = 4099
    m = matrix(kind, cols, 0, rows=5)
    d = m.device()
    with forced(gpu, slices, 2):
        check_select(gpu, m, d, (1, cols // 2, cols), what="groups")
        check_topk(gpu, m, d, (7, cols // 2), False, modes=("both",), what="groups")
        check_topk(gpu, m, d, (64,), True, modes=("both",), what="groups")


# ------------------------------------------------------------------ the existing calls
@pytest.mark.parametrize("kind", KINDS)
def test_agrees_with_rows16_calls(gpu, kind):
    """Bit for bit at cols = 8192 against kth_select_rows_k16 and kth_topk_rows_k16."""
    cols = 8192
    for rowset in (0, 1):
        m = matrix(kind, cols, rowset)
        d = m.device()
        for k in (1, 2, 4096, 8191, 8192):
            a, b = Out(m.rows), Out(m.rows)
            run(gpu, lambda: gpu.rows16(d, m.rows, cols, k, a.t, kind=kind))
            run(gpu, lambda: gpu.rows_wide16(d, m.rows, cols, k, b.t, kind=kind))
            assert np.array_equal(a.get(), b.get()), (k, rowset)
            assert np.array_equal(b.get(), m.want_select(k)), (k, rowset)
        for largest in (False, True):
            for k in (1, 64, 4096, 8192):
                a_v, a_i, b_v, b_i = Out(m.rows * k), Out(m.rows * k, True), Out(m.rows * k), Out(m.rows * k, True)
                run(gpu, lambda: gpu.topk_rows16(d, m.rows, cols, k, a_v.t, a_i.t, largest=largest, kind=kind))
                run(gpu, lambda: gpu.topk_rows_wide16(d, m.rows, cols, k, b_v.t, b_i.t, largest=largest, kind=kind))
                assert np.array_equal(a_v.get(), b_v.get()) and np.array_equal(a_i.get(), b_i.get()), (k, largest)


def _widen_host(bits, kind):
    if kind == "bf16":
        return bits.astype(np.uint32) << np.uint32(16)
    return bits.view(np.float16).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_agrees_with_f32_wide_rows(gpu, kind):
    """cols = 20001: the same keys widened exactly to float32 on the device go
    through kth_select_wide_rows_f32 / kth_topk_wide_rows_f32 -- identical
    columns, values equal to the widened 16-bit outputs."""
    import torch
    cols = 20001
    m = matrix(kind, cols, 0)
    d = m.device()
    flat = d[:m.rows * cols]
    if kind == "bf16":
        wide = ((flat.to(torch.int32) & 0xFFFF) << 16).view(torch.float32)
    else:
        wide = flat.view(torch.float16).to(torch.float32)
    wide = wide.contiguous()
    for k in (1, cols // 2, cols):
        a = Out(m.rows)
        b = torch.full((m.rows,), -1.0, dtype=torch.float32, device="cuda")
        run(gpu, lambda: gpu.rows_wide16(d, m.rows, cols, k, a.t, kind=kind))
        run(gpu, lambda: gpu.rows_wide(wide, m.rows, cols, k, b, f32=True))
        assert np.array_equal(_widen_host(a.get(), kind), b.cpu().numpy().view(np.uint32)), k
    for largest in (False, True):
        for k in (50, cols // 2):
            a_v, a_i = Out(m.rows * k), Out(m.rows * k, True)
            b_v = torch.full((m.rows * k,), -1.0, dtype=torch.float32, device="cuda")
            b_i = torch.full((m.rows * k,), -1, dtype=torch.int32, device="cuda")
            run(gpu, lambda: gpu.topk_rows_wide16(d, m.rows, cols, k, a_v.t, a_i.t, largest=largest, kind=kind))
            run(gpu, lambda: gpu.topk_rows_wide(wide, m.rows, cols, k, b_v, b_i, largest=largest, f32=True))
            assert np.array_equal(a_i.get().view(np.int32), b_i.cpu().numpy()), (k, largest)
            assert np.array_equal(_widen_host(a_v.get(), kind), b_v.cpu().numpy().view(np.uint32)), (k, largest)


# ------------------------------------------------------------------ the workload's shape
def test_logits_shape_bf16(gpu):
    """4 x 128256 bfloat16 randn: the median per row and the top-50 largest."""
    rows, cols = 4, 128256
    x = np.random.default_rng(7).standard_normal((rows, cols)).astype(np.float32)
    m = Matrix("bf16", cols, words=to_kind_bits(x, "bf16"))
    d = m.device()
    check_select(gpu, m, d, (cols // 2,), what="logits")
    check_topk(gpu, m, d, (50,), True, modes=("both",), what="logits")


def test_many_rows_i16(gpu):
    """300 x 32768 int16 uniform, automatic plan: the median per row and the top-64 smallest."""
    rows, cols = 300, 32768
    words = np.random.default_rng(8).integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(np.uint16)
    m = Matrix("i16", cols, words=words)
    d = m.device()
    check_select(gpu, m, d, (cols // 2,), what="many rows")
    check_topk(gpu, m, d, (64,), False, modes=("both",), what="many rows")


# ------------------------------------------------------------------ neighbours
def test_neighbours_on_one_ctx(gpu):
    """An int32 select, a 32-bit wide top-k (3 slices), a 16-bit wide select (3
    slices), a topk16, a fused 16-bit wide top-k and a rows16 call on one ctx, in
    two orders: every result equals that of the call alone on a ctx of its own,
    and the int32 select's stats survive the wide calls."""
    import torch
    import kselect
    n = (1 << 20) + 7
    rng = np.random.default_rng(11)
    arr = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)).cuda()
    arr16 = torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, n, dtype=np.int64).astype(np.int16)).cuda()
    cols = 20001
    m32 = np.random.default_rng(12).standard_normal((6, cols)).astype(np.float32)
    d32 = torch.from_numpy(m32).cuda()
    m = matrix("bf16", cols, 0)
    dw = m.device()
    mr = matrix("f16", 1000, 1)
    dr = mr.device()
    kw = cols // 2

    def forced_call(sel, slices, fn):
        def go():
            sel.wide_rows_force(slices, 0)
            try:
                fn()
            finally:
                sel.wide_rows_force(0, 0)
        return go

    def calls(sel):
        o_sel = torch.full((1,), POISON32, dtype=torch.int32, device="cuda")
        o_tv = torch.full((6 * 64,), -1.0, dtype=torch.float32, device="cuda")
        o_ti = torch.full((6 * 64,), -1, dtype=torch.int32, device="cuda")
        o_ws = Out(m.rows)
        o16v = torch.full((100,), POISON16, dtype=torch.int16, device="cuda")
        o16i = torch.full((100,), -1, dtype=torch.int64, device="cuda")
        o_wv, o_wi = Out(m.rows * 64), Out(m.rows * 64, True)
        o_rows = Out(mr.rows)
        return [
            (lambda: sel.select_async(arr, n, n // 2, o_sel), lambda: [o_sel.cpu().numpy()]),
            (forced_call(sel, 3, lambda: sel.topk_rows_wide(d32, 6, cols, 64, o_tv, o_ti, largest=True, f32=True)),
             lambda: [o_tv.cpu().numpy().view(np.uint32), o_ti.cpu().numpy()]),
            (forced_call(sel, 3, lambda: sel.rows_wide16(dw, m.rows, cols, kw, o_ws.t, kind="bf16")),
             lambda: [o_ws.get()]),
            (lambda: sel.topk16(arr16, n, 100, o16v, o16i), lambda: [o16v.cpu().numpy(), o16i.cpu().numpy()]),
            (forced_call(sel, 1, lambda: sel.topk_rows_wide16(dw, m.rows, cols, 64, o_wv.t, o_wi.t, largest=True,
                                                              kind="bf16")),
             lambda: [o_wv.get(), o_wi.get()]),
            (lambda: sel.rows16(dr, mr.rows, 1000, 500, o_rows.t, kind="f16"), lambda: [o_rows.get()]),
        ]

    TOPK16 = 3  # the call that takes the stats over
    alone = []
    for i in range(6):
        with kselect.Selector(0) as sel:
            call, read = calls(sel)[i]
            run(sel, call)
            alone.append(read())
    # the 16-bit wide results are the reference's, so "alone" is not merely self-consistent
    assert np.array_equal(alone[2][0], m.want_select(kw))
    want_v, want_i = m.want_topk(64, True)
    assert np.array_equal(alone[4][0], want_v.ravel()) and np.array_equal(alone[4][1].view(np.int32), want_i.ravel())
    assert np.array_equal(alone[5][0], mr.want_select(500))
    with kselect.Selector(0) as sel:
        for order in ((0, 1, 2, 3, 4, 5), (4, 2, 1, 0, 2, 1, 4, 5, 3, 2)):
            cs = calls(sel)
            select_last = False  # the int32 select is the last call that owns the stats
            for i in order:
                call, read = cs[i]
                run(sel, call)
                for got, want in zip(read(), alone[i]):
                    assert np.array_equal(got, want), (order, i)
                select_last = i == 0 or (select_last and i != TOPK16)
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


@pytest.mark.parametrize("kind", ["i16", "bf16"])
def test_graph_replay(gpu, kind):
    """After reserve_wide_rows: one 16-bit wide select and one 16-bit wide top-k
    captured at a forced slices = 3 (frozen in the graph), force back to
    automatic, two replays with the key buffer refilled in between, then an
    eager select."""
    cols, kt = 20001, 64
    k = cols // 3
    ma, mb = matrix(kind, cols, 0), Matrix(kind, cols, 0, seed=5)
    rows = ma.rows
    b = Bench()
    g = None
    try:
        d = ma.device()
        o_s, o_v, o_i = Out(rows), Out(rows * kt), Out(rows * kt, True)
        b.sel.reserve_wide_rows(rows, cols)
        b.sel.wide_rows_force(3, 0)
        g = b.capture(lambda: (b.sel.rows_wide16(d, rows, cols, k, o_s.t, kind=kind),
                               b.sel.topk_rows_wide16(d, rows, cols, kt, o_v.t, o_i.t, largest=True, kind=kind)))
        b.sel.wide_rows_force(0, 0)
        for m in (ma, mb):
            d.copy_(m.device())
            for o in (o_s, o_v, o_i):
                o.buf.fill_(o.poison)
            b.replay(g)
            want_v, want_i = m.want_topk(kt, True)
            assert np.array_equal(o_s.get(), m.want_select(k))
            assert np.array_equal(o_v.get(), want_v.ravel()) and np.array_equal(o_i.get().view(np.int32), want_i.ravel())
        o_e = Out(rows)
        b.eager(lambda: b.sel.rows_wide16(d, rows, cols, cols // 2, o_e.t, kind=kind))
        assert np.array_equal(o_e.get(), mb.want_select(cols // 2))
    finally:
        del g
        b.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", KINDS)
def test_bad_arguments(gpu, kind):
    import kselect
    cols = 1000
    m = matrix(kind, cols, 0)
    d = m.device()
    o, v, i = Out(m.rows), Out(m.rows * 4), Out(m.rows * 4, True)
    good_kind = KINDS.index(kind)
    bad = [dict(cols=0), dict(cols=(1 << 24) + 1, ld=(1 << 24) + 1), dict(ld=cols - 1), dict(k=0), dict(k=cols + 1),
           dict(rows=-1), dict(kind=-1), dict(kind=4)]
    for kw in bad:
        a = dict(rows=m.rows, cols=cols, ld=cols, k=4, kind=good_kind)
        a.update(kw)
        with pytest.raises(kselect.KthError) as e:
            gpu.rows_wide16(d, a["rows"], a["cols"], a["k"], o.t, kind=a["kind"], ld=a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
        with pytest.raises(kselect.KthError) as e:
            gpu.topk_rows_wide16(d, a["rows"], a["cols"], a["k"], v.t, i.t, kind=a["kind"], ld=a["ld"])
        assert e.value.code == kselect.KTH_EINVAL, kw
    with pytest.raises(kselect.KthError) as e:
        gpu.topk_rows_wide16(d, m.rows, cols, 4, None, None, kind=kind)
    assert e.value.code == kselect.KTH_EINVAL
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched()
    # rows == 0 is fine and launches nothing
    gpu.rows_wide16(d, 0, cols, 4, o.t, kind=kind)
    gpu.topk_rows_wide16(d, 0, cols, 4, v.t, i.t, kind=kind)
    gpu.sync()
    assert o.untouched() and v.untouched() and i.untouched()
    # and the automatic plan still answers afterwards
    check_select(gpu, m, d, (cols // 2,), what="after errors")
