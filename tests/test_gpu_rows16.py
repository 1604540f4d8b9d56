"""GPU checks of the 16-bit rows calls (include/kth.h "16-bit rows",
csrc/kth_rows16.hpp).  The reference is numpy's stable argsort of the
documented order keys, restated here; outputs are compared as exact bits, a
canonical NaN expected wherever the reference key is 0xFFFF for a float kind.
Inputs are uint16 bit patterns, moved to the device as int16 views with kind=
given."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("i16", "u16", "f16", "bf16")
INF = {"f16": 0x7C00, "bf16": 0x7F80}
CANON = {"f16": 0x7E00, "bf16": 0x7FC0}
ROWS = 67  # not a multiple of the four rows of a workgroup
SELECT_COLS = (1, 7, 8, 63, 64, 65, 512, 520, 1000, 1024, 2048, 4093, 4096, 5000, 8192)
TOPK_SHAPES = ((7, 3), (64, 8), (256, 8), (512, 1), (1000, 7), (4096, 1), (4096, 64), (4096, 4096), (4093, 4092),
               (8192, 100), (8192, 8192))


def rule_key(bits, kind):
    """The documented order as uint16 keys (tests/test_abi_k16.py's rule_key, restated)."""
    b = np.asarray(bits, dtype=np.uint16)
    if kind == "i16":
        return b ^ np.uint16(0x8000)
    if kind == "u16":
        return b.copy()
    key = np.where(b >> 15 != 0, ~b, b | np.uint16(0x8000)).astype(np.uint16)
    return np.where((b & np.uint16(0x7FFF)) > np.uint16(INF[kind]), np.uint16(0xFFFF), key)


def canon(bits, keys, kind):
    """bits with every NaN of a float kind replaced by the canonical one."""
    if kind not in CANON:
        return bits
    return np.where(keys == np.uint16(0xFFFF), np.uint16(CANON[kind]), bits)


def to_kind_bits(x, kind):
    """float32 values rounded to the kind, as bits (float kinds only)."""
    if kind == "f16":
        return x.astype(np.float16).view(np.uint16)
    w = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even


def make_rows(kind, cols, seed=0):
    """ROWS rows of `cols` bit patterns: the fixed special rows, then random
    patterns over all 65536 values (NaNs of both signs, infinities, subnormals)."""
    rng = np.random.default_rng(1000 * cols + seed + KINDS.index(kind))
    rnd = lambda: rng.integers(0, 1 << 16, cols, dtype=np.uint32).astype(np.uint16)  # noqa: E731
    rows = [np.full(cols, v, dtype=np.uint16) for v in (0x0000, 0x8000, 0x7FFF, 0xFFFF)]  # all equal
    rows.append(np.where(rng.integers(0, 2, cols) != 0, 0x3C01, 0x3C00).astype(np.uint16))  # differ in bit 0
    rows.append(np.where(rng.integers(0, 2, cols) != 0, 0x3D80, 0x3C80).astype(np.uint16))  # differ only in bit 8
    rows.append((rnd() & np.uint16(0x00FF)) | np.uint16(0xBE00))  # constant high byte, random low byte
    rows.append((rnd() & np.uint16(0xFF00)) | np.uint16(0x005A))  # random high byte, constant low byte
    rows.append(np.where(np.arange(cols) % 2 == 0, 0x8000, 0x0000).astype(np.uint16))  # -0.0 / +0.0 alternating
    inf = INF.get(kind, 0x7F80)
    nan = (rnd() % np.uint16(0x7FFF - inf)) + np.uint16(inf + 1)  # every payload ...
    rows.append(nan | (rnd() & np.uint16(0x8000)))                 # ... of either sign
    if kind in INF:
        rows.append(to_kind_bits(rng.standard_normal(cols).astype(np.float32), kind))
    r = rnd()
    asc = r[np.argsort(rule_key(r, kind), kind="stable")]
    rows.append(asc)
    rows.append(asc[::-1].copy())
    while len(rows) < ROWS:
        rows.append(rnd())
    return np.ascontiguousarray(np.stack(rows), dtype=np.uint16)


class Case:
    """A matrix: its bits, its order keys, and the stable argsorts (ascending;
    descending with ties by column) every test of this (kind, cols) shares."""

    def __init__(self, kind, cols):
        self.kind, self.cols = kind, cols
        self.bits = make_rows(kind, cols)
        self.bits.setflags(write=False)
        self.keys = rule_key(self.bits, kind)
        self.asc = np.argsort(self.keys, axis=1, kind="stable")
        self.desc = np.argsort(~self.keys, axis=1, kind="stable")

    def want_select(self, k):
        col = self.asc[:, k - 1:k]
        return canon(np.take_along_axis(self.bits, col, 1), np.take_along_axis(self.keys, col, 1), self.kind)[:, 0]

    def want_topk(self, k, largest):
        idx = np.sort((self.desc if largest else self.asc)[:, :k], axis=1)
        vals = canon(np.take_along_axis(self.bits, idx, 1), np.take_along_axis(self.keys, idx, 1), self.kind)
        return vals, idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(kind, cols):
    return Case(kind, cols)


def to_dev(bits, off=0):
    """The bits as an int16 device tensor starting `off` elements past a 16-byte boundary."""
    import torch
    flat = np.ascontiguousarray(bits).reshape(-1)
    base = torch.zeros(flat.size + 16, dtype=torch.int16, device="cuda")
    dev = base[off:off + flat.size]
    dev.copy_(torch.from_numpy(flat.view(np.int16).copy()))
    assert dev.data_ptr() % 16 == (2 * off) % 16
    return dev


def out16(n, off=0, poison=0x5A5A):
    import torch
    base = torch.full((n + 16,), poison, dtype=torch.int16, device="cuda")
    out = base[off:off + n]
    assert out.data_ptr() % 16 == (2 * off) % 16
    return out


def ready():
    """Inputs and poisoned outputs are built on torch's stream and the selector
    runs on its own: finish the former before a call is enqueued on the latter."""
    import torch
    torch.cuda.synchronize()


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def select_ks(cols):
    return sorted({k for k in (1, 2, min(64, cols), (cols + 1) // 2, cols - 1, cols) if 1 <= k <= cols})


def check_select(gpu, c, dev, rows, ks, out_off=0):
    for k in ks:
        out = out16(rows, out_off)
        ready()
        gpu.rows16(dev, rows, c.cols, k, out, kind=c.kind)
        gpu.sync()
        got, want = host16(out), c.want_select(k)[:rows]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (c.kind, c.cols, k, [(int(r), hex(int(got[r])), hex(int(want[r]))) for r in bad[:5]])


def check_topk(gpu, c, dev, k, largest, with_vals=True, with_idx=True, out_off=0):
    import torch
    rows = c.bits.shape[0]
    vals = out16(rows * k, out_off) if with_vals else None
    idx = torch.full((rows * k,), -1, dtype=torch.int32, device="cuda") if with_idx else None
    ready()
    gpu.topk_rows16(dev, rows, c.cols, k, vals, idx, largest=largest, kind=c.kind)
    gpu.sync()
    want_vals, want_idx = c.want_topk(k, largest)
    if with_idx:
        got = idx.cpu().numpy().reshape(rows, k)
        assert got.min() >= 0 and got.max() < c.cols  # never a padded column
        bad = np.nonzero((got != want_idx).any(axis=1))[0]
        assert bad.size == 0, (c.kind, c.cols, k, largest, [(int(r), got[r][:8], want_idx[r][:8]) for r in bad[:3]])
    if with_vals:
        got = host16(vals).reshape(rows, k)
        bad = np.nonzero((got != want_vals).any(axis=1))[0]
        assert bad.size == 0, (c.kind, c.cols, k, largest, [(int(r), got[r][:8], want_vals[r][:8]) for r in bad[:3]])


@pytest.mark.parametrize("cols", SELECT_COLS)
@pytest.mark.parametrize("kind", KINDS)
def test_select_every_kind_and_width(gpu, kind, cols):
    c = case(kind, cols)
    check_select(gpu, c, to_dev(c.bits), ROWS, select_ks(cols))


@pytest.mark.parametrize("kind", KINDS)
def test_select_unaligned(gpu, kind):
    """The guarded load path: a base 2 bytes off 16-byte alignment (every row
    misaligned), cols = 4093 from an aligned base (most rows misaligned), and
    d_out starting at an odd element."""
    c = case(kind, 4096)
    check_select(gpu, c, to_dev(c.bits, off=1), ROWS, (1, 64, 2048, 4096), out_off=1)
    c = case(kind, 4093)
    check_select(gpu, c, to_dev(c.bits), ROWS, (1, 64, 2047, 4093), out_off=1)
    c = case(kind, 4096)
    check_select(gpu, c, to_dev(c.bits), ROWS, (64,), out_off=1)  # the 16-byte path with an odd d_out


@pytest.mark.parametrize("largest", (False, True))
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_topk_every_kind_and_shape(gpu, kind, shape, largest):
    cols, k = shape
    c = case(kind, cols)
    check_topk(gpu, c, to_dev(c.bits), k, largest)


@pytest.mark.parametrize("kind", KINDS)
def test_topk_one_output_and_unaligned(gpu, kind):
    c = case(kind, 4096)
    dev = to_dev(c.bits)
    check_topk(gpu, c, dev, 64, True, with_vals=False)
    check_topk(gpu, c, dev, 64, False, with_idx=False)
    check_topk(gpu, c, dev, 65, True, out_off=1)           # d_vals at an odd element
    check_topk(gpu, c, to_dev(c.bits, off=1), 64, True, out_off=1)  # a base 2 bytes off alignment
    check_topk(gpu, c, to_dev(c.bits, off=1), 2000, False)          # ... past what the LDS stages


def test_topk_never_emits_a_padded_column(gpu):
    """uint16 rows holding 0xFFFF with cols = 4093: the padding has the value of
    real keys (and, flipped for largest, of the smallest key 0x0000)."""
    c = case("u16", 4093)
    assert (c.bits == 0xFFFF).all(axis=1).any() and (c.bits == 0x0000).all(axis=1).any()
    dev = to_dev(c.bits)
    for k in (1, 5, 4092, 4093):
        for largest in (False, True):
            check_topk(gpu, c, dev, k, largest)


@pytest.mark.parametrize("what", ("select", "topk_smallest", "topk_largest"))
def test_many_rows(gpu, what):
    """1048579 x 64 int16, k = 8: a grid far larger than the device, the last
    workgroup partly idle.  Checked on the device with integer compares of
    order keys: #(key < v) < k <= #(key <= v), and for top-k the kept columns
    against the mask the k-th value and the tie rule define."""
    import torch
    rows, cols, k = 1048579, 64, 8
    g = torch.Generator(device="cuda").manual_seed(16)
    # few values per row: ties at the k-th key are the rule, not the exception
    keys = torch.randint(-40, 40, (rows, cols), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    keys[-1] = torch.arange(cols, dtype=torch.int16, device="cuda") - 32768  # the last row, alone in its workgroup
    largest = what == "topk_largest"
    o = -keys.int() if largest else keys.int()  # ascends in the selection order
    if what == "select":
        out = torch.full((rows,), 0x5A5A, dtype=torch.int16, device="cuda")
        ready()
        gpu.rows16(keys, rows, cols, k, out)
        gpu.sync()
        v = out.int()[:, None]
    else:
        vals = torch.full((rows, k), 0x5A5A, dtype=torch.int16, device="cuda")
        idx = torch.full((rows, k), -1, dtype=torch.int32, device="cuda")
        ready()
        gpu.topk_rows16(keys, rows, cols, k, vals, idx, largest=largest)
        gpu.sync()
        assert int(idx.min()) >= 0 and int(idx.max()) < cols
        assert bool((idx[:, 1:] > idx[:, :-1]).all())  # column order, no column twice
        assert bool((torch.gather(keys, 1, idx.long()) == vals).all())
        ov = -vals.int() if largest else vals.int()
        v = ov.max(dim=1, keepdim=True).values  # the k-th in the selection order
    lt = (o < v).sum(dim=1)
    le = (o <= v).sum(dim=1)
    assert bool(((lt < k) & (le >= k)).all())  # the rank certificate
    if what != "select":
        eq = o == v
        keep = (o < v) | (eq & (torch.cumsum(eq.int(), dim=1) <= (k - lt)[:, None]))
        assert bool((keep.sum(dim=1) == k).all())
        want = keep.nonzero()[:, 1].reshape(rows, k).int()
        assert bool((want == idx).all())


def test_errors(gpu):
    import torch

    import kselect
    keys = torch.zeros(4 * 8200, dtype=torch.int16, device="cuda")
    out = torch.full((64,), 0x5A5A, dtype=torch.int16, device="cuda")
    idx = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    ready()
    bad = ((8193, 1, "i16"), (8, 0, "i16"), (8, 9, "i16"), (8, 1, 4), (8, 1, -1), (0, 1, "bf16"))
    for cols, k, kind in bad:
        with pytest.raises(kselect.KthError) as e:
            gpu.rows16(keys, 4, cols, k, out, kind=kind)
        assert e.value.code == kselect.KTH_EINVAL, (cols, k, kind)
        with pytest.raises(kselect.KthError) as e:
            gpu.topk_rows16(keys, 4, cols, k, out, idx, kind=kind)
        assert e.value.code == kselect.KTH_EINVAL, (cols, k, kind)
    with pytest.raises(kselect.KthError) as e:
        gpu.topk_rows16(keys, 4, 8, 1, None, None, kind="i16")
    assert e.value.code == kselect.KTH_EINVAL
    with pytest.raises(kselect.KthError) as e:
        gpu.rows16(keys, -1, 8, 1, out, kind="i16")
    assert e.value.code == kselect.KTH_EINVAL
    # rows == 0: KTH_OK, nothing launched, the poison stays
    gpu.rows16(keys, 0, 8, 1, out, kind="i16")
    gpu.topk_rows16(keys, 0, 8, 1, out, idx, kind="i16")
    gpu.sync()
    assert bool((out == 0x5A5A).all()) and bool((idx == -1).all())


def test_neighbours_on_one_ctx(gpu):
    """A one-array select, then rows16, then the same select: the rows call
    uses no ctx scratch, so the answers around it agree."""
    c = case("bf16", 4096)
    dev = to_dev(c.bits)
    n = c.bits.size
    ks = [1, n // 3, n // 2, n]
    ready()
    before = gpu.select16_multi(dev, ks, n=n, kind="bf16")
    check_select(gpu, c, dev, ROWS, (64, 2048))
    after = gpu.select16_multi(dev, ks, n=n, kind="bf16")
    flat_keys = np.sort(rule_key(c.bits.reshape(-1), "bf16"))
    want = flat_keys[np.asarray(ks) - 1]
    for got in (before, after):
        bits = (got.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        assert (rule_key(bits, "bf16") == want).all()
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
