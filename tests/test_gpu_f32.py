"""GPU: float32 keys through the one-array select and top-k (kth_select_f32*,
kth_topk_f32; include/kth.h "float32 keys").

Everything is compared on bit patterns after turning NaNs into 0x7FC00000.  The
order is restated here as numpy code (_f32_order_key): IEEE total order on the
bits, -0.0 < +0.0, subnormals distinct, every NaN above +inf and equal to every
other NaN.  Expected select: the element whose key is the k-th of the sorted
keys (a[argsort(key, stable)[k - 1]] up to NaN canonicalisation); expected
top-k: sort(argsort(key or ~key, stable)[:k]).
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANON_NAN = 0x7FC00000
NAN_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
NEG0, POS0, PINF, NINF = 0x80000000, 0x00000000, 0x7F800000, 0xFF800000
SMALL_N, RADIX_MAX_N = 16384, 1 << 22  # the library's path thresholds (LDS / radix / window)


def _f32_order_key(bits):
    b = np.asarray(bits, dtype=np.uint32)
    key = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key)


def _bits_of_key(key):
    key = np.asarray(key, dtype=np.uint32)
    b = np.where(key >> 31 != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return np.where(key == np.uint32(0xFFFFFFFF), np.uint32(CANON_NAN), b)


def _canon(bits):
    b = np.asarray(bits, dtype=np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(CANON_NAN), b)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


FAMILIES = ["uniform", "normal_wide", "narrow", "zeros", "specials", "all_equal_3", "all_equal_neg0", "all_equal_nan",
            "ulp_cluster", "sorted_asc", "sorted_desc", "spike"]


@functools.lru_cache(maxsize=4)
def make(family, n):
    """n float32 bit patterns (uint32) of a family, seeded by (family, n)."""
    rng = np.random.default_rng([zlib.crc32(family.encode()), n])
    uni = lambda: _bits(rng.uniform(-1.0, 1.0, n))  # noqa: E731
    if family == "uniform":
        b = uni()
    elif family == "normal_wide":
        b = _bits(rng.standard_normal(n) * 1e20)
    elif family == "narrow":
        b = _bits(rng.standard_normal(4096))[rng.integers(0, 4096, n)]
    elif family == "zeros":
        pool = np.concatenate([np.array([NEG0, POS0, 0x00000001, 0x80000001], dtype=np.uint32),
                               _bits(np.array([1e-30, -1e-30]))])
        b = pool[rng.integers(0, pool.size, n)]
    elif family == "specials":
        b = uni().copy()
        r = rng.random(n)
        for i, pat in enumerate([PINF, NINF, *NAN_BITS.tolist()]):
            b[(r >= 0.01 * i) & (r < 0.01 * (i + 1))] = pat
    elif family == "all_equal_3":
        b = np.full(n, _bits(np.array([3.0]))[0], dtype=np.uint32)
    elif family == "all_equal_neg0":
        b = np.full(n, NEG0, dtype=np.uint32)
    elif family == "all_equal_nan":
        b = NAN_BITS[rng.integers(0, 4, n)]
    elif family == "ulp_cluster":
        b = (np.uint32(0x3F800000) + rng.integers(0, 8, n).astype(np.uint32)).astype(np.uint32)  # 1 + j 2^-23
    elif family == "sorted_asc":
        b = _bits(np.sort(rng.uniform(-1.0, 1.0, n).astype(np.float32)))
    elif family == "sorted_desc":
        b = _bits(np.sort(rng.uniform(-1.0, 1.0, n).astype(np.float32))[::-1])
    elif family == "spike":
        b = uni().copy()
        b[rng.random(n) < 0.3] = _bits(np.array([0.001]))[0]
    else:
        raise KeyError(family)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    b.setflags(write=False)
    return b


def _dev(bits):
    import torch
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32)).cuda()


def _got_bits(x):
    return int(np.float32(x).view(np.uint32))


def _ranks(n, skeys):
    ks = {k for k in (1, 2, n // 2, n - 1, n) if 1 <= k <= n}
    # the last -0.0, the first +0.0, the first +inf and the first NaN, where present
    for bits, last in ((NEG0, True), (POS0, False), (PINF, False), (0x7FC00000, False)):
        key = _f32_order_key(np.array([bits], dtype=np.uint32))[0]
        lo, hi = int(np.searchsorted(skeys, key, "left")), int(np.searchsorted(skeys, key, "right"))
        if hi > lo:
            ks.add(hi if last else lo + 1)
    return sorted(ks)


def _expected_path(n):
    return (1,) if n <= SMALL_N else (2,) if n <= RADIX_MAX_N else (3, 4)


# ------------------------------------------------------------------- paths
PATH_NS = [1, 2, 3, 100, 16384, 16385, 100003, 1 << 22, (1 << 22) + 1, 5_000_008, (1 << 23) + 4096]


@pytest.mark.parametrize("n", PATH_NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_select_every_path(gpu, family, n):
    bits = make(family, n)
    skeys = np.sort(_f32_order_key(bits))
    d = _dev(bits)
    for k in _ranks(n, skeys):
        got = _got_bits(gpu.select(d, k, f32=True))
        want = int(_bits_of_key(skeys[k - 1]))
        assert got == want, (family, n, k, hex(got), hex(want))
        st = gpu.stats()
        assert st["path"] in _expected_path(n) and st["error"] == 0, (family, n, k, st)
        assert st["answer"] & 0xFFFFFFFF == want  # kth_stats.answer: the answer's bits
    assert np.array_equal(_bits(d.cpu().numpy()), bits)  # the input is not modified


# ------------------------------------------------------------- entry forms
@pytest.mark.parametrize("n", [100003, (1 << 22) + 123])
def test_entry_forms_agree(gpu, n):
    import kselect
    bits = make("specials", n)
    host = bits.view(np.float32)
    skeys = np.sort(_f32_order_key(bits))
    d = _dev(bits)
    for k in (1, n // 3, n):
        want = int(_bits_of_key(skeys[k - 1]))
        assert _got_bits(gpu.select(host, k, f32=True)) == want
        assert _got_bits(gpu.select(d, k, f32=True)) == want
        assert _got_bits(kselect.kth_select(host, k, f32=True)) == want
        assert _got_bits(kselect.kth_select(d, k, f32=True)) == want


def test_unaligned_device_pointers(gpu):
    n = (1 << 22) + 123
    base_bits = make("specials", n + 3)
    base = _dev(base_bits)
    for off in (1, 2, 3):
        d = base[off:off + n]
        assert d.data_ptr() % 16 == 4 * off
        skeys = np.sort(_f32_order_key(base_bits[off:off + n]))
        for k in (1, n // 2, n):
            assert _got_bits(gpu.select(d, k, f32=True)) == int(_bits_of_key(skeys[k - 1])), (off, k)


def test_async_four_ranks(gpu):
    import torch
    n = 1 << 24
    bits = make("normal_wide", n)
    d = _dev(bits)
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    ks = (1, 1000, n // 2, n)
    for i, k in enumerate(ks):
        gpu.select_async(d, n, k, out[i:i + 1], f32=True)
    gpu.sync()
    skeys = np.sort(_f32_order_key(bits))
    assert _bits(out.cpu().numpy()).tolist() == [int(_bits_of_key(skeys[k - 1])) for k in ks]
    st = gpu.stats()
    assert st["path"] == 3 and st["error"] == 0 and st["n"] == n and st["k"] == n


# ---------------------------------------------------- fallback, per-level path
def test_window_fallback_is_exact_f32():
    """The sampled chunks all hold one value, so the window misses: the exact
    fallback levels then read the float input (path 4)."""
    import torch

    import kselect
    from kselect._lib import load
    lib = load()
    n = 1 << 24
    d = _dev(make("uniform", n))
    s, c = int(lib.kth_dist_sample_size(n)), int(lib.kth_sample_chunk())
    nch = -(-s // c)
    stride = n // nch
    idx = (torch.arange(nch, device="cuda") * stride).repeat_interleave(c) + torch.arange(c, device="cuda").repeat(nch)
    # (a value inside the keys' range that is the answer for none of the ranks
    # below: a planted maximum would be found by the window itself at k = n)
    d[idx] = 0.25
    skeys = np.sort(_f32_order_key(_bits(d.cpu().numpy())))
    fresh = kselect.Selector(0)
    try:
        for k in (1, n // 2, n):
            assert _got_bits(fresh.select(d, k, f32=True)) == int(_bits_of_key(skeys[k - 1])), k
            assert fresh.stats()["path"] == 4 and fresh.stats()["error"] == 0
    finally:
        fresh.close()


def test_per_level_path_takes_f32():
    """One reported barrier timeout (the software hook, value 2: once) sends the
    synchronous select to the per-level kernels, where the ctx stays for the
    next selections: select and top-k must be exact there too."""
    import torch

    import kselect
    n = (1 << 24) + 3
    bits = make("specials", n)
    key = _f32_order_key(bits)
    skeys = np.sort(key)
    d = _dev(bits)
    sel = kselect.Selector(0)
    sel.test_hook(kselect.KTH_HOOK_FAULT_BARRIER, 2)
    try:
        assert sel.coop()
        assert _got_bits(sel.select(d, n // 2, f32=True)) == int(_bits_of_key(skeys[n // 2 - 1]))
        assert not sel.coop()
        assert _got_bits(sel.select(d, n // 3, f32=True)) == int(_bits_of_key(skeys[n // 3 - 1]))
        assert sel.stats()["error"] == 0
        k = n // 64
        vals = torch.empty(k, dtype=torch.float32, device="cuda")
        idx = torch.empty(k, dtype=torch.int64, device="cuda")
        sel.topk(d, n, k, vals, idx, largest=True, f32=True)
        sel.sync()
        assert not sel.coop() and sel.stats()["error"] == 0
        want = _ref_idx(key, k, True)
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _canon(bits[want]))
    finally:
        sel.close()


# -------------------------------------------------------------------- top-k
def _ref_idx(key, k, largest):
    return np.sort(np.argsort(~key if largest else key, kind="stable")[:k])


def _run_topk(sel, d, n, k, largest):
    import torch
    vals = torch.full((k,), -7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    sel.topk(d, n, k, vals, idx, largest=largest, f32=True)
    sel.sync()
    assert sel.stats()["error"] == 0, (n, k, largest, sel.stats())
    return vals, idx


def _check_topk(sel, d, bits, order, n, k, largest, tag):
    vals, idx = _run_topk(sel, d, n, k, largest)
    want = np.sort(order[:k])
    np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"{tag} n={n} k={k} largest={largest}")
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _canon(bits[want]),
                                  err_msg=f"{tag} n={n} k={k} largest={largest}")


# (`all_equal` is three inputs: 3.0, all -0.0, all NaN)
TOPK_SMALL_FAMS = ["uniform", "zeros", "specials", "all_equal_3", "all_equal_neg0", "all_equal_nan", "sorted_desc"]


@pytest.mark.parametrize("n", [1, 7, 4096, 5000, 100003, (1 << 22) + 5])
@pytest.mark.parametrize("family", TOPK_SMALL_FAMS)
def test_topk_small(gpu, family, n):
    bits = make(family, n)
    key = _f32_order_key(bits)
    d = _dev(bits)
    for largest in (False, True):
        order = np.argsort(~key if largest else key, kind="stable")
        for k in sorted({k for k in (1, 2, 64, n // 2, n - 1, n) if 1 <= k <= n}):
            _check_topk(gpu, d, bits, order, n, k, largest, family)


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("family", ["uniform", "narrow", "specials", "spike", "sorted_asc"])
def test_topk_window_path(gpu, family, largest):
    """Every top-k variant of the streaming pass the dispatch reaches for
    float32 keys: flag bytes (small k), row words (the rest, the staged range
    n / 65536 < k <= n / 16 included)."""
    n = (1 << 23) + 4099
    bits = make(family, n)
    key = _f32_order_key(bits)
    d = _dev(bits)
    assert d.data_ptr() % 16 == 0
    order = np.argsort(~key if largest else key, kind="stable")
    for k in (1, 37, n // 65536 + 1, n // 1024, n // 1024 + 1, n // 64, n // 16, n // 16 + 1, n // 3, n - 5):
        _check_topk(gpu, d, bits, order, n, k, largest, family)


def test_topk_unaligned(gpu):
    n = (1 << 23) + 3
    base_bits = make("specials", n + 3)
    base = _dev(base_bits)
    for off in (1, 3):
        d = base[off:off + n]
        bits = base_bits[off:off + n]
        key = _f32_order_key(bits)
        for largest in (False, True):
            order = np.argsort(~key if largest else key, kind="stable")
            for k in (1, 100, 8191):
                _check_topk(gpu, d, bits, order, n, k, largest, f"off={off}")


def test_topk_values_only_indices_only_and_errors(gpu):
    import torch

    import kselect
    n, k = 100003, 777
    bits = make("specials", n)
    key = _f32_order_key(bits)
    d = _dev(bits)
    want = _ref_idx(key, k, True)
    vals = torch.empty(k, dtype=torch.float32, device="cuda")
    idx = torch.empty(k, dtype=torch.int64, device="cuda")
    gpu.topk(d, n, k, d_vals=vals, largest=True, f32=True)
    gpu.topk(d, n, k, d_idx=idx, largest=True, f32=True)
    gpu.sync()
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _canon(bits[want]))
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    for bad_k in (0, n + 1):
        with pytest.raises(kselect.KthError) as e:
            gpu.topk(d, n, bad_k, vals, idx, f32=True)
        assert e.value.code == kselect.KTH_EINVAL
    with pytest.raises(kselect.KthError) as e:
        gpu.topk(d, n, k, None, None, f32=True)
    assert e.value.code == kselect.KTH_EINVAL
    with pytest.raises(kselect.KthError) as e:
        gpu.select(d, n + 1, f32=True)
    assert e.value.code == kselect.KTH_EINVAL
    with pytest.raises(TypeError, match="float32"):
        gpu.topk(d.view(torch.int32), n, k, vals, idx, f32=True)
    # the C entry points on a real ctx (tests/test_abi_f32.py can only pass a NULL ctx):
    # NULL keys / outputs, n < 1, k < 1, k > n are refused and nothing is written
    lib, ctx = kselect.LIB, gpu.handle
    out = torch.full((1,), -7.0, dtype=torch.float32, device="cuda")
    host_out = ctypes.c_float(-7.0)
    dp, op, vp, ip = d.data_ptr(), out.data_ptr(), vals.data_ptr(), idx.data_ptr()
    vals.fill_(-7.0)
    idx.fill_(-1)
    for keys_p, nn, kk in ((None, n, 1), (dp, 0, 1), (dp, -1, 1), (dp, n, 0), (dp, n, -1), (dp, n, n + 1)):
        assert lib.kth_select_f32_ctx(ctx, keys_p, nn, kk, ctypes.byref(host_out)) == kselect.KTH_EINVAL, (nn, kk)
        assert lib.kth_select_f32_async(ctx, keys_p, nn, kk, op) == kselect.KTH_EINVAL, (nn, kk)
        assert lib.kth_topk_f32(ctx, keys_p, nn, kk, 0, vp, ip) == kselect.KTH_EINVAL, (nn, kk)
        assert lib.kth_select_f32(keys_p, nn, kk, ctypes.byref(host_out)) == kselect.KTH_EINVAL, (nn, kk)
    assert lib.kth_select_f32_ctx(ctx, dp, n, 1, None) == kselect.KTH_EINVAL
    assert lib.kth_select_f32_async(ctx, dp, n, 1, None) == kselect.KTH_EINVAL
    assert lib.kth_select_f32(dp, n, 1, None) == kselect.KTH_EINVAL
    assert lib.kth_topk_f32(ctx, dp, n, 1, 0, None, None) == kselect.KTH_EINVAL
    gpu.sync()
    assert host_out.value == -7.0 and float(out[0]) == -7.0
    assert bool((vals == -7.0).all()) and bool((idx == -1).all())


# ---------------------------------------------------------------- full size
def _ordered_i32(t):
    """torch: float32 tensor -> the ordered int32 words (NaN -> INT32_MAX), integer ops only."""
    import torch
    b = t.view(torch.int32)
    s = torch.where(b < 0, b ^ 0x7FFFFFFF, b)
    return torch.where((b & 0x7FFFFFFF) > 0x7F800000, torch.full_like(b, 0x7FFFFFFF), s)


def _ordered_of_bits(bits):
    b = bits & 0xFFFFFFFF
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0x7FFFFFFF
    s = b ^ 0x7FFFFFFF if b >> 31 else b
    return s - (1 << 32) if s >> 31 else s


@pytest.fixture(scope="module")
def full_size():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1 << 28
    g = torch.Generator(device="cuda")
    g.manual_seed(0xF32)
    d = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    plant = torch.tensor([POS0, NEG0, PINF, NINF, 0x7FC00000, 0xFFC00000], dtype=torch.int64)
    plant = torch.where(plant >= 1 << 31, plant - (1 << 32), plant).to(torch.int32).cuda()
    at = torch.arange(1000, device="cuda") * (n // 1000) + 7
    d.view(torch.int32)[at] = plant[torch.arange(1000, device="cuda") % plant.numel()]
    s = _ordered_i32(d)
    yield n, d, s
    del d, s
    torch.cuda.empty_cache()


def test_full_size_select_rank_certificate(gpu, full_size):
    n, d, s = full_size
    for k in (1, n // 2, n):
        v = _ordered_of_bits(_got_bits(gpu.select(d, k, f32=True)))
        lt, le = int((s < v).sum()), int((s <= v).sum())
        assert lt < k <= le, (k, v, lt, le)
        assert gpu.stats()["error"] == 0
    assert _ordered_of_bits(_got_bits(gpu.select(d, n, f32=True))) == 0x7FFFFFFF  # the planted NaNs are last


@pytest.mark.parametrize("largest", [False, True])
def test_full_size_topk_properties(gpu, full_size, largest):
    import torch
    n, d, s = full_size
    k = 1 << 20
    vals, idx = _run_topk(gpu, d, n, k, largest)
    idx_c = idx.cpu().numpy()
    assert np.all(np.diff(idx_c) > 0) and idx_c[0] >= 0 and idx_c[-1] < n
    vv = _ordered_i32(vals)
    assert torch.equal(vv, s[idx])  # the kept values are the input's, as keys (NaNs canonical)
    assert np.array_equal(_bits(vals.cpu().numpy()), _canon(_bits(d[idx].cpu().numpy())))
    v = _ordered_of_bits(_got_bits(gpu.select(d, n - k + 1 if largest else k, f32=True)))
    sgn = -1 if largest else 1
    dd, vv, v = s.to(torch.int64) * sgn, vv.to(torch.int64) * sgn, v * sgn
    assert int(vv.max()) == v  # the k-th is kept, nothing beyond it
    n_better = int((dd < v).sum())
    assert int((vv < v).sum()) == n_better  # every strictly better key is kept
    ties = torch.nonzero(dd == v).flatten()[: k - n_better].cpu().numpy()  # the first ties by index
    np.testing.assert_array_equal(idx_c[(vv == v).cpu().numpy()], ties)


# ------------------------------------------------- int32 results are unchanged
@pytest.mark.parametrize("family", ["uniform_full", "few_distinct", "sorted_desc"])
def test_int32_results_unchanged(gpu, family):
    import torch
    n = (1 << 24) + 5
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.fill(d, n, family, param=7)
    gpu.sync()
    host = d.cpu().numpy()
    srt = np.sort(host)
    for k in (1, n // 2, n):
        assert gpu.select(d, k) == srt[k - 1], (family, k)
    k = n // 64
    vals = torch.empty(k, dtype=torch.int32, device="cuda")
    idx = torch.empty(k, dtype=torch.int64, device="cuda")
    gpu.topk(d, n, k, vals, idx)
    gpu.sync()
    assert gpu.stats()["error"] == 0
    want = np.sort(np.argsort(host, kind="stable")[:k])
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(vals.cpu().numpy(), host[want])
