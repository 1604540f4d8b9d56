"""GPU: several ranks of one array in one call (kth_select_multi_*; include/kth.h
"several ranks of one array").

Every answer is compared with the host-sorted array's element and with the
single select of the same rank; float32 keys are compared on bit patterns
after turning NaNs into 0x7FC00000, in the order restated as numpy code below
(as tests/test_gpu_f32.py does).
"""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANON_NAN = 0x7FC00000
NAN_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
NEG0, POS0, PINF, NINF = 0x80000000, 0x00000000, 0x7F800000, 0xFF800000
SMALL_N, RADIX_MAX_N = 16384, 1 << 22  # the library's path thresholds (LDS / radix / window)

I32_FAMILIES = ["uniform_full", "all_equal", "few_distinct", "sorted_asc", "sorted_desc", "mod_1000"]
F32_FAMILIES = ["specials", "zeros", "all_equal_nan", "spike"]
PATH_NS = [1, 100, 16385, 100003, 1 << 22, (1 << 22) + 1, 5_000_008, (1 << 23) + 4096]


def _f32_order_key(bits):
    b = np.asarray(bits, dtype=np.uint32)
    key = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key)


def _bits_of_key(key):
    key = np.asarray(key, dtype=np.uint32)
    b = np.where(key >> 31 != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return np.where(key == np.uint32(0xFFFFFFFF), np.uint32(CANON_NAN), b)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=2)
def make_f32(family, n):
    """n float32 bit patterns (uint32) of a family, seeded by (family, n)."""
    rng = np.random.default_rng([zlib.crc32(family.encode()), n])
    uni = lambda: _bits(rng.uniform(-1.0, 1.0, n))  # noqa: E731
    if family == "uniform":
        b = uni()
    elif family == "zeros":
        pool = np.concatenate([np.array([NEG0, POS0, 0x00000001, 0x80000001], dtype=np.uint32),
                               _bits(np.array([1e-30, -1e-30]))])
        b = pool[rng.integers(0, pool.size, n)]
    elif family == "specials":
        b = uni().copy()
        r = rng.random(n)
        for i, pat in enumerate([PINF, NINF, *NAN_BITS.tolist()]):
            b[(r >= 0.01 * i) & (r < 0.01 * (i + 1))] = pat
    elif family == "all_equal_nan":
        b = NAN_BITS[rng.integers(0, 4, n)]
    elif family == "spike":
        b = uni().copy()
        b[rng.random(n) < 0.3] = _bits(np.array([0.001]))[0]
    else:
        raise KeyError(family)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    b.setflags(write=False)
    return b


def _dev_f32(bits):
    import torch
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32)).cuda()


def _dev_i32(sel, family, n):
    import torch
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    sel.fill(d, n, family)
    sel.sync()
    return d


def rank_lists(n):
    clip = lambda ks: [min(max(int(k), 1), n) for k in ks]  # noqa: E731
    return [clip(ks) for ks in ([n // 2], [1, n], [n // 2, n // 2 + 1, n // 2],
                                [n, 1, n // 4, 3 * n // 4, n // 2, n // 100 + 1, n - n // 100, 2])]


def _expected_path(n):
    return (1,) if n <= SMALL_N else (2,) if n <= RADIX_MAX_N else (3, 4)


class I32:
    """int32 keys: the device tensor, the sorted host copy, answers as ints."""
    f32 = False

    def __init__(self, d):
        self.d = d
        self.host = np.ascontiguousarray(d.cpu().numpy())
        self.sorted = np.sort(self.host)

    def want(self, k):
        return int(self.sorted[k - 1])

    @staticmethod
    def got(x):
        return int(x)

    def unchanged(self):
        return np.array_equal(self.d.cpu().numpy(), self.host)


class F32:
    """float32 keys: answers as bit patterns, NaNs canonical."""
    f32 = True

    def __init__(self, d):
        self.d = d
        self.host = _bits(d.cpu().numpy()).copy()
        self.sorted = np.sort(_f32_order_key(self.host))

    def want(self, k):
        return int(_bits_of_key(self.sorted[k - 1]))

    @staticmethod
    def got(x):
        return int(np.float32(x).view(np.uint32))

    def unchanged(self):
        return np.array_equal(_bits(self.d.cpu().numpy()), self.host)


def _check_multi(sel, data, n, ks, tag, paths=None):
    """One multi call: exact, equal to the single selects, clean stats."""
    out = sel.select_multi(data.d, ks, n=n, f32=data.f32)
    assert out.dtype == (np.float32 if data.f32 else np.int32) and out.shape == (len(ks),)
    got = [data.got(x) for x in out]
    assert got == [data.want(k) for k in ks], (tag, n, ks, got)
    stats = [sel.multi_stats(i) for i in range(len(ks))]
    for i, (k, st) in enumerate(zip(ks, stats)):
        assert st["error"] == 0 and st["n"] == n and st["k"] == k, (tag, n, ks, i, st)
        assert st["path"] in (paths or _expected_path(n)), (tag, n, ks, i, st)
    assert sel.stats() == stats[-1]  # kth_ctx_last_stats: the last rank's
    for k, g in zip(ks, got):
        assert data.got(sel.select(data.d, k, n=n, f32=data.f32)) == g, (tag, n, k)
    return stats


# ------------------------------------------------------------------- paths
@pytest.mark.parametrize("n", PATH_NS)
@pytest.mark.parametrize("family", I32_FAMILIES)
def test_multi_every_path_i32(gpu, family, n):
    data = I32(_dev_i32(gpu, family, n))
    for ks in rank_lists(n):
        stats = _check_multi(gpu, data, n, ks, family)
        if family == "uniform_full" and n > RADIX_MAX_N:
            assert [st["path"] for st in stats] == [3] * len(ks), (n, ks, stats)
    assert data.unchanged()


@pytest.mark.parametrize("n", PATH_NS)
@pytest.mark.parametrize("family", F32_FAMILIES)
def test_multi_every_path_f32(gpu, family, n):
    data = F32(_dev_f32(make_f32(family, n)))
    for ks in rank_lists(n):
        _check_multi(gpu, data, n, ks, family)
    assert data.unchanged()


# ------------------------------------------------------------- entry forms
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n", [100003, (1 << 22) + 123])
def test_entry_forms_agree(gpu, n, f32):
    import torch

    import kselect
    data = F32(_dev_f32(make_f32("specials", n))) if f32 else I32(_dev_i32(gpu, "uniform_full", n))
    host = data.host.view(np.float32) if f32 else data.host
    ks = rank_lists(n)[3] + [n // 3, n // 2]  # ten ranks: the wrappers send two groups
    want = [data.want(k) for k in ks]
    bits = lambda out: [data.got(x) for x in out]  # noqa: E731
    assert bits(gpu.select_multi(host, ks, f32=f32)) == want
    assert bits(gpu.select_multi(data.d, ks, f32=f32)) == want
    assert bits(kselect.kth_select_multi(host, ks, f32=f32)) == want
    assert bits(kselect.kth_select_multi(data.d, ks, f32=f32)) == want
    out = torch.zeros(len(ks), dtype=torch.float32 if f32 else torch.int32, device="cuda")
    gpu.reserve_multi(n, len(ks))
    gpu.select_multi_async(data.d, n, ks, out, f32=f32)
    gpu.sync()
    assert bits(out.cpu().numpy()) == want
    assert gpu.multi_stats(1)["k"] == ks[9] and gpu.multi_stats(1)["error"] == 0  # the second group's
    with pytest.raises(kselect.KthError) as e:
        gpu.select_multi(data.d, [1, n + 1], f32=f32)
    assert e.value.code == kselect.KTH_EINVAL


@pytest.mark.parametrize("f32", [False, True])
def test_unaligned_device_pointers(gpu, f32):
    n = (1 << 22) + 123
    base = _dev_f32(make_f32("specials", n + 3)) if f32 else _dev_i32(gpu, "uniform_full", n + 3)
    for off in (1, 2, 3):
        d = base[off:off + n]
        assert d.data_ptr() % 16 == 4 * off
        data = (F32 if f32 else I32)(d)
        ks = rank_lists(n)[3]
        got = [data.got(x) for x in gpu.select_multi(d, ks, n=n, f32=f32)]
        assert got == [data.want(k) for k in ks], (off, got)
        assert all(gpu.multi_stats(i)["error"] == 0 for i in range(len(ks)))


# --------------------------------------------------------------- one pass
def test_eight_ranks_are_one_streaming_launch():
    """With timing on, an eight-rank call on the window path is ONE select with
    one timed streaming launch."""
    import kselect
    n = (1 << 23) + 4096
    sel = kselect.Selector(0)
    try:
        data = I32(_dev_i32(sel, "uniform_full", n))
        ks = rank_lists(n)[3]
        sel.reserve_multi(n, len(ks))
        sel.enable_timing(True)
        sel.take_timing()
        got = [int(x) for x in sel.select_multi(data.d, ks)]
        nsel, main_ms, total_ms = sel.take_timing()
        assert got == [data.want(k) for k in ks]
        assert nsel == 1 and main_ms > 0 and total_ms >= main_ms, (nsel, main_ms, total_ms)
    finally:
        sel.close()


# ------------------------------------------------------------ fallbacks
def _sampled_index(n):
    """Indices of the keys the sample phase reads (kth_sample_chunk's layout)."""
    import torch

    from kselect._lib import load
    lib = load()
    s, c = int(lib.kth_dist_sample_size(n)), int(lib.kth_sample_chunk())
    nch = -(-s // c)
    stride = n // nch
    return (torch.arange(nch, device="cuda") * stride).repeat_interleave(c) + torch.arange(c, device="cuda").repeat(nch)


def test_one_rank_falls_back_the_others_do_not():
    """Off the sampled chunks, every key of the central fifth of the int32 range
    is squeezed into [-2^20, 2^20): the sample shows no cluster, so the
    median's window (about 1 % of the range) holds ~3 M keys, over the 2^20
    capacity, and that rank takes the exact fallback; the outer ranks' windows
    are untouched."""
    import torch

    import kselect
    n = 1 << 24
    sel = kselect.Selector(0)
    try:
        d = _dev_i32(sel, "uniform_full", n)
        free = torch.ones(n, dtype=torch.bool, device="cuda")
        free[_sampled_index(n)] = False
        band = (1 << 32) // 10  # the central fifth: |v| < 2^32 / 10
        inside = free & (d > -band) & (d < band)
        d = torch.where(inside, torch.remainder(d, 1 << 21) - (1 << 20), d).contiguous()
        assert int(inside.sum()) > (1 << 21)
        data = I32(d)
        assert data.got(sel.select(d, n // 2)) == data.want(n // 2) and sel.stats()["path"] == 4
        assert data.got(sel.select(d, n // 100)) == data.want(n // 100) and sel.stats()["path"] == 3
        ks = [n // 100, n // 2, n - n // 100]
        got = [int(x) for x in sel.select_multi(d, ks)]
        stats = [sel.multi_stats(i) for i in range(3)]
        assert got == [data.want(k) for k in ks], got
        assert [st["path"] for st in stats] == [3, 4, 3], stats
        assert [st["error"] for st in stats] == [0, 0, 0], stats
        assert data.unchanged()
    finally:
        sel.close()


@pytest.mark.parametrize("f32", [False, True])
def test_window_miss_is_exact_for_every_rank(f32):
    """The sampled chunks all hold one value, so every rank's window misses:
    each takes the exact fallback over the input (path 4)."""
    import kselect
    n = 1 << 24
    sel = kselect.Selector(0)
    try:
        d = _dev_f32(make_f32("uniform", n)) if f32 else _dev_i32(sel, "uniform_full", n)
        # (a value inside the keys' range that is the answer for none of the ranks below)
        d[_sampled_index(n)] = 0.25 if f32 else 123456789
        data = (F32 if f32 else I32)(d)
        ks = [1, n // 2, n]
        got = [data.got(x) for x in sel.select_multi(d, ks, f32=f32)]
        assert got == [data.want(k) for k in ks], got
        for i in range(3):
            st = sel.multi_stats(i)
            assert st["path"] == 4 and st["error"] == 0, (i, st)
    finally:
        sel.close()


def test_per_level_path_takes_multi():
    """One reported barrier timeout (the software hook, value 2: once) sends the
    synchronous multi call to the per-level kernels, where the ctx stays: that
    call and the next are exact there."""
    import kselect
    n = (1 << 24) + 3
    sel = kselect.Selector(0)
    sel.test_hook(kselect.KTH_HOOK_FAULT_BARRIER, 2)
    try:
        data = I32(_dev_i32(sel, "uniform_full", n))
        assert sel.coop()
        ks = [n // 4, n // 2, 3 * n // 4, n]
        assert [int(x) for x in sel.select_multi(data.d, ks)] == [data.want(k) for k in ks]
        assert not sel.coop()
        assert all(sel.multi_stats(i)["error"] == 0 for i in range(4))
        ks = [1, n // 3, n // 3, n - 1]
        assert [int(x) for x in sel.select_multi(data.d, ks)] == [data.want(k) for k in ks]
        assert not sel.coop()
        assert all(sel.multi_stats(i)["error"] == 0 and sel.multi_stats(i)["k"] == ks[i] for i in range(4))
    finally:
        sel.close()
