"""GPU checks of the 16-bit one-array select (include/kth.h "16-bit keys",
csrc/kth_k16.hpp).  The expected value is always the numpy restatement: the
bits of sort(order_key(a))[k - 1] mapped back, compared on bit patterns."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("i16", "u16", "f16", "bf16")
KIND_ID = {"i16": 0, "u16": 1, "f16": 2, "bf16": 3}
INF = {"f16": 0x7C00, "bf16": 0x7F80}
CANON = {"f16": 0x7E00, "bf16": 0x7FC0}
SMALL_N = 32768  # csrc/kth_k16.hpp K16_SMALL_N: at most this many keys take the full-histogram path
SIZES = (1, 2, 7, 8, 9, 63, 65, 1000, 4093, SMALL_N - 1, SMALL_N, SMALL_N + 1, 65536, (1 << 18) + 3, (1 << 20) + 5,
         (1 << 22) + 5)


def order_key(bits, kind):
    b = np.asarray(bits, dtype=np.uint16)
    if kind == "i16":
        return b ^ np.uint16(0x8000)
    if kind == "u16":
        return b.copy()
    key = np.where(b >> 15 != 0, ~b, b | np.uint16(0x8000)).astype(np.uint16)
    return np.where((b & np.uint16(0x7FFF)) > np.uint16(INF[kind]), np.uint16(0xFFFF), key)


def of_order_key(key, kind):
    key = np.asarray(key, dtype=np.uint16)
    if kind == "i16":
        return key ^ np.uint16(0x8000)
    if kind == "u16":
        return key.copy()
    b = np.where(key >> 15 != 0, key & np.uint16(0x7FFF), ~key).astype(np.uint16)
    return np.where(key == np.uint16(0xFFFF), np.uint16(CANON[kind]), b)


class Data:
    """An input: its bits on the host, on the device (an int16 tensor holding
    the same bytes, `off` elements past a 16-byte boundary), its sorted order keys."""

    def __init__(self, bits, kind, off=0):
        import torch
        self.bits = np.ascontiguousarray(bits, dtype=np.uint16)
        self.kind = kind
        self.n = self.bits.size
        base = torch.zeros(self.n + 16, dtype=torch.int16, device="cuda")
        self.dev = base[off:off + self.n]
        self.dev.copy_(torch.from_numpy(self.bits.view(np.int16)))
        assert self.dev.data_ptr() % 16 == (2 * off) % 16
        self.sorted_keys = np.sort(order_key(self.bits, kind))

    def want(self, ks):
        return of_order_key(self.sorted_keys[np.asarray(ks, dtype=np.int64) - 1], self.kind)

    def ranks(self):
        """{1, 2, n/2, n-1, n} and, where present, the last -0.0, the first +0.0, the first +inf, the first NaN."""
        n = self.n
        ks = {1, 2, n // 2, n - 1, n}
        if self.kind in INF:
            for key, side in ((0x7FFF, "right"), (0x8000, "left"), (0x8000 | INF[self.kind], "left"), (0xFFFF, "left")):
                i = int(np.searchsorted(self.sorted_keys, np.uint16(key), side=side))
                k = i if side == "right" else i + 1
                if 1 <= k <= n and self.sorted_keys[k - 1] == key:
                    ks.add(k)
        return sorted(k for k in ks if 1 <= k <= n)


def to_bits(vals, kind):
    vals = np.asarray(vals)
    if kind == "bf16":
        w = vals.view(np.uint32)
        assert not (w & np.uint32(0xFFFF)).any()
        return (w >> np.uint32(16)).astype(np.uint16)
    return vals.view(np.uint16)


def select(sel, d, ks):
    """The ranks ks through Selector.select16_multi (groups of 8) as bits."""
    return to_bits(sel.select16_multi(d.dev, list(ks), n=d.n, kind=d.kind), d.kind)


def check(sel, d, ks, what=""):
    got, want = select(sel, d, ks), d.want(ks)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, d.kind, d.n, [(int(ks[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def randn_bits(rng, n, kind):
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "f16":
        return x.astype(np.float16).view(np.uint16)
    if kind == "bf16":
        return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    if kind == "u16":  # centred in the unsigned range (int16 bits read as uint16 would be bimodal)
        return np.clip(x * 8192 + 32768, 0, 65535).astype(np.uint16)
    return np.clip(x * 8192, -32768, 32767).astype(np.int16).view(np.uint16)


def family(name, n, kind, seed=1):
    rng = np.random.default_rng([seed, n, KIND_ID[kind]])
    uni = rng.integers(0, 1 << 16, size=n, dtype=np.uint32).astype(np.uint16)
    ordinary = np.uint16(0x3C00 if kind in INF else 0x1234)
    if name == "uniform":
        return uni
    if name == "randn":
        return randn_bits(rng, n, kind)
    if name == "all_equal":
        return np.full(n, ordinary, dtype=np.uint16)
    if name == "all_neg_zero":
        return np.full(n, 0x8000, dtype=np.uint16)
    if name == "all_nan":  # NaNs of both signs and several payloads (integer kinds: just four values)
        inf = INF.get(kind, 0x7C00)
        return rng.choice(np.array([inf + 1, inf + 0x23, 0x8000 | (inf + 1), 0xFFFF, 0x7FFF], dtype=np.uint16), size=n)
    if name == "two_bit0":
        return np.where(uni & 1, ordinary, ordinary ^ np.uint16(1)).astype(np.uint16)
    if name == "two_top_byte":
        return np.where(uni & 1, np.uint16(0x1234), np.uint16(0xC234)).astype(np.uint16)
    if name == "four":
        return np.array([0x0001, 0x8001, 0x3C00, 0xBC00], dtype=np.uint16)[uni & 3]
    if name in ("sorted_asc", "sorted_desc"):
        keys = np.sort(order_key(randn_bits(rng, n, kind), kind))
        return of_order_key(keys if name == "sorted_asc" else keys[::-1], kind)
    if name == "spike":
        return np.where(rng.random(n) < 0.3, ordinary, uni).astype(np.uint16)
    if name == "specials":
        inf = INF.get(kind, 0x7C00)
        sp = np.array([inf, 0x8000 | inf, inf + 1, 0x8000 | (inf + 1), inf + 0x55, 0xFFFF, 0x7FFF, 0x0001, 0x8001,
                       0x0000, 0x8000, 0x003F, 0x803F], dtype=np.uint16)
        out = randn_bits(rng, n, kind)
        pick = rng.random(n) < 0.01 * sp.size
        out[pick] = rng.choice(sp, size=int(pick.sum()))
        return out
    raise KeyError(name)


@pytest.mark.parametrize("kind", KINDS)
def test_sizes_uniform_and_randn(gpu, kind):
    for n in SIZES:
        for fam in ("uniform", "randn"):
            d = Data(family(fam, n, kind), kind)
            check(gpu, d, d.ranks(), fam)


def test_one_large_case(gpu):
    d = Data(family("randn", (1 << 24) + 5, "bf16"), "bf16")
    check(gpu, d, d.ranks(), "large")


@pytest.mark.parametrize("kind", KINDS)
def test_every_pattern_once(gpu, kind):
    """All 65536 patterns, permuted: pins the whole transform on the device."""
    rng = np.random.default_rng(65536)
    d = Data(rng.permutation(1 << 16).astype(np.uint16), kind)
    ks = sorted(set([1, d.n] + [int(x) for x in np.linspace(1, d.n, 33)]))
    check(gpu, d, ks, "patterns")
    # ... and through the streaming path: every pattern 17 times
    d = Data(rng.permutation(np.tile(np.arange(1 << 16, dtype=np.uint16), 17)), kind)
    ks = sorted(set([1, d.n] + [int(x) for x in np.linspace(1, d.n, 33)]))
    check(gpu, d, ks, "patterns x 17")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (4093, (1 << 18) + 3))
def test_duplicate_heavy_and_ordered_families(gpu, kind, n):
    for fam in ("all_equal", "all_neg_zero", "all_nan", "two_bit0", "two_top_byte", "four", "sorted_asc", "sorted_desc",
                "spike", "specials"):
        d = Data(family(fam, n, kind), kind)
        check(gpu, d, d.ranks(), fam)


@pytest.mark.parametrize("off", (0, 1, 3, 4, 7))
def test_alignment_heads_and_tails(gpu, off):
    """n = 2^18 + {0..8} at a pointer `off` elements past a 16-byte boundary:
    the head is (8 - off) % 8 keys, and the nine sizes give every tail 0..7."""
    tails = set()
    for extra in range(9):
        n = (1 << 18) + extra
        tails.add((n - (8 - off) % 8) % 8)
        for kind in ("bf16", "i16"):
            d = Data(family("specials", n, kind, seed=off), kind, off=off)
            check(gpu, d, d.ranks(), f"off {off}")
    assert tails == set(range(8))


def _fresh():
    import kselect
    return kselect.Selector(0)


@pytest.mark.parametrize("kind", KINDS)
def test_paths_and_the_miss_hook(kind):
    """randn keys above the threshold settle in the one streaming pass.  (The
    float kinds' median window spans the patterns around zero: at this n the
    sample is 16384 keys, the window about |x| < 0.05, ~21800 float16 patterns.
    Its ends are exact over 8192 patterns = 8 binades each, which leaves
    |x| < ~2e-4 to the coarse middle: ~1.6e-4 of the keys against a rank
    uncertainty of 4e-3.  bfloat16's ends are 64 binades: no key is left.)  With
    KTH_HOOK_K16_MISS the window holds nothing, the later passes produce the
    same bits and the path says so."""
    import kselect
    sel = _fresh()
    n = (1 << 20) + 5
    d = Data(family("randn", n, kind), kind)
    for k in (n // 4, n // 2, n - n // 4, 1, n):
        want = d.want([k])[0]
        assert select(sel, d, [k])[0] == want
        st = sel.stats()
        assert st["path"] == kselect.KTH_PATH_K16 and st["error"] == 0 and st["answer"] & 0xFFFF == want, (k, st)
        assert st["cnt_lt"] < k <= st["cnt_lt"] + st["candidates"], (k, st)
        lo, hi = st["lo_key"], st["hi_key"]
        assert st["cnt_lt"] == int(np.searchsorted(d.sorted_keys, np.uint16(lo), side="left")), (k, st)
        assert lo <= int(order_key([want], kind)[0]) <= hi, (k, st)
        sel.test_hook(kselect.KTH_HOOK_K16_MISS, 1)
        assert select(sel, d, [k])[0] == want
        st = sel.stats()
        assert st["path"] == kselect.KTH_PATH_K16_FALLBACK and st["error"] == 0 and st["answer"] & 0xFFFF == want, (k, st)
        sel.test_hook(kselect.KTH_HOOK_K16_MISS, 0)
    # below the threshold the full histogram decides, hook or not
    d = Data(family("randn", SMALL_N, kind), kind)
    sel.test_hook(kselect.KTH_HOOK_K16_MISS, 1)
    check(sel, d, d.ranks(), "small")
    assert sel.stats()["path"] == kselect.KTH_PATH_K16
    sel.close()


def test_wide_window_with_a_crowded_middle_stays_exact():
    """The sampled chunks (1024 consecutive keys, n / ceil(s / 1024) apart, s =
    kth_dist_sample_size(n)) hold only -1.0 and +1.0, every other key is a
    uniformly random pattern: the median's window spans [-1, +1], ~30000
    patterns, far more than the exact bins at its ends, and the median lies in
    the coarse middle.  The second pass settles it exactly."""
    import kselect
    sel = _fresh()
    n = (1 << 22) + 5
    rng = np.random.default_rng(22)
    bits = rng.integers(0, 1 << 16, size=n, dtype=np.uint32).astype(np.uint16)
    s = kselect.LIB.kth_dist_sample_size(n)
    nchunks = -(-s // 1024)
    stride = n // nchunks
    for c in range(nchunks):
        bits[c * stride:c * stride + 1024] = np.where(rng.random(1024) < 0.5, 0x3C00, 0xBC00)
    d = Data(bits, "f16")
    for ks in ([n // 2], [n // 2, 1, n, n // 3, 2 * n // 3, n // 2 + 1, 7, n - 7]):
        check(sel, d, ks, "wide")
    st = sel.multi_stats(0)
    assert st["path"] == kselect.KTH_PATH_K16_FALLBACK and st["error"] == 0, st
    sel.close()


@pytest.mark.parametrize("kind", ("bf16", "u16"))
@pytest.mark.parametrize("n", (SMALL_N, (1 << 20) + 5))
def test_multi(kind, n):
    import kselect
    sel = _fresh()
    d = Data(family("specials", n, kind), kind)
    single = {}
    for m in (2, 4, 8):
        ks = [int(x) for x in np.linspace(n, 1, m)]  # descending: unsorted for the call
        ks[-1] = ks[0]  # a duplicate rank
        ks[1] = max(1, n // 2)
        out = np.full(m, 0xAAAA, dtype=np.uint16)
        arr = (ctypes.c_int64 * m)(*ks)
        assert kselect.LIB.kth_select_multi_k16_ctx(sel.handle, d.dev.data_ptr(), n, arr, m, KIND_ID[kind],
                                                    out.ctypes.data) == 0
        assert np.array_equal(out, d.want(ks)), (m, ks)
        for i, k in enumerate(ks):
            if k not in single:
                single[k] = select(sel, d, [k])[0]
            assert out[i] == single[k]
    # nine ranks: Python groups them
    ks = [int(x) for x in np.linspace(1, n, 9)]
    check(sel, d, ks, "nine")
    # every rank forced to miss: each one's stats
    sel.test_hook(kselect.KTH_HOOK_K16_MISS, 1)
    ks = [n, 1, n // 2, n // 3]
    check(sel, d, ks, "miss")
    for i, k in enumerate(ks):
        st = sel.multi_stats(i)
        assert st["k"] == k and st["n"] == n and st["error"] == 0 and st["answer"] & 0xFFFF == d.want([k])[0], st
        assert st["path"] == (kselect.KTH_PATH_K16 if n <= SMALL_N else kselect.KTH_PATH_K16_FALLBACK), st
    sel.close()


def test_async_on_a_torch_stream():
    import torch

    import kselect
    stream = torch.cuda.Stream()
    sel = kselect.Selector(0, stream=stream)
    n = (1 << 20) + 5
    x = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    keys = x.to(torch.bfloat16)
    torch.cuda.synchronize()
    bits = keys.view(torch.int16).cpu().numpy().view(np.uint16)
    sk = np.sort(order_key(bits, "bf16"))
    sel.reserve16(n, 4)
    out1 = torch.zeros(1, dtype=torch.bfloat16, device="cuda")
    out4 = torch.zeros(4, dtype=torch.bfloat16, device="cuda")
    ks = [n // 4, n // 2, n, n // 4]
    with torch.cuda.stream(stream):
        sel.select16_async(keys, n, n // 2, out1)
        sel.select16_multi_async(keys, n, ks, out4)
    stream.synchronize()
    assert out1.view(torch.int16).cpu().numpy().view(np.uint16)[0] == of_order_key(sk[n // 2 - 1], "bf16")
    assert np.array_equal(out4.view(torch.int16).cpu().numpy().view(np.uint16),
                          of_order_key(sk[np.array(ks) - 1], "bf16"))
    # the dtype decides the kind: the same bits as float16 keys
    half = keys.view(torch.float16)
    got = sel.select16(half, n // 2)
    assert got.dtype == np.float16
    assert got.view(np.uint16) == of_order_key(np.sort(order_key(bits, "f16"))[n // 2 - 1], "f16")
    sel.close()


def test_host_keys_one_shot_and_input_untouched(gpu):
    import kselect
    n = (1 << 18) + 3
    for kind in KINDS:
        bits = family("specials", n, kind)
        d = Data(bits, kind)
        before = d.dev.clone()
        check(gpu, d, d.ranks(), "device")
        assert bool((before == d.dev).all())
        host = bits.copy()
        arr = host.view(np.int16) if kind == "i16" else host.view(np.float16) if kind == "f16" else host
        k = n // 3
        got = kselect.kth_select16(arr, k, kind=kind)
        assert to_bits(np.array([got]), kind)[0] == d.want([k])[0]
        got = kselect.kth_select16_multi(arr, [k, 1, n], kind=kind)
        assert np.array_equal(to_bits(got, kind), d.want([k, 1, n]))
        assert np.array_equal(host, bits)


def test_argument_checks_on_a_real_ctx(gpu):
    import kselect
    lib = kselect.LIB
    d = Data(family("uniform", 1000, "u16"), "u16")
    out = np.full(8, 0xAAAA, dtype=np.uint16)
    p, o, h = d.dev.data_ptr(), out.ctypes.data, gpu.handle
    E = kselect.KTH_EINVAL
    for n, k, kind in ((0, 1, 1), (1000, 0, 1), (1000, 1001, 1), (1000, 1, 4), (1000, 1, -1)):
        assert lib.kth_select_k16_ctx(h, p, n, k, kind, o) == E
        assert lib.kth_select_k16_async(h, p, n, k, kind, o) == E
    assert lib.kth_select_k16_ctx(h, None, 1000, 1, 1, o) == E
    assert lib.kth_select_k16_ctx(h, p, 1000, 1, 1, None) == E
    ks = (ctypes.c_int64 * 9)(*range(1, 10))
    assert lib.kth_select_multi_k16_ctx(h, p, 1000, ks, 0, 1, o) == E
    assert lib.kth_select_multi_k16_ctx(h, p, 1000, ks, 9, 1, o) == E
    bad = (ctypes.c_int64 * 3)(1, 1001, 2)
    assert lib.kth_select_multi_k16_ctx(h, p, 1000, bad, 3, 1, o) == E
    assert lib.kth_select_multi_k16_async(h, p, 1000, bad, 3, 1, o) == E
    assert lib.kth_ctx_reserve_k16(h, 1000, 0) == E and lib.kth_ctx_reserve_k16(h, 1000, 9) == E
    assert (out == 0xAAAA).all()
    assert lib.kth_ctx_test_hook(h, kselect.KTH_HOOK_K16_MISS, -1) == E


def test_timing_counts_one_select():
    sel = _fresh()
    n = (1 << 20) + 5
    d = Data(family("randn", n, "bf16"), "bf16")
    sel.enable_timing(True)
    select(sel, d, [n // 2])
    select(sel, d, [1, n // 2, n])
    cnt, main_ms, total_ms = sel.take_timing()
    assert cnt == 2 and 0 < main_ms <= total_ms
    sel.close()


FLUSH_N = (1 << 25) + 5


@pytest.mark.parametrize("fam,kind", (("all_equal", "i16"), ("two_bit0", "i16"), ("randn", "bf16")))
def test_field_flush_between_tiles(monkeypatch, fam, kind):
    """The 16-bit LDS fields of k16_main are swapped out by a wave once it has
    added K16_WAVE_BUDGET = 12000 keys to a window (checked after each tile; a
    wave adds at most 4096 keys a tile).  With one workgroup a CU (256 on an
    MI355X, 16384 keys a tile) 2^25 keys are eight tiles a workgroup, so on an
    input whose keys all lie in the window every wave flushes after its third
    and sixth tile and carries its counts from tile to tile; without the flush
    a field would reach 8 * 4096 * 4 = 131072 and carry into its neighbour.
    all-equal and two values: every key is in the sample window (leader adds,
    a flush of one or two words).  KTH_HOOK_K16_MISS: the second pass's window
    is the whole key range in the coarse layout; randn keys then take the
    one-add-a-lane path and the whole-range flush.  Several ranks share the LDS."""
    import kselect
    monkeypatch.setenv("KTH_MAIN_WG_PER_CU", "1")
    import torch
    sel = kselect.Selector(0)
    n = FLUSH_N
    # (one workgroup a CU, 16384 keys a tile: at least four tiles a workgroup, so the budget is passed)
    assert n // 16384 // torch.cuda.get_device_properties(0).multi_processor_count >= 4
    d = Data(family(fam, n, kind), kind)
    ks = [1, n // 2, n]
    for hook in (0, 1):
        sel.test_hook(kselect.KTH_HOOK_K16_MISS, hook)
        for k in ks:
            check(sel, d, [k], f"{fam} hook {hook}")
            st = sel.stats()
            assert st["error"] == 0 and st["path"] == (kselect.KTH_PATH_K16_FALLBACK if hook else kselect.KTH_PATH_K16), st
            assert st["cnt_lt"] < k <= st["cnt_lt"] + st["candidates"], st
        check(sel, d, [n // 4, n // 2, n - n // 4, n - n // 100], f"{fam} multi hook {hook}")
    if fam != "randn":  # the first pass counted every key inside the window, exactly
        sel.test_hook(kselect.KTH_HOOK_K16_MISS, 0)
        check(sel, d, [n // 2])
        st = sel.stats()
        assert st["cnt_lt"] == 0 and st["candidates"] == n, st
    sel.close()
