"""GPU checks of the 16-bit one-array top-k (include/kth.h "top-k of one array,
16-bit keys", csrc/kth_topk16.hpp).  The expected result is the numpy
restatement: the order keys of the bits (0xFFFF - key for largest), a stable
argsort's first k re-sorted into index order, the values of_order_key of the
kept keys (so a NaN is canonical); compared on bit patterns."""
import types

import numpy as np
import pytest

import test_gpu_k16 as k16t
from test_gpu_k16 import Data, family, of_order_key, order_key

pytestmark = pytest.mark.gpu

KINDS = k16t.KINDS
SMALL_N = k16t.SMALL_N
TILE = 2048  # csrc/kth_topk16.hpp TK16_TILE
SIZES = (1, 7, 8, 9, TILE - 1, TILE, TILE + 1, SMALL_N - 1, SMALL_N, SMALL_N + 1, 65536, (1 << 18) + 3)
# 2^23 + 2053: two k_topk_bases workgroups (4096 tiles x 2048 keys) plus a partial tile
LARGE_SIZES = ((1 << 22) + 5, (1 << 23) + 2053)
FAMILIES = ("uniform", "randn", "all_equal", "all_nan", "all_neg_zero", "two_bit0", "four", "sorted_asc", "sorted_desc",
            "spike", "specials")
SENT_V, SENT_I = 0x5A5A, -7


class Ref:
    """The restatement of one input and direction: the stable order once, any k from it."""

    def __init__(self, d, largest):
        key = order_key(d.bits, d.kind)
        self.key = (np.uint16(0xFFFF) - key) if largest else key
        self.order = np.argsort(self.key, kind="stable")
        self.canon = of_order_key(key, d.kind)

    def want(self, k):
        idx = np.sort(self.order[:k])
        return self.canon[idx], idx.astype(np.int64)


def run(sel, d, k, largest, vals=True, idx=True):
    import torch
    v = torch.full((k,), SENT_V, dtype=torch.int16, device="cuda") if vals else None
    i = torch.full((k,), SENT_I, dtype=torch.int64, device="cuda") if idx else None
    torch.cuda.synchronize()  # the sentinels are filled on torch's stream, the call runs on the ctx's
    sel.topk16(d.dev, d.n, k, v, i, largest=largest, kind=d.kind)
    sel.sync()
    return (v.cpu().numpy().view(np.uint16) if vals else None), (i.cpu().numpy() if idx else None)


def check(sel, d, ref, k, largest, what="", vals=True, idx=True):
    got_v, got_i = run(sel, d, k, largest, vals, idx)
    want_v, want_i = ref.want(k)
    tag = (what, d.kind, d.n, k, largest)
    if idx:
        np.testing.assert_array_equal(got_i, want_i, err_msg=str(tag))
    if vals:
        np.testing.assert_array_equal(got_v, want_v, err_msg=str(tag))
    return got_v, got_i


def ranks(n):
    return sorted(k for k in {1, 2, 64, n // 2, n - 1, n} if 1 <= k <= n)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_kinds_directions_ranks(gpu, kind, fam):
    for n in SIZES:
        d = Data(family(fam, n, kind), kind)
        for largest in (False, True):
            ref = Ref(d, largest)
            for k in ranks(n):
                check(gpu, d, ref, k, largest, fam)


@pytest.mark.parametrize("fam", ("randn", "spike"))
@pytest.mark.parametrize("kind", KINDS)
def test_large_sizes(gpu, kind, fam):
    for n in LARGE_SIZES:
        d = Data(family(fam, n, kind), kind)
        for largest in (False, True):
            ref = Ref(d, largest)
            for k in ranks(n):
                check(gpu, d, ref, k, largest, fam)


@pytest.mark.parametrize("kind", KINDS)
def test_tie_quota_keeps_the_first_by_index(gpu, kind):
    n = (1 << 18) + 3
    d = Data(family("all_equal", n, kind), kind)
    k = n // 3
    for largest in (False, True):
        _, idx = check(gpu, d, Ref(d, largest), k, largest, "all_equal")
        np.testing.assert_array_equal(idx, np.arange(k, dtype=np.int64))
    # two values; k cuts through the second value's group (in the call's direction)
    d = Data(family("two_bit0", n, kind), kind)
    key = order_key(d.bits, kind)
    for largest in (False, True):
        first = key.max() if largest else key.min()
        n_first = int((key == first).sum())
        k = n_first + (n - n_first) // 2
        vals, idx = check(gpu, d, Ref(d, largest), k, largest, "two_bit0")
        second = np.nonzero(key != first)[0]
        np.testing.assert_array_equal(idx[key[idx] != first], second[: k - n_first])


@pytest.mark.parametrize("off", (1, 3, 7))
def test_alignment_and_null_outputs(gpu, off):
    """Keys `off` elements past a 16-byte boundary; values only, indices only, both."""
    n = 300001
    for kind in ("bf16", "u16"):
        d = Data(family("specials", n, kind, seed=off), kind, off=off)
        for largest in (False, True):
            ref = Ref(d, largest)
            for k in (1, 64, n // 2, n):
                check(gpu, d, ref, k, largest, f"off {off}")
                check(gpu, d, ref, k, largest, f"off {off} vals", idx=False)
                check(gpu, d, ref, k, largest, f"off {off} idx", vals=False)


def _fresh():
    import kselect
    return kselect.Selector(0)


@pytest.mark.parametrize("kind,fam", (("bf16", "randn"), ("i16", "uniform")))
def test_skipping_tiles_the_select_proved_empty(kind, fam):
    """k <= n / 16384: the streaming pass records which rows can hold output
    and the count pass loads only those.  Same results as with the flags
    ignored (KTH_HOOK_K16_TOPK_NOSKIP), which reads every tile, as k = n // 2
    does; a window that holds no key (KTH_HOOK_K16_MISS) stays exact."""
    import kselect
    sel = _fresh()
    n = (1 << 22) + 5
    for off in (0, 3):
        d = Data(family(fam, n, kind, seed=5 + off), kind, off=off)
        for largest in (False, True):
            ref = Ref(d, largest)
            for k in (1, 64, 200):
                got = check(sel, d, ref, k, largest, "skip")
                tiles, read = sel.topk16_tiles()
                assert tiles == (n + off + TILE - 1) // TILE and 0 < read < tiles, (k, largest, off, tiles, read)
                assert sel.stats()["path"] in (kselect.KTH_PATH_K16, kselect.KTH_PATH_K16_FALLBACK)
                sel.test_hook(kselect.KTH_HOOK_K16_TOPK_NOSKIP, 1)
                ref_run = check(sel, d, ref, k, largest, "noskip")
                assert sel.topk16_tiles() == (tiles, tiles)
                sel.test_hook(kselect.KTH_HOOK_K16_TOPK_NOSKIP, 0)
                np.testing.assert_array_equal(got[0], ref_run[0])
                np.testing.assert_array_equal(got[1], ref_run[1])
                sel.test_hook(kselect.KTH_HOOK_K16_MISS, 1)
                check(sel, d, ref, k, largest, "miss")
                assert sel.stats()["path"] == kselect.KTH_PATH_K16_FALLBACK
                sel.test_hook(kselect.KTH_HOOK_K16_MISS, 0)
            check(sel, d, ref, n // 2, largest, "half")
            tiles, read = sel.topk16_tiles()
            assert read == tiles
    sel.close()


def test_interleaved_calls_leave_the_scratch_clean():
    """topk16, select16_multi of 4 ranks, the int32 top-k, topk16 of another kind and n, on one ctx."""
    import torch
    sel = _fresh()
    n = (1 << 20) + 11
    d = Data(family("specials", n, "bf16"), "bf16")
    check(sel, d, Ref(d, True), 100, True, "first")
    k16t.check(sel, d, [1, n // 3, n // 2, n], "multi")
    a = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, size=1 << 18, dtype=np.int64).astype(np.int32)
    t = torch.from_numpy(a).cuda()
    vals = torch.empty(500, dtype=torch.int32, device="cuda")
    idx = torch.empty(500, dtype=torch.int64, device="cuda")
    sel.topk(t, a.size, 500, vals, idx)
    sel.sync()
    want = np.sort(np.argsort(a, kind="stable")[:500])
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(vals.cpu().numpy(), a[want])
    d2 = Data(family("spike", (1 << 19) + 77, "i16"), "i16", off=1)
    for largest in (False, True):
        ref = Ref(d2, largest)
        check(sel, d2, ref, 20, largest, "second")
        check(sel, d2, ref, d2.n // 2, largest, "second")
    check(sel, d, Ref(d, False), n // 5, False, "third")
    sel.close()


def test_argument_errors(gpu):
    import torch

    import kselect
    d = torch.zeros(16, dtype=torch.int16, device="cuda")
    v = torch.zeros(16, dtype=torch.int16, device="cuda")
    i = torch.zeros(16, dtype=torch.int64, device="cuda")
    for n, k in ((10, 0), (10, 11), (0, 1)):
        with pytest.raises(kselect.KthError) as e:
            gpu.topk16(d, n, k, v, i)
        assert e.value.code == kselect.KTH_EINVAL
    with pytest.raises(kselect.KthError) as e:
        gpu.topk16(d, 10, 1, None, None)
    assert e.value.code == kselect.KTH_EINVAL


def test_rank_fault_hook_reports_the_bracket_failure():
    """With KTH_HOOK_FAULT_TOPK_RANK the call selects a neighbouring rank; the
    keys are distinct (a uint16 permutation), so that is another value and the
    counts cannot bracket k: error 32, outputs untouched, the ctx usable after."""
    import kselect
    sel = _fresh()
    n = 40000
    assert n > SMALL_N
    d = Data(np.random.default_rng(9).permutation(n).astype(np.uint16), "u16")
    for largest in (False, True):
        ref = Ref(d, largest)
        for k in (1, 100, n // 2, n):
            sel.test_hook(kselect.KTH_HOOK_FAULT_TOPK_RANK, 1)
            vals, idx = run(sel, d, k, largest)
            assert sel.stats()["error"] == 32, (k, largest)
            assert (vals == SENT_V).all() and (idx == SENT_I).all(), (k, largest)
            sel.test_hook(kselect.KTH_HOOK_FAULT_TOPK_RANK, 0)
            check(sel, d, ref, k, largest, "after the fault hook")
            assert sel.stats()["error"] == 0
    sel.close()


def test_full_size_properties(gpu):
    """2^28 bfloat16 randn keys made on the device, largest: the properties that
    pin the exact top-k, all compares on integer order keys on the device."""
    import torch
    n = 1 << 28
    g = torch.Generator(device="cuda")
    g.manual_seed(28)
    keys = torch.randn(n, dtype=torch.float32, device="cuda", generator=g).to(torch.bfloat16)
    keys[12345] = float("nan")
    keys[n - 7] = -float("nan")

    def okey(x):  # int32 order keys of bfloat16 / int16 words
        b = x.view(torch.int16).to(torch.int32) & 0xFFFF
        key = torch.where(b >> 15 != 0, ~b & 0xFFFF, b | 0x8000)
        return torch.where((b & 0x7FFF) > 0x7F80, torch.full_like(key, 0xFFFF), key)

    dk = 0xFFFF - okey(keys)  # largest: smaller is better
    d = types.SimpleNamespace(dev=keys.view(torch.int16), n=n, kind="bf16")
    for k in (1000, 1 << 20):
        vals = torch.full((k,), SENT_V, dtype=torch.int16, device="cuda")
        idx = torch.full((k,), SENT_I, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu.topk16(keys, n, k, vals.view(torch.bfloat16), idx, largest=True)
        gpu.sync()
        assert bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < n
        picked = keys[idx].view(torch.int16)
        nan = (picked.to(torch.int32) & 0x7FFF) > 0x7F80
        assert torch.equal(vals, torch.where(nan, torch.full_like(picked, 0x7FC0), picked))
        kth_bits = int(k16t.select(gpu, d, [n - k + 1])[0])
        v = 0xFFFF - int(order_key([kth_bits], "bf16")[0])
        vv = 0xFFFF - okey(vals)
        assert int(vv.max()) == v  # the k-th is kept, nothing beyond it
        n_better = int((dk < v).sum())
        assert int((vv < v).sum()) == n_better  # every strictly better key is kept
        ties = torch.nonzero(dk == v).flatten()[: k - n_better]
        assert torch.equal(idx[vv == v], ties)  # the ties kept are the first by index
