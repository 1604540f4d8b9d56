"""CPU checks of the 16-bit one-array entry points (include/kth.h "16-bit
keys"): the order-key helpers against the documented rule over every pattern,
the argument checks that precede any device work, the Python wrappers' dtype
check, and header / exports / PROTOS agreement."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"i16": 0, "u16": 1, "f16": 2, "bf16": 3}
INF = {"f16": 0x7C00, "bf16": 0x7F80}
CANON = {"f16": 0x7E00, "bf16": 0x7FC0}
NAMES = ("kth_k16_order_key", "kth_k16_of_order_key", "kth_select_k16", "kth_select_k16_ctx", "kth_select_k16_async",
         "kth_select_multi_k16", "kth_select_multi_k16_ctx", "kth_select_multi_k16_async", "kth_ctx_reserve_k16")
ALL = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def rule_key(bits, kind):
    """The documented order as uint16 keys."""
    b = np.asarray(bits, dtype=np.uint16)
    if kind == "i16":
        return b ^ np.uint16(0x8000)
    if kind == "u16":
        return b.copy()
    key = np.where(b >> 15 != 0, ~b, b | np.uint16(0x8000)).astype(np.uint16)
    return np.where((b & np.uint16(0x7FFF)) > np.uint16(INF[kind]), np.uint16(0xFFFF), key)


def widen(bits, kind):
    """The non-NaN patterns of a float kind as float64 values."""
    if kind == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def lib_keys(lib, kind):
    return np.array([lib.kth_k16_order_key(int(b), KINDS[kind]) for b in ALL], dtype=np.uint16)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_order_key_is_the_documented_rule_over_every_pattern(lib, kind):
    got, want = lib_keys(lib, kind), rule_key(ALL, kind)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(ALL[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_round_trip_over_every_pattern(lib, kind):
    keys = lib_keys(lib, kind)
    back = np.array([lib.kth_k16_of_order_key(int(k), KINDS[kind]) for k in keys], dtype=np.uint16)
    if kind in INF:
        nan = (ALL & np.uint16(0x7FFF)) > np.uint16(INF[kind])
        assert nan.sum() == 2 * (0x7FFF - INF[kind])
        want = np.where(nan, np.uint16(CANON[kind]), ALL)
        assert lib.kth_k16_of_order_key(0xFFFF, KINDS[kind]) == CANON[kind]
        # no non-NaN pattern has the NaNs' key; the largest other key is +inf's
        assert not (keys[~nan] == 0xFFFF).any() and int(keys[~nan].max()) == (0x8000 | INF[kind])
    else:
        want = ALL
        assert np.unique(keys).size == 1 << 16
    bad = np.nonzero(back != want)[0]
    assert bad.size == 0, [(hex(int(ALL[i])), hex(int(back[i]))) for i in bad[:5]]


@pytest.mark.parametrize("kind", ("f16", "bf16"))
def test_key_order_is_numeric_order(lib, kind):
    keys = lib_keys(lib, kind)
    nan = (ALL & np.uint16(0x7FFF)) > np.uint16(INF[kind])
    bits, k = ALL[~nan], keys[~nan]
    order = np.argsort(k, kind="stable")
    assert np.unique(k).size == k.size  # subnormals and the two zeros are all distinct
    vals = widen(bits[order], kind)
    assert (np.diff(vals) >= 0).all() and vals[0] == -np.inf and vals[-1] == np.inf
    flat = np.nonzero(np.diff(vals) == 0)[0]  # the only tie in value: -0.0 directly below +0.0
    assert flat.size == 1 and bits[order][flat[0]] == 0x8000 and bits[order][flat[0] + 1] == 0x0000


def test_integer_key_order(lib):
    ki, ku = lib_keys(lib, "i16"), lib_keys(lib, "u16")
    assert (np.diff(ALL.view(np.int16)[np.argsort(ki)].astype(np.int64)) == 1).all()
    assert (np.diff(ALL[np.argsort(ku)].astype(np.int64)) == 1).all()


def test_unknown_kind_gives_zero(lib):
    for kind in (4, -1, 100):
        assert lib.kth_k16_order_key(0x1234, kind) == 0 and lib.kth_k16_of_order_key(0x1234, kind) == 0


def test_argument_checks_precede_device_work(lib):
    """All KTH_EINVAL on a machine with or without a GPU: the one-shot forms
    check before they look for a device, the ctx forms are given no ctx."""
    import kselect
    E = kselect.KTH_EINVAL
    a = np.arange(16, dtype=np.uint16)
    out = np.full(9, 0xAAAA, dtype=np.uint16)
    p, o = a.ctypes.data, out.ctypes.data
    for keys, n, k, kind, dst in ((p, 0, 1, 1, o), (p, 16, 0, 1, o), (p, 16, 17, 1, o), (p, -1, 1, 1, o),
                                  (p, 16, 1, 4, o), (p, 16, 1, -1, o), (None, 16, 1, 1, o), (p, 16, 1, 1, None)):
        assert lib.kth_select_k16(keys, n, k, kind, dst) == E, (keys, n, k, kind, dst)
        assert lib.kth_select_k16_ctx(None, keys, n, k, kind, dst) == E
        assert lib.kth_select_k16_async(None, keys, n, k, kind, dst) == E
    one = (ctypes.c_int64 * 1)(1)
    nine = (ctypes.c_int64 * 9)(*range(1, 10))
    bad_rank = (ctypes.c_int64 * 3)(1, 17, 2)
    zero_rank = (ctypes.c_int64 * 3)(1, 0, 2)
    for keys, n, ks, m, kind, dst in ((p, 16, one, 0, 1, o), (p, 16, nine, 9, 1, o), (p, 16, bad_rank, 3, 1, o),
                                      (p, 16, zero_rank, 3, 1, o), (p, 0, one, 1, 1, o), (p, 16, one, 1, 4, o),
                                      (p, 16, one, 1, -1, o), (None, 16, one, 1, 1, o), (p, 16, None, 1, 1, o),
                                      (p, 16, one, 1, 1, None)):
        assert lib.kth_select_multi_k16(keys, n, ks, m, kind, dst) == E, (n, m, kind)
        assert lib.kth_select_multi_k16_ctx(None, keys, n, ks, m, kind, dst) == E
        assert lib.kth_select_multi_k16_async(None, keys, n, ks, m, kind, dst) == E
    # a valid call without a ctx is still refused, and so is a reserve
    assert lib.kth_select_k16_ctx(None, p, 16, 1, 1, o) == E
    assert lib.kth_select_multi_k16_async(None, p, 16, one, 1, 1, o) == E
    assert lib.kth_ctx_reserve_k16(None, 16, 1) == E
    assert (out == 0xAAAA).all()


def test_no_cpu_fallback_k16(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import kselect
    a = np.arange(100, dtype=np.int16)
    out = np.full(3, 0xAAAA, dtype=np.uint16)
    assert lib.kth_select_k16(a.ctypes.data, 100, 50, 0, out.ctypes.data) == kselect.KTH_ENODEV
    ks = (ctypes.c_int64 * 3)(1, 50, 100)
    assert lib.kth_select_multi_k16(a.ctypes.data, 100, ks, 3, 0, out.ctypes.data) == kselect.KTH_ENODEV
    assert (out == 0xAAAA).all()
    for call in (lambda: kselect.kth_select16(a, 50), lambda: kselect.kth_select16_multi(a, [1, 50])):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_ENODEV


def test_wrappers_refuse_other_dtypes():
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    out = torch.zeros(4, dtype=torch.int16)
    for dt in (torch.int32, torch.float32, torch.float64):
        keys = torch.zeros(8, dtype=dt)
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            sel.select16(keys, 1)
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            sel.select16_multi(keys, [1, 2], kind="i16")
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            sel.select16_async(keys, 8, 1, out)
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            sel.select16_multi_async(torch.zeros(8, dtype=torch.int16), 8, [1], torch.zeros(1, dtype=dt))
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            kselect.kth_select16(keys, 1)
    for dt in (np.int32, np.float32, np.float64):
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            kselect.kth_select16(np.zeros(8, dtype=dt), 1)
        with pytest.raises(TypeError, match="int16, uint16, float16 or bfloat16"):
            kselect.kth_select16_multi(np.zeros(8, dtype=dt), [1], kind="bf16")
    with pytest.raises(ValueError):
        kselect.kth_select16(np.zeros(8, dtype=np.uint16), 1, kind="f8")
    # the kind comes from the dtype; bfloat16 bits travel as uint16 with kind="bf16"
    assert kselect._k16_kind(torch.zeros(1, dtype=torch.bfloat16), None) == kselect.KTH_K16_BF16
    assert kselect._k16_kind(np.zeros(1, dtype=np.float16), None) == kselect.KTH_K16_F16
    assert kselect._k16_kind(np.zeros(1, dtype=np.uint16), "bf16") == kselect.KTH_K16_BF16
    v = kselect._k16_values(np.array([0x7FC0, 0x3F80, 0x8000], dtype=np.uint16), kselect.KTH_K16_BF16)
    assert v.dtype == np.float32 and list(v.view(np.uint32)) == [0x7FC00000, 0x3F800000, 0x80000000]
    assert kselect._k16_values(np.array([0x8000], dtype=np.uint16), kselect.KTH_K16_I16)[0] == -32768


def test_header_exports_and_protos_agree(lib):
    import kselect
    header = open(os.path.join(REPO, "include", "kth.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in kselect._lib.PROTOS and hasattr(lib, name), name
    for macro, value in (("KTH_K16_I16", 0), ("KTH_K16_U16", 1), ("KTH_K16_F16", 2), ("KTH_K16_BF16", 3),
                         ("KTH_PATH_K16", 5), ("KTH_PATH_K16_FALLBACK", 6), ("KTH_HOOK_K16_MISS", 4)):
        m = re.search(r"#define\s+%s\s+(-?\d+)" % macro, header)
        assert m and int(m.group(1)) == value == getattr(kselect, macro), macro
    # the argument counts of the prototypes match the header's
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(kselect._lib.PROTOS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
