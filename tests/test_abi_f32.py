"""CPU checks of the float32 one-array entry points (include/kth.h "float32
keys"): the order-key helpers against the documented total order, the argument
checks that precede any device work, and the Python wrapper's dtype check."""
import ctypes

import numpy as np
import pytest

NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
CANON_NAN = 0x7FC00000
# +-0, +-inf, the smallest / largest subnormal and normal of each sign
EDGE_BITS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,
             0x00800000, 0x7F7FFFFF, 0x80800000, 0xFF7FFFFF)


def _f32_order_key(bits):
    """The documented order as uint32 keys: IEEE total order on the bit
    patterns (-0.0 < +0.0, subnormals distinct), every NaN -> 0xFFFFFFFF."""
    b = np.asarray(bits, dtype=np.uint32)
    key = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), key)


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


@pytest.fixture(scope="module")
def patterns():
    rng = np.random.default_rng(0xF32)
    rand = rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([np.array(EDGE_BITS + NAN_BITS, dtype=np.uint32), rand])


def _lib_key(lib, bits):
    # the raw bits travel in a ctypes float built from memory, never through a
    # Python float (a double round trip may quiet a signalling NaN)
    return lib.kth_f32_order_key(ctypes.c_float.from_buffer_copy(np.uint32(bits).tobytes()))


def _lib_bits_of_key(lib, key):
    # (float -> Python float -> float is exact for every non-NaN, and the only
    # NaN that comes back is the canonical quiet one)
    box = ctypes.c_float(lib.kth_f32_of_order_key(int(key)))
    return int(np.frombuffer(bytes(box), dtype=np.uint32)[0])


def test_order_key_matches_the_documented_rule(lib, patterns):
    want = _f32_order_key(patterns)
    got = np.array([_lib_key(lib, b) for b in patterns], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(patterns[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


def test_order_key_orders_the_edges(lib):
    f = lambda b: _lib_key(lib, b)  # noqa: E731
    chain = [0xFF800000, 0xFF7FFFFF, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
             0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000]  # -inf .. -0.0 < +0.0 .. +inf
    keys = [f(b) for b in chain]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for b in NAN_BITS:
        assert f(b) == 0xFFFFFFFF and f(b) > keys[-1]


def test_round_trip(lib, patterns):
    """of_order_key(order_key(x)) over every pattern: the identity off the NaNs, every NaN -> 0x7FC00000."""
    nan = (patterns & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    assert nan.sum() >= len(NAN_BITS) and (~nan).sum() >= len(EDGE_BITS)
    back = np.array([_lib_bits_of_key(lib, _lib_key(lib, b)) for b in patterns], dtype=np.uint32)
    want = np.where(nan, np.uint32(CANON_NAN), patterns)
    bad = np.nonzero(back != want)[0]
    assert bad.size == 0, [(hex(int(patterns[i])), hex(int(back[i]))) for i in bad[:5]]
    assert _lib_bits_of_key(lib, 0xFFFFFFFF) == CANON_NAN


def test_argument_checks_precede_device_work(lib):
    """kth_select_f32 creates its ctx itself, so its n / k / pointer checks are
    really exercised here.  The three ctx-taking entry points can only be given
    a NULL ctx on a machine without a device (no ctx can be created), so for
    them this is a NULL-ctx check only; their n / k / pointer checks run on a
    real ctx in tests/test_gpu_f32.py."""
    import kselect
    a = np.arange(16, dtype=np.float32)
    out = ctypes.c_float(7.0)
    p = a.ctypes.data
    bad = ((None, 16, 1, True), (p, 16, 1, False), (p, 0, 1, True), (p, 16, 0, True), (p, 16, 17, True), (p, -1, 1, True))
    for keys, n, k, with_out in bad:
        o = ctypes.byref(out) if with_out else None
        assert lib.kth_select_f32(keys, n, k, o) == kselect.KTH_EINVAL, (keys, n, k, with_out)
        assert lib.kth_select_f32_ctx(None, keys, n, k, o) == kselect.KTH_EINVAL
        assert lib.kth_select_f32_async(None, keys, n, k, o) == kselect.KTH_EINVAL
    assert out.value == 7.0
    vals = np.zeros(16, dtype=np.float32)
    for n, k in ((16, 0), (16, 17), (0, 1)):
        assert lib.kth_topk_f32(None, a.ctypes.data, n, k, 0, vals.ctypes.data, None) == kselect.KTH_EINVAL
    assert lib.kth_topk_f32(None, a.ctypes.data, 16, 1, 0, None, None) == kselect.KTH_EINVAL
    assert lib.kth_topk_f32(None, None, 16, 1, 0, vals.ctypes.data, None) == kselect.KTH_EINVAL


def test_no_cpu_fallback_f32(lib):
    """Without a GPU the float32 one-shot fails loudly, as kth_select_i32 does."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import kselect
    a = np.linspace(-1, 1, 100, dtype=np.float32)
    out = ctypes.c_float(123.5)
    assert lib.kth_select_f32(a.ctypes.data, 100, 50, ctypes.byref(out)) == kselect.KTH_ENODEV
    assert out.value == 123.5
    with pytest.raises(kselect.KthError) as e:
        kselect.kth_select(a, 50, f32=True)
    assert e.value.code == kselect.KTH_ENODEV


def test_f32_wrappers_refuse_other_dtypes():
    """f32=True with an int tensor is a TypeError before any library call (no
    ctx is needed to find out: the Selector here has no ctx at all)."""
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    keys = torch.zeros(8, dtype=torch.int32)
    fout = torch.zeros(1, dtype=torch.float32)
    with pytest.raises(TypeError, match="float32"):
        sel.select(keys, 1, f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.select_async(keys, 8, 1, fout, f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.select_async(keys.float(), 8, 1, torch.zeros(1, dtype=torch.int32), f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.topk(keys, 8, 1, d_vals=fout, f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.topk(keys.float(), 8, 1, d_vals=torch.zeros(1, dtype=torch.int32), f32=True)
    with pytest.raises(TypeError, match="float32"):
        kselect.kth_select(keys, 1, f32=True)
    with pytest.raises(TypeError, match="float32"):
        kselect.kth_select(torch.zeros(8, dtype=torch.float64), 1, f32=True)
