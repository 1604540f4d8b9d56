"""CPU checks of the multi-rank entry points (include/kth.h "several ranks of
one array"): the prototypes, the argument checks that precede any device work,
the no-fallback rule and the Python wrappers' dtype check."""
import ctypes

import numpy as np
import pytest

MULTI = ("kth_select_multi_i32", "kth_select_multi_i32_ctx", "kth_select_multi_i32_async", "kth_select_multi_f32",
         "kth_select_multi_f32_ctx", "kth_select_multi_f32_async", "kth_ctx_reserve_multi", "kth_ctx_multi_stats")


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def _ks(*ranks):
    return (ctypes.c_int64 * len(ranks))(*ranks)


def test_prototypes_are_bound(lib):
    from kselect._lib import KTH_MULTI_MAX_RANKS, PROTOS
    assert KTH_MULTI_MAX_RANKS == 8
    for name in MULTI:
        assert name in PROTOS, name
        assert getattr(lib, name).argtypes == PROTOS[name][1]


@pytest.mark.parametrize("f32", [False, True])
def test_argument_checks_precede_device_work(lib, f32):
    """The one-shot form makes its own ctx, so it is given real arguments; the
    ctx forms are given a NULL ctx (no ctx can be made without a device)."""
    import kselect
    n = 16
    a = np.arange(n, dtype=np.float32 if f32 else np.int32)
    out = np.full(9, 7, dtype=a.dtype)
    p, o = a.ctypes.data, out.ctypes.data
    one = lib.kth_select_multi_f32 if f32 else lib.kth_select_multi_i32
    ctx = lib.kth_select_multi_f32_ctx if f32 else lib.kth_select_multi_i32_ctx
    asy = lib.kth_select_multi_f32_async if f32 else lib.kth_select_multi_i32_async
    good = _ks(1, 8, 16)
    bad = [
        (p, n, good, 0, o),                        # m = 0
        (p, n, _ks(*range(1, 10)), 9, o),          # m = 9
        (p, n, None, 3, o),                        # NULL ks
        (None, n, good, 3, o),                     # NULL keys
        (p, n, good, 3, None),                     # NULL out
        (p, n, _ks(1, 0, 16), 3, o),               # a rank of 0
        (p, n, _ks(1, n + 1, 16), 3, o),           # a rank of n + 1
        (p, 0, good, 3, o),                        # n = 0
        (p, n, good, -1, o),                       # m < 0
    ]
    for keys, nn, ks, m, dst in bad:
        assert one(keys, nn, ks, m, dst) == kselect.KTH_EINVAL, (nn, m)
        assert ctx(None, keys, nn, ks, m, dst) == kselect.KTH_EINVAL, (nn, m)
        assert asy(None, keys, nn, ks, m, dst) == kselect.KTH_EINVAL, (nn, m)
    # a NULL ctx is refused for valid arguments too
    assert ctx(None, p, n, good, 3, o) == kselect.KTH_EINVAL
    assert asy(None, p, n, good, 3, o) == kselect.KTH_EINVAL
    assert (out == 7).all()
    st = kselect.KthStats()
    assert lib.kth_ctx_reserve_multi(None, n, 3) == kselect.KTH_EINVAL
    assert lib.kth_ctx_multi_stats(None, 0, ctypes.byref(st)) == kselect.KTH_EINVAL


def test_no_cpu_fallback_multi(lib):
    """Without a GPU a valid multi call fails loudly and leaves out alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import kselect
    a = np.arange(100, dtype=np.int32)
    out = np.full(3, -5, dtype=np.int32)
    assert lib.kth_select_multi_i32(a.ctypes.data, 100, _ks(1, 50, 100), 3, out.ctypes.data) == kselect.KTH_ENODEV
    f = a.astype(np.float32)
    fout = np.full(3, -5, dtype=np.float32)
    assert lib.kth_select_multi_f32(f.ctypes.data, 100, _ks(1, 50, 100), 3, fout.ctypes.data) == kselect.KTH_ENODEV
    assert (out == -5).all() and (fout == -5).all()
    for f32 in (False, True):
        with pytest.raises(kselect.KthError) as e:
            kselect.kth_select_multi(f if f32 else a, [1, 50, 100], f32=f32)
        assert e.value.code == kselect.KTH_ENODEV


def test_multi_wrappers_refuse_other_dtypes():
    """f32=True with an int tensor is a TypeError before any library call (the
    Selector here has no ctx at all)."""
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    keys = torch.zeros(8, dtype=torch.int32)
    fout = torch.zeros(2, dtype=torch.float32)
    with pytest.raises(TypeError, match="float32"):
        sel.select_multi(keys, [1, 2], f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.select_multi_async(keys, 8, [1, 2], fout, f32=True)
    with pytest.raises(TypeError, match="float32"):
        sel.select_multi_async(keys.float(), 8, [1, 2], torch.zeros(2, dtype=torch.int32), f32=True)
    with pytest.raises(TypeError, match="float32"):
        kselect.kth_select_multi(keys, [1, 2], f32=True)
    with pytest.raises(TypeError, match="float32"):
        kselect.kth_select_multi(torch.zeros(8, dtype=torch.float64), [1, 2], f32=True)
