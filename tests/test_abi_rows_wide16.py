"""CPU checks of the 16-bit wide-rows entry points (include/kth.h "wide rows,
16-bit keys"): header / exports / PROTOS agreement, the argument check that
precedes any device work, the plan's invariants (host arithmetic) and the
Python wrappers' dtype refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_select_wide_rows_k16", "kth_topk_wide_rows_k16", "kth_wide_rows_plan_k16")
MIB32 = 32 << 20


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def test_header_exports_and_protos_agree(lib):
    import kselect
    header = open(os.path.join(REPO, "include", "kth.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in kselect._lib.PROTOS and hasattr(lib, name), name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(kselect._lib.PROTOS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    assert len(kselect._lib.PROTOS["kth_select_wide_rows_k16"][1]) == 8
    assert len(kselect._lib.PROTOS["kth_topk_wide_rows_k16"][1]) == 10
    assert len(kselect._lib.PROTOS["kth_wide_rows_plan_k16"][1]) == 7
    # the section stands after kth_ctx_wide_rows_force and before "synthetic inputs"
    force, synth = header.index("kth_ctx_wide_rows_force("), header.index("kth_fill_synthetic(")
    for name in NAMES:
        assert force < header.index(name + "(") < synth, name


def test_null_ctx_is_einval_for_valid_arguments(lib):
    """No ctx: KTH_EINVAL before any device work, with or without a GPU, outputs untouched."""
    import kselect
    keys = np.arange(64, dtype=np.uint16)
    out = np.full(8, 0xAAAA, dtype=np.uint16)
    idx = np.full(8, -7, dtype=np.int32)
    for kind in range(4):
        assert lib.kth_select_wide_rows_k16(None, keys.ctypes.data, 8, 8, 8, 3, kind,
                                            out.ctypes.data) == kselect.KTH_EINVAL
        for largest in (0, 1):
            assert lib.kth_topk_wide_rows_k16(None, keys.ctypes.data, 8, 8, 8, 1, largest, kind, out.ctypes.data,
                                              idx.ctypes.data) == kselect.KTH_EINVAL
    assert (out == 0xAAAA).all() and (idx == -7).all()


ROWS = (1, 2, 7, 64, 255, 256, 257, 5000, 10 ** 6)
COLS = (1, 3, 7, 8, 4096, 4097, 16385, 128256, 1 << 20, 1 << 24)
CUS = (1, 64, 256)


def test_plan_invariants():
    import kselect
    for num_cu in CUS:
        for rows in ROWS:
            for cols in COLS:
                slices, slice_keys, group_rows, scratch = kselect.wide_rows_plan16(rows, cols, num_cu)
                what = (rows, cols, num_cu, slices, slice_keys, group_rows, scratch)
                assert 1 <= slices <= 256, what
                assert slice_keys % 8 == 0, what
                assert slices * slice_keys >= cols, what
                assert (slices - 1) * slice_keys < cols, what  # the last slice is never empty
                assert 1 <= group_rows <= max(rows, 1), what
                assert 0 <= scratch <= MIB32, what
                if rows >= 8 * num_cu:
                    assert slices == 1, what
    # the same arguments give the same plan, and a long single row is split
    assert kselect.wide_rows_plan16(8, 128256, 256) == kselect.wide_rows_plan16(8, 128256, 256)
    slices, _, group_rows, _ = kselect.wide_rows_plan16(1, 1 << 20, 256)
    assert slices > 1 and group_rows == 1


def test_plan_bad_arguments(lib):
    import kselect
    s = ctypes.c_int32(-5)
    b = ctypes.c_int64(-5)
    p, q = ctypes.byref(s), ctypes.byref(b)
    for rows, cols, num_cu in ((-1, 8, 256), (8, 0, 256), (8, -3, 256), (8, (1 << 24) + 1, 256), (8, 8, 0), (8, 8, -1)):
        assert lib.kth_wide_rows_plan_k16(rows, cols, num_cu, p, p, p, q) == kselect.KTH_EINVAL, (rows, cols, num_cu)
        with pytest.raises(kselect.KthError):
            kselect.wide_rows_plan16(rows, cols, num_cu)
    assert s.value == -5 and b.value == -5
    assert lib.kth_wide_rows_plan_k16(8, 1 << 24, 256, None, None, None, None) == kselect.KTH_OK  # outputs are optional


def test_wrappers_refuse_other_dtypes():
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    two_byte = "int16, uint16, float16 or bfloat16"
    out16 = torch.zeros(4, dtype=torch.int16)
    idx = torch.zeros(4, dtype=torch.int32)
    # keys that are not 2 bytes wide
    for dt in (torch.int32, torch.float32):
        keys = torch.zeros(4, 8, dtype=dt)
        with pytest.raises(TypeError, match=two_byte):
            sel.rows_wide16(keys, 4, 8, 1, out16)
        with pytest.raises(TypeError, match=two_byte):
            sel.rows_wide16(keys, 4, 8, 1, out16, kind="i16")
        with pytest.raises(TypeError, match=two_byte):
            sel.topk_rows_wide16(keys, 4, 8, 1, out16, idx)
    # an output of another kind, or not 2 bytes wide
    bf = torch.zeros(4, 8, dtype=torch.bfloat16)
    for other in (torch.float16, torch.int16):
        with pytest.raises(TypeError, match="16-bit kind"):
            sel.rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=other))
        with pytest.raises(TypeError, match="16-bit kind"):
            sel.topk_rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=other), idx)
    i16 = torch.zeros(4, 8, dtype=torch.int16)
    with pytest.raises(TypeError, match="16-bit kind"):
        sel.rows_wide16(i16, 4, 8, 1, torch.zeros(4, dtype=torch.float16), kind="bf16")
    for wide in (torch.float32, torch.int32):
        with pytest.raises(TypeError, match=two_byte):
            sel.rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=wide))
        with pytest.raises(TypeError, match=two_byte):
            sel.topk_rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=wide), idx)
    # a non-int32 d_idx
    for dt in (torch.int64, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=dt))
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide16(i16, 4, 8, 1, None, torch.zeros(4, dtype=dt), kind="f16", ld=8)
    with pytest.raises(ValueError):
        sel.rows_wide16(i16, 4, 8, 1, out16, kind="f8")
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for call in (lambda: sel.rows_wide16(i16, 4, 8, 1, out16, kind="bf16"),
                 lambda: sel.rows_wide16(bf, 4, 8, 1, torch.zeros(4, dtype=torch.bfloat16), ld=8),
                 lambda: sel.topk_rows_wide16(i16, 4, 8, 1, out16, idx, kind="u16"),
                 lambda: sel.topk_rows_wide16(bf, 4, 8, 1, None, idx, largest=True, ld=8)):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL
