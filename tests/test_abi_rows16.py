"""CPU checks of the 16-bit rows entry points (include/kth.h "16-bit rows"):
header / exports / PROTOS agreement, the argument check that precedes any
device work, and the Python wrappers' dtype refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_select_rows_k16", "kth_topk_rows_k16")


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
    m = re.search(r"#define\s+KTH_ROWS16_MAX_COLS\s+(\d+)", header)
    assert m and int(m.group(1)) == kselect.KTH_ROWS16_MAX_COLS == kselect._lib.KTH_ROWS16_MAX_COLS == 8192
    # the section stands after "top-k per row"
    assert header.index("kth_topk_rows_f32(") < header.index("kth_select_rows_k16(") < header.index("kth_topk_i32(")


def test_null_ctx_is_einval_for_valid_arguments(lib):
    """No ctx: KTH_EINVAL before any device work, with or without a GPU, outputs untouched."""
    import kselect
    keys = np.arange(64, dtype=np.uint16)
    out = np.full(8, 0xAAAA, dtype=np.uint16)
    idx = np.full(8, -7, dtype=np.int32)
    for kind in range(4):
        assert lib.kth_select_rows_k16(None, keys.ctypes.data, 8, 8, 3, kind, out.ctypes.data) == kselect.KTH_EINVAL
        for largest in (0, 1):
            assert lib.kth_topk_rows_k16(None, keys.ctypes.data, 8, 8, 1, largest, kind, out.ctypes.data,
                                         idx.ctypes.data) == kselect.KTH_EINVAL
    assert (out == 0xAAAA).all() and (idx == -7).all()


def test_wrappers_refuse_other_dtypes():
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    two_byte = "int16, uint16, float16 or bfloat16"
    out16 = torch.zeros(4, dtype=torch.int16)
    idx = torch.zeros(4, dtype=torch.int32)
    # int32 / float32 keys
    for dt in (torch.int32, torch.float32):
        keys = torch.zeros(4, 8, dtype=dt)
        with pytest.raises(TypeError, match=two_byte):
            sel.rows16(keys, 4, 8, 1, out16)
        with pytest.raises(TypeError, match=two_byte):
            sel.rows16(keys, 4, 8, 1, out16, kind="i16")
        with pytest.raises(TypeError, match=two_byte):
            sel.topk_rows16(keys, 4, 8, 1, out16, idx)
    # an output of another kind, or not 2 bytes wide
    bf = torch.zeros(4, 8, dtype=torch.bfloat16)
    for other in (torch.float16, torch.int16):
        with pytest.raises(TypeError, match="16-bit kind"):
            sel.rows16(bf, 4, 8, 1, torch.zeros(4, dtype=other))
        with pytest.raises(TypeError, match="16-bit kind"):
            sel.topk_rows16(bf, 4, 8, 1, torch.zeros(4, dtype=other), idx)
    i16 = torch.zeros(4, 8, dtype=torch.int16)
    with pytest.raises(TypeError, match="16-bit kind"):
        sel.rows16(i16, 4, 8, 1, torch.zeros(4, dtype=torch.float16), kind="bf16")
    for wide in (torch.float32, torch.int32):
        with pytest.raises(TypeError, match=two_byte):
            sel.rows16(bf, 4, 8, 1, torch.zeros(4, dtype=wide))
        with pytest.raises(TypeError, match=two_byte):
            sel.topk_rows16(bf, 4, 8, 1, torch.zeros(4, dtype=wide), idx)
    # a non-int32 d_idx
    for dt in (torch.int64, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows16(bf, 4, 8, 1, torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=dt))
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows16(i16, 4, 8, 1, None, torch.zeros(4, dtype=dt), kind="f16")
    with pytest.raises(ValueError):
        sel.rows16(i16, 4, 8, 1, out16, kind="f8")
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for call in (lambda: sel.rows16(i16, 4, 8, 1, out16, kind="bf16"),
                 lambda: sel.rows16(bf, 4, 8, 1, torch.zeros(4, dtype=torch.bfloat16)),
                 lambda: sel.topk_rows16(i16, 4, 8, 1, out16, idx, kind="u16"),
                 lambda: sel.topk_rows16(bf, 4, 8, 1, None, idx, largest=True)):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL
