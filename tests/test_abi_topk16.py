"""CPU checks of the 16-bit one-array top-k (include/kth.h "top-k of one array,
16-bit keys"): header / exports / PROTOS agreement, the argument check that
precedes any device work, and the Python wrapper's dtype refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_topk_k16", "kth_ctx_last_topk_k16_tiles")


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
    m = re.search(r"#define\s+KTH_HOOK_K16_TOPK_NOSKIP\s+(\d+)", header)
    assert m and int(m.group(1)) == kselect.KTH_HOOK_K16_TOPK_NOSKIP == kselect._lib.KTH_HOOK_K16_TOPK_NOSKIP
    # every hook id, this one included, is distinct and they count up from 1
    ids = sorted(int(v) for v in re.findall(r"#define\s+KTH_HOOK_\w+\s+(\d+)", header))
    assert ids == list(range(1, len(ids) + 1)) and ids[-1] == kselect.KTH_HOOK_K16_TOPK_NOSKIP
    # the section stands after "top-k of one array"
    assert header.index("kth_topk_f32(") < header.index("kth_topk_k16(") < header.index("kth_fill_synthetic(")
    # the rank-fault hook's comment names this call too
    hook = header[header.index("KTH_HOOK_FAULT_TOPK_RANK  value"):header.index("KTH_HOOK_FAULT_BARRIER    1")]
    assert "kth_topk_k16" in hook


def test_null_ctx_is_einval_for_valid_arguments(lib):
    """No ctx: KTH_EINVAL before any device work, with or without a GPU, outputs untouched."""
    import kselect
    keys = np.arange(64, dtype=np.uint16)
    vals = np.full(8, 0xAAAA, dtype=np.uint16)
    idx = np.full(8, -7, dtype=np.int64)
    for kind in range(4):
        for largest in (0, 1):
            assert lib.kth_topk_k16(None, keys.ctypes.data, 64, 8, largest, kind, vals.ctypes.data,
                                    idx.ctypes.data) == kselect.KTH_EINVAL
            assert lib.kth_topk_k16(None, keys.ctypes.data, 64, 8, largest, kind, None,
                                    idx.ctypes.data) == kselect.KTH_EINVAL
    assert (vals == 0xAAAA).all() and (idx == -7).all()
    tiles, read = ctypes.c_uint64(5), ctypes.c_uint64(6)
    assert lib.kth_ctx_last_topk_k16_tiles(None, ctypes.byref(tiles), ctypes.byref(read)) == kselect.KTH_EINVAL
    assert (tiles.value, read.value) == (5, 6)


def test_wrapper_refuses_other_dtypes():
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    two_byte = "int16, uint16, float16 or bfloat16"
    out16 = torch.zeros(4, dtype=torch.int16)
    idx = torch.zeros(4, dtype=torch.int64)
    # int32 / float32 keys
    for dt in (torch.int32, torch.float32):
        keys = torch.zeros(32, dtype=dt)
        with pytest.raises(TypeError, match=two_byte):
            sel.topk16(keys, 32, 4, out16, idx)
        with pytest.raises(TypeError, match=two_byte):
            sel.topk16(keys, 32, 4, out16, idx, kind="i16")
    # a d_vals of another kind, or not 2 bytes wide
    bf = torch.zeros(32, dtype=torch.bfloat16)
    i16 = torch.zeros(32, dtype=torch.int16)
    for other in (torch.float16, torch.int16):
        with pytest.raises(TypeError, match="16-bit kind"):
            sel.topk16(bf, 32, 4, torch.zeros(4, dtype=other), idx)
    with pytest.raises(TypeError, match="16-bit kind"):
        sel.topk16(i16, 32, 4, torch.zeros(4, dtype=torch.float16), idx, kind="bf16")
    for wide in (torch.float32, torch.int32):
        with pytest.raises(TypeError, match=two_byte):
            sel.topk16(bf, 32, 4, torch.zeros(4, dtype=wide), idx)
    # a non-int64 d_idx
    for dt in (torch.int32, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="d_idx must be int64"):
            sel.topk16(bf, 32, 4, torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=dt))
        with pytest.raises(TypeError, match="d_idx must be int64"):
            sel.topk16(i16, 32, 4, None, torch.zeros(4, dtype=dt), kind="f16")
    with pytest.raises(ValueError):
        sel.topk16(i16, 32, 4, out16, idx, kind="f8")
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for call in (lambda: sel.topk16(i16, 32, 4, out16, idx, kind="bf16"),
                 lambda: sel.topk16(bf, 32, 4, torch.zeros(4, dtype=torch.bfloat16), idx),
                 lambda: sel.topk16(i16, 32, 4, out16, None, kind="u16"),
                 lambda: sel.topk16(bf, 32, 4, None, idx, largest=True),
                 lambda: sel.topk16_tiles()):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL
