"""CPU checks of the wide-rows entry points (include/kth.h "wide rows"):
header / exports / PROTOS agreement, the argument check that precedes any
device work, the plan's invariants (host arithmetic) and the Python wrappers'
dtype refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_select_wide_rows_i32", "kth_select_wide_rows_f32", "kth_topk_wide_rows_i32", "kth_topk_wide_rows_f32",
         "kth_ctx_reserve_wide_rows", "kth_wide_rows_plan", "kth_ctx_wide_rows_force")
MIB32 = 32 << 20


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def _header():
    return open(os.path.join(REPO, "include", "kth.h")).read()


def test_header_exports_and_protos_agree(lib):
    import kselect
    header = _header()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in kselect._lib.PROTOS and hasattr(lib, name), name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(kselect._lib.PROTOS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    m = re.search(r"#define\s+KTH_WIDE_MAX_COLS\s+\(1\s*<<\s*(\d+)\)", header)
    assert m and 1 << int(m.group(1)) == kselect.KTH_WIDE_MAX_COLS == kselect._lib.KTH_WIDE_MAX_COLS == 1 << 24
    m = re.search(r"#define\s+KTH_WIDE_MAX_SLICES\s+(\d+)", header)
    assert m and int(m.group(1)) == kselect.KTH_WIDE_MAX_SLICES == kselect._lib.KTH_WIDE_MAX_SLICES == 256
    # the section stands directly before "synthetic inputs"
    assert header.index("kth_topk_k16(") < header.index("kth_select_wide_rows_i32(")
    assert header.index("kth_ctx_wide_rows_force(") < header.index("kth_fill_synthetic(")


def test_no_new_hook_path_or_finish_define():
    """The test control is a function: the sets of these defines are as they were."""
    header = _header()
    assert sorted(re.findall(r"#define\s+(KTH_HOOK_\w+)", header)) == sorted(
        ["KTH_HOOK_FAULT_TOPK_RANK", "KTH_HOOK_FAULT_BARRIER", "KTH_HOOK_TOPK_SEG_CAP", "KTH_HOOK_K16_MISS",
         "KTH_HOOK_FINISH_SLICES", "KTH_HOOK_K16_TOPK_NOSKIP"])
    assert sorted(re.findall(r"#define\s+(KTH_PATH_\w+)", header)) == sorted(
        ["KTH_PATH_LDS", "KTH_PATH_RADIX", "KTH_PATH_WINDOW", "KTH_PATH_WINDOW_FALLBACK", "KTH_PATH_K16",
         "KTH_PATH_K16_FALLBACK"])
    assert sorted(re.findall(r"#define\s+(KTH_FINISH_\w+)", header)) == sorted(
        ["KTH_FINISH_NONE", "KTH_FINISH_COUNTS", "KTH_FINISH_SLICES", "KTH_FINISH_GROUPED", "KTH_FINISH_LEVELS"])


def test_null_ctx_is_einval_for_valid_arguments(lib):
    """No ctx: KTH_EINVAL before any device work, with or without a GPU, outputs untouched."""
    import kselect
    keys = np.arange(64, dtype=np.int32)
    out = np.full(8, 0x5A5A5A5A, dtype=np.int32)
    idx = np.full(8, -7, dtype=np.int32)
    for sel_fn, topk_fn in ((lib.kth_select_wide_rows_i32, lib.kth_topk_wide_rows_i32),
                            (lib.kth_select_wide_rows_f32, lib.kth_topk_wide_rows_f32)):
        assert sel_fn(None, keys.ctypes.data, 8, 8, 8, 3, out.ctypes.data) == kselect.KTH_EINVAL
        for largest in (0, 1):
            assert topk_fn(None, keys.ctypes.data, 8, 8, 8, 1, largest, out.ctypes.data,
                           idx.ctypes.data) == kselect.KTH_EINVAL
    assert (out == 0x5A5A5A5A).all() and (idx == -7).all()
    assert lib.kth_ctx_wide_rows_force(None, 0, 0) == kselect.KTH_EINVAL
    assert lib.kth_ctx_wide_rows_force(None, 3, 2) == kselect.KTH_EINVAL
    assert lib.kth_ctx_reserve_wide_rows(None, 8, 8) == kselect.KTH_EINVAL


ROWS = (1, 2, 7, 64, 255, 256, 257, 5000, 10 ** 6)
COLS = (1, 3, 4096, 4097, 16385, 128256, 1 << 20, 1 << 24)
CUS = (1, 64, 256)


def test_plan_invariants():
    import kselect
    for num_cu in CUS:
        for rows in ROWS:
            for cols in COLS:
                slices, slice_keys, group_rows, scratch = kselect.wide_rows_plan(rows, cols, num_cu)
                what = (rows, cols, num_cu, slices, slice_keys, group_rows, scratch)
                assert 1 <= slices <= 256, what
                assert slice_keys % 4 == 0, what
                assert slices * slice_keys >= cols, what
                assert (slices - 1) * slice_keys < cols, what  # the last slice is never empty
                assert 1 <= group_rows <= max(rows, 1), what
                assert 0 <= scratch <= MIB32, what
                if rows >= 4 * num_cu:
                    assert slices == 1, what
    # rows == 0 is a legal shape of the calls: the plan holds its invariants there too
    slices, slice_keys, group_rows, scratch = kselect.wide_rows_plan(0, 4096, 256)
    assert slices >= 1 and group_rows == 1 and scratch <= MIB32


def test_plan_cases():
    import kselect
    for num_cu in CUS:
        slices, _, group_rows, scratch = kselect.wide_rows_plan(10 ** 6, 16385, num_cu)
        assert group_rows < 10 ** 6 and scratch <= MIB32
    slices, slice_keys, group_rows, _ = kselect.wide_rows_plan(1, 1 << 20, 256)
    assert slices > 1 and group_rows == 1
    # the same arguments give the same plan
    assert kselect.wide_rows_plan(8, 128256, 256) == kselect.wide_rows_plan(8, 128256, 256)


def test_plan_bad_arguments(lib):
    import kselect
    s = ctypes.c_int32(-5)
    b = ctypes.c_int64(-5)
    p, q = ctypes.byref(s), ctypes.byref(b)
    for rows, cols, num_cu in ((-1, 8, 256), (8, 0, 256), (8, -3, 256), (8, (1 << 24) + 1, 256), (8, 8, 0), (8, 8, -1)):
        assert lib.kth_wide_rows_plan(rows, cols, num_cu, p, p, p, q) == kselect.KTH_EINVAL, (rows, cols, num_cu)
        with pytest.raises(kselect.KthError):
            kselect.wide_rows_plan(rows, cols, num_cu)
    assert s.value == -5 and b.value == -5
    assert lib.kth_wide_rows_plan(8, 1 << 24, 256, None, None, None, None) == kselect.KTH_OK  # outputs are optional


def test_wrappers_refuse_other_dtypes():
    import torch

    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    f = torch.zeros(4, 8, dtype=torch.float32)
    i = torch.zeros(4, 8, dtype=torch.int32)
    outf, outi = torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int32)
    # f32=True: keys, d_out and d_vals must be float32
    for bad in (i, torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4, 8, dtype=torch.float64)):
        with pytest.raises(TypeError, match="d_keys must be float32"):
            sel.rows_wide(bad, 4, 8, 1, outf, f32=True)
        with pytest.raises(TypeError, match="d_keys must be float32"):
            sel.topk_rows_wide(bad, 4, 8, 1, outf, idx, f32=True)
    with pytest.raises(TypeError, match="d_out must be float32"):
        sel.rows_wide(f, 4, 8, 1, outi, f32=True)
    with pytest.raises(TypeError, match="d_vals must be float32"):
        sel.topk_rows_wide(f, 4, 8, 1, outi, idx, f32=True)
    # a non-int32 d_idx, either key type
    for dt in (torch.int64, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide(f, 4, 8, 1, outf, torch.zeros(4, dtype=dt), f32=True)
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide(i, 4, 8, 1, None, torch.zeros(4, dtype=dt))
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for call in (lambda: sel.rows_wide(i, 4, 8, 1, outi),
                 lambda: sel.rows_wide(f, 4, 8, 1, outf, f32=True, ld=8),
                 lambda: sel.topk_rows_wide(i, 4, 8, 1, outi, idx),
                 lambda: sel.topk_rows_wide(f, 4, 8, 1, None, idx, largest=True, f32=True, ld=8),
                 lambda: sel.reserve_wide_rows(4, 8),
                 lambda: sel.wide_rows_force(3, 2)):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL
