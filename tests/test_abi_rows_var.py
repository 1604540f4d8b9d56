"""CPU checks of the ragged wide-rows entry points (include/kth.h "wide rows,
ragged"): header / exports / PROTOS agreement, the section's place, the
argument check that precedes any device work and the Python wrappers' dtype
refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_select_wide_rows_var_i32", "kth_select_wide_rows_var_f32", "kth_select_wide_rows_var_k16",
         "kth_topk_wide_rows_var_i32", "kth_topk_wide_rows_var_f32", "kth_topk_wide_rows_var_k16")


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
    # a section of its own, after "wide rows, 16-bit keys" and directly before "synthetic inputs"
    last16, synth = header.index("kth_wide_rows_plan_k16("), header.index("kth_fill_synthetic(")
    for name in NAMES:
        assert last16 < header.index(name + "(") < synth, name
    between = header[max(header.index(n + "(") for n in NAMES):synth]
    assert not re.search(r"\bkth_\w+\s*\(", between.split(";", 1)[1]), "a declaration stands between the section and synthetic inputs"
    assert "--- wide rows, ragged" in header[last16:synth]


def test_null_ctx_is_einval_for_valid_arguments(lib):
    """No ctx: KTH_EINVAL before any device work, with or without a GPU, outputs untouched."""
    import kselect
    keys = np.arange(64, dtype=np.int32)
    lens = np.full(8, 5, dtype=np.int32)
    ks = np.full(8, 2, dtype=np.int32)
    out = np.full(24, 0x5A5A5A5A, dtype=np.int32)
    idx = np.full(24, -7, dtype=np.int32)
    cnt = np.full(8, -9, dtype=np.int32)
    K, L, O, I, C = keys.ctypes.data, lens.ctypes.data, out.ctypes.data, idx.ctypes.data, cnt.ctypes.data
    for lp, kp in ((L, ks.ctypes.data), (None, ks.ctypes.data), (L, None), (None, None)):
        for fn in (lib.kth_select_wide_rows_var_i32, lib.kth_select_wide_rows_var_f32):
            assert fn(None, K, 8, 8, 8, lp, kp, 3, O) == kselect.KTH_EINVAL
        for kind in (kselect.KTH_K16_I16, kselect.KTH_K16_U16, kselect.KTH_K16_F16, kselect.KTH_K16_BF16):
            assert lib.kth_select_wide_rows_var_k16(None, K, 8, 8, 8, lp, kp, 3, kind, O) == kselect.KTH_EINVAL
            for largest in (0, 1):
                assert lib.kth_topk_wide_rows_var_k16(None, K, 8, 8, 8, lp, kp, 3, largest, kind, O, I,
                                                      C) == kselect.KTH_EINVAL
        for fn in (lib.kth_topk_wide_rows_var_i32, lib.kth_topk_wide_rows_var_f32):
            for largest in (0, 1):
                assert fn(None, K, 8, 8, 8, lp, kp, 3, largest, O, I, C) == kselect.KTH_EINVAL
                assert fn(None, K, 8, 8, 8, lp, kp, 3, largest, O, I, None) == kselect.KTH_EINVAL
    assert (out == 0x5A5A5A5A).all() and (idx == -7).all() and (cnt == -9).all()
    assert (lens == 5).all() and (ks == 2).all()


def _no_ctx_selector():
    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    return sel


def test_wrappers_refuse_other_dtypes_32bit():
    import torch

    import kselect
    sel = _no_ctx_selector()
    f = torch.zeros(4, 8, dtype=torch.float32)
    i = torch.zeros(4, 8, dtype=torch.int32)
    outf, outi = torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.int32)
    idx, i32 = torch.zeros(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for bad in (i, torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4, 8, dtype=torch.float64)):
        with pytest.raises(TypeError, match="d_keys must be float32"):
            sel.rows_wide_var(bad, 4, 8, 1, outf, f32=True, d_lens=i32)
        with pytest.raises(TypeError, match="d_keys must be float32"):
            sel.topk_rows_wide_var(bad, 4, 8, 1, outf, idx, f32=True, d_ks=i32)
    with pytest.raises(TypeError, match="d_out must be float32"):
        sel.rows_wide_var(f, 4, 8, 1, outi, f32=True)
    with pytest.raises(TypeError, match="d_vals must be float32"):
        sel.topk_rows_wide_var(f, 4, 8, 1, outi, idx, f32=True)
    for dt in (torch.int64, torch.int16, torch.float32, torch.uint8):
        other = torch.zeros(8, dtype=dt)
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide_var(i, 4, 8, 1, outi, other)
        for name in ("d_lens", "d_ks"):
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.rows_wide_var(i, 4, 8, 1, outi, **{name: other})
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.rows_wide_var(f, 4, 8, 1, outf, f32=True, **{name: other})
        for name in ("d_lens", "d_ks", "d_cnt"):
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.topk_rows_wide_var(i, 4, 8, 2, outi, idx, **{name: other})
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.topk_rows_wide_var(f, 4, 8, 2, outf, None, largest=True, f32=True, **{name: other})
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for call in (lambda: sel.rows_wide_var(i, 4, 8, 1, outi),
                 lambda: sel.rows_wide_var(i, 4, 8, 1, outi, d_lens=i32, d_ks=i32, ld=8),
                 lambda: sel.rows_wide_var(f, 4, 8, 1, outf, f32=True, d_ks=i32),
                 lambda: sel.topk_rows_wide_var(i, 4, 8, 2, outi, idx, d_lens=i32, d_ks=i32, d_cnt=i32),
                 lambda: sel.topk_rows_wide_var(f, 4, 8, 2, None, idx, largest=True, f32=True, d_cnt=i32, ld=8),
                 lambda: sel.topk_rows_wide_var(i, 4, 8, 2, outi, None, d_lens=np.zeros(4, dtype=np.int32))):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL


def test_wrappers_refuse_other_dtypes_16bit():
    import torch

    import kselect
    sel = _no_ctx_selector()
    bf = torch.zeros(4, 8, dtype=torch.bfloat16)
    h = torch.zeros(4, 8, dtype=torch.float16)
    w = torch.zeros(4, 8, dtype=torch.int16)
    obf, oh, ow = (torch.zeros(8, dtype=t) for t in (torch.bfloat16, torch.float16, torch.int16))
    idx, i32 = torch.zeros(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for bad in (torch.zeros(4, 8, dtype=torch.float32), torch.zeros(4, 8, dtype=torch.int32)):
        with pytest.raises(TypeError, match="d_keys must be int16, uint16, float16 or bfloat16"):
            sel.rows_wide16_var(bad, 4, 8, 1, obf, d_lens=i32)
        with pytest.raises(TypeError, match="d_keys must be int16, uint16, float16 or bfloat16"):
            sel.topk_rows_wide16_var(bad, 4, 8, 1, obf, idx, d_ks=i32)
    with pytest.raises(TypeError, match="d_out must have the keys' 16-bit kind"):
        sel.rows_wide16_var(bf, 4, 8, 1, oh)
    with pytest.raises(TypeError, match="d_vals must have the keys' 16-bit kind"):
        sel.topk_rows_wide16_var(h, 4, 8, 1, obf, idx)
    with pytest.raises(TypeError):
        sel.rows_wide16_var(bf, 4, 8, 1, torch.zeros(4, dtype=torch.float32))
    for dt in (torch.int64, torch.int16, torch.float32):
        other = torch.zeros(8, dtype=dt)
        with pytest.raises(TypeError, match="d_idx must be int32"):
            sel.topk_rows_wide16_var(bf, 4, 8, 1, obf, other)
        for name in ("d_lens", "d_ks"):
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.rows_wide16_var(bf, 4, 8, 1, obf, **{name: other})
        for name in ("d_lens", "d_ks", "d_cnt"):
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.topk_rows_wide16_var(w, 4, 8, 2, ow, idx, kind="u16", **{name: other})
    for call in (lambda: sel.rows_wide16_var(bf, 4, 8, 1, obf, d_lens=i32, d_ks=i32),
                 lambda: sel.rows_wide16_var(w, 4, 8, 1, ow, kind="bf16", ld=8),
                 lambda: sel.topk_rows_wide16_var(h, 4, 8, 2, oh, idx, largest=True, d_lens=i32, d_ks=i32, d_cnt=i32),
                 lambda: sel.topk_rows_wide16_var(w, 4, 8, 2, None, idx, d_cnt=i32, ld=8)):
        with pytest.raises(kselect.KthError) as e:
            call()
        assert e.value.code == kselect.KTH_EINVAL
