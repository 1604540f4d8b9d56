"""CPU checks of the sorted top-k entry points (include/kth.h "rows, sorted
top-k"): header / exports / PROTOS agreement, the contract's phrases, the
argument check that precedes any device work (buffers untouched), rows == 0,
the Python wrappers' dtype refusals, the three ValueErrors of sorted=True and
the no-device answer."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_sort_topk_rows_i32", "kth_sort_topk_rows_f32", "kth_sort_topk_rows_k16")


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def test_header_exports_and_protos_agree(lib):
    import kselect
    header = open(os.path.join(REPO, "include", "kth.h")).read()
    for name in NAMES:
        assert name in kselect._lib.PROTOS and hasattr(lib, name), name
        args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(kselect._lib.PROTOS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    at = header.index("--- rows, sorted top-k")
    assert header.index("--- wide rows, sampling") < header.index("int kth_ctx_reserve_sample_rows(") < at
    for name in NAMES:
        assert at < header.index("int " + name + "(")
    section = " ".join(header[at:header.index("int kth_sort_topk_rows_i32(")].replace(" * ", " ").split())
    for phrase in ("stable", "bit for bit", "neither read nor written", "clamp(d_cnt[r], 0, k)", "keep their input order",
                   "kth_f32_order_key", "kth_k16_order_key", "kth_ctx_last_stats is unaffected", "KTH_ENODEV"):
        assert phrase in section, phrase
    assert int(re.search(r"#define KTH_SORT_MAX_K (\d+)", header).group(1)) == kselect.KTH_SORT_MAX_K == 4096
    assert kselect._lib.KTH_SORT_MAX_K == kselect.KTH_SORT_MAX_K


class Args:
    """Valid arguments over host buffers that no call may touch; a ctx that is never dereferenced,
    because every case here ends in the argument check (or rows == 0)."""

    def __init__(self):
        self.fake_ctx = ctypes.create_string_buffer(1 << 16)
        self.vals = np.arange(64, 0, -1, dtype=np.int32)
        self.idx = np.arange(64, dtype=np.int32)
        self.cnt = np.full(8, 5, dtype=np.int32)

    def base(self):
        return dict(ctx=ctypes.addressof(self.fake_ctx), vals=self.vals.ctypes.data, idx=self.idx.ctypes.data, rows=8,
                    k=8, cnt=self.cnt.ctypes.data, largest=1)

    def untouched(self):
        return (np.array_equal(self.vals, np.arange(64, 0, -1, dtype=np.int32))
                and np.array_equal(self.idx, np.arange(64, dtype=np.int32)) and (self.cnt == 5).all())


def call(lib, kind, a):
    """kind: "i32", "f32", or a KTH_K16_* value."""
    head = (a["ctx"], a["vals"], a["idx"], a["rows"], a["k"], a["cnt"], a["largest"])
    if kind == "i32":
        return lib.kth_sort_topk_rows_i32(*head)
    if kind == "f32":
        return lib.kth_sort_topk_rows_f32(*head)
    return lib.kth_sort_topk_rows_k16(*head, kind)


BAD = [dict(ctx=None), dict(vals=None), dict(rows=-1), dict(k=0), dict(k=-3), dict(k=4097), dict(k=1 << 30)]


def test_einval_before_any_device_work(lib):
    import kselect
    args = Args()
    for kind in ("i32", "f32", kselect.KTH_K16_I16, kselect.KTH_K16_U16, kselect.KTH_K16_F16, kselect.KTH_K16_BF16):
        for bad in BAD:
            for optional in (dict(), dict(idx=None), dict(cnt=None)):
                a = args.base()
                a.update(optional)
                a.update(bad)
                assert call(lib, kind, a) == kselect.KTH_EINVAL, (kind, bad, optional)
    assert args.untouched()


def test_unknown_kinds_are_rejected(lib):
    import kselect
    args = Args()
    for kind in (-1, -2, 4, 99):
        assert call(lib, kind, args.base()) == kselect.KTH_EINVAL, kind
        a = args.base()
        a.update(rows=0)  # the check comes first even then
        assert call(lib, kind, a) == kselect.KTH_EINVAL, kind
    assert args.untouched()


def test_rows_zero_is_ok(lib):
    import kselect
    args = Args()
    for kind in ("i32", "f32", kselect.KTH_K16_I16, kselect.KTH_K16_BF16):
        for k in (1, 8, 4096):
            a = args.base()
            a.update(rows=0, k=k)
            assert call(lib, kind, a) == kselect.KTH_OK
            a.update(idx=None, cnt=None, largest=0)
            assert call(lib, kind, a) == kselect.KTH_OK
    assert args.untouched()


def test_no_device_no_ctx():
    """Without a GPU no ctx exists (KTH_ENODEV from its creation), so no sort can run on the host
    instead; with one, the ctx is created and a sort of no rows succeeds."""
    import torch

    import kselect
    if torch.cuda.is_available():
        sel = kselect.Selector(0)
        sel.sort_topk_rows(torch.zeros(8, dtype=torch.int32, device="cuda"), None, 0, 8)
        sel.close()
        return
    with pytest.raises(kselect.KthError) as e:
        kselect.Selector(0)
    assert e.value.code == kselect.KTH_ENODEV


def _no_ctx_selector():
    import kselect
    sel = kselect.Selector.__new__(kselect.Selector)  # no kth_ctx_create: works without a device
    sel._ctx = ctypes.c_void_p()
    return sel


def test_sort_wrapper_refuses_other_dtypes():
    import torch

    import kselect
    sel = _no_ctx_selector()
    i32, f32 = torch.zeros(32, dtype=torch.int32), torch.zeros(32, dtype=torch.float32)
    bf, h, i16 = (torch.zeros(32, dtype=dt) for dt in (torch.bfloat16, torch.float16, torch.int16))
    for bad in (f32, torch.zeros(32, dtype=torch.int64), torch.zeros(32, dtype=torch.float64)):
        with pytest.raises(TypeError, match="d_vals must be int32"):
            sel.sort_topk_rows(bad, i32, 4, 8)
    for bad in (i32, bf, torch.zeros(32, dtype=torch.float64)):
        with pytest.raises(TypeError, match="d_vals must be float32"):
            sel.sort_topk_rows(bad, i32, 4, 8, f32=True)
    for bad in (i32, f32):
        with pytest.raises(TypeError, match="d_vals must be int16, uint16, float16 or bfloat16"):
            sel.sort_topk_rows(bad, i32, 4, 8, kind="bf16")
    with pytest.raises(ValueError, match="unknown 16-bit key kind"):
        sel.sort_topk_rows(i16, i32, 4, 8, kind="f8")
    for vals, kw in ((i32, {}), (f32, dict(f32=True)), (bf, {}), (i16, dict(kind="bf16"))):
        for other in (torch.zeros(32, dtype=torch.int64), f32, i16):
            with pytest.raises(TypeError, match="d_idx must be int32"):
                sel.sort_topk_rows(vals, other, 4, 8, **kw)
            with pytest.raises(TypeError, match="d_cnt must be int32"):
                sel.sort_topk_rows(vals, i32, 4, 8, d_cnt=other, **kw)
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for fn in (lambda: sel.sort_topk_rows(i32, i32, 4, 8, largest=True, d_cnt=i32),
               lambda: sel.sort_topk_rows(f32, None, 4, 8, f32=True),
               lambda: sel.sort_topk_rows(h, i32, 4, 8),
               lambda: sel.sort_topk_rows(bf, None, 4, 8, d_cnt=i32),
               lambda: sel.sort_topk_rows(i16, i32, 4, 8, kind="bf16", largest=True)):
        with pytest.raises(kselect.KthError) as e:
            fn()
        assert e.value.code == kselect.KTH_EINVAL


def _wrappers(sel):
    """(name, needs d_cnt, call(d_vals, d_idx, k, d_cnt, sorted)) of the eight wrappers, over host
    tensors: every call here is refused before it reaches the library."""
    import torch
    keys = {"i32": torch.zeros(4, 8192, dtype=torch.int32), "f32": torch.zeros(4, 8192, dtype=torch.float32),
            "bf16": torch.zeros(4, 8192, dtype=torch.bfloat16)}
    return [
        ("topk_rows", False, "i32", lambda v, i, k, c, s: sel.topk_rows(keys["i32"], 4, 8192, k, v, i, sorted=s)),
        ("topk_rows16", False, "bf16", lambda v, i, k, c, s: sel.topk_rows16(keys["bf16"], 4, 8192, k, v, i, sorted=s)),
        ("topk_rows_wide", False, "f32",
         lambda v, i, k, c, s: sel.topk_rows_wide(keys["f32"], 4, 8192, k, v, i, f32=True, sorted=s)),
        ("topk_rows_wide16", False, "bf16",
         lambda v, i, k, c, s: sel.topk_rows_wide16(keys["bf16"], 4, 8192, k, v, i, sorted=s)),
        ("topk_rows_wide_var", True, "i32",
         lambda v, i, k, c, s: sel.topk_rows_wide_var(keys["i32"], 4, 8192, k, v, i, d_cnt=c, sorted=s)),
        ("topk_rows_wide16_var", True, "bf16",
         lambda v, i, k, c, s: sel.topk_rows_wide16_var(keys["bf16"], 4, 8192, k, v, i, d_cnt=c, sorted=s)),
        ("topp_rows_wide", True, "f32",
         lambda v, i, k, c, s: sel.topp_rows_wide(keys["f32"], 4, 8192, k, v, i, p=0.9, d_cnt=c, sorted=s)),
        ("topp_rows_wide16", True, "bf16",
         lambda v, i, k, c, s: sel.topp_rows_wide16(keys["bf16"], 4, 8192, k, v, i, p=0.9, d_cnt=c, sorted=s)),
    ]


def test_sorted_true_value_errors_before_anything_is_enqueued():
    """sorted=True without d_vals, with k above KTH_SORT_MAX_K, and (var, top-p) without d_cnt:
    ValueError from each of the eight wrappers, on a Selector that has no ctx to enqueue on, with
    the outputs as they were; the same arguments with sorted=False reach the library."""
    import torch

    import kselect
    sel = _no_ctx_selector()
    dts = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16}
    for name, needs_cnt, flavour, fn in _wrappers(sel):
        vals = torch.full((4 * 5000,), 7, dtype=dts[flavour])
        idx = torch.full((4 * 5000,), -9, dtype=torch.int32)
        cnt = torch.full((4,), 3, dtype=torch.int32)
        with pytest.raises(ValueError, match="needs d_vals"):
            fn(None, idx, 8, cnt, True)
        with pytest.raises(ValueError, match="needs k <= 4096"):
            fn(vals, idx, 4097, cnt, True)
        if needs_cnt:
            with pytest.raises(ValueError, match="needs d_cnt"):
                fn(vals, idx, 8, None, True)
        # in reach of the sort: only the library's refusal of the missing ctx is left
        for args in ((vals, idx, 8, cnt, True), (vals, idx, 8, cnt, False), (None, idx, 8, None, False),
                     (vals, idx, 4097, None, False)):
            with pytest.raises(kselect.KthError) as e:
                fn(*args)
            assert e.value.code == kselect.KTH_EINVAL, name
        assert (vals == 7).all() and (idx == -9).all() and (cnt == 3).all(), name
