"""CPU checks of the sampling entry points (include/kth.h "wide rows, sampling"):
header / exports / PROTOS agreement, the contract's phrases, the argument check
that precedes any device work (outputs untouched), the key kinds, rows == 0,
the Python wrappers' dtype refusals and the no-device answer."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kth_sample_wide_rows_f32", "kth_sample_wide_rows_k16", "kth_ctx_reserve_sample_rows")
NAN = float("nan")


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
    at = header.index("--- wide rows, sampling")
    assert header.index("--- wide rows, top-p") < header.index("int kth_ctx_reserve_topp_rows(") < at
    for name in NAMES:
        assert at < header.index("int " + name + "(")
    section = header[at:header.index("int kth_sample_wide_rows_f32(")]
    for phrase in ("S(j) >= A (1 - e)", "(j == 1 or S(j - 1) <= A (1 + e))", "e = 2 * eps", "eps = 2^-16 + cols * 2^-39",
                   "Determinism", "no cap", "floor(u_r * S_fix(n_r)) + 1", "d_tok[r] = -1", "bit for bit"):
        assert phrase in section, phrase


class Args:
    """Valid arguments of the two calls over host buffers that no call may touch; a ctx that is
    never dereferenced, because every case here ends in the argument check (or rows == 0)."""

    def __init__(self):
        self.fake_ctx = ctypes.create_string_buffer(1 << 16)
        self.keys = np.arange(64, dtype=np.float32)
        self.lens = np.full(8, 5, dtype=np.int32)
        self.ks = np.full(8, 2, dtype=np.int32)
        self.ps = np.full(8, 0.5, dtype=np.float32)
        self.temps = np.full(8, 1.0, dtype=np.float32)
        self.us = np.full(8, 0.25, dtype=np.float32)
        self.tok = np.full(8, -7, dtype=np.int32)
        self.cnt = np.full(8, -9, dtype=np.int32)

    def base(self):
        a = self
        return dict(ctx=ctypes.addressof(a.fake_ctx), keys=a.keys.ctypes.data, rows=8, cols=8, ld=8,
                    lens=a.lens.ctypes.data, ks=a.ks.ctypes.data, k=3, ps=a.ps.ctypes.data, p=0.9,
                    temps=a.temps.ctypes.data, temp=1.0, us=a.us.ctypes.data, tok=a.tok.ctypes.data,
                    cnt=a.cnt.ctypes.data)

    def untouched(self):
        return ((self.tok == -7).all() and (self.cnt == -9).all() and (self.lens == 5).all() and (self.ks == 2).all()
                and (self.us == 0.25).all() and (self.ps == 0.5).all())


def call(lib, kind, a):
    """kind: None for float32 keys, else a KTH_K16_* value."""
    head = (a["ctx"], a["keys"], a["rows"], a["cols"], a["ld"], a["lens"], a["ks"], a["k"], a["ps"], a["p"], a["temps"],
            a["temp"], a["us"])
    if kind is None:
        return lib.kth_sample_wide_rows_f32(*head, a["tok"], a["cnt"])
    return lib.kth_sample_wide_rows_k16(*head, kind, a["tok"], a["cnt"])


BAD = [dict(ctx=None), dict(keys=None), dict(us=None), dict(tok=None), dict(rows=-1), dict(cols=0), dict(cols=-4),
       dict(cols=(1 << 24) + 1, ld=1 << 25), dict(ld=7), dict(temp=0.0), dict(temp=-1.0), dict(temp=NAN),
       dict(temp=float("inf")), dict(ps=None, p=NAN)]


def test_einval_before_any_device_work(lib):
    import kselect
    args = Args()
    for kind in (None, kselect.KTH_K16_F16, kselect.KTH_K16_BF16):
        for bad in BAD:
            a = args.base()
            a.update(bad)
            assert call(lib, kind, a) == kselect.KTH_EINVAL, (kind, bad)
    assert args.untouched()


def test_integer_and_unknown_kinds_are_rejected(lib):
    import kselect
    args = Args()
    for kind in (kselect.KTH_K16_I16, kselect.KTH_K16_U16, -1, 4, 99):
        assert call(lib, kind, args.base()) == kselect.KTH_EINVAL, kind
    assert args.untouched()


def test_rows_zero_is_ok_whatever_the_cap(lib):
    import kselect
    args = Args()
    for kind in (None, kselect.KTH_K16_F16, kselect.KTH_K16_BF16):
        for k in (3, 0, -1, 1 << 30):  # no cap is refused, none is checked against cols
            a = args.base()
            a.update(rows=0, k=k)
            assert call(lib, kind, a) == kselect.KTH_OK
            a.update(ks=None, cnt=None)
            assert call(lib, kind, a) == kselect.KTH_OK
        a.update(ps=None, p=NAN)  # the check comes first even then
        assert call(lib, kind, a) == kselect.KTH_EINVAL
    assert args.untouched()


def test_reserve_checks_its_arguments(lib):
    import kselect
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(fake)
    assert lib.kth_ctx_reserve_sample_rows(None, 4, 1024) == kselect.KTH_EINVAL
    for rows, cols in ((-1, 1024), (4, 0), (4, (1 << 24) + 1)):
        assert lib.kth_ctx_reserve_sample_rows(ctx, rows, cols) == kselect.KTH_EINVAL


def test_no_device_no_ctx():
    """Without a GPU no ctx exists (KTH_ENODEV from its creation), so no sample call can run on
    the host instead; with one, the ctx is created and a reserve succeeds."""
    import torch

    import kselect
    if torch.cuda.is_available():
        sel = kselect.Selector(0)
        sel.reserve_sample_rows(4, 4096)
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


def test_wrappers_refuse_other_dtypes():
    import torch

    import kselect
    sel = _no_ctx_selector()
    f = torch.zeros(4, 8, dtype=torch.float32)
    bf = torch.zeros(4, 8, dtype=torch.bfloat16)
    h = torch.zeros(4, 8, dtype=torch.float16)
    i32, f32 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float32)
    for bad in (torch.zeros(4, 8, dtype=torch.int32), h, torch.zeros(4, 8, dtype=torch.float64)):
        with pytest.raises(TypeError, match="d_keys must be float32"):
            sel.sample_rows_wide(bad, 4, 8, f32, i32)
    with pytest.raises(TypeError, match="d_keys must be int16, uint16, float16 or bfloat16"):
        sel.sample_rows_wide16(f, 4, 8, f32, i32)
    for dt in (torch.int64, torch.float64, torch.float16):
        other = torch.zeros(4, dtype=dt)
        for name in ("d_ps", "d_temps"):
            with pytest.raises(TypeError, match=name + " must be float32"):
                sel.sample_rows_wide(f, 4, 8, f32, i32, **{name: other})
            with pytest.raises(TypeError, match=name + " must be float32"):
                sel.sample_rows_wide16(bf, 4, 8, f32, i32, **{name: other})
        with pytest.raises(TypeError, match="d_us must be float32"):
            sel.sample_rows_wide(f, 4, 8, other, i32)
        with pytest.raises(TypeError, match="d_us must be float32"):
            sel.sample_rows_wide16(h, 4, 8, other, i32)
        with pytest.raises(TypeError, match="d_tok must be int32"):
            sel.sample_rows_wide(f, 4, 8, f32, other)
        with pytest.raises(TypeError, match="d_tok must be int32"):
            sel.sample_rows_wide16(bf, 4, 8, f32, other)
        for name in ("d_lens", "d_ks", "d_cnt"):
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.sample_rows_wide(f, 4, 8, f32, i32, **{name: other})
            with pytest.raises(TypeError, match=name + " must be int32"):
                sel.sample_rows_wide16(bf, 4, 8, f32, i32, **{name: other})
    # accepted dtypes reach the library, which refuses the missing ctx (no device needed)
    for fn in (lambda: sel.sample_rows_wide(f, 4, 8, f32, i32, k=2, p=0.9, d_ps=f32, d_temps=f32, d_lens=i32, d_ks=i32),
               lambda: sel.sample_rows_wide16(bf, 4, 8, f32, i32, p=0.5, temp=2.0, d_cnt=i32),
               lambda: sel.sample_rows_wide16(h, 4, 8, f32, i32, k=-1, d_ps=f32, ld=8),
               lambda: sel.reserve_sample_rows(4, 8)):
        with pytest.raises(kselect.KthError) as e:
            fn()
        assert e.value.code == kselect.KTH_EINVAL
