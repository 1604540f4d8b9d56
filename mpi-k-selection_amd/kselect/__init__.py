"""kselect -- Python host mirror of the libkth.so C-ABI (include/kth.h).

Mirrors the reference's selection interface (laertispappas/MPI-k-selection):

  * ``IntVec`` wraps the reference's ``IntVector`` (vector.h:7-11) through
    the ABI twin in libkth.so; ``IntVec.kth_select(k)`` is the drop-in for the
    select block ``VecQuickSort(pVec); VecGet(pVec, k - 1)``
    (kth-problem-seq.c:32-33), keeping the VecGet sentinels (-1 NULL, -2 out of
    range, vector.c:209-218).
  * ``kth_select(keys, k)`` / ``Selector`` -- the (data, n, k) -> value contract
    with explicit errors (``KthError``) instead of in-band sentinels.  Keys are
    int32 by default; ``f32=True`` on ``kth_select``, ``Selector.select``,
    ``Selector.select_async`` and ``Selector.topk`` (as on ``rows`` and
    ``topk_rows``) takes float32 keys in IEEE total order: -0.0 < +0.0,
    subnormals distinct, every NaN above +inf and returned as 0x7FC00000.
    Without it a float array is still converted to int32 (numpy) or read as
    int32 words (tensors), as before.
  * ``kselect.dist`` -- the sharded (one process per GPU) replacement of the CGM
    driver TODO-kth-problem-cgm.c:76-278, with RCCL collectives through
    torch.distributed.

PyTorch is used only as plumbing (device memory, streams, collectives); every
selection runs in the HIP kernels of libkth.so.  There is no CPU fallback:
without the library ``kselect`` fails to import, and without a GPU every
compute call raises ``KthError(KTH_ENODEV)``.
"""
import ctypes

import numpy as np

from ._lib import (  # noqa: F401
    KTH_DIST_DONE,
    KTH_DIST_MAX_LEVELS,
    KTH_ECOMM,
    KTH_EINTERNAL,
    KTH_EINVAL,
    KTH_ENODEV,
    KTH_FINISH_COUNTS,
    KTH_FINISH_GROUPED,
    KTH_FINISH_LEVELS,
    KTH_FINISH_NONE,
    KTH_FINISH_SLICES,
    KTH_HOOK_FAULT_BARRIER,
    KTH_HOOK_FAULT_TOPK_RANK,
    KTH_HOOK_FINISH_SLICES,
    KTH_HOOK_K16_MISS,
    KTH_HOOK_K16_TOPK_NOSKIP,
    KTH_HOOK_TOPK_SEG_CAP,
    KTH_MULTI_MAX_RANKS,
    KTH_K16_BF16,
    KTH_K16_F16,
    KTH_K16_I16,
    KTH_K16_U16,
    KTH_OK,
    KTH_PATH_K16,
    KTH_PATH_K16_FALLBACK,
    KTH_PATH_LDS,
    KTH_PATH_RADIX,
    KTH_PATH_WINDOW,
    KTH_PATH_WINDOW_FALLBACK,
    KTH_ROWS16_MAX_COLS,
    KTH_ROWS_MAX_COLS,
    KTH_SORT_MAX_K,
    KTH_STATS_WORDS,
    KTH_TOPK_MAX_COLS,
    KTH_WIDE_MAX_COLS,
    KTH_WIDE_MAX_SLICES,
    IntVector,
    KthError,
    KthLibraryMissing,
    KthStats,
    check,
    check_single_runtime,
    hip_runtimes,
    load,
    strerror,
)

LIB = load()

# synthetic input families (oracle/kth_oracle.h enum ko_dist)
UNIFORM_FULL, UNIFORM_HALF, UNIFORM_REF, ALL_EQUAL, FEW_DISTINCT, SORTED_ASC, SORTED_DESC, MOD_1000 = range(8)
FAMILIES = {
    "uniform_full": UNIFORM_FULL,
    "uniform_half": UNIFORM_HALF,
    "uniform_ref": UNIFORM_REF,
    "all_equal": ALL_EQUAL,
    "few_distinct": FEW_DISTINCT,
    "sorted_asc": SORTED_ASC,
    "sorted_desc": SORTED_DESC,
    "mod_1000": MOD_1000,
}
DEFAULT_SEED = 0x5EED0001


def device_count():
    return LIB.kth_device_count()


def wide_rows_plan(rows, cols, num_cu):
    """(slices, slice_keys, group_rows, scratch_bytes) of the automatic
    wide-rows plan (kth_wide_rows_plan; host arithmetic, no device needed)."""
    s, sk, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    b = ctypes.c_int64()
    check(LIB.kth_wide_rows_plan(int(rows), int(cols), int(num_cu), ctypes.byref(s), ctypes.byref(sk), ctypes.byref(g),
                                 ctypes.byref(b)), "kth_wide_rows_plan")
    return s.value, sk.value, g.value, b.value


def wide_rows_plan16(rows, cols, num_cu):
    """wide_rows_plan for the 16-bit wide-rows calls (kth_wide_rows_plan_k16):
    slice_keys is a multiple of 8."""
    s, sk, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    b = ctypes.c_int64()
    check(LIB.kth_wide_rows_plan_k16(int(rows), int(cols), int(num_cu), ctypes.byref(s), ctypes.byref(sk),
                                     ctypes.byref(g), ctypes.byref(b)), "kth_wide_rows_plan_k16")
    return s.value, sk.value, g.value, b.value


def _ptr(x):
    """Raw address of a torch tensor / numpy array / int."""
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError(f"cannot take the address of {type(x)}")


def _numel(x):
    return x.numel() if hasattr(x, "numel") else len(x)


def _need_f32(x, what):
    """f32=True: anything that carries a dtype (tensor or array) must be float32."""
    dt = getattr(x, "dtype", None)
    if dt is not None and str(dt).rsplit(".", 1)[-1] != "float32":
        raise TypeError(f"{what} must be float32 with f32=True, got {dt}")


def _need_i32(x, what):
    """Anything that carries a dtype (tensor or array) must be int32; None passes."""
    dt = getattr(x, "dtype", None)
    if dt is not None and str(dt).rsplit(".", 1)[-1] != "int32":
        raise TypeError(f"{what} must be int32, got {dt}")


def _ptr_or_none(x):
    return None if x is None else _ptr(x)


def _f32_from_bits(bits):
    """np.float32 holding exactly these 32 bits (signed zeros, subnormals and the NaN kept)."""
    return np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


def _rank_groups(ks):
    """The ranks as (offset, ctypes int64 array) groups of at most KTH_MULTI_MAX_RANKS."""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("ks is empty")
    for at in range(0, len(ks), KTH_MULTI_MAX_RANKS):
        part = ks[at:at + KTH_MULTI_MAX_RANKS]
        yield at, (ctypes.c_int64 * len(part))(*part)


def _multi_host_keys(keys, f32):
    """select_multi's keys: a host array in the call's dtype, a tensor checked with f32=True."""
    if isinstance(keys, np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=np.float32 if f32 else np.int32)
    if f32:
        _need_f32(keys, "keys")
    return keys


K16_KINDS = {"i16": KTH_K16_I16, "u16": KTH_K16_U16, "f16": KTH_K16_F16, "bf16": KTH_K16_BF16}
_K16_OF_DTYPE = {"int16": KTH_K16_I16, "uint16": KTH_K16_U16, "float16": KTH_K16_F16, "bfloat16": KTH_K16_BF16}
_K16_NUMPY = {KTH_K16_I16: np.int16, KTH_K16_U16: np.uint16, KTH_K16_F16: np.float16}


def _k16_kind(x, kind, what="keys"):
    """The KTH_K16_* kind of 16-bit keys: from the dtype (torch int16 / uint16 /
    float16 / bfloat16, numpy int16 / uint16 / float16), or `kind` ("i16", "u16",
    "f16", "bf16" or a KTH_K16_* value) over any 2-byte dtype -- a numpy uint16
    array with kind="bf16" carries bfloat16 bits.  Anything else is a TypeError:
    nothing is converted."""
    dt = getattr(x, "dtype", None)
    name = str(dt).rsplit(".", 1)[-1] if dt is not None else None
    if name is not None and name not in _K16_OF_DTYPE:
        raise TypeError(f"{what} must be int16, uint16, float16 or bfloat16, got {dt}")
    if kind is None:
        if name is None:
            raise TypeError(f"{what} carries no dtype: pass kind=")
        return _K16_OF_DTYPE[name]
    if isinstance(kind, str):
        if kind not in K16_KINDS:
            raise ValueError(f"unknown 16-bit key kind {kind!r}")
        return K16_KINDS[kind]
    return int(kind)


def _k16_same_kind(keys, out, kind, what):
    """An output of the 16-bit rows calls: a 2-byte dtype that names the call's
    kind, or the keys' own dtype (int16 words carrying bfloat16 bits, kind="bf16",
    come back as int16 words).  Anything else is a TypeError."""
    dt = getattr(out, "dtype", None)
    if dt is None:
        return
    if _k16_kind(out, None, what) != kind and str(dt) != str(getattr(keys, "dtype", None)):
        raise TypeError(f"{what} must have the keys' 16-bit kind, got {dt}")


def _k16_host_keys(keys):
    return np.ascontiguousarray(keys) if isinstance(keys, np.ndarray) else keys


def _k16_values(bits, kind):
    """The answers' bits (numpy uint16 array) as exact values: int16 / uint16 /
    float16, and for bfloat16 np.float32 whose upper 16 bits are the answer."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if kind == KTH_K16_BF16:
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(_K16_NUMPY[kind])


def _sort_kind(d_vals, d_idx, d_cnt, f32, kind):
    """The dtype checks of sort_topk_rows.  Returns the call's flavour: "i32",
    "f32" or a KTH_K16_* kind (kind given, or d_vals of a 16-bit dtype)."""
    _need_i32(d_idx, "d_idx")
    _need_i32(d_cnt, "d_cnt")
    if f32:
        _need_f32(d_vals, "d_vals")
        return "f32"
    name = str(getattr(d_vals, "dtype", "")).rsplit(".", 1)[-1]
    if kind is not None or name in _K16_OF_DTYPE:
        return _k16_kind(d_vals, kind, "d_vals")
    _need_i32(d_vals, "d_vals")
    return "i32"


def _sorted_check(d_vals, k, d_cnt=None, need_cnt=False):
    """sorted=True of the top-k wrappers: what the sort that follows cannot do
    without, refused before anything is enqueued."""
    if d_vals is None:
        raise ValueError("sorted=True needs d_vals: the sort orders the values")
    if int(k) > KTH_SORT_MAX_K:
        raise ValueError(f"sorted=True needs k <= {KTH_SORT_MAX_K}, got {int(k)}")
    if need_cnt and d_cnt is None:
        raise ValueError("sorted=True needs d_cnt: the sort must know where each row's padding starts")


def _stream_handle(stream):
    """hipStream_t of a torch stream (0 / None = the null stream, torch's default)."""
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream or None
    return stream.cuda_stream or None  # torch.cuda.Stream


class Selector:
    """A kth_ctx: scratch, stream and timing for repeated selections on one GPU."""

    def __init__(self, device=0, stream=None):
        self._ctx = ctypes.c_void_p()
        check(LIB.kth_ctx_create(device, ctypes.byref(self._ctx)), "kth_ctx_create")
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if self._ctx:
            LIB.kth_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._ctx

    def set_stream(self, stream):
        if stream is not None and not isinstance(stream, int):
            check_single_runtime()  # a torch stream handle is only meaningful to torch's runtime
        check(LIB.kth_ctx_set_stream(self._ctx, _stream_handle(stream)), "kth_ctx_set_stream")

    def sync(self):
        check(LIB.kth_ctx_sync(self._ctx), "kth_ctx_sync")

    def reserve(self, n):
        check(LIB.kth_ctx_reserve(self._ctx, int(n)), "kth_ctx_reserve")

    # -- selection ---------------------------------------------------------
    def select(self, keys, k, n=None, f32=False):
        """k-th smallest (1-based) of int32 keys (host numpy array or device tensor).
        f32=True: float32 keys (a host array is taken as np.float32, a tensor must
        be float32); returns an np.float32 with the answer's exact bits."""
        if n is None:
            n = keys.numel() if hasattr(keys, "numel") else len(keys)
        if f32:
            if isinstance(keys, np.ndarray):
                keys = np.ascontiguousarray(keys, dtype=np.float32)
            _need_f32(keys, "keys")
            bits = ctypes.c_uint32()
            check(LIB.kth_select_f32_ctx(self._ctx, _ptr(keys), int(n), int(k), ctypes.byref(bits)),
                  "kth_select_f32_ctx")
            return _f32_from_bits(bits.value)
        if isinstance(keys, np.ndarray):
            keys = np.ascontiguousarray(keys, dtype=np.int32)
        out = ctypes.c_int32()
        check(LIB.kth_select_i32_ctx(self._ctx, _ptr(keys), int(n), int(k), ctypes.byref(out)),
              "kth_select_i32_ctx")
        return out.value

    def select_async(self, d_keys, n, k, d_out, f32=False):
        """Enqueue a select of device keys; the answer lands in device int32 *d_out
        (f32=True: float32 keys, float32 *d_out)."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_out, "d_out")
            check(LIB.kth_select_f32_async(self._ctx, _ptr(d_keys), int(n), int(k), _ptr(d_out)),
                  "kth_select_f32_async")
            return
        check(LIB.kth_select_i32_async(self._ctx, _ptr(d_keys), int(n), int(k), _ptr(d_out)),
              "kth_select_i32_async")

    def select_multi(self, keys, ks, n=None, f32=False):
        """The ks[i]-th smallest (1-based) of the keys for every rank in ks, in one
        streaming pass per group of KTH_MULTI_MAX_RANKS ranks (kth_select_multi_*_ctx):
        a numpy int32 array (f32=True: float32 with the answers' exact bits).  Keys
        as Selector.select; any order of ranks, duplicates allowed."""
        keys = _multi_host_keys(keys, f32)
        if n is None:
            n = _numel(keys)
        fn, what = ((LIB.kth_select_multi_f32_ctx, "kth_select_multi_f32_ctx") if f32
                    else (LIB.kth_select_multi_i32_ctx, "kth_select_multi_i32_ctx"))
        groups = list(_rank_groups(ks))
        out = np.empty(sum(len(g) for _, g in groups), dtype=np.float32 if f32 else np.int32)
        for at, g in groups:
            check(fn(self._ctx, _ptr(keys), int(n), g, len(g), out[at:].ctypes.data), what)
        return out

    def select_multi_async(self, d_keys, n, ks, d_out, f32=False):
        """Enqueue the selection of every rank in ks over device keys; answer i lands
        in device int32 d_out[i] (f32=True: float32 keys, float32 d_out).  d_out holds
        len(ks) contiguous elements."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_out, "d_out")
        fn, what = ((LIB.kth_select_multi_f32_async, "kth_select_multi_f32_async") if f32
                    else (LIB.kth_select_multi_i32_async, "kth_select_multi_i32_async"))
        for at, g in _rank_groups(ks):
            check(fn(self._ctx, _ptr(d_keys), int(n), g, len(g), _ptr(d_out) + 4 * at), what)

    def reserve_multi(self, n, m):
        """Pre-size the scratch of multi calls of m ranks (at most a group's
        KTH_MULTI_MAX_RANKS at a time) over n keys."""
        check(LIB.kth_ctx_reserve_multi(self._ctx, int(n), min(int(m), KTH_MULTI_MAX_RANKS)), "kth_ctx_reserve_multi")

    def multi_stats(self, i):
        """Stats of rank i of the last group of ranks sent (kth_ctx_multi_stats)."""
        st = KthStats()
        check(LIB.kth_ctx_multi_stats(self._ctx, int(i), ctypes.byref(st)), "kth_ctx_multi_stats")
        return st.as_dict()

    # -- 16-bit keys ---------------------------------------------------------
    def select16(self, keys, k, n=None, kind=None):
        """k-th smallest (1-based) of int16 / uint16 / float16 / bfloat16 keys (host
        numpy array or device tensor; `kind` as _k16_kind): a numpy scalar of the
        keys' type with the answer's exact bits (bfloat16: np.float32)."""
        return self.select16_multi(keys, [k], n=n, kind=kind)[0]

    def select16_async(self, d_keys, n, k, d_out, kind=None):
        """Enqueue a 16-bit select of device keys; the answer's bits land in the
        2-byte element *d_out."""
        self.select16_multi_async(d_keys, n, [k], d_out, kind=kind)

    def select16_multi(self, keys, ks, n=None, kind=None):
        """The ks[i]-th smallest of 16-bit keys for every rank in ks, one streaming
        pass per group of KTH_MULTI_MAX_RANKS ranks (kth_select_multi_k16_ctx)."""
        kind = _k16_kind(keys, kind)
        keys = _k16_host_keys(keys)
        if n is None:
            n = _numel(keys)
        groups = list(_rank_groups(ks))
        out = np.empty(sum(len(g) for _, g in groups), dtype=np.uint16)
        for at, g in groups:
            check(LIB.kth_select_multi_k16_ctx(self._ctx, _ptr(keys), int(n), g, len(g), kind, out[at:].ctypes.data),
                  "kth_select_multi_k16_ctx")
        return _k16_values(out, kind)

    def select16_multi_async(self, d_keys, n, ks, d_out, kind=None):
        """Enqueue the 16-bit selection of every rank in ks over device keys; answer
        i's bits land in the 2-byte element d_out[i] (len(ks) contiguous elements)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        _k16_kind(d_out, kind, "d_out")
        for at, g in _rank_groups(ks):
            check(LIB.kth_select_multi_k16_async(self._ctx, _ptr(d_keys), int(n), g, len(g), kind, _ptr(d_out) + 2 * at),
                  "kth_select_multi_k16_async")

    def reserve16(self, n, m=1):
        """Pre-size the scratch of 16-bit calls (kth_ctx_reserve_k16)."""
        check(LIB.kth_ctx_reserve_k16(self._ctx, int(n), min(int(m), KTH_MULTI_MAX_RANKS)), "kth_ctx_reserve_k16")

    def coop(self):
        """True while the ctx runs the cooperative grid-barrier kernels (kth_ctx_coop)."""
        r = LIB.kth_ctx_coop(self._ctx)
        if r < 0:
            check(r, "kth_ctx_coop")
        return bool(r)

    def test_hook(self, hook, value):
        """TESTS ONLY: turn a fault injector of this ctx on or off
        (kth_ctx_test_hook; KTH_HOOK_* in include/kth.h)."""
        check(LIB.kth_ctx_test_hook(self._ctx, int(hook), int(value)), "kth_ctx_test_hook")

    def stats(self):
        st = KthStats()
        check(LIB.kth_ctx_last_stats(self._ctx, ctypes.byref(st)), "kth_ctx_last_stats")
        return st.as_dict()

    def finish_form(self):
        """How the cooperative finish of the last select ended: one of KTH_FINISH_*
        (kth_ctx_last_finish_form; synchronises)."""
        form = ctypes.c_int(-1)
        check(LIB.kth_ctx_last_finish_form(self._ctx, ctypes.byref(form)), "kth_ctx_last_finish_form")
        return form.value

    def rows(self, d_keys, rows, cols, k, d_out, f32=False):
        fn = LIB.kth_select_rows_f32 if f32 else LIB.kth_select_rows_i32
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(k), _ptr(d_out)), "kth_select_rows")

    def sort_topk_rows(self, d_vals, d_idx, rows, k, largest=False, f32=False, kind=None, d_cnt=None):
        """Stable in-place sort of each row of a rows x k top-k output, best
        first (kth_sort_topk_rows_*; asynchronous on the ctx stream): the first
        clamp(d_cnt[r], 0, k) entries of row r (all k when d_cnt is None),
        ascending in the order key, descending with largest=True; equal keys
        keep their input order; the other entries are neither read nor written.
        d_vals: int32, float32 with f32=True, or 16-bit elements (`kind` as
        _k16_kind); d_idx: the int32 payload moved with the values, or None."""
        flavour = _sort_kind(d_vals, d_idx, d_cnt, f32, kind)
        head = (self._ctx, _ptr(d_vals), _ptr_or_none(d_idx), int(rows), int(k), _ptr_or_none(d_cnt),
                1 if largest else 0)
        if flavour == "f32":
            check(LIB.kth_sort_topk_rows_f32(*head), "kth_sort_topk_rows_f32")
        elif flavour == "i32":
            check(LIB.kth_sort_topk_rows_i32(*head), "kth_sort_topk_rows_i32")
        else:
            check(LIB.kth_sort_topk_rows_k16(*head, flavour), "kth_sort_topk_rows_k16")

    def topk_rows(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, f32=False, sorted=False):
        """Per row: the k smallest (largest=True: largest) keys and their columns,
        in column order, ties broken by column (kth_topk_rows_*).  sorted=True:
        best first instead, ties still by column (sort_topk_rows on the same
        stream; needs d_vals and k <= KTH_SORT_MAX_K)."""
        if sorted:
            _sorted_check(d_vals, k)
            _sort_kind(d_vals, d_idx, None, f32, None)
        fn = LIB.kth_topk_rows_f32 if f32 else LIB.kth_topk_rows_i32
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(k), 1 if largest else 0,
                 _ptr(d_vals) if d_vals is not None else None, _ptr(d_idx) if d_idx is not None else None),
              "kth_topk_rows")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, f32=f32)

    def rows16(self, d_keys, rows, cols, k, d_out, kind=None):
        """Per row of a rows x cols matrix of 16-bit device keys: the bits of the
        k-th smallest into the 2-byte element d_out[r] (kth_select_rows_k16;
        asynchronous on the ctx stream).  `kind` as _k16_kind; d_out must be a
        2-byte dtype of the keys' kind.  Nothing is converted."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        _k16_same_kind(d_keys, d_out, kind, "d_out")
        check(LIB.kth_select_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols), int(k), kind, _ptr(d_out)),
              "kth_select_rows_k16")

    def topk_rows16(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, kind=None, sorted=False):
        """Per row of 16-bit device keys: the k smallest (largest=True: largest)
        keys and their int32 columns, in column order, ties broken by column
        (kth_topk_rows_k16).  d_vals: rows x k 2-byte elements of the keys' kind
        (a NaN canonical), d_idx: rows x k int32; either may be None, not both.
        sorted as in topk_rows."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_vals is not None:
            _k16_same_kind(d_keys, d_vals, kind, "d_vals")
        dt = getattr(d_idx, "dtype", None)
        if dt is not None and str(dt).rsplit(".", 1)[-1] != "int32":
            raise TypeError(f"d_idx must be int32, got {dt}")
        if sorted:
            _sorted_check(d_vals, k)
        check(LIB.kth_topk_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols), int(k), 1 if largest else 0, kind,
                                    _ptr(d_vals) if d_vals is not None else None,
                                    _ptr(d_idx) if d_idx is not None else None), "kth_topk_rows_k16")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, kind=kind)

    def rows_wide(self, d_keys, rows, cols, k, d_out, f32=False, ld=None):
        """Per row of a rows x cols matrix of int32 (f32=True: float32) device
        keys, cols up to KTH_WIDE_MAX_COLS: the k-th smallest into d_out[r]
        (kth_select_wide_rows_*; asynchronous on the ctx stream).  ld: elements
        from one row to the next (default cols)."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_out, "d_out")
        fn, what = ((LIB.kth_select_wide_rows_f32, "kth_select_wide_rows_f32") if f32 else
                    (LIB.kth_select_wide_rows_i32, "kth_select_wide_rows_i32"))
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld), int(k), _ptr(d_out)),
              what)

    def topk_rows_wide(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, f32=False, ld=None,
                       sorted=False):
        """Per row of such a matrix: the k smallest (largest=True: largest) keys
        and their int32 columns, in column order, ties broken by column
        (kth_topk_wide_rows_*).  d_vals: rows x k of the keys' type, d_idx: rows
        x k int32; either may be None, not both.  sorted as in topk_rows."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_vals, "d_vals")
        dt = getattr(d_idx, "dtype", None)
        if dt is not None and str(dt).rsplit(".", 1)[-1] != "int32":
            raise TypeError(f"d_idx must be int32, got {dt}")
        if sorted:
            _sorted_check(d_vals, k)
            _sort_kind(d_vals, d_idx, None, f32, None)
        fn, what = ((LIB.kth_topk_wide_rows_f32, "kth_topk_wide_rows_f32") if f32 else
                    (LIB.kth_topk_wide_rows_i32, "kth_topk_wide_rows_i32"))
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld), int(k),
                 1 if largest else 0, _ptr(d_vals) if d_vals is not None else None,
                 _ptr(d_idx) if d_idx is not None else None), what)
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, f32=f32)

    def rows_wide16(self, d_keys, rows, cols, k, d_out, kind=None, ld=None):
        """rows16 for rows of up to KTH_WIDE_MAX_COLS columns: per row of 16-bit
        device keys the bits of the k-th smallest into the 2-byte element
        d_out[r] (kth_select_wide_rows_k16; asynchronous on the ctx stream).
        ld: elements from one row to the next (default cols)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        _k16_same_kind(d_keys, d_out, kind, "d_out")
        check(LIB.kth_select_wide_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols),
                                           int(cols if ld is None else ld), int(k), kind, _ptr(d_out)),
              "kth_select_wide_rows_k16")

    def topk_rows_wide16(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, kind=None, ld=None,
                         sorted=False):
        """topk_rows16 for such rows: the k smallest (largest=True: largest) keys
        and their int32 columns, in column order, ties broken by column
        (kth_topk_wide_rows_k16).  d_vals: rows x k 2-byte elements of the keys'
        kind (a NaN canonical), d_idx: rows x k int32; either may be None.
        sorted as in topk_rows."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_vals is not None:
            _k16_same_kind(d_keys, d_vals, kind, "d_vals")
        dt = getattr(d_idx, "dtype", None)
        if dt is not None and str(dt).rsplit(".", 1)[-1] != "int32":
            raise TypeError(f"d_idx must be int32, got {dt}")
        if sorted:
            _sorted_check(d_vals, k)
        check(LIB.kth_topk_wide_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld),
                                         int(k), 1 if largest else 0, kind,
                                         _ptr(d_vals) if d_vals is not None else None,
                                         _ptr(d_idx) if d_idx is not None else None), "kth_topk_wide_rows_k16")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, kind=kind)

    def rows_wide_var(self, d_keys, rows, cols, k, d_out, f32=False, d_lens=None, d_ks=None, ld=None):
        """rows_wide with a length and a rank per row, read on the device when
        the launches run (kth_select_wide_rows_var_*): row r is its first
        clamp(d_lens[r], 0, cols) columns and its rank clamp(d_ks[r], 1, that);
        an empty row writes the zero word.  d_lens, d_ks: `rows` int32 device
        elements, None: cols / k for every row."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_out, "d_out")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        fn, what = ((LIB.kth_select_wide_rows_var_f32, "kth_select_wide_rows_var_f32") if f32 else
                    (LIB.kth_select_wide_rows_var_i32, "kth_select_wide_rows_var_i32"))
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld), _ptr_or_none(d_lens),
                 _ptr_or_none(d_ks), int(k), _ptr(d_out)), what)

    def topk_rows_wide_var(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, f32=False,
                           d_lens=None, d_ks=None, d_cnt=None, ld=None, sorted=False):
        """topk_rows_wide with a length and a k per row, read on the device when
        the launches run (kth_topk_wide_rows_var_*).  k is the output stride and
        the bound of every row's k_r = min(clamp(d_ks[r], 0, k), len_r); entries
        [k_r, k) of a row are written as padding (index -1, the zero word) and
        d_cnt[r] = k_r.  d_lens, d_ks, d_cnt: `rows` int32 device elements, each
        may be None.  sorted=True: the k_r entries best first, the padding left
        where it is (sort_topk_rows with this d_cnt, which it then needs)."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_vals, "d_vals")
        _need_i32(d_idx, "d_idx")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        if sorted:
            _sorted_check(d_vals, k, d_cnt, need_cnt=True)
            _sort_kind(d_vals, d_idx, d_cnt, f32, None)
        fn, what = ((LIB.kth_topk_wide_rows_var_f32, "kth_topk_wide_rows_var_f32") if f32 else
                    (LIB.kth_topk_wide_rows_var_i32, "kth_topk_wide_rows_var_i32"))
        check(fn(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld), _ptr_or_none(d_lens),
                 _ptr_or_none(d_ks), int(k), 1 if largest else 0, _ptr_or_none(d_vals), _ptr_or_none(d_idx),
                 _ptr_or_none(d_cnt)), what)
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, f32=f32, d_cnt=d_cnt)

    def rows_wide16_var(self, d_keys, rows, cols, k, d_out, kind=None, d_lens=None, d_ks=None, ld=None):
        """rows_wide_var for rows of 16-bit keys (kth_select_wide_rows_var_k16)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        _k16_same_kind(d_keys, d_out, kind, "d_out")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        check(LIB.kth_select_wide_rows_var_k16(self._ctx, _ptr(d_keys), int(rows), int(cols),
                                               int(cols if ld is None else ld), _ptr_or_none(d_lens),
                                               _ptr_or_none(d_ks), int(k), kind, _ptr(d_out)),
              "kth_select_wide_rows_var_k16")

    def topk_rows_wide16_var(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, largest=False, kind=None,
                             d_lens=None, d_ks=None, d_cnt=None, ld=None, sorted=False):
        """topk_rows_wide_var for rows of 16-bit keys (kth_topk_wide_rows_var_k16)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_vals is not None:
            _k16_same_kind(d_keys, d_vals, kind, "d_vals")
        _need_i32(d_idx, "d_idx")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        if sorted:
            _sorted_check(d_vals, k, d_cnt, need_cnt=True)
        check(LIB.kth_topk_wide_rows_var_k16(self._ctx, _ptr(d_keys), int(rows), int(cols),
                                             int(cols if ld is None else ld), _ptr_or_none(d_lens), _ptr_or_none(d_ks),
                                             int(k), 1 if largest else 0, kind, _ptr_or_none(d_vals),
                                             _ptr_or_none(d_idx), _ptr_or_none(d_cnt)), "kth_topk_wide_rows_var_k16")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=largest, kind=kind, d_cnt=d_cnt)

    def nucleus_rows_wide(self, d_keys, rows, cols, d_n=None, d_thr=None, p=1.0, temp=1.0, d_lens=None, d_ps=None,
                          d_temps=None, ld=None):
        """The top-p nucleus of every row of a float32 matrix
        (kth_nucleus_wide_rows_f32): d_n[r] = the number of the largest logits
        whose softmax mass (at temperature T_r) reaches p_r, d_thr[r] = the
        smallest of them.  d_ps, d_temps: `rows` float32 device elements, None:
        the scalars p / temp for every row; d_lens as in rows_wide_var.
        d_n (int32) and d_thr (float32) may each be None, not both."""
        _need_f32(d_keys, "d_keys")
        _need_f32(d_thr, "d_thr")
        _need_i32(d_n, "d_n")
        _need_i32(d_lens, "d_lens")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        check(LIB.kth_nucleus_wide_rows_f32(self._ctx, _ptr(d_keys), int(rows), int(cols),
                                            int(cols if ld is None else ld), _ptr_or_none(d_lens), _ptr_or_none(d_ps),
                                            float(p), _ptr_or_none(d_temps), float(temp), _ptr_or_none(d_n),
                                            _ptr_or_none(d_thr)), "kth_nucleus_wide_rows_f32")

    def nucleus_rows_wide16(self, d_keys, rows, cols, d_n=None, d_thr=None, p=1.0, temp=1.0, kind=None, d_lens=None,
                            d_ps=None, d_temps=None, ld=None):
        """nucleus_rows_wide for float16 / bfloat16 rows (kth_nucleus_wide_rows_k16)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_thr is not None:
            _k16_same_kind(d_keys, d_thr, kind, "d_thr")
        _need_i32(d_n, "d_n")
        _need_i32(d_lens, "d_lens")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        check(LIB.kth_nucleus_wide_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols),
                                            int(cols if ld is None else ld), _ptr_or_none(d_lens), _ptr_or_none(d_ps),
                                            float(p), _ptr_or_none(d_temps), float(temp), kind, _ptr_or_none(d_n),
                                            _ptr_or_none(d_thr)), "kth_nucleus_wide_rows_k16")

    def topp_rows_wide(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, p=1.0, temp=1.0, d_lens=None, d_ks=None,
                       d_ps=None, d_temps=None, d_cnt=None, ld=None, sorted=False):
        """Top-k cap and top-p nucleus of every float32 row in one call
        (kth_topp_wide_rows_f32): the outputs of topk_rows_wide_var(largest=True)
        with each row's rank min(n_r, clamp(d_ks[r], 0, k)), n_r the nucleus size
        of nucleus_rows_wide.  k is the output stride.  sorted=True: each row's
        kept entries largest first (as topk_rows_wide_var; needs d_cnt)."""
        _need_f32(d_keys, "d_keys")
        _need_f32(d_vals, "d_vals")
        _need_i32(d_idx, "d_idx")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        if sorted:
            _sorted_check(d_vals, k, d_cnt, need_cnt=True)
        check(LIB.kth_topp_wide_rows_f32(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld),
                                         _ptr_or_none(d_lens), _ptr_or_none(d_ks), int(k), _ptr_or_none(d_ps), float(p),
                                         _ptr_or_none(d_temps), float(temp), _ptr_or_none(d_vals), _ptr_or_none(d_idx),
                                         _ptr_or_none(d_cnt)), "kth_topp_wide_rows_f32")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=True, f32=True, d_cnt=d_cnt)

    def topp_rows_wide16(self, d_keys, rows, cols, k, d_vals=None, d_idx=None, p=1.0, temp=1.0, kind=None, d_lens=None,
                         d_ks=None, d_ps=None, d_temps=None, d_cnt=None, ld=None, sorted=False):
        """topp_rows_wide for float16 / bfloat16 rows (kth_topp_wide_rows_k16)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_vals is not None:
            _k16_same_kind(d_keys, d_vals, kind, "d_vals")
        _need_i32(d_idx, "d_idx")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        if sorted:
            _sorted_check(d_vals, k, d_cnt, need_cnt=True)
        check(LIB.kth_topp_wide_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld),
                                         _ptr_or_none(d_lens), _ptr_or_none(d_ks), int(k), _ptr_or_none(d_ps), float(p),
                                         _ptr_or_none(d_temps), float(temp), kind, _ptr_or_none(d_vals),
                                         _ptr_or_none(d_idx), _ptr_or_none(d_cnt)), "kth_topp_wide_rows_k16")
        if sorted:
            self.sort_topk_rows(d_vals, d_idx, rows, k, largest=True, kind=kind, d_cnt=d_cnt)

    def reserve_topp_rows(self, rows, cols):
        """Pre-size the scratch of the top-p calls, the var top-k's included
        (kth_ctx_reserve_topp_rows): later calls of up to `rows` rows allocate
        nothing."""
        check(LIB.kth_ctx_reserve_topp_rows(self._ctx, int(rows), int(cols)), "kth_ctx_reserve_topp_rows")

    def sample_rows_wide(self, d_keys, rows, cols, d_us, d_tok, k=0, p=1.0, temp=1.0, d_lens=None, d_ks=None,
                         d_ps=None, d_temps=None, d_cnt=None, ld=None):
        """One token per float32 row drawn from the top-k / top-p filtered
        softmax (kth_sample_wide_rows_f32): d_tok[r] = the column at which the
        running mass of the kept keys, largest first and ties by column, passes
        d_us[r] times their total; d_cnt[r] = how many keys were kept,
        min(nucleus size, cap).  d_us: `rows` float32 device elements the caller
        draws, uniform on [0, 1).  k / d_ks: the cap, <= 0 for none; p / d_ps,
        temp / d_temps, d_lens as in nucleus_rows_wide.  d_cnt may be None."""
        _need_f32(d_keys, "d_keys")
        _need_f32(d_us, "d_us")
        _need_i32(d_tok, "d_tok")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        check(LIB.kth_sample_wide_rows_f32(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld),
                                           _ptr_or_none(d_lens), _ptr_or_none(d_ks), int(k), _ptr_or_none(d_ps),
                                           float(p), _ptr_or_none(d_temps), float(temp), _ptr(d_us), _ptr(d_tok),
                                           _ptr_or_none(d_cnt)), "kth_sample_wide_rows_f32")

    def sample_rows_wide16(self, d_keys, rows, cols, d_us, d_tok, k=0, p=1.0, temp=1.0, kind=None, d_lens=None,
                           d_ks=None, d_ps=None, d_temps=None, d_cnt=None, ld=None):
        """sample_rows_wide for float16 / bfloat16 rows (kth_sample_wide_rows_k16)."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        _need_f32(d_us, "d_us")
        _need_i32(d_tok, "d_tok")
        _need_i32(d_lens, "d_lens")
        _need_i32(d_ks, "d_ks")
        _need_i32(d_cnt, "d_cnt")
        _need_f32(d_ps, "d_ps")
        _need_f32(d_temps, "d_temps")
        check(LIB.kth_sample_wide_rows_k16(self._ctx, _ptr(d_keys), int(rows), int(cols), int(cols if ld is None else ld),
                                           _ptr_or_none(d_lens), _ptr_or_none(d_ks), int(k), _ptr_or_none(d_ps),
                                           float(p), _ptr_or_none(d_temps), float(temp), _ptr(d_us), kind, _ptr(d_tok),
                                           _ptr_or_none(d_cnt)), "kth_sample_wide_rows_k16")

    def reserve_sample_rows(self, rows, cols):
        """Pre-size the scratch of the sample calls (kth_ctx_reserve_sample_rows):
        later calls of up to `rows` rows allocate nothing."""
        check(LIB.kth_ctx_reserve_sample_rows(self._ctx, int(rows), int(cols)), "kth_ctx_reserve_sample_rows")

    def reserve_wide_rows(self, rows, cols):
        """Pre-size the wide-rows scratch (kth_ctx_reserve_wide_rows): later
        calls of up to `rows` rows allocate nothing."""
        check(LIB.kth_ctx_reserve_wide_rows(self._ctx, int(rows), int(cols)), "kth_ctx_reserve_wide_rows")

    def wide_rows_force(self, slices=0, group_rows=0):
        """Tests and tuning: force this ctx's wide-rows plan; 0 = automatic for
        that field (kth_ctx_wide_rows_force)."""
        check(LIB.kth_ctx_wide_rows_force(self._ctx, int(slices), int(group_rows)), "kth_ctx_wide_rows_force")

    def topk(self, d_keys, n, k, d_vals=None, d_idx=None, largest=False, f32=False):
        """The k smallest (largest=True: largest) int32 keys of n device keys and
        their int64 indices, in index order, ties broken by index (kth_topk_i32;
        asynchronous on the ctx stream).  f32=True: float32 keys and values
        (kth_topk_f32; NaNs come first for largest)."""
        if f32:
            _need_f32(d_keys, "d_keys")
            _need_f32(d_vals, "d_vals")
        fn, what = (LIB.kth_topk_f32, "kth_topk_f32") if f32 else (LIB.kth_topk_i32, "kth_topk_i32")
        check(fn(self._ctx, _ptr(d_keys), int(n), int(k), 1 if largest else 0,
                 _ptr(d_vals) if d_vals is not None else None,
                 _ptr(d_idx) if d_idx is not None else None), what)

    def topk16(self, d_keys, n, k, d_vals=None, d_idx=None, largest=False, kind=None):
        """The k smallest (largest=True: largest) of n 16-bit device keys and their
        int64 indices, in index order, ties broken by index (kth_topk_k16;
        asynchronous on the ctx stream).  `kind` as _k16_kind; d_vals: k 2-byte
        elements of the keys' kind (a NaN canonical), d_idx: k int64; either may
        be None, not both.  Nothing is converted."""
        kind = _k16_kind(d_keys, kind, "d_keys")
        if d_vals is not None:
            _k16_same_kind(d_keys, d_vals, kind, "d_vals")
        dt = getattr(d_idx, "dtype", None)
        if dt is not None and str(dt).rsplit(".", 1)[-1] != "int64":
            raise TypeError(f"d_idx must be int64, got {dt}")
        check(LIB.kth_topk_k16(self._ctx, _ptr(d_keys), int(n), int(k), 1 if largest else 0, kind,
                               _ptr(d_vals) if d_vals is not None else None,
                               _ptr(d_idx) if d_idx is not None else None), "kth_topk_k16")

    def topk16_tiles(self):
        """(tiles, tiles_read) of the last topk16: its count-pass tiles and how
        many of them were loaded from the input (kth_ctx_last_topk_k16_tiles;
        synchronises)."""
        tiles, read = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(LIB.kth_ctx_last_topk_k16_tiles(self._ctx, ctypes.byref(tiles), ctypes.byref(read)),
              "kth_ctx_last_topk_k16_tiles")
        return tiles.value, read.value

    def fill(self, d_out, n, family=UNIFORM_FULL, seed=DEFAULT_SEED, param=0, offset=0, n_total=None):
        if isinstance(family, str):
            family = FAMILIES[family]
        if n_total is None:
            n_total = offset + n
        check(LIB.kth_fill_synthetic(self._ctx, _ptr(d_out), int(n), int(offset), int(n_total), int(family),
                                      ctypes.c_uint64(seed), int(param)), "kth_fill_synthetic")

    # -- timing ------------------------------------------------------------
    def enable_timing(self, on=True):
        check(LIB.kth_ctx_enable_timing(self._ctx, 1 if on else 0), "kth_ctx_enable_timing")

    def take_timing(self):
        """(selects, dominant-kernel ms summed, whole-select ms summed) since the last call."""
        n = ctypes.c_int64()
        m = ctypes.c_double()
        t = ctypes.c_double()
        check(LIB.kth_ctx_take_timing(self._ctx, ctypes.byref(n), ctypes.byref(m), ctypes.byref(t)),
              "kth_ctx_take_timing")
        return n.value, m.value, t.value


def kth_select(keys, k, f32=False):
    """One-shot (data, n, k) -> value: kth_select_i32 (kth-problem-seq.c:32-33);
    f32=True: kth_select_f32 on float32 keys, as Selector.select."""
    if f32:
        if isinstance(keys, np.ndarray):
            keys = np.ascontiguousarray(keys, dtype=np.float32)
        _need_f32(keys, "keys")
        n = keys.size if isinstance(keys, np.ndarray) else keys.numel()
        bits = ctypes.c_uint32()
        check(LIB.kth_select_f32(_ptr(keys), int(n), int(k), ctypes.byref(bits)), "kth_select_f32")
        return _f32_from_bits(bits.value)
    if isinstance(keys, np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        n = keys.size
    else:
        n = keys.numel()
    out = ctypes.c_int32()
    check(LIB.kth_select_i32(_ptr(keys), int(n), int(k), ctypes.byref(out)), "kth_select_i32")
    return out.value


def kth_select_multi(keys, ks, f32=False):
    """One-shot (data, n, ranks) -> values: kth_select_multi_i32 (f32=True:
    kth_select_multi_f32), as Selector.select_multi."""
    keys = _multi_host_keys(keys, f32)
    fn, what = ((LIB.kth_select_multi_f32, "kth_select_multi_f32") if f32
                else (LIB.kth_select_multi_i32, "kth_select_multi_i32"))
    groups = list(_rank_groups(ks))
    out = np.empty(sum(len(g) for _, g in groups), dtype=np.float32 if f32 else np.int32)
    for at, g in groups:
        check(fn(_ptr(keys), int(_numel(keys)), g, len(g), out[at:].ctypes.data), what)
    return out


def kth_select16_multi(keys, ks, kind=None):
    """One-shot kth_select_multi_k16 over 16-bit keys, as Selector.select16_multi."""
    kind = _k16_kind(keys, kind)
    keys = _k16_host_keys(keys)
    groups = list(_rank_groups(ks))
    out = np.empty(sum(len(g) for _, g in groups), dtype=np.uint16)
    for at, g in groups:
        check(LIB.kth_select_multi_k16(_ptr(keys), int(_numel(keys)), g, len(g), kind, out[at:].ctypes.data),
              "kth_select_multi_k16")
    return _k16_values(out, kind)


def kth_select16(keys, k, kind=None):
    """One-shot kth_select_k16: the k-th smallest of 16-bit keys, as Selector.select16."""
    kind = _k16_kind(keys, kind)
    keys = _k16_host_keys(keys)
    out = np.empty(1, dtype=np.uint16)
    check(LIB.kth_select_k16(_ptr(keys), int(_numel(keys)), int(k), kind, out.ctypes.data), "kth_select_k16")
    return _k16_values(out, kind)[0]


class ShardedSelector:
    """One process, several GPUs (kth_sharded_*): shard i lives on devices[i];
    the union's k-th smallest through grouped RCCL collectives
    (replaces TODO-kth-problem-cgm.c:81-278 without one process per rank)."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self._h = ctypes.c_void_p()
        check(LIB.kth_sharded_create(arr, len(self.devices), ctypes.byref(self._h)), "kth_sharded_create")

    def select(self, shards, k, sizes=None):
        """shards: one device tensor per device (int32); sizes default to numel()."""
        if len(shards) != len(self.devices):
            raise ValueError(f"{len(shards)} shards for {len(self.devices)} devices")
        sizes = [_numel(s) for s in shards] if sizes is None else [int(x) for x in sizes]
        ptrs = (ctypes.c_void_p * len(shards))(*[_ptr(s) for s in shards])
        ns = (ctypes.c_int64 * len(shards))(*sizes)
        out = ctypes.c_int32()
        check(LIB.kth_sharded_select_i32(self._h, ptrs, ns, int(k), ctypes.byref(out)), "kth_sharded_select_i32")
        return out.value

    def enqueue_us(self):
        """Host microseconds the last select spent enqueueing (kth_sharded_enqueue_us)."""
        return LIB.kth_sharded_enqueue_us(self._h)

    def close(self):
        if self._h:
            LIB.kth_sharded_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def select_sharded(shards, k, sizes=None):
    """One-shot kth_select_i32_sharded: each shard's device from its pointer."""
    sizes = [_numel(s) for s in shards] if sizes is None else [int(x) for x in sizes]
    ptrs = (ctypes.c_void_p * len(shards))(*[_ptr(s) for s in shards])
    ns = (ctypes.c_int64 * len(shards))(*sizes)
    out = ctypes.c_int32()
    check(LIB.kth_select_i32_sharded(ptrs, ns, len(shards), int(k), ctypes.byref(out)), "kth_select_i32_sharded")
    return out.value


class IntVec:
    """The reference's IntVector (vector.h:7-11) owned through libkth.so's twin."""

    def __init__(self, capacity):
        self.p = LIB.VecNew(int(capacity))
        if not self.p:
            raise MemoryError("VecNew")

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        v = cls(max(1, a.size))
        ctypes.memmove(v.p.contents.data, a.ctypes.data, a.size * 4)
        v.p.contents.size = a.size
        return v

    def add(self, x):
        return LIB.VecAdd(self.p, int(x))

    def get(self, i):
        return LIB.VecGet(self.p, int(i))

    def size(self):
        return LIB.VecGetSize(self.p)

    def array(self):
        n = self.p.contents.size
        return np.ctypeslib.as_array(self.p.contents.data, shape=(n,)).copy() if n else np.empty(0, np.int32)

    def quicksort(self):
        LIB.VecQuickSort(self.p)

    def kth_select(self, k):
        """VecKthSelect: GPU drop-in for VecQuickSort + VecGet(k-1), VecGet sentinels kept."""
        return LIB.VecKthSelect(self.p, int(k))

    def kth_select_ex(self, k):
        out = ctypes.c_int()
        check(LIB.VecKthSelectEx(self.p, int(k), ctypes.byref(out)), "VecKthSelectEx")
        return out.value

    def close(self):
        if self.p:
            LIB.VecDelete(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
