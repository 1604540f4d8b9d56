"""CPU: the inputs of tests/rows_edges.py have the structure they claim, proved on the
model alone, so that the exact comparisons of tests/test_gpu_rows_edges.py mean what
they are named for: the form matrix reaches every kernel form, every probe of an edge
row is its named boundary (the count in the picked bin, below + cnt, the span, the top
bytes of the first key slot), and every named path occurs in every form it applies to.
No device work and no library call.
"""
import re
import os

import numpy as np
import pytest

import rows_edges as E
import test_gpu_parity as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd", "csrc")


def _traces(dtype, cols, call, off=0):
    """[(edge, k, claimed fields, trace)] over the claimed probes of every edge row."""
    out = []
    for e in E.edges(dtype, cols):
        for k, want in e.claimed(call):
            out.append((e, k, want, E.trace(dtype, e.row, k, call, off)))
    return out


def _all_traces(dtype, cols, call, off=0):
    return E.once(("traces", dtype, cols, call, off),
                  lambda: [(e, k, E.trace(dtype, e.row, k, call, off)) for e in E.edges(dtype, cols) for k in e.probes(call)])


# ------------------------------------------------------------------ constants and the reference
def test_constants_are_the_kernel_s():
    with open(os.path.join(CSRC, "kth_rows.hpp")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "kth_api.hip")) as f:
        api = f.read()
    assert int(re.search(r"RW_STRIDE = RW_BINS \+ (\d+);", src).group(1)) + 256 == E.RW_STRIDE
    assert int(re.search(r"#define KTH_ROWS_R0 (\d+)", api).group(1)) == E.R0
    assert "(uint32_t)(R0 * RW_STRIDE - STAGE_OFF) / 2" in src and "constexpr int STAGE_OFF = WAVE;" in src
    assert "2 * k <= (uint32_t)(R0 * RW_STRIDE)" in src and "cnt > (uint32_t)WAVE" in src
    assert (E.STAGE_CAP, E.LDS_OUT_MAX, E.LIST_MAX) == (488, 520, 64)


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_ref_is_the_documented_argsort(dtype):
    """Ref's one argsort sliced at k is test_gpu_parity's _topk_ref at that k, on its order keys."""
    ref = E.matrix(dtype, 65)
    x = ref.bits.view(np.float32 if dtype == "f32" else np.int32)
    keys = P._f32_order_key(x).astype(np.int64) if dtype == "f32" else P._i32_order_key(x)
    for k in (1, 2, 33, 64, 65):
        for largest in (False, True):
            want = P._topk_ref(keys, k, largest)
            vals, idx = ref.topk(k, largest)
            assert np.array_equal(idx, want)
            raw = np.take_along_axis(ref.bits, want, 1)
            nan = np.take_along_axis(keys, want, 1) == 0xFFFFFFFF if dtype == "f32" else np.zeros(raw.shape, bool)
            assert np.array_equal(vals, np.where(nan, np.uint32(E.CANON_NAN), raw))
        col = np.argsort(keys, axis=1, kind="stable")[:, k - 1]
        got = ref.select(k)
        raw = ref.bits[np.arange(ref.bits.shape[0]), col]
        assert np.array_equal(got[E.order_key(dtype, got) != 0xFFFFFFFF if dtype == "f32" else slice(None)],
                              raw[E.order_key(dtype, raw) != 0xFFFFFFFF if dtype == "f32" else slice(None)])
        assert np.array_equal(E.order_key(dtype, got), E.order_key(dtype, raw))
    if dtype == "f32":  # non-canonical NaNs are there and are expected canonical
        nan = E.order_key("f32", ref.bits) == 0xFFFFFFFF
        assert (ref.bits[nan] >> 31).any() and not (ref.bits[nan] >> 31).all() and np.unique(ref.bits[nan]).size > 20
        assert (ref.select(65)[nan.any(axis=1)] == E.CANON_NAN).all()


# ------------------------------------------------------------------ the form matrix
def test_matrix_reaches_every_form():
    seen = {E.form_of(d, c, off, topk) for d in E.DTYPES for c in E.WIDTHS for off in E.OFFS for topk in (False, True)}
    assert seen == E.all_forms() and len(seen) == 36
    loads = {(d, E.wide_row_load(c, off, r)) for d in E.DTYPES for c in E.WIDE_WIDTHS for off in E.OFFS
             for r in range(E.WIDE_ROWS)}
    assert loads == {(d, p) for d in E.DTYPES for p in ("vec", "scalar")}
    for c in E.WIDE_WIDTHS:
        assert E.form_of("i32", c, 0, False).kernel == "k_rows"
    assert 520 in E.topk_ranks(1000) and 521 in E.topk_ranks(1000) and E.topk_ranks(256)[-1] == 256


def test_matrix_rows_are_the_named_ones():
    for cols in (8, 1000, 4096):
        m = E.matrix_bits(cols)
        assert m.shape == (E.ROWS, cols) and E.ROWS % 4 != 0
        x = m.view(np.float32)
        for v in (0x80000000, 0x7FFFFFFF, 0xFF7FFFFF, 0x7F7FFFFF):
            assert (m == v).all(axis=1).any()
        assert (m[6, 0::2] == E.NEG0).all() and (m[6, 1::2] == E.POS0).all()
        assert np.isinf(x[7]).all() and np.isnan(x[9]).all()
        assert ((m[8] & 0x7F800000) == 0).all()
        assert (np.diff(E.order_key("i32", m[11]).astype(np.int64)) >= 0).all()
        assert (np.diff(E.order_key("f32", m[14]).astype(np.int64)) <= 0).all()
        if cols >= 1000:
            assert np.unique(m[9]).size > cols // 2 and (m[9] >> 31).any() and not (m[9] >> 31).all()
            assert np.unique(m[15]).size == 2 and np.unique(m[20:]).size > 0.99 * m[20:].size
    w = E.matrix_bits(5000, E.WIDE_ROWS)
    assert w.shape == (E.WIDE_ROWS, 5000) and np.isnan(w.view(np.float32)).any()


# ------------------------------------------------------------------ the edge rows
@pytest.mark.parametrize("cols", E.FULL_WIDTHS + E.RAGGED_WIDTHS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_every_probe_is_its_named_boundary(dtype, cols):
    offs = (0,) if cols in E.FULL_WIDTHS else E.OFFS
    n = 0
    for off in offs:
        for call in E.CALLS:
            for e, k, want, t in _traces(dtype, cols, call, off):
                got = {f: t.get(f) for f in want}
                assert got == want, (e.name, call, k, off, got, want)
                n += 1
    assert n > 50


@pytest.mark.parametrize("cols", E.FULL_WIDTHS)
def test_float_rows_are_on_the_unit_grid(cols):
    """Every float edge row but the six that are meant to leave the value map is modelled exactly."""
    byte = {"sampled_equal", "sampled_subnormal", "sampled_3e38", "pinf_sampled", "ninf_sampled", "nan_last_column"}
    for e in E.edges("f32", cols):
        for largest in (False, True):
            mp, exact, bins, _ = E.first_pass("f32", e.row, largest, True)
            assert (mp, exact) == (("byte", True) if e.name in byte else ("value", True)), e.name
            if mp == "value":
                s = e.row.view(np.float32)[0::4]
                assert s.max() == 256.0 and 0.0 <= s.min() <= 1e-40, e.name


@pytest.mark.parametrize("cols", E.FULL_WIDTHS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_full_rows_reach_every_named_path(dtype, cols):
    seen = {call: set() for call in E.CALLS}
    cnts, totals, stage = set(), set(), set()
    for call in E.CALLS:
        for e, k, t in _all_traces(dtype, cols, call):
            seen[call].add((t["map"], t["finish"]))
            if t["finish"] in ("list", "radix") and "cnt" in t:
                cnts.add(t["cnt"])
            if call != "select":
                seen[call].add(("store", t["store"], t["out"]))
                if t["finish"] == "list":
                    totals.add(t["below"] + t["cnt"])
                if t["staged"]:
                    stage.add(("fast" if t["coll_groups"] == 0 else "collide" if t["fast_groups"] == 0 else "both",
                               t["n_staged"] > E.WAVE, t["kk"] == t["eqn"]))
    assert {1, 63, 64, 65} <= cnts
    mp = "value" if dtype == "f32" else "byte"
    want = {(mp, "list"), (mp, "span0"), (mp, "count8"), (mp, "radix")}
    if dtype == "f32":
        want |= {("byte", "list")}
        assert ("value", "zero-bin") in seen["select"] and ("value", "two-zeros") not in seen["select"]
        assert ("value", "two-zeros") in seen["smallest"] and ("value", "two-zeros") in seen["largest"]
    else:
        want |= {("few", "count8")}
    for call in E.CALLS:
        assert want <= seen[call], (call, want - seen[call])
    for call in ("smallest", "largest"):
        stores = {s for s in seen[call] if s[0] == "store"}
        other = {("store", "regs", "lds"), ("store", "regs", "direct")} if dtype == "i32" else \
            {("store", "all-ties", "lds"), ("store", "all-ties", "direct"), ("store", "reread", "lds"),
             ("store", "reread", "direct")}
        assert stores == {("store", "staged", "direct")} | other, (call, stores)
    assert {E.STAGE_CAP, E.STAGE_CAP + 1} <= totals
    # staged rows: no lane with two keys / lanes with two, more than 64 staged, every tie kept / ties cut
    assert {("fast", True, True), ("fast", True, False)} <= stage
    assert any(s[0] != "fast" and s[2] for s in stage) and any(s[0] != "fast" and not s[2] for s in stage)


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_pick_row_meets_every_lane_boundary(dtype):
    """k = cum lands on a lane's last bin and cum + 1 on the next lane's first: bins 3 | 4, 127 | 128,
    251 | 252 of wave_pick (lane = bin // 4), in both directions and on the ragged float rows."""
    for cols in E.FULL_WIDTHS + (E.RAGGED_WIDTHS if dtype == "f32" else ()):
        pick = [e for e in E.edges(dtype, cols) if e.name == "pick"][0]
        for call in E.CALLS:
            bins = {}
            for k in pick.probes(call):
                bins[k] = E.trace(dtype, pick.row, k, call)["bin"]
            pairs = {(bins[k], bins[k + 1]) for k in bins if k + 1 in bins}
            assert {(3, 4), (127, 128), (251, 252)} <= pairs, (cols, call, sorted(pairs))
            assert {0, 255} <= set(bins.values())


@pytest.mark.parametrize("cols", E.RAGGED_WIDTHS)
def test_ragged_rows_reach_every_named_path(cols):
    for off in E.OFFS:
        form = E.form_of("i32", cols, off, True)
        assert form.load == ("vec" if off == 0 and cols % 4 == 0 else "scalar")
        for call in E.CALLS:
            seen = {(t.get("width"), t["finish"]) for _, _, t in _all_traces("i32", cols, call, off)}
            assert {w for w, _ in seen} == set(E.INT_WIDTHS)
            assert {f for _, f in seen} >= {"one-pass", "digits"}
            seen = {(t["map"], t["finish"]) for _, _, t in _all_traces("f32", cols, call, off)}
            assert seen >= {("range-value", "digits"), ("range-value", "interval-one"), ("range-int", "digits")}
            if call != "select":
                outs = {t["out"] for _, _, t in _all_traces("f32", cols, call, off)}
                assert outs == {"lds", "direct"}
    # a valid key equal to the padding, asked for at k = cols
    wide = [e for e in E.edges("i32", cols) if e.name == "width32"][0]
    assert (wide.row == 0x7FFFFFFF).sum() == 3 and (wide.row == 0x80000000).sum() == 3
    assert cols in wide.probes("smallest") and cols in wide.probes("largest")
    nan = [e for e in E.edges("f32", cols) if e.name == "nan"][0]
    assert cols in nan.probes("select") and E.order_key("f32", nan.row).max() == 0xFFFFFFFF
    assert {0x7FC00001, 0xFFC00000, 0xFF800001} <= set(nan.row.tolist())


def test_probe_counts_stay_small():
    """Every row of a case meets every rank of it: the calls of the GPU file."""
    total = 0
    for dtype in E.DTYPES:
        for cols in E.FULL_WIDTHS + E.RAGGED_WIDTHS:
            _, ranks = E.edge_case(dtype, cols)
            total += sum(len(v) for v in ranks.values()) * (1 if cols in E.FULL_WIDTHS else 2)
    assert total < 9000, total
