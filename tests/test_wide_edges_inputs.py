"""CPU: the inputs of tests/wide_edges.py have the structure they claim, proved on the
references alone (V.expect_select / V.expect_topk, test_gpu_topp.RowRef), so that the
exact comparisons of tests/test_gpu_wide_edges.py mean what they are named for.
No device work; the only library call is the plan's host arithmetic (slice sizes).
"""
import numpy as np
import pytest

import test_gpu_rows_var as V
import test_gpu_sample as S
import wide_edges as E


def _sorted_keys(keys, largest):
    k = np.sort(np.asarray(keys, dtype=np.uint64))
    return k[::-1] if largest else k


@pytest.mark.parametrize("name", E.FLAVORS)
def test_shape_is_derived_from_the_constants(name):
    fl = V.Flavor(name)
    cols, tile = E.cols_of(fl), E.tile_of(fl)
    assert E.fused_block() == 512 and tile == (4096 if fl.w16 else 2048)
    assert cols == (8195 if fl.w16 else 4099)
    assert 2 * tile < cols < 3 * tile and cols % fl.align == 3  # two whole tiles, a 3-key tail
    for slices in (3, 7):
        units = E.units_of(fl, cols, slices)
        sk = fl.slice_keys(cols, slices)
        assert len(units) == slices and 0 < units[-1][1] - units[-1][0] < sk and sk % fl.align == 0
    # no smaller length does
    for c in range(2 * tile + 1, cols):
        assert not (c % fl.align == 3 and E.short_last(fl, c, 3) and E.short_last(fl, c, 7))


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", E.FLAVORS)
def test_staircase_probes_are_the_named_boundaries(name):
    st = E.staircase(name)
    fl, digs = st.fl, E.digits_of(st.fl)
    assert E.populated(fl, st.values).all()
    # the bins asked for, and what stands in where a side cannot be populated
    if name in ("f32", "f16", "bf16"):
        ninf, pinf = E.value_key(fl, -np.inf), E.value_key(fl, np.inf)
        s0 = digs[0][0]
        assert st.subs == [(0, 0, 1, (ninf >> s0) + 1), (0, 0, digs[0][1] - 1, pinf >> s0),
                           (1, "first", 0, (ninf >> s0) + 1), (1, "last", digs[0][1] - 1, (pinf >> s0) - 1)]
        assert st.ends == (ninf, (1 << E.nbits(fl)) - 1)
    else:
        assert st.subs == [] and st.ends == (0, (1 << E.nbits(fl)) - 1)
    for p in st.pairs:
        shift, bins = digs[p.digit]
        assert p.b == p.a + 1 and (p.a >> shift) % bins == p.bin - 1 and (p.b >> shift) % bins == p.bin
        assert p.digit == 0 or (p.a >> digs[p.digit - 1][0]) == (p.b >> digs[p.digit - 1][0]) == p.prefix
    assert {(p.digit, p.want_b) for p in st.pairs} == {(d, b) for d, (_, n) in enumerate(digs) for b in (1, n // 2, n - 1)}
    half = 1 << (E.nbits(fl) - 1)
    assert {half - 1, half}.issubset(st.values)  # (for the float kinds: -0.0 beside +0.0)
    for largest in (False, True):
        order = _sorted_keys(st.keys, largest)
        probes = st.probes(largest)
        ranks = {k for k, _, _ in probes}
        assert len(probes) == 2 * len(st.values)
        for k, key, edge in probes:
            assert order[k - 1] == key
            if edge == "last":
                assert k == st.cols or order[k] != key
            else:
                assert k == 1 or order[k - 2] != key
        # every pair: the last rank of one side is followed by the first rank of the other
        for p in st.pairs:
            first, second = (p.b, p.a) if largest else (p.a, p.b)
            k = int(np.nonzero(order == first)[0][-1]) + 1
            assert order[k] == second and k in ranks and k + 1 in ranks, (p, largest)
        # the selects' reference answers at the probes are those keys
        if not largest:
            words, ks = st.case(False)
            got = V.expect_select(fl, words, None, ks, max(ks))
            assert np.array_equal(fl.keys(got[:-1]).astype(np.uint64), [key for _, key, _ in probes])
            assert got[-1] == fl.canon(st.equal[:1])[0]


@pytest.mark.parametrize("name", E.FLAVORS)
def test_staircase_reaches_every_early_end(name):
    """The distinct values among the keys that share the answer's picked digits: every end of the
    descent occurs (16-bit: a one-valued row, or both digits)."""
    st = E.staircase(name)
    seen = {E.digits_picked(st.fl, st.keys, key) for _, key, _ in st.probes(False)}
    seen.add(E.digits_picked(st.fl, st.fl.keys(st.equal), int(st.fl.keys(st.equal)[0])))
    assert seen == ({0, 2} if st.fl.w16 else {0, 1, 2, 3}), seen
    counts = np.unique(st.keys, return_counts=True)[1]
    assert counts.min() >= 2 and len(set(counts.tolist())) >= 3  # groups of several sizes: first != last rank


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("slices", (1, 3, 7))
@pytest.mark.parametrize("name", E.FLAVORS)
def test_fence_probes_end_on_the_named_columns(name, slices):
    f = E.fence(name, slices)
    fl = f.fl
    t_cols = np.array(f.t_cols)
    last = f.units[-1]
    assert f.keys[last[0]] == f.t and f.keys[last[1] - 1] == f.t and last[1] - last[0] < f.units[0][1] - f.units[0][0]
    only = [u for u, (b, e) in enumerate(f.units) if (f.keys[b:e] >= f.t).all() and (f.keys[b:e] == f.t).any()]
    none = [u for u, (b, e) in enumerate(f.units) if not (f.keys[b:e] == f.t).any()]
    assert only == [1] and (none == [3] if len(f.units) == 7 else none == [])
    both = [u for u in range(len(f.units) - 1) if f.keys[f.units[u][1] - 1] == f.t]  # T on a unit's last column
    assert both and all(f.e[u] < len(t_cols) for u in both)
    for largest in (False, True):
        words, ks = f.case(largest)
        _, idx, cnt = V.expect_topk(fl, words, None, ks, max(ks), largest)
        assert cnt.tolist() == ks
        kept_last = {}  # j -> the column of the last tie kept
        for r, j in enumerate(f.js):
            kept = idx[r, :ks[r]]
            ties = np.intersect1d(kept, t_cols)
            assert ties.size == j and kept.size - j == f.below and np.array_equal(ties, t_cols[:j])
            kept_last[j] = int(ties[-1])
        for u in both:  # the quota ends on the unit's last column, and on the next T's first column
            nxt = min(v for v in range(u + 1, len(f.units)) if f.e[v] > f.e[u])
            assert kept_last[f.e[u]] == f.units[u][1] - 1
            assert kept_last[f.e[u] + 1] == f.units[nxt][0] and nxt == u + 1
        # the T-only unit is reached with quota 0: every tie kept lies before it
        assert any(kept_last[j] < f.units[1][0] for j in f.js)
        # a quota that ends strictly inside a unit
        inside = [j for j in f.js if any(b < kept_last[j] < e - 1 for b, e in f.units)]
        assert inside, f.js


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("temp", (1.0, 0.5))
@pytest.mark.parametrize("name", E.FLOATS)
def test_mass_probes_admit_one_answer(name, temp):
    m = E.mass(name, temp)
    assert m.weighted >= 40 and len(m.edges) >= 30 and E.REACH <= 4.0
    x = E.T.values(m.fl, m.row)
    top = x.max()
    assert top == E.M_TOP and (x[m.ref.order[:m.weighted]] >= top - E.REACH * temp).all()
    rest = x[m.ref.order[m.weighted:]]
    assert ((rest == -np.inf) | ((rest <= top - 40 * temp) & (rest >= top - 100 * temp))).all()
    assert (rest == -np.inf).sum() > 100 and (rest != -np.inf).sum() > 100
    # the tie group lies across the boundaries it names
    tie = m.row[m.tie_cols[0]]
    assert (m.row[m.tie_cols] == tie).all() and (m.row == tie).sum() == E.TIES
    for slices in (7, 3, 1):
        units = E.units_of(m.fl, m.cols, slices)
        assert units[0][1] - 1 in m.tie_cols and units[1][0] in m.tie_cols
    assert m.cols - 1 in m.tie_cols and E.units_of(m.fl, m.cols, 7)[6][0] in m.tie_cols
    tie_ranks = [j for j in range(1, m.weighted + 1) if m.ref.bits[j - 1] == m.fl.canon(np.array([tie]))[0]]
    assert tie_ranks[0] in m.edges and tie_ranks[-1] in m.edges and len(tie_ranks) == E.TIES
    margins = []
    for j, p in m.nuc:
        ref = m.ref_at(p)
        assert ref.band() == [j], (j, p, ref.band())
        margins.append(E.nucleus_margin(ref, p))
    for j, p, cap in m.capped:
        assert m.ref_at(p).band() == [j] and cap in (j - 1, j, j + 1)
    refs = {}
    for p, cap, n in m.configs:
        refs[p] = ref = m.ref_at(p)
        assert ref.band() == [n], (p, ref.band(), n)
        cnt = min(n, cap) if cap > 0 else n
        assert S.cnt_ok(ref, cnt, cap) and not S.cnt_ok(ref, cnt - 1, cap) and not S.cnt_ok(ref, cnt + 1, cap)
        if p < 1.0:
            margins.append(E.nucleus_margin(ref, p))
    assert {cap - n for p, cap, n in m.configs if cap > 0 and p < 1.0} == {-1, 0, 1}
    for p, cap, cnt, j, u in m.draws:
        assert S.j_band(refs[p], cnt, u) == [j], (p, cap, cnt, j, u, S.j_band(refs[p], cnt, u))
        margins.append(E.draw_margin(refs[p], cnt, u))
    assert min(margins) >= 4.0, min(margins)
    for p, cap, n in m.configs:  # every configuration draws its first and its last kept key
        cnt = min(n, cap) if cap > 0 else n
        js = [d[3] for d in m.draws if d[:3] == (p, cap, cnt)]
        assert js[0] == 1 and js[-1] == min(cnt, m.weighted)
