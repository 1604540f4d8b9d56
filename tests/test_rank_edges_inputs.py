"""CPU: every input of tests/rank_edges.py has the structure it claims, from numpy
and the published formulas alone (kth_window_z, kth_dist_sample_size,
kth_sample_chunk; host arithmetic in libkth.so, no GPU):

* every plateau margin holds: the window's sample rank lies at least
  MARGIN_SIGMAS sample sigmas inside the run it is meant to fall on;
* every planted band margin holds: at least BAND_MARGIN sample ranks;
* every probed rank is the boundary it is named for, for the exact window an honest
  sample gives (plateaus) or the planted window (bands).

test_gpu_rank_edges.py runs the same inputs through the library.
"""
import numpy as np
import pytest

import rank_edges as re_

PLATEAUS = [(name, re_.N_SMALL) for name in re_.I32_CASES + re_.F32_CASES] + [(name, re_.N_MID) for name in re_.I32_CASES]


def test_formulas_match_the_host_restatement():
    """window_ranks and the sampler layout here against tests/dist_cpu_backend.py's restatement."""
    import dist_cpu_backend as cb
    for n in (re_.N_SMALL, re_.N_MID):
        s = re_.sample_size(n)
        assert s == 64 * (s // 64) and s == min(1 << 20, n // 64) // 64 * 64
        for k in (1, 2, 4000, n // 100, n // 2, n - n // 100, n - 4000, n):
            assert re_.window_ranks(n, k, s) == cb.window_ranks(n, k, s), (n, k)
        assert np.array_equal(re_.sample_indices(n), cb.sample_indices(n, s))


@pytest.mark.parametrize("name,n", PLATEAUS)
def test_plateau_structure_and_margins(name, n):
    c = re_.plateau_case(name, n)
    ref = c.ref
    assert ref.n == n and c.probes
    # the runs are tie groups of exactly the stated ranks, every other key is distinct
    for key, first, last in c.groups:
        assert ref.counts(key, key)[:2] == (first - 1, last - first + 1), (name, hex(key))
    others = ref.sorted[~np.isin(ref.sorted, np.array([g[0] for g in c.groups], dtype=np.uint32))]
    assert np.all(others[1:] > others[:-1])
    assert ref.n - others.size == c.total
    # the keys lie in random positions: the run is spread over the whole array
    at = np.flatnonzero(ref.key == np.uint32(c.groups[0][0]))
    assert at[0] < n // 8 and at[-1] > n - n // 8 or at.size < 64
    if name in re_.NOT_BY_MARGIN:
        # 40000 keys between the runs: the window cannot straddle them with the margin
        s = re_.sample_size(n)
        k = c.groups[1][1]
        r_lo, r_hi = re_.window_ranks(n, k, s)
        assert r_hi - r_lo - 40000 * s / n < 2 * re_.MARGIN_SIGMAS * re_.sigma(n, k, s)
        assert 40000 > re_.FIN_LDS_KEYS
        return
    for p, which, g in c.margins:
        assert c.margin_sigmas(p, which, g) >= re_.MARGIN_SIGMAS, (name, p, which, g, c.margin_sigmas(p, which, g))
    # with the exact window of the honest sample, every probe is the boundary it is named for
    for p in c.probes:
        lo, hi = ref.exact_window(p.k)
        assert p.reached(ref, lo, hi), (name, p, hex(lo), hex(hi), ref.branch(p.k, lo, hi))


def test_every_branch_is_probed_at_both_ends():
    """Over the int32 plateau cases: first and last rank of lo, cand and hi, and the
    lo == hi, hi == lo + 1 and W == 0 shapes."""
    seen, shapes = set(), set()
    for name in re_.I32_CASES:
        for p in re_.plateau_case(name).probes:
            seen.add((p.branch, "first" if p.pos == "only" else p.pos))
            seen.add((p.branch, "last" if p.pos == "only" else p.pos))
            shapes.add(p.shape)
    # an honest window's upper rank lies z sigmas above k's, so it never ends ON the last
    # rank of the run it fell in: the last rank of hi is the planted inputs' alone
    assert {(b, e) for b in ("lo", "cand", "hi") for e in ("first", "last")} - seen == {("hi", "last")}
    assert {"lo==hi", "hi==lo+1", "W==0"} <= shapes
    c = re_.planted_case("wide")
    for k, _ in c.bounds:
        br, at, size = c.ref.branch(k, c.lo_key, c.hi_key)
        seen.update({(br, "first")} if at == 1 else set(), {(br, "last")} if at == size else set())
    assert {(b, e) for b in ("lo", "cand", "hi") for e in ("first", "last")} <= seen


def test_float_cases_hold_the_special_words():
    f = re_.f32t
    for name, words in (("f32_zero_mid", [f.NEG0]), ("f32_zero_adjacent", [f.NEG0, f.POS0]),
                        ("f32_subnormal_mid", [1]), ("f32_subnormal_adjacent", [1, 2]),
                        ("f32_inf_nan", [f.PINF, *f.NAN_BITS.tolist()]), ("f32_nan_top", f.NAN_BITS.tolist())):
        w = re_.plateau_case(name).ref.words
        for x in words:
            assert np.count_nonzero(w == np.uint32(x)) > 1000, (name, hex(x))


@pytest.mark.parametrize("variant", list(re_.PlantedCase.VARIANTS))
def test_planted_bands(variant):
    c = re_.planted_case(variant)
    n, s, ref = c.n, c.s, c.ref
    # the sample the library reads, sorted: filler, A, B, filler, at the stated sample ranks
    srt = ref.sample_sorted()
    assert np.all(srt[c.a_first - 1:c.split] == np.uint32(c.lo_key))
    assert np.all(srt[c.split:c.b_last] == np.uint32(c.hi_key))
    assert srt[c.a_first - 2] < c.lo_key and srt[c.b_last] > c.hi_key
    # band margins, for every k of the stated interval (the window ranks are monotone in k)
    for k in (c.k_lo, c.k_hi, *c.ks()):
        assert c.k_lo <= k <= c.k_hi
        r_lo, r_hi = re_.window_ranks(n, k, s)
        assert c.a_first + re_.BAND_MARGIN <= r_lo <= c.split - re_.BAND_MARGIN, (variant, k, r_lo)
        hi_first = c.split + 1 if c.B != c.A else c.a_first
        assert hi_first + re_.BAND_MARGIN <= r_hi <= c.b_last - re_.BAND_MARGIN, (variant, k, r_hi)
        assert ref.exact_window(k) == (c.lo_key, c.hi_key)
        # the bands outweigh the early window's slack: a default ctx publishes the same window
        assert ref.early_window(k) == (c.lo_key, c.hi_key) == ref.early_window(k, abs_div=0)
    # exact counts, and the eight boundaries are the boundaries
    assert ref.counts(c.lo_key, c.hi_key) == (c.L, c.E1, c.M, c.E2 if c.B != c.A else c.E1)
    want = ["miss_below", "lo", "lo", "cand", "cand", "hi", "hi", "miss_above"]
    if c.M == 0:
        want[3:5] = ["hi", "lo"] if c.E2 else ["miss_above", "lo"]
    if c.E2 == 0:
        want[5:7] = ["miss_above", "lo"]
    for (k, what), br in zip(c.bounds, want):
        got = ref.branch(k, c.lo_key, c.hi_key)
        assert got[0] == br, (variant, what, k, got)
        assert c.expect(k) == (4 if br.startswith("miss") else 3, br)
    L, E1, M, E2 = c.L, c.E1, c.M, c.E2
    assert ref.branch(L, c.lo_key, c.hi_key)[:2] == ("miss_below", 1)
    assert ref.branch(L + E1 + M + E2 + 1, c.lo_key, c.hi_key)[:2] == ("miss_above", 1)
    assert ref.branch(L + 1, c.lo_key, c.hi_key) == ("lo", 1, E1) and ref.branch(L + E1, c.lo_key, c.hi_key) == ("lo", E1, E1)
    if M:
        assert ref.branch(L + E1 + 1, c.lo_key, c.hi_key) == ("cand", 1, M)
        assert ref.branch(L + E1 + M, c.lo_key, c.hi_key) == ("cand", M, M)
    if E2:
        assert ref.branch(L + E1 + M + 1, c.lo_key, c.hi_key) == ("hi", 1, E2)
        assert ref.branch(L + E1 + M + E2, c.lo_key, c.hi_key) == ("hi", E2, E2)
    if variant == "plus2":
        assert c.hi_key == c.lo_key + 2 and M > re_.FIN_LDS_KEYS and np.all(ref.sorted[L + E1:L + E1 + M] == c.lo_key + 1)


def test_staircase():
    vals = re_.staircase_values()
    key = re_.i32_key(vals).astype(np.int64)
    assert vals[0] == -(1 << 31) and vals[-1] == (1 << 31) - 1 and 120 <= vals.size <= 130
    for b in range(32):  # both sides of every power of two, either sign
        for v in (-(1 << b) - 1, -(1 << b), (1 << b) - 1, 1 << b):
            assert np.clip(v, -(1 << 31), (1 << 31) - 1) in vals
    # every adjacent pair {x - 1, x} around a power of two differs in the order key's bit b
    # and in nothing above it or in everything above it: a bin boundary of every digit split
    # whose low edge is at or below bit b
    for b in range(31):
        for x in ((1 << b), -(1 << b)):
            k0, k1 = int(re_.i32_key([x - 1])[0]), int(re_.i32_key([x])[0])
            assert k1 == k0 + 1 and k1 % (1 << b) == 0
    assert np.all(key[1:] > key[:-1])
    for n in (1, 2, 63, 64, 65, 2049, 16385, 100003, 1 << 22):
        ref, first, last = re_.staircase(n)
        G = min(n, vals.size)
        assert ref.n == n and first.size == G and first[0] == 1 and last[-1] == n
        assert np.all(first[1:] == last[:-1] + 1)
        mult = last - first + 1
        assert mult.min() >= 1 and (n < vals.size or mult.max() <= 2 * n // vals.size)
        # first[i] / last[i] are the first and last rank of a tie group
        assert np.all(ref.sorted[first - 1] == ref.sorted[last - 1])
        assert np.all(ref.sorted[last[:-1] - 1] < ref.sorted[last[:-1]])


@pytest.mark.parametrize("kind", re_.k16t.KINDS)
def test_k16_edges(kind):
    for n in re_.K16_SIZES:
        d = re_.k16_input(kind, n)
        ks = d.edge_ranks()
        assert ks and ks[0] == 1 and ks[-1] == n
        for k in ks:  # every probed rank is the first or the last of its tie group
            assert k == 1 or k == n or d.sorted[k - 2] != d.sorted[k - 1] or d.sorted[k] != d.sorted[k - 1], (kind, n, k)
        if kind in re_.k16t.INF:
            groups = d.probed_groups()
            for key in (0x7FFF, 0x8000, 0x8000 | re_.k16t.INF[kind], 0xFFFF):
                assert key in groups, (kind, n, hex(key))


def test_topk_reference_is_the_stable_argsort():
    """The O(n) top-k reference against sort(argsort(key, stable)[:k]) on a small input with ties."""
    rng = np.random.default_rng(5)
    key = rng.integers(0, 50, 3000).astype(np.uint32)
    skey = np.sort(key)
    for k in (1, 2, 59, 60, 61, 1500, 2999, 3000):
        assert np.array_equal(re_.topk_ref(key, skey, k, False), np.sort(np.argsort(key, kind="stable")[:k]))
        assert np.array_equal(re_.topk_ref(key, skey, k, True), np.sort(np.argsort(~key, kind="stable")[:k]))


def test_topk_variants_named_by_the_cases():
    """The k of each top-k test selects the variant the test names (thresholds of include/kth.h)."""
    n = re_.N_SMALL
    floor, low, mid = (re_.plateau_case(x) for x in ("floor", "low", "mid"))
    assert floor.total <= n // 1024
    for k in (floor.total, floor.total + 1):
        assert re_.topk_variant(n, k, aligned=False, f32=False) == "tile-flag"
        assert re_.topk_variant(n, k, aligned=True, f32=False) == "staged"
    assert {re_.topk_variant(n, k, True, False) for k in low.ks()} == {"staged"}
    assert {re_.topk_variant(n, k, True, False) for k in mid.ks()} == {"row-word"}
    assert {re_.topk_variant(n, k, True, True) for k in low.ks()} == {"row-word"}
    assert re_.topk_variant(100003, 50, True, False) == "tile-flag" and re_.topk_variant(100003, 5000, True, False) == "plain"
