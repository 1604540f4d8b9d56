"""GPU: every one-array select at the ranks where its case split changes.

The window path's decide() (csrc/kth_kernels.hip), the per-digit bin pick of the
radix and LDS paths, the 16-bit select, the multi-rank select, both top-ks and the
sharded protocol, each probed on the FIRST and the LAST rank of a branch.  Inputs,
the reference (one np.sort per input) and the branch arithmetic are in
tests/rank_edges.py; tests/test_rank_edges_inputs.py proves on the CPU that every
input has the structure it claims.

A failing id names the input and the ctx; the assert message names the probe (the
branch and the boundary rank) and the window, counts and finish form the library
reported.  What each case reaches is tabulated in DESIGN.md "Rank edges".

For every window-path probe:
  * the answer is the reference's, bit for bit, and stats()["error"] == 0;
  * cnt_lt, cnt_eq_lo, candidates and cnt_eq_hi equal numpy's counts over the host
    array for the reported lo_key / hi_key;
  * the branch and the position in it are read off those numpy counts (never off the
    answer) and must be the ones the probe is named for, with the finish form that
    belongs to it: KTH_FINISH_COUNTS where no level runs (lo, hi, W == 0).

Ctxs: "default" (the shared fixture), "slack0" (created under KTH_HEAD_SLACK=0: the
exact window, no early window), "slices" (KTH_HOOK_FINISH_SLICES), "perlevel"
(created under KTH_COOP=0; its sample phase has no early window either).  Every
named probe is asserted reached on slack0 and perlevel; on default and slices too,
except NEEDS_SLACK0 below.
"""
import numpy as np
import pytest

import rank_edges as re_

pytestmark = pytest.mark.gpu

N_SMALL, N_MID = re_.N_SMALL, re_.N_MID
# Probes a default ctx does not reach: the plain select's early window takes a first-level
# bin of up to s / 1024 sample keys whatever it holds (kth_api.hip head_abs_div), so at
# k = n (k = 1) its lo (hi) is the bin's edge, not the run's key, and the probe lands
# among the candidates.  Reached on the KTH_HEAD_SLACK=0 and per-level ctxs.
NEEDS_SLACK0 = {("ceiling", N_SMALL, "k=n"), ("floor", N_MID, "k=1")}


# ------------------------------------------------------------------------ ctxs
@pytest.fixture(scope="module")
def ctxs(gpu):
    import kselect
    made = {"default": gpu}

    def get(name):
        if name not in made:
            env = {"slack0": ("KTH_HEAD_SLACK", "0"), "perlevel": ("KTH_COOP", "0")}.get(name)
            with pytest.MonkeyPatch.context() as mp:
                if env:
                    mp.setenv(*env)
                made[name] = kselect.Selector(0)
            if name == "slices":
                made[name].test_hook(kselect.KTH_HOOK_FINISH_SLICES, 1)
            assert made[name].coop() == (name != "perlevel")
        return made[name]

    yield get
    for name, sel in made.items():
        if name != "default":
            sel.close()


def _fresh(name="default"):
    import kselect
    with pytest.MonkeyPatch.context() as mp:
        if name == "perlevel":
            mp.setenv("KTH_COOP", "0")
        sel = kselect.Selector(0)
    if name == "slices":
        sel.test_hook(kselect.KTH_HOOK_FINISH_SLICES, 1)
    return sel


_DEV = {}


def _dev(ref, off=0):
    """The input on the device, `off` words past a 16-byte boundary (one upload per input and offset)."""
    import torch
    if (id(ref), off) not in _DEV:
        if len(_DEV) >= 6:
            _DEV.clear()
        host = ref.host()
        base = torch.zeros(ref.n + 4, dtype=torch.float32 if ref.f32 else torch.int32, device="cuda")
        d = base[off:off + ref.n]
        d.copy_(torch.from_numpy(host))
        assert d.data_ptr() % 16 == 4 * off
        _DEV[(id(ref), off)] = (ref, d)
    return _DEV[(id(ref), off)][1]


def _bits(x):
    return int(np.asarray(x).reshape(1).view(np.uint32)[0])


def _counts_match(ref, st):
    """The reported counts against numpy's for the reported window; returns (lo, hi)."""
    lo, hi = st["lo_key"], st["hi_key"]
    got = (st["cnt_lt"], st["cnt_eq_lo"], st["candidates"], st["cnt_eq_hi"])
    assert got == ref.counts(lo, hi), (hex(lo), hex(hi), got, ref.counts(lo, hi), st)
    return lo, hi


def _must_reach(case, ctx, p):
    if case.name in re_.NOT_BY_MARGIN:
        return p.reached(case.ref, *case.ref.exact_window(p.k)) and ctx in ("slack0", "perlevel")
    return ctx in ("slack0", "perlevel") or (case.name, case.n, p.name) not in NEEDS_SLACK0


def _check_probe(case, ctx, p, got_bits, st, form):
    """One window-path probe: exact, no error, counts re-derived, the named boundary, the finish form."""
    import kselect
    ref, tag = case.ref, (case.name, case.n, ctx, p)
    assert got_bits == ref.want(p.k) and st["error"] == 0, (tag, hex(got_bits), hex(ref.want(p.k)), st)
    assert st["path"] == 3 and st["k"] == p.k and st["n"] == ref.n, (tag, st)
    lo, hi = _counts_match(ref, st)
    br = ref.branch(p.k, lo, hi)
    reached = p.reached(ref, lo, hi)
    if _must_reach(case, ctx, p):
        assert reached, (tag, "landed on", br, hex(lo), hex(hi), st)
    if form is None:
        return reached
    if ctx == "perlevel":
        assert form == kselect.KTH_FINISH_NONE, (tag, form)
    elif br[0] in ("lo", "hi") or hi - lo == 2:  # no level runs
        assert form == kselect.KTH_FINISH_COUNTS, (tag, br, form, st)
    else:
        assert form in (kselect.KTH_FINISH_SLICES, kselect.KTH_FINISH_GROUPED, kselect.KTH_FINISH_LEVELS), (tag, form)
        assert ctx != "slices" or form != kselect.KTH_FINISH_GROUPED, (tag, form)
    return reached


PLATEAU_RUNS = ([(name, N_SMALL, ctx) for name in re_.I32_CASES + re_.F32_CASES for ctx in ("default", "slack0", "slices")]
                + [(name, N_SMALL, "perlevel") for name in re_.PER_LEVEL_CASES]
                + [(name, N_MID, ctx) for name in re_.I32_CASES for ctx in ("default", "slack0")])


# ------------------------------------------------ 1. window path, honest sample
@pytest.mark.parametrize("name,n,ctx", PLATEAU_RUNS)
def test_plateau_select(ctxs, name, n, ctx):
    """The single select at every probe of a plateau case."""
    case, sel = re_.plateau_case(name, n), ctxs(ctx)
    d = _dev(case.ref)
    for p in case.probes:
        got = _bits(sel.select(d, p.k, f32=case.ref.f32))
        _check_probe(case, ctx, p, got, sel.stats(), sel.finish_form())


@pytest.mark.parametrize("name", re_.I32_CASES + re_.F32_CASES)
@pytest.mark.parametrize("ctx", ["default", "slack0", "slices"])
def test_plateau_multi(ctxs, name, ctx):
    """All probes of a case in ONE select_multi call (one streaming pass, a window per
    rank): bit-identical to the single select, and every rank's own counts and boundary."""
    case, sel = re_.plateau_case(name), ctxs(ctx)
    ref, ks = case.ref, case.ks()
    assert len(ks) <= 8
    d = _dev(ref)
    single = [_bits(sel.select(d, k, f32=ref.f32)) for k in ks]
    got = sel.select_multi(d, ks, f32=ref.f32)
    stats = [sel.multi_stats(i) for i in range(len(ks))]
    assert [_bits(x) for x in got] == single == ref.wants(ks), (name, ctx, ks)
    for p, g, st in zip(case.probes, got, stats):
        _check_probe(case, ctx, p, _bits(g), st, None)


# --------------------------------------------------------------------- top-k
def _check_topk(sel, ref, d, k, largest, tag, path=None):
    import torch
    vals = torch.full((k,), -7, dtype=d.dtype, device="cuda")
    idx = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    sel.topk(d, ref.n, k, vals, idx, largest=largest, f32=ref.f32)
    sel.sync()
    st = sel.stats()
    assert st["error"] == 0 and (path is None or st["path"] == path), (tag, k, largest, st)
    want = ref.topk(k, largest)
    assert want.size == k
    np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"{tag} k={k} largest={largest} idx {st}")
    np.testing.assert_array_equal(vals.cpu().numpy().view(np.uint32), ref.out_bits(ref.words[want]),
                                  err_msg=f"{tag} k={k} largest={largest} vals {st}")
    return st


def _topk_k(ref, rank, largest):
    """The top-k size whose embedded select is rank `rank`: the plateau mirrored for largest."""
    return ref.n - rank + 1 if largest else rank


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("name", re_.I32_CASES + re_.F32_CASES)
def test_plateau_topk(gpu, name, largest):
    """topk with the k-th key on every probe (largest: the mirrored k, so the embedded select
    takes the same rank), values and indices against the O(n) reference.  The variant
    each k selects (rank_edges.topk_variant, thresholds of include/kth.h), smallest:
      floor    k = c, c + 1 with c <= n / 1024: tile-flag on keys one word off 16 bytes,
               staged on aligned keys (both are run)
      low      n / 65536 < k <= n / 16, aligned int32: staged
      mid, adjacent, between_*, high: k > n / 16, aligned: row-word
      float32 cases: never staged: row-word
    largest mirrors them: ceiling takes tile-flag / staged, high staged, floor and low row-word."""
    case = re_.plateau_case(name)
    ref, n = case.ref, case.n
    want_variant = {("floor", False): "staged", ("low", False): "staged", ("ceiling", True): "staged",
                    ("high", True): "staged"}.get((name, largest), "row-word")
    inner = [p for p in case.probes if p.k not in (1, n)]
    for p in case.probes:
        k = _topk_k(ref, p.k, largest)
        if p in inner:
            assert re_.topk_variant(n, k, True, ref.f32) == want_variant, (name, p, k)
        _check_topk(gpu, ref, _dev(ref), k, largest, (name, p), path=3)
        if (name, largest) in (("floor", False), ("ceiling", True)) and p in inner:
            assert re_.topk_variant(n, k, False, False) == "tile-flag"
            _check_topk(gpu, ref, _dev(ref, off=1), k, largest, (name, p, "unaligned"), path=3)


# ----------------------------------------------- 2. window path, planted sample
@pytest.mark.parametrize("ctx", ["default", "slices", "perlevel"])
@pytest.mark.parametrize("variant", list(re_.PlantedCase.VARIANTS))
def test_planted_select(variant, ctx):
    """The eight boundaries of a planted window: L (miss below by one), L+1, L+E1, L+E1+1,
    L+E1+M, L+E1+M+1, L+E1+M+E2, L+E1+M+E2+1 (miss above by one).  Path 4 for the two
    misses, 3 for the rest; lo_key / hi_key are the keys of A and B; the counts are the
    planted ones.  A fresh ctx: the shared one's candidate capacity may have grown."""
    import kselect
    c = re_.planted_case(variant)
    ref = c.ref
    d = _dev(ref)
    sel = _fresh(ctx)
    try:
        for k, what in c.bounds:
            tag = (variant, ctx, what, k)
            got = _bits(sel.select(d, k))
            st, form = sel.stats(), sel.finish_form()
            assert got == ref.want(k) and st["error"] == 0, (tag, hex(got), hex(ref.want(k)), st)
            assert (st["lo_key"], st["hi_key"]) == (c.lo_key, c.hi_key), (tag, st)
            assert _counts_match(ref, st) == (c.lo_key, c.hi_key)
            assert (st["cnt_lt"], st["cnt_eq_lo"], st["candidates"]) == (c.L, c.E1, c.M), (tag, st)
            path, br = c.expect(k)
            assert st["path"] == path, (tag, br, st)
            if ctx == "perlevel":
                assert form == kselect.KTH_FINISH_NONE, (tag, form)
            elif br in ("lo", "hi") or (br == "cand" and variant == "plus2"):
                assert form == kselect.KTH_FINISH_COUNTS, (tag, br, form)
            else:
                assert form != kselect.KTH_FINISH_COUNTS, (tag, br, form)
    finally:
        sel.close()


@pytest.mark.parametrize("variant", list(re_.PlantedCase.VARIANTS))
def test_planted_multi(variant):
    """The eight boundaries in one select_multi call: the two misses fall back, the six
    others are not disturbed; every rank's stats carry the planted window and counts."""
    c = re_.planted_case(variant)
    ref, ks = c.ref, [k for k, _ in c.bounds]
    d = _dev(ref)
    sel = _fresh()
    try:
        single = [_bits(sel.select(d, k)) for k in ks]
        got = [_bits(x) for x in sel.select_multi(d, ks)]
        stats = [sel.multi_stats(i) for i in range(len(ks))]
        assert got == single == ref.wants(ks), (variant, ks)
        for (k, what), st in zip(c.bounds, stats):
            assert st["error"] == 0 and st["k"] == k and st["path"] == c.expect(k)[0], (variant, what, st)
            assert _counts_match(ref, st) == (c.lo_key, c.hi_key), (variant, what, st)
    finally:
        sel.close()


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("variant", list(re_.PlantedCase.VARIANTS))
def test_planted_topk(variant, largest):
    """topk whose embedded select misses the window by one rank, on either side (path 4:
    a window that missed on the far side turns the count pass's skipping off), and at the
    first rank of lo and the last of hi (path 3).  k is near n / 2 on aligned keys: the
    row-word variant."""
    c = re_.planted_case(variant)
    ref = c.ref
    d = _dev(ref)
    sel = _fresh()
    try:
        for at in (0, 1, 6, 7):
            rank, what = c.bounds[at]
            k = _topk_k(ref, rank, largest)
            assert re_.topk_variant(ref.n, k, True, False) == "row-word"
            _check_topk(sel, ref, d, k, largest, (variant, what), path=c.expect(rank)[0])
    finally:
        sel.close()


# --------------------------------------------------- sharded, local transport
def _one_shard_layout(case):
    """The input reordered so that every key of the runs lies in the middle shard:
    (words, sizes).  The same multiset, so the same reference."""
    ref = case.ref
    run = np.isin(ref.key, np.array([g[0] for g in case.groups], dtype=np.uint32))
    others, runs = ref.words[~run], ref.words[run]
    h = others.size // 3
    words = np.concatenate([others[:h], runs, others[h:h + 1000], others[h + 1000:]])
    return words, [h, runs.size + 1000, ref.n - h - runs.size - 1000]


@pytest.mark.parametrize("layout", ["unequal", "one_shard"])
@pytest.mark.parametrize("name", re_.SHARDED_CASES)
def test_plateau_sharded(name, layout):
    """ShardedSelector([0, 0, 0]) on three contiguous shards: unequal ones of the input
    as it is, then with the whole plateau in one shard (that shard's sample is nearly
    all one key).  Exactness at every probe (the sharded call reports no window)."""
    import kselect
    import torch
    case = re_.plateau_case(name)
    ref = case.ref
    if layout == "unequal":
        words, sizes = ref.words, [ref.n // 2 + 11, ref.n // 3 - 7, 0]
        sizes[2] = ref.n - sizes[0] - sizes[1]
    else:
        words, sizes = _one_shard_layout(case)
    assert sum(sizes) == ref.n and min(sizes) > 64
    t = torch.from_numpy(np.array(words)).cuda()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    shards = [t[int(offs[i]):int(offs[i + 1])] for i in range(3)]
    sh = kselect.ShardedSelector([0, 0, 0])
    try:
        got = [sh.select(shards, p.k, sizes) & 0xFFFFFFFF for p in case.probes]
        assert got == ref.wants(case.ks()), (name, layout, case.probes, [hex(g) for g in got])
    finally:
        sh.close()


# ----------------------------------- 4. radix and LDS paths: every rank, every digit
def _all_ranks(sel, ref, ks):
    got = sel.select_multi(_dev(ref), ks, f32=ref.f32)
    return np.ascontiguousarray(got).view(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2049, 16385])
@pytest.mark.parametrize("content", ["random", "f32_specials", "staircase"])
def test_every_rank_of_a_small_input(gpu, content, n):
    """Every rank 1..n of an LDS-path input (n <= 16384) and of the smallest radix-path
    input, eight a call through select_multi (below 4 Mi keys it runs the single select
    per rank): the whole result against the sorted array, in one assert."""
    import kselect
    ref = re_.small_content(content, n)
    got = _all_ranks(gpu, ref, list(range(1, n + 1)))
    want = np.array([ref.key_bits(v) for v in ref.sorted], dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (content, n, "first wrong ranks", (bad[:8] + 1).tolist(), [hex(x) for x in got[bad[:8]]],
                           [hex(x) for x in want[bad[:8]]])
    st = gpu.stats()
    assert st["error"] == 0 and st["path"] == (kselect.KTH_PATH_LDS if n <= re_.SMALL_N else kselect.KTH_PATH_RADIX), st


@pytest.mark.parametrize("n", [100003, 1 << 22])
def test_staircase_group_edges(gpu, n):
    """The radix path (1 << 22 is its largest size) at the first and the last rank of every
    staircase tie group: every digit split has a bin boundary between two groups."""
    ref, first, last = re_.staircase(n)
    ks = np.unique(np.concatenate([first, last])).tolist()
    got = _all_ranks(gpu, ref, ks)
    want = np.array(ref.wants(ks), dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (n, [(ks[i], hex(got[i]), hex(want[i])) for i in bad[:8]])
    assert gpu.stats()["error"] == 0 and gpu.stats()["path"] == 2


@pytest.mark.parametrize("largest", [False, True])
def test_staircase_topk(gpu, largest):
    """topk below the window path with the k-th key on the first and last rank of every
    staircase group (tile-flag for k <= n / 1024, plain above)."""
    n = 100003
    ref, first, last = re_.staircase(n)
    d = _dev(ref)
    for rank in np.unique(np.concatenate([first, last])).tolist():
        _check_topk(gpu, ref, d, _topk_k(ref, rank, largest), largest, ("staircase", rank), path=2)


# ------------------------------------------------------------------ 5. 16-bit keys
def _k16_dev(d):
    import torch
    base = torch.zeros(d.n + 8, dtype=torch.int16, device="cuda")
    dev = base[:d.n]
    dev.copy_(torch.from_numpy(d.bits.view(np.int16)))
    return dev


def _k16_select(sel, d, dev, ks):
    return re_.k16t.to_bits(sel.select16_multi(dev, list(ks), n=d.n, kind=d.kind), d.kind)


def _k16_counts(d, st, k):
    """cnt_lt and candidates against numpy's counts for the reported window [lo, hi]."""
    lo, hi = st["lo_key"], st["hi_key"]
    lt = int(np.searchsorted(d.sorted, np.uint16(lo), side="left"))
    inside = int(np.searchsorted(d.sorted, np.uint16(hi), side="right")) - lt
    assert (st["cnt_lt"], st["candidates"]) == (lt, inside) and lt < k <= lt + inside, (d.kind, d.n, k, lt, inside, st)


@pytest.mark.parametrize("n", re_.K16_SIZES)
@pytest.mark.parametrize("kind", re_.k16t.KINDS)
def test_k16_group_edges(gpu, kind, n):
    """First and last rank of the tie groups nearest the quantiles {0, .01, .5, .99, 1} and of
    their neighbours (float kinds: also of -0.0, +0.0, +inf, NaN): select16_multi eight a
    call, the single select with its counts, and topk16 smallest and largest."""
    import torch
    d = re_.k16_input(kind, n)
    dev = _k16_dev(d)
    ks = d.edge_ranks()
    want = d.wants(ks)
    got = _k16_select(gpu, d, dev, ks)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (kind, n, [(ks[i], hex(got[i]), hex(want[i])) for i in bad[:8]])
    for k, w in zip(ks, want):
        assert _k16_select(gpu, d, dev, [k])[0] == w, (kind, n, k)
        st = gpu.stats()
        assert st["error"] == 0 and st["answer"] & 0xFFFF == w and st["k"] == k, (kind, n, k, st)
        _k16_counts(d, st, k)
    for largest in (False, True):
        for rank in ks:
            k = n - rank + 1 if largest else rank
            vals = torch.full((k,), 0x5A5A, dtype=torch.int16, device="cuda")
            idx = torch.full((k,), -1, dtype=torch.int64, device="cuda")
            gpu.topk16(dev, n, k, vals, idx, largest=largest, kind=kind)
            gpu.sync()
            assert gpu.stats()["error"] == 0, (kind, n, k, largest, gpu.stats())
            wi = d.topk(k, largest)
            np.testing.assert_array_equal(idx.cpu().numpy(), wi, err_msg=f"{kind} n={n} k={k} largest={largest}")
            np.testing.assert_array_equal(vals.cpu().numpy().view(np.uint16), re_.k16t.of_order_key(d.key[wi], kind),
                                          err_msg=f"{kind} n={n} k={k} largest={largest}")


@pytest.mark.parametrize("n", re_.K16_SIZES)
@pytest.mark.parametrize("kind", re_.k16t.KINDS)
def test_k16_median_edges_with_the_miss_hook(kind, n):
    """The quantile-0.5 groups' edges on a ctx whose sample window holds no key
    (KTH_HOOK_K16_MISS): the later passes produce every answer."""
    import kselect
    d = re_.k16_input(kind, n)
    dev = _k16_dev(d)
    ks = d.edge_ranks(quantiles=(0.5,))
    sel = kselect.Selector(0)
    try:
        sel.test_hook(kselect.KTH_HOOK_K16_MISS, 1)
        got = _k16_select(sel, d, dev, ks)
        assert np.array_equal(got, d.wants(ks)), (kind, n, ks, got, d.wants(ks))
        for i, k in enumerate(ks[:8] if len(ks) <= 8 else []):
            st = sel.multi_stats(i)
            assert st["error"] == 0 and st["k"] == k, st
            assert st["path"] == (kselect.KTH_PATH_K16 if n <= re_.k16t.SMALL_N else kselect.KTH_PATH_K16_FALLBACK), st
            _k16_counts(d, st, k)
    finally:
        sel.close()
