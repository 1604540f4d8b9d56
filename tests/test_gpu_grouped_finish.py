"""GPU: the grouped finish of the single-GPU window select.

k_main<0> writes each workgroup's candidates grouped by their first digit and
a directory row; k_finish then gathers the picked bin in one workgroup
(KTH_FINISH_GROUPED) instead of scanning every slice (KTH_FINISH_SLICES, which
KTH_HOOK_FINISH_SLICES forces and which serves as the reference form here).
Every answer is compared, as a bit pattern, with a host sort of the same words
(each content is sorted once a module run).

Sizes: the smallest on the window path (n > 2^22).  At 2^22 + 5 half of
k_main's workgroups stream no tile at all, so their rows hold no candidate.

A plain sorted input does not make a wave flush at these sizes: every
workgroup streams at most two tiles that lie n / 2 apart, and the window covers
far less, so a wave stages at most its 2048 keys of one tile -- exactly its
region.  The flushing input here is therefore two interleaved sorted runs
(`two_runs`): the window's keys then fill both tiles of a workgroup.
"""
import numpy as np
import pytest

import test_gpu_f32 as f32t

pytestmark = pytest.mark.gpu

N_SMALL, N_MID, N_BIG = (1 << 22) + 5, (1 << 23) + 3, (1 << 24) + 5
TILE = 8192          # keys of one k_main tile (256 threads x 8 loads x 4 keys)
WAVE_REGION = 2048   # keys a k_main wave stages before it has to flush
FIN_LDS_KEYS = 32768  # keys the finishing workgroup holds
SENT = 0x5A5A5A5A


def _forms():
    import kselect
    return kselect.KTH_FINISH_COUNTS, kselect.KTH_FINISH_SLICES, kselect.KTH_FINISH_GROUPED, kselect.KTH_FINISH_LEVELS


class Content:
    """int32 words (or float32 bit patterns) and their sorted order."""

    def __init__(self, words, f32=False):
        self.f32 = f32
        self.words = np.ascontiguousarray(words)
        self.n = self.words.size
        self.sorted = np.sort(f32t._f32_order_key(self.words)) if f32 else np.sort(self.words)

    def want(self, k):
        v = self.sorted[k - 1]
        return int(f32t._bits_of_key(v)) if self.f32 else int(v) & 0xFFFFFFFF

    def dev(self, pad=0):
        import torch
        host = np.array(self.words.view(np.float32) if self.f32 else self.words)
        if pad:
            host = np.concatenate([np.zeros(pad, dtype=host.dtype), host])
        return torch.from_numpy(host).cuda()


def _uniform(n, seed=0):
    rng = np.random.default_rng([n, seed])
    return rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)


def _make(name, n):
    if name == "uniform":
        return Content(_uniform(n))
    if name == "uniform_b":
        return Content(_uniform(n, 1))
    if name == "uniform_c":
        return Content(_uniform(n, 2))
    if name == "uniform_f32":
        return Content(f32t.make("uniform", n), f32=True)
    if name == "dense_source":
        # 1500 consecutive positions at the start of a tile, all within +-64 of
        # the median: one workgroup holds them, <= 1024 + 476 of them in the two
        # 1024-key rows they span, so <= 512 a wave -- far under its region
        # even with the tile's uniform candidates (at most 2048 - 512 more)
        w = _uniform(n)
        med = int(np.sort(w)[n // 2])
        run, at = 1500, 3 * TILE
        per_wave = -(-run // 1024) * 256
        assert run < WAVE_REGION and per_wave + 256 < WAVE_REGION and at % TILE == 0 and at + run <= n
        rng = np.random.default_rng(7)
        w[at:at + run] = (med + rng.integers(-64, 65, run)).astype(np.int32)
        return Content(w)
    if name == "heavy_ties":
        # 40000 copies of the median at random positions: ~5 a workgroup, so no
        # wave flushes, yet the picked first-digit bin holds more keys than the
        # finishing workgroup's LDS
        w = _uniform(n)
        med = np.sort(w)[n // 2]
        pos = np.random.default_rng(11).choice(n, 40000, replace=False)
        w[pos] = med
        assert 40000 > FIN_LDS_KEYS
        return Content(w)
    if name == "sorted":
        return Content(np.sort(_uniform(n)))
    if name == "two_runs":
        s = np.sort(_uniform(n))
        return Content(np.concatenate([s[0::2], s[1::2]]))
    if name == "all_equal":
        return Content(np.full(n, 77, dtype=np.int32))
    if name == "few_distinct":
        return Content(np.random.default_rng(5).integers(0, 5, n).astype(np.int32))
    raise KeyError(name)


_CACHE = {}


def content(name, n):
    if (name, n) not in _CACHE:
        _CACHE[(name, n)] = _make(name, n)
    return _CACHE[(name, n)]


def _select_bits(sel, d, k, f32):
    got = sel.select(d, k, f32=f32)
    return f32t._got_bits(got) if f32 else int(got) & 0xFFFFFFFF


def _check(sel, c, d, k, what):
    """One select: exact, no error; returns the finish form."""
    got = _select_bits(sel, d, k, c.f32)
    st, form = sel.stats(), sel.finish_form()
    assert got == c.want(k) and st["error"] == 0, (what, c.n, k, hex(got), hex(c.want(k)), form, st)
    return form


@pytest.mark.parametrize("name,n", [("uniform", N_SMALL), ("uniform", N_MID), ("uniform", N_BIG),
                                    ("uniform_f32", N_SMALL), ("uniform_f32", N_MID)])
def test_uniform_takes_the_grouped_form(gpu, name, n):
    """Uniform int32 and float32, k in {1, n/2, n}: grouped, and equal to the slice tail's answer."""
    import kselect
    _, slices, grouped, _ = _forms()
    c = content(name, n)
    d = c.dev()
    for k in (1, n // 2, n):
        assert _check(gpu, c, d, k, "grouped") == grouped, (name, n, k)
        gpu.test_hook(kselect.KTH_HOOK_FINISH_SLICES, 1)
        try:
            assert _check(gpu, c, d, k, "slices hook") == slices, (name, n, k)
        finally:
            gpu.test_hook(kselect.KTH_HOOK_FINISH_SLICES, 0)
    assert _check(gpu, c, d, n // 3, "grouped after the hook") == grouped


def test_one_dense_source(gpu):
    """One workgroup holds 1500 keys of the picked bin: the gather copies them cooperatively."""
    grouped = _forms()[2]
    c = content("dense_source", N_MID)
    d = c.dev()
    for k in (N_MID // 2, N_MID // 2 + 700, N_MID // 2 - 700):
        assert _check(gpu, c, d, k, "dense source") == grouped, k


def test_heavy_ties_fall_back(gpu):
    """The picked bin exceeds the finisher's LDS: every workgroup takes the slices, exact answer."""
    _, slices, grouped, levels = _forms()
    c = content("heavy_ties", N_MID)
    d = c.dev()
    form = _check(gpu, c, d, N_MID // 2, "heavy ties")
    st = gpu.stats()
    assert st["path"] == 3 and st["candidates"] > FIN_LDS_KEYS, st
    assert form in (slices, levels), form
    assert _check(gpu, content("uniform", N_MID), content("uniform", N_MID).dev(), N_MID // 2, "after") == grouped


@pytest.mark.parametrize("name,n,other_form_at", [("two_runs", N_BIG, "median"), ("all_equal", N_MID, "all"),
                                                  ("few_distinct", N_MID, "all"), ("sorted", N_MID, "none")])
def test_fallback_inputs_then_grouped(gpu, name, n, other_form_at):
    """Inputs that leave the common case (flushing waves: PreHist incomplete; answers from the
    edge counts), then a grouped select on the same ctx: no stale directory or PreHist.
    other_form_at: the ranks that must not take the grouped form.  two_runs flushes where the
    window fills both tiles of a workgroup: at the median (about 200 K candidates), not at
    k = 1 or n, whose windows hold a few thousand keys; plain sorted never does at this size
    (module docstring), so there only exactness and the next select are checked."""
    grouped = _forms()[2]
    c = content(name, n)
    d = c.dev()
    for k in (1, n // 2, n):
        form = _check(gpu, c, d, k, name)
        if other_form_at == "all" or (other_form_at == "median" and k == n // 2):
            assert form != grouped, (name, k, form)
        u = content("uniform", N_SMALL)
        assert _check(gpu, u, u.dev(), N_SMALL // 2, "grouped after " + name) == grouped


def test_unaligned_pointers_and_empty_workgroups(gpu):
    """Key pointers 1-3 words off 16 bytes; at this n half of k_main's workgroups have no candidate."""
    grouped = _forms()[2]
    c = content("uniform", N_SMALL)
    for off in (1, 2, 3):
        base = c.dev(pad=off)
        d = base[off:]
        assert d.data_ptr() % 16 == 4 * off and d.numel() == c.n
        for k in (1, c.n // 2, c.n):
            assert _check(gpu, c, d, k, "unaligned") == grouped, (off, k)


def test_graph_replay_of_a_grouped_select():
    """One captured grouped select, replayed three times over changed contents."""
    import torch

    import kselect
    grouped = _forms()[2]
    n, k = N_MID, N_MID // 2
    stream = torch.cuda.Stream()
    sel = kselect.Selector(0, stream=stream)
    try:
        keys = torch.zeros(n, dtype=torch.int32, device="cuda")
        out = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
        first = content("uniform", n)
        keys.copy_(first.dev())
        torch.cuda.synchronize()
        sel.reserve(n)
        with torch.cuda.stream(stream):  # eager once: the capture below allocates nothing
            sel.select_async(keys, n, k, out)
        torch.cuda.synchronize()
        assert int(out.cpu().numpy().view(np.uint32)[0]) == first.want(k)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            sel.select_async(keys, n, k, out)
        torch.cuda.synchronize()
        for name in ("uniform_b", "uniform_c", "uniform"):
            c = content(name, n)
            keys.copy_(c.dev())
            out.fill_(SENT)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                g.replay()
            torch.cuda.synchronize()
            got = int(out.cpu().numpy().view(np.uint32)[0])
            assert got == c.want(k) and c.want(k) != SENT, (name, hex(got), hex(c.want(k)))
            assert sel.finish_form() == grouped and sel.stats()["error"] == 0, (name, sel.finish_form(), sel.stats())
    finally:
        torch.cuda.synchronize()
        sel.close()
