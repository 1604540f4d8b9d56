"""GPU: graph capture and replay of the asynchronous selects (include/kth.h
"graph capture": kth_select_{i32,f32}_async, kth_select_multi_{i32,f32}_async,
kth_select_{,multi_}k16_async), and the ctx state one call leaves for the next.

A captured graph freezes the launches a call enqueued -- kernel arguments,
clears, copies -- and runs them again, any number of times, between any other
calls on the ctx.  So whatever a select needs from the ctx's scratch must hold
whenever its launches run again as enqueued: after itself, after another form,
after a call that ended in a reported error.

Every graph is captured on the one stream the ctx is bound to and replayed on
it.  Every expected value is a numpy restatement computed on the host from the
buffer's current contents (int32: np.sort; float32 and 16-bit: the sort of the
order keys, tests/test_gpu_f32.py and tests/test_gpu_k16.py), compared on bit
patterns; each content is sorted once a module run.  Every output word is set
to a sentinel before the launch that writes it.
"""
import numpy as np
import pytest

import test_gpu_f32 as f32t
import test_gpu_k16 as k16t

pytestmark = pytest.mark.gpu

N_RADIX = (1 << 20) + 7    # cooperative radix path: k_finish alone
N_WINDOW = (1 << 23) + 13  # window path: k_head + k_main + k_finish
K16_NS = (32768, (1 << 20) + 5)  # full histogram / streaming
SENT = 0x5A5A5A5A          # (no content below has it as an answer: asserted where it matters)
SENT16 = 0x5A5A
CONTENTS = {"i32": ("uniform", "narrow", "spike", "sorted_desc"),
            "f32": ("uniform", "specials", "spike", "sorted_desc"),
            "k16": ("randn", "specials", "all_equal", "uniform")}


def ranks(n):
    return [1, n // 3, n // 2, n]


# ---------------------------------------------------------------- contents
def _sampled_index(n):
    """The keys the window path samples: ceil(s / C) chunks of C keys, n / chunks apart (include/kth.h)."""
    import kselect
    s, c = int(kselect.LIB.kth_dist_sample_size(n)), int(kselect.LIB.kth_sample_chunk())
    nch = -(-s // c)
    return ((np.arange(nch, dtype=np.int64) * (n // nch))[:, None] + np.arange(c, dtype=np.int64)[None, :]).ravel()


def _spike(words, band, value):
    """One value in place of every key of the band around the median, except in
    the sampled chunks: the sample shows no cluster, so the median's window
    holds about a fifth of the keys -- over the candidate capacity -- and that
    rank takes the exact fallback over the input; the outer ranks do not.
    (This follows the library's sample layout, kth_dist_sample_size and
    kth_sample_chunk.  The tests assert path 4 / 3 on this content, so a change
    of the sampling scheme shows as those assertions failing, not as a silent
    loss of the fallback case: then this fixture needs the new layout.)"""
    off = np.ones(words.size, dtype=bool)
    idx = _sampled_index(words.size)
    off[idx[idx < words.size]] = False
    out = words.copy()
    out[off & band] = value
    return out


def _make(kind, name, n):
    """The raw words of a content: int32, float32 bits (uint32) or 16-bit patterns (uint16)."""
    rng = np.random.default_rng([n, len(name), ord(name[0])])
    if kind == "i32":
        uni = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
        if name == "uniform":
            return uni
        if name == "narrow":  # heavy ties on the window's edges
            return rng.integers(-300, 300, n).astype(np.int32)
        if name == "spike":
            return _spike(uni, np.abs(uni.astype(np.int64)) < (1 << 32) // 10, np.int32(12345))
        if name == "sorted_desc":
            return np.sort(uni)[::-1].copy()
    elif kind == "f32":
        if name == "spike":
            uni = f32t.make("uniform", n)
            return _spike(uni, np.abs(uni.view(np.float32)) < 0.2, f32t._bits(np.array([0.001]))[0])
        return np.array(f32t.make(name, n))
    else:
        return k16t.family(name, n, kind)
    raise KeyError((kind, name))


class Content:
    """A content of n keys: the raw words and the sorted order keys."""

    def __init__(self, kind, name, n):
        self.kind, self.name, self.n = kind, name, n
        self.words = np.ascontiguousarray(_make(kind, name, n))
        if kind == "i32":
            self.sorted = np.sort(self.words)
        elif kind == "f32":
            self.sorted = np.sort(f32t._f32_order_key(self.words))
        else:
            self.sorted = np.sort(k16t.order_key(self.words, kind))

    def want(self, k):
        """The k-th smallest as its bit pattern (an int)."""
        v = self.sorted[k - 1]
        if self.kind == "i32":
            return int(v) & 0xFFFFFFFF
        if self.kind == "f32":
            return int(f32t._bits_of_key(v))
        return int(k16t.of_order_key(v, self.kind))

    def tensor(self):
        import torch
        if self.kind in ("i32", "f32"):
            return torch.from_numpy(self.words.view(np.int32))
        return torch.from_numpy(self.words.view(np.int16))


_CACHE = {}


def content(kind, name, n):
    key = (kind, name, n)
    if key not in _CACHE:
        _CACHE[key] = Content(kind, name, n)
    return _CACHE[key]


def reinterpret(c, kind, n):
    """The first n keys of an int32 content read as another kind (the same device words)."""
    key = (kind, "as " + c.name, n, c.n)
    if key not in _CACHE:
        r = Content.__new__(Content)
        r.kind, r.name, r.n = kind, c.name, n
        r.words = c.words.view(np.uint32) if kind == "f32" else c.words.view(np.uint16)[:n]
        r.sorted = np.sort(f32t._f32_order_key(r.words) if kind == "f32" else k16t.order_key(r.words, kind))
        _CACHE[key] = r
    return _CACHE[key]


# ------------------------------------------------------------------ plumbing
class Bench:
    """One stream, one ctx bound to it, one key buffer whose contents change between replays."""

    def __init__(self, kind, n):
        import torch
        import kselect
        self.kind, self.n = kind, n
        self.stream = torch.cuda.Stream()
        self.sel = kselect.Selector(0, stream=self.stream)
        self.words = torch.zeros(n, dtype=torch.int16 if kind not in ("i32", "f32") else torch.int32, device="cuda")
        self.keys = self.words.view(torch.float32) if kind == "f32" else self.words
        self.now = None
        torch.cuda.synchronize()

    def load(self, c):
        import torch
        self.words.copy_(c.tensor())
        torch.cuda.synchronize()
        self.now = c

    def out(self, m):
        import torch
        if self.kind == "i32":
            return torch.full((m,), SENT, dtype=torch.int32, device="cuda")
        if self.kind == "f32":
            return torch.full((m,), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
        return torch.full((m,), SENT16, dtype=torch.int16, device="cuda")

    def capture(self, enqueue):
        """A graph of what enqueue() sends to the ctx; an error inside the capture fails the test."""
        import torch
        import kselect
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=self.stream):
                enqueue()
        except (kselect.KthError, RuntimeError) as e:
            pytest.fail(f"the capture did not complete: {e!r}")
        torch.cuda.synchronize()
        return g

    def replay(self, g, *outs):
        import torch
        for o in outs:
            reset(o)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            g.replay()
        torch.cuda.synchronize()

    def eager(self, fn, *outs):
        """fn() enqueues on the ctx stream; returns after it has run."""
        import torch
        for o in outs:
            reset(o)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            fn()
        torch.cuda.synchronize()

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.sel.close()


def reset(o):
    import torch
    if o.dtype == torch.int16:
        o.fill_(SENT16)
    elif o.dtype == torch.float32:
        o.view(torch.int32).fill_(SENT)
    elif o.dtype == torch.int64:
        o.fill_(-1)
    else:
        o.fill_(SENT)


def bits(o):
    """A device output's words as Python ints (bit patterns)."""
    import torch
    if o.dtype == torch.int16:
        return [int(x) for x in o.cpu().numpy().view(np.uint16)]
    if o.dtype == torch.float32:
        o = o.view(torch.int32)
    return [int(x) for x in o.cpu().numpy().view(np.uint32)]


def expect(o, c, ks, what):
    got, want = bits(o), [c.want(k) for k in ks]
    assert got == want, (what, c.kind, c.name, c.n, list(ks), [hex(x) for x in got], [hex(x) for x in want])


def check_stats(st, c, k, what):
    mask = 0xFFFF if c.kind not in ("i32", "f32") else 0xFFFFFFFF
    assert st["error"] == 0 and st["n"] == c.n and st["k"] == k and st["answer"] & mask == c.want(k), (
        what, c.kind, c.name, k, hex(c.want(k)), st)


def schedule(b, kind, n):
    """The replay schedule: (content, is the buffer to be rewritten first).  The
    first two replays run back to back on unchanged contents, then one a new content."""
    names = CONTENTS["k16" if kind not in ("i32", "f32") else kind]
    first = content(kind, names[0], n)
    b.load(first)
    yield first
    yield first
    for name in names[1:]:
        c = content(kind, name, n)
        b.load(c)
        yield c


def select_call(b, k, o):
    """One asynchronous select of b's buffer, of its kind."""
    if b.kind in ("i32", "f32"):
        return lambda: b.sel.select_async(b.keys, b.n, k, o, f32=b.kind == "f32")
    return lambda: b.sel.select16_async(b.keys, b.n, k, o, kind=b.kind)


# --------------------------------------------------------------- the selects
@pytest.mark.parametrize("nsel", [1, 2, 3])
@pytest.mark.parametrize("n", [N_RADIX, N_WINDOW])
@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_one_select_graph_replayed(kind, n, nsel):
    """A graph of one, two and three selects (an odd count is the case the
    alternating k_finish slot sets could not run twice in a row)."""
    ks = {1: [n // 2], 2: [1, n], 3: [n // 3, n // 2, n]}[nsel]
    b = Bench(kind, n)
    try:
        b.sel.reserve(n)
        o = b.out(nsel)
        b.load(content(kind, CONTENTS[kind][0], n))
        g = b.capture(lambda: [select_call(b, k, o[i:i + 1])() for i, k in enumerate(ks)])
        for r, c in enumerate(schedule(b, kind, n)):
            b.replay(g, o)
            expect(o, c, ks, f"replay {r}")
            check_stats(b.sel.stats(), c, ks[-1], f"replay {r}")
            if c.name == "spike" and n == N_WINDOW:
                assert b.sel.stats()["path"] == (4 if ks[-1] == n // 2 else 3), b.sel.stats()
    finally:
        b.close()


@pytest.mark.parametrize("kind", ["i32", "f32"])
def test_multi_graph_replayed(kind):
    """Rank lists of 2, 3 and 8 distinct ranks and one duplicate each.  With 2
    and 3 distinct ranks the list is one call, the duplicate's device-to-device
    copy a graph node, and on the spike content exactly the median takes the
    fallback while the other ranks stay on the window path.  The list of 9 goes
    as the wrapper sends it: a call of 8 distinct ranks and a call of one (the
    single select's launches), both in the one graph; multi_stats then speaks
    of that last call."""
    n = N_WINDOW
    lists = [[n // 3, n // 2, n // 3], [1, n // 2, n, n // 2],
             [1, n // 3, n // 2, n, n // 4, 3 * n // 4, n // 100 + 1, 2, n // 2]]
    for ks in lists:
        b = Bench(kind, n)
        try:
            b.sel.reserve_multi(n, 8)
            o = b.out(len(ks))
            b.load(content(kind, CONTENTS[kind][0], n))
            g = b.capture(lambda: b.sel.select_multi_async(b.keys, n, ks, o, f32=kind == "f32"))
            last = ks[len(ks) - len(ks) % 8:] if len(ks) > 8 else ks  # multi_stats: the last group of 8 sent
            for r, c in enumerate(schedule(b, kind, n)):
                b.replay(g, o)
                expect(o, c, ks, f"replay {r} of {len(ks)} ranks")
                stats = [b.sel.multi_stats(i) for i in range(len(last))]
                for i, st in enumerate(stats):
                    check_stats(st, c, last[i], f"replay {r} rank {i}")
                if c.name == "spike":
                    assert [st["path"] for st in stats] == [4 if k == n // 2 else 3 for k in last], stats
        finally:
            b.close()


@pytest.mark.parametrize("n", K16_NS)
@pytest.mark.parametrize("kind", ["bf16", "i16"])
def test_k16_graph_replayed(kind, n):
    """The single and the multi (4 ranks) 16-bit forms, and a second set captured
    with KTH_HOOK_K16_MISS on: the sample phase publishes an empty window, so the
    later passes do the work."""
    import kselect
    ks = ranks(n)
    b = Bench(kind, n)
    try:
        b.sel.reserve16(n, 8)
        o1, o4 = b.out(1), b.out(4)
        b.load(content(kind, CONTENTS["k16"][0], n))
        for miss in (0, 1):
            b.sel.test_hook(kselect.KTH_HOOK_K16_MISS, miss)
            g1 = b.capture(select_call(b, n // 2, o1))
            g4 = b.capture(lambda: b.sel.select16_multi_async(b.keys, n, ks, o4, kind=kind))
            b.sel.test_hook(kselect.KTH_HOOK_K16_MISS, 0)  # frozen at capture: turning it off changes no replay
            for r, c in enumerate(schedule(b, kind, n)):
                b.replay(g1, o1)
                expect(o1, c, [n // 2], f"single, miss {miss}, replay {r}")
                b.replay(g4, o4)
                expect(o4, c, ks, f"multi, miss {miss}, replay {r}")
                for i, k in enumerate(ks):
                    st = b.sel.multi_stats(i)
                    check_stats(st, c, k, f"multi, miss {miss}, replay {r}")
                    if n > k16t.SMALL_N:
                        assert st["path"] == (kselect.KTH_PATH_K16_FALLBACK if miss else kselect.KTH_PATH_K16), st
    finally:
        b.close()


# ------------------------------------------------- replays among eager calls
def _topk_want(c, k):
    """Indices of the k smallest in index order, ties by index."""
    key = ("argsort", c.kind, c.name, c.n)
    if key not in _CACHE:
        _CACHE[key] = np.argsort(c.words, kind="stable")
    return np.sort(_CACHE[key][:k])


def _eager_topk(b, other, c, k):
    import torch
    vals = torch.empty(k, dtype=torch.int32, device="cuda")
    idx = torch.empty(k, dtype=torch.int64, device="cuda")
    b.eager(lambda: b.sel.topk(other, c.n, k, vals, idx), vals, idx)
    want = _topk_want(c, k)
    np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"top-{k} indices")
    np.testing.assert_array_equal(vals.cpu().numpy(), c.words[want], err_msg=f"top-{k} values")
    assert b.sel.stats()["error"] == 0, b.sel.stats()


def test_replay_between_eager_calls():
    """One ctx, one captured select, and between its replays every other kind of
    call the ctx takes, each on other keys: an odd number of selects, a multi
    call of three ranks, top-k with each kind of k_main record, the rows
    kernels, a 16-bit select.  stats() follows the launches that ran last,
    replayed or eager."""
    import torch
    n, n16 = N_WINDOW, K16_NS[1]
    b = Bench("i32", n)
    try:
        sel = b.sel
        c = content("i32", "uniform", n)
        b.load(c)
        oc = content("i32", "narrow", n)
        other = oc.tensor().cuda()
        c16 = content("i16", "randn", n16)
        keys16 = c16.tensor().cuda()
        rows, cols, kr = 64, 4096, 1000
        mat = oc.words[:rows * cols].reshape(rows, cols)
        dmat = torch.from_numpy(mat).cuda()
        mat_order = np.argsort(mat, axis=1, kind="stable")
        o, oe, om, o16 = b.out(1), b.out(1), b.out(3), torch.zeros(1, dtype=torch.int16, device="cuda")
        orow = torch.zeros(rows, dtype=torch.int32, device="cuda")
        rvals = torch.zeros(rows, kr, dtype=torch.int32, device="cuda")
        ridx = torch.zeros(rows, kr, dtype=torch.int32, device="cuda")
        kg, mks = n // 2, [n // 3, n // 2, n]

        def one_select():
            b.eager(lambda: sel.select_async(other, n, n // 3, oe), oe)
            expect(oe, oc, [n // 3], "eager select")
            check_stats(sel.stats(), oc, n // 3, "eager select")

        def multi3():
            b.eager(lambda: sel.select_multi_async(other, n, mks, om), om)
            expect(om, oc, mks, "eager multi")
            assert all(sel.multi_stats(i)["error"] == 0 for i in range(3))

        def rows_calls():
            b.eager(lambda: sel.rows(dmat, rows, cols, kr, orow), orow)
            np.testing.assert_array_equal(orow.cpu().numpy(), np.sort(mat, axis=1)[:, kr - 1])
            b.eager(lambda: sel.topk_rows(dmat, rows, cols, kr, rvals, ridx), rvals, ridx)
            want = np.sort(mat_order[:, :kr], axis=1)
            np.testing.assert_array_equal(ridx.cpu().numpy(), want)
            np.testing.assert_array_equal(rvals.cpu().numpy(), np.take_along_axis(mat, want, axis=1))

        def select16():
            b.eager(lambda: sel.select16_async(keys16, n16, n16 // 3, o16, kind="i16"), o16)
            expect(o16, c16, [n16 // 3], "eager 16-bit select")

        steps = [one_select, multi3, lambda: _eager_topk(b, other, oc, 100), lambda: _eager_topk(b, other, oc, n // 32),
                 lambda: _eager_topk(b, other, oc, n // 4), rows_calls, select16]
        # every buffer the eager calls need exists before the capture: none may grow while the graph is alive
        sel.reserve(n)
        sel.reserve_multi(n, 3)
        sel.reserve16(n16, 1)
        for step in steps:
            step()
        g = b.capture(select_call(b, kg, o))
        for i, step in enumerate(steps + [select16]):
            b.replay(g, o)
            expect(o, c, [kg], f"replay before step {i}")
            # (the last round: a replay that follows a 16-bit call)
            check_stats(sel.stats(), c, kg, f"replay before step {i}")
            step()
        # a 16-bit call that follows a replay
        check_stats(sel.stats(), c16, n16 // 3, "16-bit select after a replay")
        b.replay(g, o)
        b.replay(g, o)
        expect(o, c, [kg], "the last replays")
        check_stats(sel.stats(), c, kg, "the last replays")
        # the host's rank map is the 16-bit call's; what ran last is not: no stale state is decoded
        import kselect
        with pytest.raises(kselect.KthError):
            sel.multi_stats(0)
    finally:
        b.close()


@pytest.mark.parametrize("second", ["f32", "i16"])
def test_two_graphs_one_ctx(second):
    """Graph A selects the buffer's int32 words, graph B the same words as
    float32 keys or as 16-bit keys, on one ctx, in the order A A B A B B A."""
    n = N_WINDOW
    nb = n if second == "f32" else K16_NS[1]
    a = Bench("i32", n)
    try:
        import torch
        bb = Bench.__new__(Bench)  # the same ctx, stream and device words, read as the other kind
        bb.kind, bb.n, bb.sel, bb.stream = second, nb, a.sel, a.stream
        bb.keys = a.words.view(torch.float32) if second == "f32" else a.words.view(torch.int16)[:nb]
        a.sel.reserve(n)
        a.sel.reserve16(nb, 1)
        ca = content("i32", "uniform", n)
        cb = reinterpret(ca, second, nb)
        a.load(ca)
        oa, ob = a.out(1), bb.out(1)
        ka, kb = n // 2, nb // 3
        ga = a.capture(select_call(a, ka, oa))
        gb = a.capture(select_call(bb, kb, ob))
        for i, which in enumerate("AABABBA"):
            if which == "A":
                a.replay(ga, oa)
                expect(oa, ca, [ka], f"step {i} A")
                check_stats(a.sel.stats(), ca, ka, f"step {i} A")
            else:
                a.replay(gb, ob)
                expect(ob, cb, [kb], f"step {i} B")
                check_stats(a.sel.stats(), cb, kb, f"step {i} B")
    finally:
        a.close()


@pytest.mark.parametrize("form", ["select", "select_f32", "multi", "k16", "k16_multi"])
def test_capture_after_reserve_allocates_nothing(form):
    """A fresh ctx gets only its reserve call; the first call of the form then
    runs inside a capture (torch's default, global capture mode, where an
    allocation or a synchronisation is an error).  The capture completes and
    its first replay is exact."""
    n = K16_NS[1] if form.startswith("k16") else N_WINDOW
    kind = {"select": "i32", "select_f32": "f32", "multi": "i32", "k16": "bf16", "k16_multi": "bf16"}[form]
    b = Bench(kind, n)
    try:
        c = content(kind, CONTENTS["k16" if form.startswith("k16") else kind][0], n)
        b.load(c)
        ks = [n // 2] if form in ("select", "select_f32", "k16") else [1, n // 3, n // 2, n, n // 4, n - 1, 2, n // 3]
        o = b.out(len(ks))
        if form in ("select", "select_f32"):
            b.sel.reserve(n)
            call = select_call(b, ks[0], o)
        elif form == "multi":
            b.sel.reserve_multi(n, 8)
            call = lambda: b.sel.select_multi_async(b.keys, n, ks, o)  # noqa: E731
        else:
            b.sel.reserve16(n, 8)
            call = select_call(b, ks[0], o) if form == "k16" else (
                lambda: b.sel.select16_multi_async(b.keys, n, ks, o, kind=kind))
        g = b.capture(call)
        b.replay(g, o)
        expect(o, c, ks, form)
        assert b.sel.stats()["error"] == 0, b.sel.stats()
    finally:
        b.close()


def test_per_level_ctx_graph(monkeypatch):
    """KTH_COOP=0: the per-level launches.  A top-k with candidate rows leaves
    the candidate count to be cleared later; a graph captured on the clean ctx
    holds no such clear and must still find clean slots."""
    monkeypatch.setenv("KTH_COOP", "0")
    n = N_WINDOW
    b = Bench("i32", n)
    try:
        assert not b.sel.coop()
        b.sel.reserve(n)
        c = content("i32", "uniform", n)
        b.load(c)
        # (uniform keys: the top-k's window holds ~10^5 candidates, the count it leaves is not 0)
        _eager_topk(b, b.keys, c, n // 4)  # (its buffers exist before the capture)
        b.eager(lambda: b.sel.select_async(b.keys, n, 1, b.out(1)))  # the ctx is clean again
        o = b.out(1)
        g = b.capture(select_call(b, n // 2, o))
        for r in range(2):
            b.replay(g, o)
            expect(o, c, [n // 2], f"replay {r}")
        _eager_topk(b, b.keys, c, n // 4)
        b.replay(g, o)
        expect(o, c, [n // 2], "replay after a top-k with candidate rows")
        check_stats(b.sel.stats(), c, n // 2, "replay after a top-k with candidate rows")
        assert b.sel.stats()["path"] == 3
    finally:
        b.close()


# ------------------------------------------------ after a reported timeout
@pytest.mark.parametrize("n", [N_RADIX, N_WINDOW])
@pytest.mark.parametrize("first", ["select", "multi"])
def test_async_error_then_next_call(first, n):
    """An asynchronous call ends in a reported barrier timeout (the software
    hook, value 2: the next cooperative launch only) and the host never looks:
    no stats(), no sync().  The calls that follow on the stream are exact, and
    the timed-out call wrote no unverified answer."""
    import torch
    import kselect
    n16 = K16_NS[1]
    b = Bench("i32", n)
    try:
        sel = b.sel
        c = content("i32", "uniform", n)
        b.load(c)
        c16 = content("i16", "randn", n16)
        keys16 = c16.tensor().cuda()
        mks = [n // 3, n // 2, n]
        bad, o1, om, o16 = b.out(3), b.out(1), b.out(3), torch.full((1,), SENT16, dtype=torch.int16, device="cuda")
        kt = 100
        vals = torch.full((kt,), SENT, dtype=torch.int32, device="cuda")
        idx = torch.full((kt,), -1, dtype=torch.int64, device="cuda")
        sel.reserve(n)
        sel.reserve_multi(n, 3)
        sel.reserve16(n16, 1)
        torch.cuda.synchronize()
        sel.test_hook(kselect.KTH_HOOK_FAULT_BARRIER, 2)
        with torch.cuda.stream(b.stream):
            if first == "select":
                sel.select_async(b.keys, n, n // 2, bad[0:1])
            else:
                sel.select_multi_async(b.keys, n, mks, bad)
            sel.select_async(b.keys, n, n // 3, o1)
            sel.select_multi_async(b.keys, n, mks, om)
            sel.select16_async(keys16, n16, n16 // 2, o16, kind="i16")
            sel.topk(b.keys, n, kt, vals, idx)
        torch.cuda.synchronize()
        got = bits(bad)
        assert got[0] == SENT, hex(got[0])  # the launch that timed out resolved this rank
        if first == "multi":  # its other ranks: verified answers or nothing
            assert all(g in (SENT, c.want(k)) for g, k in zip(got[1:], mks[1:])), [hex(g) for g in got]
        else:
            assert got[1:] == [SENT, SENT]
        expect(o1, c, [n // 3], "select after the timeout")
        expect(om, c, mks, "multi call after the timeout")
        expect(o16, c16, [n16 // 2], "16-bit select after the timeout")
        want = _topk_want(c, kt)
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        np.testing.assert_array_equal(vals.cpu().numpy(), c.words[want])
        assert sel.stats()["error"] == 0, sel.stats()
    finally:
        b.close()
