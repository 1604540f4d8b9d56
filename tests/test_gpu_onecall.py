"""kth_dist_select_rccl -- the one library call kselect.dist.DistSelector.select
makes over RCCL, so what bench.py --gpus N runs -- at world 2 and 3 on one GPU.

Over RCCL the call has only ever run at world 1 on the one-GPU pool.  Its
world > 1 sequence (the all-gather of s_local words into s_local * world, the
window over that, the in-place all-reduce of each slot, the early result
before level 1, the level loop between collectives) runs here as P threads
with stand-in collectives (tests/onecall_ranks.py, which also says what the
stand-ins check on every collective and what they cannot reach).

References: the answer is a sort of the union; the collectives and their
payloads are those of the scripted form (kselect.dist.lockstep over
HipBackend) on the same shards and of the CPU restatement
(tests/dist_cpu_backend.py); the reference's own CGM answers for its golden
fixtures (TODO-kth-problem-cgm.c, `mpirun -n world`).
"""
import numpy as np
import pytest

import dist_inputs as di
from conftest import load_input

pytestmark = pytest.mark.gpu

WORLDS = [2, 3]


@pytest.fixture(scope="module")
def ranks(gpu):
    """Ranks(world) per world size, kept across the tests of the module (the
    same ctxs serve one case after the other)."""
    from onecall_ranks import Ranks
    made = {}

    def get(world):
        if world not in made:
            made[world] = Ranks(world)
        return made[world]
    yield get
    for r in made.values():
        r.close()


def _split(a, world):
    import torch
    from kselect.dist import shard_bounds
    bounds = [shard_bounds(a.size, r, world) for r in range(world)]
    return [torch.from_numpy(np.ascontiguousarray(a[s:s + m])).cuda() for s, m in bounds], [m for _, m in bounds]


def _all_exact(runs, want, what):
    from onecall_ranks import SENTINEL
    assert [r.rc for r in runs] == [0] * len(runs), (what, [r.rc for r in runs])
    assert [r.answer for r in runs] == [want] * len(runs), (what, [r.answer for r in runs], want)
    assert [r.error for r in runs] == [0] * len(runs), (what, [r.error for r in runs])
    # nothing reaches the answer tensor before the last collective is over
    assert all(v == SENTINEL for r in runs for v in r.out_seen), (what, [r.out_seen for r in runs])


@pytest.mark.parametrize("world", WORLDS)
def test_onecall_golden(ranks, golden, world):
    """The reference's fixtures by its block partition (TODO-kth-problem-cgm.c:81-100):
    every rank's answer is the true order statistic and every terminating
    `mpirun -n world` CGM answer.  (Cases under 64 keys per rank, or with a
    shard below the per-rank sample, belong to DistSelector._select_small.)"""
    rk = ranks(world)
    cache, checked, at_world, ran = {}, 0, 0, 0
    for c in golden["cases"]:
        a = load_input(c["input"])
        n = a.size
        if n // world < 64:
            continue
        if c["input"] not in cache:
            cache[c["input"]] = _split(a, world)
        shards, sizes = cache[c["input"]]
        if min(sizes) < di.s_local(n, world):
            continue
        runs = rk.select(shards, sizes, c["k"])
        _all_exact(runs, c["true"], c)
        ran += 1
        # the reference's own answers for this input and k: every terminating
        # `mpirun -n P` CGM run (this world's first of all) and its seq program
        # where that is not defective, as test_gpu_parity.test_golden_fixtures
        refs = [v for v in c["cgm_ref"].values() if v != "livelock"]
        if not c["seq_ref_defect"]:
            refs.append(c["seq_ref"])
        for v in refs:
            assert [r.answer for r in runs] == [v] * world, (c, v)
        checked += len(refs)
        at_world += c["cgm_ref"].get(str(world), "livelock") != "livelock"
    print("golden cases run", ran, "reference answers compared", checked, "of them CGM runs at this world", at_world)
    assert checked > 100 and at_world > 0, (checked, at_world, ran)


@pytest.mark.parametrize("world", WORLDS)
def test_onecall_families(gpu, ranks, world):
    """2^22 + 5 keys (uneven shards at world 3) of three families, each shard
    filled at its offset of the whole; k in {1, n/3, n/2, n}; with and without
    the early result."""
    import torch
    from kselect.dist import shard_bounds
    rk = ranks(world)
    n = (1 << 22) + 5
    for fam in ("uniform_full", "few_distinct", "sorted_desc"):
        shards, sizes = [], []
        for r in range(world):
            start, m = shard_bounds(n, r, world)
            t = torch.empty(m, dtype=torch.int32, device="cuda")
            gpu.fill(t, m, fam, param=7, offset=start, n_total=n)
            shards.append(t)
            sizes.append(m)
        gpu.sync()
        srt = np.sort(np.concatenate([t.cpu().numpy() for t in shards]))
        for k in (1, n // 3, n // 2, n):
            for early in (0, 1):
                _all_exact(rk.select(shards, sizes, k, early=early), int(srt[k - 1]), (fam, k, early))


@pytest.fixture(scope="module")
def scripted(gpu):
    """The scripted form on the device: lockstep over P HipBackends (their own
    ctxs, on the default stream), computed once per case."""
    import torch
    from kselect import Selector
    from kselect.dist import DistSelector, HipBackend, lockstep
    sels, shards, done = {}, {}, {}

    def run(case):
        P = len(case.sizes)
        if P not in sels:
            sels[P] = [Selector(0) for _ in range(P)]
        if (case.kind, case.sizes) not in shards:
            shards[(case.kind, case.sizes)] = di.device_tensors(case.kind, case.sizes)
            torch.cuda.synchronize()
        if case not in done:
            ds = [DistSelector(HipBackend(0, s), world=P) for s in sels[P]]
            seen = []
            outs = lockstep(ds, shards[(case.kind, case.sizes)], list(case.sizes), case.k,
                            observe=di.observer(seen, to_host=True))
            torch.cuda.synchronize()
            assert [d.error() for d in ds] == [0] * P
            done[case] = (seen, [int(o.item()) for o in outs])
        return shards[(case.kind, case.sizes)], done[case]
    yield run
    for ss in sels.values():
        for s in ss:
            s.close()


@pytest.mark.parametrize("case", di.CASES, ids=di.case_id)
def test_onecall_matches_scripted_and_restatement(ranks, scripted, case):
    """Every forced case (window miss, overflow on every rank, on one rank of
    three, two and three all-reduces): on every rank the one-call form makes
    the collectives of the scripted form and of the restatement, with the same
    payloads (dist_inputs.assert_payloads_equal), and the sorted union's answer;
    with the early result on, it writes nothing while more levels follow."""
    ref = di.reference(case)
    P = len(case.sizes)
    want = int(di.sorted_union(case.kind, case.sizes)[case.k - 1])
    shards, (seen, answers) = scripted(case)
    assert answers == [want] * P and ref.answer == want, (answers, ref.answer, want)
    assert ref.kinds == ("all_gather",) + ("all_reduce",) * ref.n_reduce and 2 <= ref.n_reduce <= 4
    for early in (0, 1):
        runs = ranks(P).select(shards, list(case.sizes), case.k, early=early)
        what = (di.case_id(case), "early", early)
        _all_exact(runs, want, what)
        for r in runs:
            assert r.calls == len(r.ops) == 1 + ref.n_reduce, (what, r.rank, r.calls)
            di.assert_payloads_equal(r.ops, seen, ref.ovf, what + ("rank", r.rank, "vs scripted"))
            di.assert_payloads_equal(r.ops, ref.ops, ref.ovf, what + ("rank", r.rank, "vs restatement"))


def _uniform(world):
    sizes = (1000003,) + (1000000,) * (world - 1)
    case = di.Case("uniform", sizes, sum(sizes) // 2)
    return case, int(di.sorted_union("uniform", sizes)[case.k - 1])


@pytest.mark.parametrize("world", WORLDS)
def test_onecall_per_level_ctx(gpu, world):
    """Every rank's ctx on the per-level launch sequences (after one grid-barrier
    timeout, KTH_HOOK_FAULT_BARRIER value 2: kth_dist_window level by level,
    kth_dist_scan's ADV_PICK pass) through the one call."""
    import torch
    import kselect
    from onecall_ranks import Ranks
    n = (1 << 23) + 13
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.fill(keys, n, "uniform_half")
    gpu.sync()
    k = n // 2
    want = int(torch.kthvalue(keys.cpu(), k).values)
    rk = Ranks(world)
    try:
        for s in rk.sels:
            s.test_hook(kselect.KTH_HOOK_FAULT_BARRIER, 2)
            assert s.select(keys, k) == want  # times out once, redone per level
            assert not s.coop()
        case, cwant = _uniform(world)
        shards = di.device_tensors(case.kind, case.sizes)
        for kk, w in ((case.k, cwant), (1, int(di.sorted_union(case.kind, case.sizes)[0]))):
            runs = rk.select(shards, list(case.sizes), kk)
            _all_exact(runs, w, ("per-level", kk))
            assert [r.coop for r in runs] == [False] * world
    finally:
        rk.close()


@pytest.mark.parametrize("world", WORLDS)
def test_onecall_leaves_scratch_clean(gpu, world):
    """On the same ctxs, in this order: a one-call select (a fallback case), a
    scripted lockstep select, a plain Selector.select on the window path
    (n > 4 Mi), a one-call select again -- all exact."""
    import torch
    import kselect
    from kselect.dist import DistSelector, HipBackend, lockstep
    from onecall_ranks import Ranks
    fb = next(c for c in di.CASES if len(c.sizes) == world and di.reference(c).n_reduce == 4)
    case, want = _uniform(world)
    n = (1 << 22) + (1 << 20) + 9
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.fill(keys, n, "uniform_full")
    gpu.sync()
    kwant = int(torch.kthvalue(keys.cpu(), n // 3).values)
    rk = Ranks(world)
    try:
        fshards, shards = di.device_tensors(fb.kind, fb.sizes), di.device_tensors(case.kind, case.sizes)
        _all_exact(rk.select(fshards, list(fb.sizes), fb.k), di.reference(fb).answer, "one-call, fallback")
        _all_exact(rk.select(shards, list(case.sizes), case.k), want, "one-call")
        rk.unbind()  # the scripted steps run the ctxs on this thread's stream
        ds = [DistSelector(HipBackend(0, s), world=world) for s in rk.sels]
        outs = lockstep(ds, shards, list(case.sizes), case.k)
        assert [int(o.item()) for o in outs] == [want] * world and [d.error() for d in ds] == [0] * world
        for s in rk.sels:
            assert s.select(keys, n // 3) == kwant
            assert s.stats()["path"] == kselect.KTH_PATH_WINDOW and s.stats()["error"] == 0, s.stats()
        rk.unbind()
        _all_exact(rk.select(shards, list(case.sizes), case.k), want, "one-call after the others")
        _all_exact(rk.select(fshards, list(fb.sizes), fb.k), di.reference(fb).answer, "one-call, fallback again")
    finally:
        rk.close()


@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("world", WORLDS)
def test_onecall_failed_collective(world, j, gpu):
    """Collective number j (0: the all-gather, 1: the scan's all-reduce, 2: the
    all-reduce after level 0) returns a failure code on every rank (a return
    code only): every rank's call returns KTH_ECOMM and leaves the answer
    tensor untouched, and the next select on the same ctxs is exact --
    kth_dist_begin re-zeroes after a sequence cut short."""
    import kselect
    from onecall_ranks import SENTINEL, Ranks
    case, want = _uniform(world)
    rk = Ranks(world)
    try:
        shards = di.device_tensors(case.kind, case.sizes)
        _all_exact(rk.select(shards, list(case.sizes), case.k), want, "before")
        runs = rk.select(shards, list(case.sizes), case.k, fail_at=j)
        assert [r.rc for r in runs] == [kselect.KTH_ECOMM] * world, [r.rc for r in runs]
        assert [r.answer for r in runs] == [SENTINEL] * world
        assert [r.calls for r in runs] == [j + 1] * world and [len(r.ops) for r in runs] == [j] * world
        for k in (case.k, 1, sum(case.sizes)):
            w = int(di.sorted_union(case.kind, case.sizes)[k - 1])
            _all_exact(rk.select(shards, list(case.sizes), k), w, ("after a failed collective", j, k))
    finally:
        rk.close()


def test_onecall_argument_checks(gpu):
    """With a live ctx: s_local not a multiple of 64, or a shard smaller than the
    sample, is KTH_EINVAL before any collective (world 1: no rank is left
    waiting), the answer untouched; the ctx then selects exactly."""
    import kselect
    from onecall_ranks import SENTINEL, Ranks
    case, want = _uniform(1)
    rk = Ranks(1)
    try:
        shards = di.device_tensors(case.kind, case.sizes)
        n = case.sizes[0]
        for kw in ({"s_local": 100}, {"s_local": 64 * 3 + 32}, {"s_local": 128, "sizes": [100]}):
            runs = rk.select(shards, kw.get("sizes", [n]), min(case.k, 50), s_local=kw["s_local"], n_total=n)
            assert runs[0].rc == kselect.KTH_EINVAL and runs[0].calls == 0 and runs[0].answer == SENTINEL, \
                (kw, runs[0].rc, runs[0].calls)
        _all_exact(rk.select(shards, [n], case.k), want, "after the refused calls")
    finally:
        rk.close()
