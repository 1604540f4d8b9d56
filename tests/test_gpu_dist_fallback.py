"""The exact fallback of the sharded protocol, forced on the device.

include/kth.h promises two all-reduces per selection when the window is at
most 2^24 values wide or the counts decide, three for wider windows, four for
the exact fallback after a window miss or a candidate overflow.  The fallback
is its own device code -- decide_dist taking the FULL branch on the ALL-REDUCED
overflow word, k_dlevel over the whole shard with dense_per_wg, an 8-bit digit
followed by two 12-bit ones, k_dresult after three levels, the level loops of
kth_sharded.cpp and DistSelector.steps -- and the synthetic families of
tests/test_gpu_config3.py never reach it.

tests/dist_inputs.py builds shards that miss the window, overflow the
candidate buffer on every rank, or on ONE rank of three (the others must
follow it), plus two- and three-all-reduce selections on the same data.  For
every case the P device backends (kth_dist_* through kselect.dist.HipBackend)
run kselect.dist.lockstep against the P CPU restatements
(tests/dist_cpu_backend.py): the same collectives, the gathered sample and
every all-reduced slot bit for bit (under overflow the scan slot's count words
only, see dist_inputs.assert_payloads_equal), the answer a sort of the union,
no device error; the same shards through the local transport's C++ level loop
(kselect.ShardedSelector([0] * P)); and after a fallback the same ctxs select
from ordinary keys, slot for slot again (the fallback leaves the scratch clean).
"""
import pytest

import dist_inputs as di

pytestmark = pytest.mark.gpu


class _Rig:
    """Per world size: P ctxs and a local-transport handle, kept across the
    cases; device copies of the shards per (kind, shape)."""

    def __init__(self):
        self._sels, self._sharded, self._shards = {}, {}, {}

    def sels(self, P):
        from kselect import Selector
        if P not in self._sels:
            self._sels[P] = [Selector(0) for _ in range(P)]
        return self._sels[P]

    def sharded(self, P):
        import kselect
        if P not in self._sharded:
            self._sharded[P] = kselect.ShardedSelector([0] * P)
        return self._sharded[P]

    def shards(self, kind, sizes):
        import torch
        if (kind, sizes) not in self._shards:
            self._shards[(kind, sizes)] = di.device_tensors(kind, sizes)
            torch.cuda.synchronize()
        return self._shards[(kind, sizes)]

    def close(self):
        for sels in self._sels.values():
            for s in sels:
                s.close()
        for s in self._sharded.values():
            s.close()


@pytest.fixture(scope="module")
def rig(gpu):
    r = _Rig()
    yield r
    r.close()


def test_cases_cover_every_path():
    """The restatement on the case list: a pure miss, an overflow on every
    rank, an overflow on one rank of three (each four all-reduces), and two-
    and three-all-reduce selections.  (Host arithmetic only.)"""
    di.check_coverage()


def _device_lockstep(rig, case):
    """lockstep over P HipBackends on the case's shards: ([(kind, payload)], answers, errors)."""
    import torch
    from kselect.dist import DistSelector, HipBackend, lockstep
    P = len(case.sizes)
    ds = [DistSelector(HipBackend(0, s), world=P) for s in rig.sels(P)]
    seen = []
    outs = lockstep(ds, rig.shards(case.kind, case.sizes), list(case.sizes), case.k,
                    observe=di.observer(seen, to_host=True))
    torch.cuda.synchronize()
    return seen, [int(o.item()) for o in outs], [d.error() for d in ds]


@pytest.mark.parametrize("case", di.CASES, ids=di.case_id)
def test_device_levels_match_restatement(rig, case):
    ref = di.reference(case)
    P = len(case.sizes)
    want = int(di.sorted_union(case.kind, case.sizes)[case.k - 1])
    assert ref.kinds == ("all_gather",) + ("all_reduce",) * ref.n_reduce
    seen, answers, errors = _device_lockstep(rig, case)
    print(di.case_id(case), "all-reduces", len(seen) - 1, "restatement", ref.n_reduce, ref.path, "overflow words",
          ref.ovf_local, "device scan counts", seen[1][1][:5].tolist(), "restatement", ref.ops[1][1][:5].tolist())
    di.assert_payloads_equal(seen, ref.ops, ref.ovf, di.case_id(case))
    assert answers == [want] * P and ref.answer == want, (answers, ref.answer, want)
    assert errors == [0] * P, errors
    # the local transport: kth_sharded.cpp's level loop over the same kth_dist_* steps
    assert rig.sharded(P).select(rig.shards(case.kind, case.sizes), case.k, list(case.sizes)) == want
    if ref.n_reduce == 4:
        # the same ctxs on ordinary keys right after the fallback
        plain = di.Case("uniform", case.sizes, sum(case.sizes) // 2)
        pref = di.reference(plain)
        assert pref.path == "window" and pref.n_reduce < 4 and pref.ovf == 0, pref[2:]
        seen, answers, errors = _device_lockstep(rig, plain)
        di.assert_payloads_equal(seen, pref.ops, 0, "after " + di.case_id(case))
        assert answers == [pref.answer] * P and errors == [0] * P, (answers, pref.answer, errors)
        assert rig.sharded(P).select(rig.shards(plain.kind, plain.sizes), plain.k, list(plain.sizes)) == pref.answer
