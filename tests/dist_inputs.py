"""Shards that force each path of the sharded protocol, and what the CPU
restatement (tests/dist_cpu_backend.py) says the protocol does on them.

TEST INFRASTRUCTURE ONLY (tests/test_gpu_dist_fallback.py and
tests/test_gpu_onecall.py).  A shard's sampled positions are
dist_cpu_backend.sample_indices(n_local, s_local) with the s_local of
kselect.dist.DistSelector.s_local, so writing those positions controls the
window every rank derives:

* "miss": uniform int32 keys, every sampled key 1 << 30.  The window collapses
  to lo == hi: no candidates, no overflow; a k outside the spike's ranks takes
  the exact fallback (kth_kernels.hip decide_dist, the FULL branch).
* "overflow": the sampled keys uniform over int32, every other key in
  [-10^6, 10^6).  Around k = n/2 the window is ~+-5 * 10^7 wide and holds
  nearly the whole shard: more than kth_dist_cand_capacity(n_local) = 2^20
  candidates on a rank of 1.6 M keys, fewer on one of 0.7 M -- the overflow
  word is 1 on the large shards only, and its all-reduced sum sends every rank
  to the fallback.
* "uniform": uniform int32 keys, nothing forced (the ordinary window path).

Nothing here assumes which path a case takes: reference() runs the restatement
in lockstep on the host shards and returns the sequence of collectives, their
payloads, the path and every rank's overflow word before the reduce;
check_coverage() then requires that the case list as a whole still holds a
pure miss, an overflow on every rank, an overflow on one rank of three, and
two- and three-all-reduce selections, so a change to the sampler that moves a
case off its path fails there instead of passing quietly.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import dist_cpu_backend as cpu
from kselect.dist import DistSelector, lockstep

SPIKE = 1 << 30

Case = namedtuple("Case", "kind sizes k")
Ref = namedtuple("Ref", "kinds ops n_reduce path ovf_local ovf answer")

MISS_SIZES = [(1500000, 1500000), (1000000,) * 3, (2600000, 200000, 200000)]
OVERFLOW_SIZES = [(1600000, 1600000), (1600000, 700000, 700001)]
# s_local a multiple of kth_sample_chunk() on 16-byte aligned shards: k_gather's vector path
ALIGNED_SIZES = (1 << 20, 1 << 20)


def s_local(n_total, world):
    """DistSelector.s_local."""
    return max(64, (cpu.sample_size(n_total) // world) & ~63)


def _cases():
    out = []
    for kind, shapes in (("miss", MISS_SIZES + [ALIGNED_SIZES]), ("overflow", OVERFLOW_SIZES)):
        for sizes in shapes:
            n = sum(sizes)
            ks = [1, n // 2, n // 2 + 12345, n]
            if kind == "miss":
                ks.append(int(0.76 * n))  # above the spike's ranks
            out += [Case(kind, tuple(sizes), k) for k in ks]
    return out


CASES = _cases()


def case_id(c):
    return f"{c.kind}-{'_'.join(str(s) for s in c.sizes)}-k{c.k}"


@functools.lru_cache(maxsize=None)
def host_shards(kind, sizes):
    """The P host shards (int32 numpy arrays; shared, never written) of a kind and shape."""
    n, P = sum(sizes), len(sizes)
    s = s_local(n, P)
    rng = np.random.default_rng([sum(map(ord, kind)), *sizes])
    shards = []
    for n_local in sizes:
        idx = cpu.sample_indices(n_local, s)
        idx = idx[idx < n_local]
        if kind == "overflow":
            a = rng.integers(-10 ** 6, 10 ** 6, size=n_local, dtype=np.int64).astype(np.int32)
            a[idx] = rng.integers(-2 ** 31, 2 ** 31, size=idx.size, dtype=np.int64).astype(np.int32)
        else:
            a = rng.integers(-2 ** 31, 2 ** 31, size=n_local, dtype=np.int64).astype(np.int32)
            if kind == "miss":
                a[idx] = SPIKE
        shards.append(a)
    return tuple(shards)


@functools.lru_cache(maxsize=None)
def sorted_union(kind, sizes):
    return np.sort(np.concatenate(host_shards(kind, sizes)))


def host_tensors(kind, sizes):
    return [torch.from_numpy(a) for a in host_shards(kind, sizes)]


def device_tensors(kind, sizes):
    return [torch.from_numpy(a.copy()).cuda() for a in host_shards(kind, sizes)]


class _Recording(cpu.CpuBackend):
    """CpuBackend that keeps this rank's overflow word as the scan wrote it."""

    def scan(self, shard, n_local):
        i = super().scan(shard, n_local)
        self.ovf_local = int(self.slots[i][cpu.C_OVF])
        return i


def observer(seen, to_host=False):
    """An ``observe=`` of kselect.dist.lockstep that appends (kind, payload copy)."""
    def see(kind, x):
        seen.append((kind, x.cpu().clone() if to_host else x.clone()))
    return see


@functools.lru_cache(maxsize=None)
def reference(case):
    """What the restatement does on a case: the kinds of its collectives, the
    (kind, payload) list, the number of all-reduces, the path ("window" / "fallback"),
    each rank's overflow word before the reduce, their sum, the answer."""
    P = len(case.sizes)
    backs = [_Recording() for _ in range(P)]
    seen = []
    outs = lockstep([DistSelector(b, world=P) for b in backs], host_tensors(case.kind, case.sizes),
                    list(case.sizes), case.k, observe=observer(seen))
    got = {int(o[0]) for o in outs}
    want = int(sorted_union(case.kind, case.sizes)[case.k - 1])
    assert got == {want}, (case, got, want)  # the restatement itself is exact
    assert len({b.path for b in backs}) == 1, case
    kinds = [k for k, _ in seen]
    assert kinds[0] == "all_gather" and set(kinds[1:]) == {"all_reduce"}, kinds
    ovf_local = tuple(b.ovf_local for b in backs)
    assert int(seen[1][1][cpu.C_OVF]) == sum(ovf_local), case
    return Ref(tuple(kinds), tuple(seen), len(kinds) - 1, backs[0].path, ovf_local, sum(ovf_local),
               want)


def check_coverage(cases=None):
    """The case list as a whole must hold every path (see the module text)."""
    refs = [(c, reference(c)) for c in (CASES if cases is None else cases)]
    four = [(c, r) for c, r in refs if r.n_reduce == 4]
    assert all(r.path == "fallback" for _, r in four) and all(r.n_reduce == 4 for _, r in refs if r.path == "fallback")
    assert any(r.ovf == 0 for _, r in four), "no pure miss (four all-reduces, no overflow)"
    assert any(r.ovf == len(c.sizes) for c, r in four), "no overflow on every rank"
    assert any(r.ovf == 1 and len(c.sizes) == 3 for c, r in four), "no overflow on one rank of three"
    assert any(r.n_reduce == 2 for _, r in refs), "no two-all-reduce case"
    assert any(r.n_reduce == 3 for _, r in refs), "no three-all-reduce case"
    assert all(2 <= r.n_reduce <= 4 for _, r in refs)


def assert_payloads_equal(got, want, ovf, what):
    """got, want: [(kind, host tensor)] of two runs of one case; ovf: the
    case's reduced overflow word.  Bit-equal, except the digit histogram of the
    scan's slot when ovf is nonzero: which candidates fit a full buffer is not
    part of the contract (decide_dist takes the FULL branch on that word and
    never reads the histogram), so only the five count words of that slot are
    compared."""
    assert [k for k, _ in got] == [k for k, _ in want], (what, [k for k, _ in got], [k for k, _ in want])
    for i, ((kind, x), (_, y)) in enumerate(zip(got, want)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, kind, x.shape, y.shape)
        if i == 1 and ovf:
            assert x[:5].tolist() == y[:5].tolist(), (what, "scan counts under overflow", x[:8].tolist(),
                                                      y[:8].tolist())
            continue
        if not torch.equal(x, y):
            bad = torch.nonzero(x != y).flatten()
            raise AssertionError((what, i, kind, "first differing words", bad[:8].tolist(),
                                  x[bad[:8]].tolist(), y[bad[:8]].tolist()))
