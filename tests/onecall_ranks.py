"""kth_dist_select_rccl at world > 1 on one GPU: P ranks as P threads of the
test process, the two collectives as stand-ins with RCCL's signatures.

TEST INFRASTRUCTURE ONLY (tests/test_gpu_onecall.py).  The library call takes
its collectives as function pointers (include/kth.h), so the sequence that
kselect.dist.DistSelector.select runs over RCCL -- the all-gather of s_local
words into s_local * world, the window over that, the in-place all-reduce of
each slot, the early result, the level loop -- runs here with
ctypes.CFUNCTYPE callbacks that have the ncclAllGather / ncclAllReduce
signatures and stage through host memory, as kselect.rccl.HostComm does.
ctypes releases the GIL during the call and takes it back in a callback.

Each rank thread sets device 0, makes its own torch stream current, binds its
own Selector (one ctx per thread) to it and allocates its own slots, sample,
gathered and answer tensors.  A stand-in waits for the stream it was handed,
resolves its buffer pointers to the rank's own tensors BY ADDRESS (an address
that is not one of them is a recorded failure, never dereferenced), copies to
the host, meets the other ranks at a barrier, forms the sum or the
concatenation, copies it back on that stream and returns ncclSuccess.

What the stand-ins check on every collective is part of the test: the buffer
addresses, the counts, the type and op codes of kselect/rccl.py, the stream
(the ctx's) and the communicator (the token the harness passed).  A failed
check is recorded per rank and reported after the join -- an exception inside
a callback would be swallowed by ctypes.

Ending on trouble: every barrier wait has a timeout (a cap, not a measurement:
a case takes well under a second); on a timeout or any recorded failure the
barrier is aborted, every stand-in then returns a nonzero ncclResult_t, so
every rank's call returns KTH_ECOMM instead of waiting; the threads are joined
with a timeout; after a failure the harness raises and refuses to start
anything further.  No retries.

Limit: the stand-ins synchronise the host at every collective, so an ordering
bug between a real asynchronous collective and the next kernel on the stream
is out of reach here; RCCL's own transport at N > 1 needs N GPUs.
"""
import ctypes
import threading

import torch

from kselect import KTH_STATS_WORDS, LIB, Selector
from kselect.dist import HipBackend
from kselect.rccl import _NCCL_SUM, _NCCL_UINT32, _NCCL_UINT64

BARRIER_TIMEOUT = 60.0
JOIN_TIMEOUT = 180.0
SENTINEL = -123456789
NCCL_FAIL = 1  # any nonzero ncclResult_t (rccl.h: ncclUnhandledCudaError)

_vp, _sz, _ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
ALL_REDUCE_T = ctypes.CFUNCTYPE(_ci, _vp, _vp, _sz, _ci, _ci, _vp, _vp)  # ncclAllReduce
ALL_GATHER_T = ctypes.CFUNCTYPE(_ci, _vp, _vp, _sz, _ci, _vp, _vp)  # ncclAllGather


class RankRun:
    """One rank's record of one call."""

    def __init__(self, rank):
        self.rank = rank
        self.rc = None        # kth_dist_select_rccl's return value
        self.answer = None    # the answer tensor after the call (SENTINEL: untouched)
        self.error = None     # kth_ctx_last_stats().error (None when the call failed)
        self.coop = None      # kth_ctx_coop after the call
        self.ops = []         # (kind, payload after the collective, on the host)
        self.out_seen = []    # the answer tensor as each collective found it
        self.calls = 0        # collectives entered (injected failures included)
        self.failures = []


class Ranks:
    """P rank threads' lasting state: a stream, a Selector (ctx) and a
    communicator token each.  select() runs one kth_dist_select_rccl per rank."""

    def __init__(self, world):
        self.world = int(world)
        assert 1 <= self.world <= 3  # (at most 3 rank threads beside the main one)
        self.streams = [torch.cuda.Stream(device=0) for _ in range(self.world)]
        self.sels = [Selector(0) for _ in range(self.world)]
        self.hbs = [None] * self.world  # bound to the rank's stream in its thread
        self.tokens = [ctypes.create_string_buffer(64) for _ in range(self.world)]  # stand-in ncclComm_t
        self.broken = False

    def unbind(self):
        """The ctxs are about to be used on another stream (or were): wait for
        everything, and bind them to the ranks' streams again at the next select."""
        torch.cuda.synchronize()
        self.hbs = [None] * self.world

    def close(self):
        torch.cuda.synchronize()
        for s in self.sels:
            s.close()

    def select(self, shards, sizes, k, early=1, fail_at=None, s_local=None, n_total=None):
        """One call per rank over shards[r][:sizes[r]].  fail_at=j: the stand-ins
        of EVERY rank return a nonzero ncclResult_t at collective number j
        instead of performing it (a return code only).  Returns the RankRuns;
        raises on any recorded failure, after which this object runs nothing."""
        assert not self.broken, "an earlier call failed: nothing further is started on the GPU"
        P = self.world
        assert len(shards) == len(sizes) == P
        n_total = int(sum(sizes)) if n_total is None else int(n_total)
        if s_local is None:
            s_local = max(64, (int(LIB.kth_dist_sample_size(n_total)) // P) & ~63)
        torch.cuda.synchronize()  # the shards and the ctxs' earlier work, whatever stream made them
        barrier = threading.Barrier(P)
        parts = [None] * P
        runs = [RankRun(r) for r in range(P)]
        threads = [threading.Thread(target=self._rank, daemon=True,
                                    args=(runs[r], barrier, parts, shards[r], int(sizes[r]), n_total, int(k),
                                          int(s_local), int(early), fail_at)) for r in range(P)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        stuck = [r for r, t in enumerate(threads) if t.is_alive()]
        failures = [(run.rank, f) for run in runs for f in run.failures]
        if stuck or failures:
            self.broken = True
            barrier.abort()
            raise AssertionError(f"one-call ranks: stuck {stuck}, failures {failures[:12]}")
        return runs

    # ------------------------------------------------------------ a rank thread
    def _rank(self, run, barrier, parts, shard, n_local, n_total, k, s_local, early, fail_at):
        r, P = run.rank, self.world
        try:
            torch.cuda.set_device(0)
            stream = self.streams[r]
            with torch.cuda.stream(stream):
                if self.hbs[r] is None:
                    self.hbs[r] = HipBackend(0, self.sels[r])  # (binds the ctx to this thread's current stream)
                hb = self.hbs[r]
                slots = hb.alloc_slots()
                sample = hb.alloc_sample(s_local)
                gathered = hb.alloc_sample(s_local * P)
                out = torch.full((1,), SENTINEL, dtype=torch.int32, device=hb.device)
                stream.synchronize()
                token = ctypes.addressof(self.tokens[r])
                env = _StandIns(run, barrier, parts, P, stream.cuda_stream, token, slots, sample, gathered, out,
                                s_local, fail_at)
                ar, ag = ALL_REDUCE_T(env.all_reduce), ALL_GATHER_T(env.all_gather)
                run.rc = int(LIB.kth_dist_select_rccl(
                    hb.ctx, ctypes.cast(ar, _vp), ctypes.cast(ag, _vp), _vp(token), P, _vp(shard.data_ptr()), n_local,
                    n_total, k, _vp(slots.data_ptr()), _vp(sample.data_ptr()), _vp(gathered.data_ptr()), s_local,
                    _vp(out.data_ptr()), early))
                stream.synchronize()
                run.answer = int(out.item())
                if run.rc == 0:
                    run.error = int(self.sels[r].stats()["error"])
                run.coop = self.sels[r].coop()
        except BaseException as e:  # noqa: BLE001 -- reported after the join
            run.failures.append(f"rank thread: {e!r}")
            barrier.abort()


class _StandIns:
    """The two collectives of one rank for one call."""

    def __init__(self, run, barrier, parts, world, stream_ptr, token, slots, sample, gathered, out, s_local, fail_at):
        self.run, self.barrier, self.parts, self.world = run, barrier, parts, world
        self.stream_ptr, self.token = stream_ptr, token
        self.slots, self.sample, self.gathered, self.out = slots, sample, gathered, out
        self.s_local, self.fail_at = s_local, fail_at
        self.reduces = 0

    def _expect(self, what, got, want):
        if got != want:
            self.run.failures.append(f"collective {self.run.calls - 1}: {what} is {got!r}, expected {want!r}")
            return False
        return True

    def _collective(self, kind, checks, src, dst, stream, combine):
        """Common body; returns the ncclResult_t."""
        run = self.run
        try:
            j = run.calls
            run.calls += 1
            if self.fail_at is not None and j == self.fail_at:
                return NCCL_FAIL  # injected on every rank: nobody waits
            if self.barrier.broken:
                return NCCL_FAIL
            ok = all([self._expect(w, g, e) for w, g, e in checks])  # (every check runs)
            if not ok:
                self.barrier.abort()
                return NCCL_FAIL
            ext = torch.cuda.ExternalStream(stream, device=0)
            ext.synchronize()
            with torch.cuda.stream(ext):
                run.out_seen.append(int(self.out.cpu()[0]))
                self.parts[run.rank] = src.cpu()
                self.barrier.wait(BARRIER_TIMEOUT)
                res = combine(list(self.parts))
                self.barrier.wait(BARRIER_TIMEOUT)  # every rank has read the parts before the next collective's
                dst.copy_(res)
                ext.synchronize()
            run.ops.append((kind, res))
            return 0
        except threading.BrokenBarrierError:
            run.failures.append(f"collective {run.calls - 1}: barrier broken or timed out")
            return NCCL_FAIL
        except BaseException as e:  # noqa: BLE001 -- ctypes would swallow it
            run.failures.append(f"collective {run.calls - 1}: {e!r}")
            self.barrier.abort()
            return NCCL_FAIL

    def all_reduce(self, send, recv, count, dtype, op, comm, stream):
        slot = self.reduces % 3  # the scan fills slot 0, level l slot (l + 1) % 3
        self.reduces += 1
        want = self.slots.data_ptr() + slot * KTH_STATS_WORDS * 8
        checks = [("all-reduce sendbuff", send, want), ("all-reduce recvbuff", recv, want),
                  ("all-reduce count", count, KTH_STATS_WORDS), ("all-reduce type", dtype, _NCCL_UINT64),
                  ("all-reduce op", op, _NCCL_SUM), ("all-reduce comm", comm, self.token),
                  ("all-reduce stream", stream, self.stream_ptr)]
        t = self.slots[slot]
        return self._collective("all_reduce", checks, t, t, stream, lambda ps: torch.stack(ps).sum(0))

    def all_gather(self, send, recv, count, dtype, comm, stream):
        checks = [("all-gather sendbuff", send, self.sample.data_ptr()),
                  ("all-gather recvbuff", recv, self.gathered.data_ptr()), ("all-gather count", count, self.s_local),
                  ("all-gather type", dtype, _NCCL_UINT32), ("all-gather comm", comm, self.token),
                  ("all-gather stream", stream, self.stream_ptr), ("all-gather position", self.run.calls, 0)]  # the first collective
        return self._collective("all_gather", checks, self.sample, self.gathered, stream, torch.cat)
