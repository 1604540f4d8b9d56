"""Inputs and the plain reference of the rank-edge tests (test_rank_edges_inputs.py
on the CPU, test_gpu_rank_edges.py on the GPU).  Numpy only.

Every one-array select ends in a case split on exact counts (decide() in
csrc/kth_kernels.hip).  With L = #keys < lo, E1 = #keys == lo, M = #keys inside
(lo, hi), E2 = #keys == hi (0 when lo == hi):

    k in (L, L+E1]              "lo"    answer = lo
    k in (L+E1, L+E1+M]         "cand"  rank k-L-E1 among the candidates
    k in (L+E1+M, L+E1+M+E2]    "hi"    answer = hi
    otherwise                   "miss"  exact fallback over the input

The inputs here put a probed rank on the first or the last rank of a branch:

* plateau inputs (honest sample): n distinct pseudo-random keys in random
  positions in which one value replaces a run of sorted ranks; the run is long
  enough that the window's sample rank lies inside it by MARGIN_SIGMAS sample
  standard deviations, computed from the published formula alone
  (kth_window_z, kth_dist_sample_size, the window ranks p*s -+ (z*sigma + 2));
* planted inputs: the sampled chunks (kth_sample_chunk's layout) hold a sorted,
  banded sample, so lo and hi are known whatever the rest holds, and the rest
  makes L, E1, M and E2 exact: the window can then miss by exactly one rank;
* the staircase: tie groups on both sides of every power of two of the order
  key, so every digit split of the radix and LDS paths has a bin boundary
  between two tie groups;
* 16-bit inputs, where every rank is a tie-group edge or interior.

The reference is one np.sort of the order keys per input: the answer for rank k
is sorted[k - 1], the top-k is every key better than it and the first
k - #better equal keys by index (O(n), no argsort).
"""
import functools
import math

import numpy as np

from kselect import LIB

import test_gpu_f32 as f32t
import test_gpu_k16 as k16t

N_SMALL, N_MID = (1 << 22) + 5, (1 << 23) + 3  # the smallest window-path size; one more pass for int32
MARGIN_SIGMAS = 4.0
BAND_MARGIN = 200  # sample ranks between a planted band's edge and every window rank that falls in it
BAND_EXTRA = 300   # ... and how much further the planted bands reach (PlantedCase)
FIN_LDS_KEYS = 32768  # keys the finishing workgroup holds
SIGN = np.uint32(0x80000000)
NAN_KEY = 0xFFFFFFFF
TK_TILE, TK_STAGE_MAX_FRAC, RADIX_MAX_N, SMALL_N = 1024, 16, 1 << 22, 16384  # csrc/kth_topk.hpp, kth_api.hip


# ------------------------------------------------------------ published formulas
def window_z():
    return float(LIB.kth_window_z())


def sample_size(n):
    return int(LIB.kth_dist_sample_size(int(n)))


def sample_chunk():
    return int(LIB.kth_sample_chunk())


def sigma(n, k, s):
    p = k / n
    return math.sqrt(max(1.0, s * p * (1.0 - p)))


def window_ranks(n, k, s):
    """include/kth.h kth_window_z: p*s -+ (z*sqrt(s*p*(1-p)) + 2), p = k/n, as 1-based
    sample ranks; 0 = no lower bound, s + 1 = no upper bound."""
    r = k / n * s
    half = window_z() * sigma(n, k, s) + 2.0
    lo, hi = math.floor(r - half), math.ceil(r + half)
    return (0 if lo < 1 else int(lo)), (s + 1 if hi > s else int(max(1, hi)))


def sample_indices(n):
    """include/kth.h kth_sample_chunk: ceil(s / C) chunks of C consecutive keys,
    chunk c at key c * (n / ceil(s / C))."""
    s, c = sample_size(n), sample_chunk()
    nch = -(-s // c)
    idx = (np.arange(nch, dtype=np.int64)[:, None] * (n // nch) + np.arange(c, dtype=np.int64)[None, :]).ravel()
    return idx[:s]


def topk_variant(n, k, aligned, f32):
    """The streaming-pass variant kth_topk_i32 / kth_topk_f32 take (include/kth.h "top-k of
    one array", thresholds of csrc/kth_api.hip topk_impl): "staged" for n / 65536 < k <= n / 16
    on 16-byte aligned int32 keys, "row-word" for the other aligned k above n / 65536,
    "tile-flag" for k <= n / 65536, or k <= n / 1024 on unaligned keys, "plain" otherwise;
    below the window path always tile-flag or plain."""
    window, few = n > RADIX_MAX_N, k * TK_TILE * 64 <= n
    if not f32 and aligned and window and not few and k * TK_STAGE_MAX_FRAC <= n:
        return "staged"
    if aligned and window and not few:
        return "row-word"
    return "tile-flag" if k * TK_TILE <= n else "plain"


# ------------------------------------------------------------------ the reference
def i32_key(words):
    return np.asarray(words, dtype=np.int32).view(np.uint32) ^ SIGN


def topk_ref(key, skey, k, largest):
    """Indices (ascending) of the k smallest (largest) keys, ties at the k-th to the first by index."""
    n = key.size
    if largest:
        v = skey[n - k]
        better = key > v
        nb = n - int(np.searchsorted(skey, v, side="right"))
    else:
        v = skey[k - 1]
        better = key < v
        nb = int(np.searchsorted(skey, v, side="left"))
    eq = np.flatnonzero(key == v)[:k - nb]
    return np.sort(np.concatenate([np.flatnonzero(better), eq]))


class Ref:
    """One input: its words (int32, or float32 bit patterns as uint32), their order
    keys (uint32) and ONE sort of them."""

    def __init__(self, words, f32=False):
        self.f32 = f32
        self.words = np.ascontiguousarray(words, dtype=np.uint32 if f32 else np.int32)
        self.words.setflags(write=False)
        self.n = self.words.size
        self.key = f32t._f32_order_key(self.words) if f32 else i32_key(self.words)
        self.sorted = np.sort(self.key)

    def key_bits(self, key):
        """The uint32 bit pattern of the element with this order key (a NaN canonical)."""
        return int(f32t._bits_of_key(np.uint32(key))) if self.f32 else int(np.uint32(key) ^ SIGN)

    def want(self, k):
        return self.key_bits(self.sorted[k - 1])

    def wants(self, ks):
        return [self.want(int(k)) for k in ks]

    def host(self):
        return np.array(self.words.view(np.float32) if self.f32 else self.words)

    def out_bits(self, words):
        """What a top-k writes for these input words: the bits, a NaN canonical."""
        w = np.asarray(words).view(np.uint32)
        return f32t._canon(w) if self.f32 else w

    def counts(self, lo, hi):
        """(L, E1, M, E2raw) over the input for a window [lo, hi] of order keys."""
        s = self.sorted
        l0, l1 = (int(np.searchsorted(s, np.uint32(lo), side=x)) for x in ("left", "right"))
        h0, h1 = (int(np.searchsorted(s, np.uint32(hi), side=x)) for x in ("left", "right"))
        return l0, l1 - l0, max(0, h0 - l1), h1 - h0

    def branch(self, k, lo, hi):
        """(branch, position in it, its length) decide() takes for rank k and this window."""
        L, E1, M, E2 = self.counts(lo, hi)
        if lo == hi:
            E2 = 0
        if L < k <= L + E1:
            return "lo", k - L, E1
        if L + E1 < k <= L + E1 + M:
            return "cand", k - L - E1, M
        if L + E1 + M < k <= L + E1 + M + E2:
            return "hi", k - L - E1 - M, E2
        return ("miss_below", L + 1 - k, 0) if k <= L else ("miss_above", k - (L + E1 + M + E2), 0)

    def topk(self, k, largest):
        return topk_ref(self.key, self.sorted, k, largest)

    def sample_sorted(self):
        """The sorted sample an honest sample phase reads from this input."""
        if not hasattr(self, "_sample"):
            self._sample = np.sort(self.key[sample_indices(self.n)])
        return self._sample

    def early_window(self, k, abs_div=1024):
        """(lo, hi) predicted for a default ctx: csrc/kth_kernels.hip early_window restated.
        After each of the first two sample digits (11, 11 of 11 + 11 + 10 bits) the window
        stops at the picked bins' edges when they hold at most kth_window_slack64 / 64 times
        the exact window's sample keys, or at most s / abs_div of them (the plain and the
        multi-rank select; abs_div = 0 for the top-k).  A prediction for the tables and the
        comments only: the GPU tests read the window the library reports."""
        s = sample_size(self.n)
        srt = self.sample_sorted()
        slack64 = int(LIB.kth_window_slack64())
        r_lo, r_hi = window_ranks(self.n, k, s)
        a0, a1 = 1 <= r_lo <= s, 1 <= r_hi <= s
        if slack64 and (a0 or a1):
            want = (r_hi if a1 else s) - (r_lo if a0 else 1) + 1
            for done in (11, 22):
                sh = np.uint32(32 - done)
                pre = srt >> sh
                p0 = int(srt[r_lo - 1] >> sh) if a0 else 0
                p1 = int(srt[r_hi - 1] >> sh) if a1 else 0
                below0 = int(np.searchsorted(pre, np.uint32(p0), side="left")) if a0 else 0
                upto1 = int(np.searchsorted(pre, np.uint32(p1), side="right")) if a1 else s
                span = upto1 - below0
                if span >= 0 and (span * 64 <= want * slack64 or (abs_div and span <= s // abs_div)):
                    w = 32 - done
                    return (p0 << w if a0 else 0), (((p1 << w) | ((1 << w) - 1)) if a1 else NAN_KEY)
        return self.exact_window(k)

    def exact_window(self, k):
        """(lo, hi) of the exact window (no early window: KTH_HEAD_SLACK=0, per-level path)."""
        s = sample_size(self.n)
        srt = self.sample_sorted()
        r_lo, r_hi = window_ranks(self.n, k, s)
        return (int(srt[r_lo - 1]) if 1 <= r_lo <= s else 0), (int(srt[r_hi - 1]) if 1 <= r_hi <= s else NAN_KEY)


class Probe:
    """One probed rank and the boundary it is named for: `branch` in lo / cand / hi,
    `pos` in first / last / mid / only, `shape` one of None, "lo==hi", "hi==lo+1",
    "M==0" (no key between lo and hi), "W==0" (hi == lo + 2: the candidates are one value)."""

    def __init__(self, k, name, branch, pos, shape=None):
        self.k, self.name, self.branch, self.pos, self.shape = int(k), name, branch, pos, shape

    def __repr__(self):
        return f"{self.name}(k={self.k}: {self.pos} of {self.branch}{', ' + self.shape if self.shape else ''})"

    def reached(self, ref, lo, hi):
        """True when, for the window [lo, hi], rank k is the boundary this probe is named for
        (read off numpy counts over the input, not off any answer)."""
        br, at, size = ref.branch(self.k, lo, hi)
        if br != self.branch:
            return False
        if self.pos == "first" and at != 1:
            return False
        if self.pos == "last" and at != size:
            return False
        if self.pos == "only" and not (at == 1 and size == 1):
            return False
        if self.pos == "mid" and not 1 < at < size:
            return False
        M = ref.counts(lo, hi)[2]
        return {None: True, "lo==hi": lo == hi, "hi==lo+1": hi == lo + 1, "M==0": lo < hi and M == 0,
                "W==0": hi == lo + 2}[self.shape]


# ------------------------------------------------------------- plateau inputs
def _distinct_sorted_keys(rng, n, lo, hi):
    """n distinct order keys in [lo, hi], sorted."""
    span = hi - lo + 1 - n
    assert span > 0
    return (np.sort(rng.integers(0, span + 1, n, dtype=np.int64)) + np.arange(n, dtype=np.int64) + lo).astype(np.uint32)


def plateau_len(n, frac, both=True):
    """The plateau length a case needs, from the published formula only: for a rank k
    at quantile `frac`, a window rank k*s/n -+ (z*sigma + 2) that starts at one
    edge of the plateau must still be MARGIN_SIGMAS sigmas short of the other edge
    (both: the middle rank's two window ranks lie inside, so twice that), plus 10 %."""
    s = sample_size(n)
    k = min(max(int(frac * n), 1), n)
    need = window_z() * sigma(n, k, s) + 2.0 + MARGIN_SIGMAS * sigma(n, k, s)
    c = int(math.ceil((2 if both else 1) * need * 1.1 * n / s))
    return -(-c // 64) * 64


class PlateauCase:
    """groups: [(key delta from P, count)], laid on consecutive sorted ranks from a + 1.
    anchor: a quantile of n (P is taken from the distinct keys there), "floor" (P the
    smallest key, a = 0), "ceil" (P the largest key, the run ends at n), or an order key
    (float cases: the run is laid where that key sorts)."""

    def __init__(self, name, n, f32, anchor, groups, seed, key_range=(0, 0xFFFFFFFF), top=None):
        rng = np.random.default_rng([seed, n])
        sv = _distinct_sorted_keys(rng, n, key_range[0] + 1, key_range[1] - 1)  # strictly inside the range
        total = sum(c for _, c in groups)
        if anchor == "floor":
            a, P = 0, key_range[0]
        elif anchor == "ceil":
            a, P = n - total, (key_range[1] if top is None else top) - groups[-1][0]
        elif isinstance(anchor, float):
            a = int(anchor * n) - (total // 2 if anchor == 0.5 else 0)
            P = int(sv[a + groups[0][1] - 1])  # the first run's last key: every key below it stays below
        else:
            P = int(anchor)
            a = int(np.searchsorted(sv, np.uint32(P))) - groups[0][1]
            a = min(max(a, 0), n - total)
        at = a
        self.groups = []  # (order key, first rank, last rank), 1-based
        for delta, cnt in groups:
            sv[at:at + cnt] = np.uint32(P + delta)
            self.groups.append((P + delta, at + 1, at + cnt))
            at += cnt
        # still sorted, and the neighbours of the run are strictly outside it
        assert np.all(sv[1:] >= sv[:-1])
        assert a == 0 or sv[a - 1] < sv[a]
        assert at == n or sv[at] > sv[at - 1]
        self.name, self.n, self.f32, self.a, self.total = name, n, f32, a, total
        words = sv[rng.permutation(n)]
        self.ref = Ref(f32t._bits_of_key(words) if f32 else (words ^ SIGN).view(np.int32), f32)
        assert np.array_equal(self.ref.sorted, sv)
        self.probes = []
        self.margins = []  # (probe, "lo" / "hi", group index): that window rank is meant to fall on that group

    def probe(self, k, name, branch, pos, shape=None, lo_on=None, hi_on=None):
        p = Probe(k, name, branch, pos, shape)
        self.probes.append(p)
        if lo_on is not None:
            self.margins.append((p, "lo", lo_on))
        if hi_on is not None:
            self.margins.append((p, "hi", hi_on))
        return p

    def margin_sigmas(self, p, which, g):
        """How far inside group g's share of the sample the window rank lies, in sample
        sigmas, on its tighter side.  An end of the array is no edge: a window rank
        past it is 'no bound', which is the group's own key (floor / ceiling)."""
        s = sample_size(self.n)
        _, first, last = self.groups[g]
        r = window_ranks(self.n, p.k, s)[0 if which == "lo" else 1]
        sg = sigma(self.n, p.k, s)
        below = math.inf if first == 1 else (r - (first - 1) * s / self.n) / sg
        above = math.inf if last == self.n else (last * s / self.n - r) / sg
        return min(below, above)

    def ks(self):
        return [p.k for p in self.probes]


def _five(c, g=0, shape_mid="lo==hi"):
    """The five probes of one plateau (group g of case c): last candidate below it,
    its first, middle and last rank, the first candidate above it."""
    _, first, last = c.groups[g]
    a, n = first - 1, c.n
    if a >= 1:
        c.probe(a, "below", "cand", "last", hi_on=g)
    c.probe(a + 1, "first", "hi" if a >= 1 else "lo", "first", hi_on=g if a >= 1 else None)
    c.probe((first + last) // 2, "middle", "lo", "mid", shape_mid, lo_on=g, hi_on=g)
    c.probe(last, "last", "lo" if last < n else "hi", "last", lo_on=g if last < n else None)
    if last < n:
        c.probe(last + 1, "above", "cand", "first", lo_on=g)


F32_FINITE = (0x007FFFFF, 0xFF800000)  # order keys of -inf and +inf: the distinct keys lie strictly between
KEY_NEG0, KEY_POS0, KEY_PINF, KEY_SUB1 = 0x7FFFFFFF, 0x80000000, 0xFF800000, 0x80000001


@functools.lru_cache(maxsize=None)
def plateau_case(name, n=N_SMALL):
    f32 = name.startswith("f32_")
    c_mid, c_edge = plateau_len(n, 0.5), plateau_len(n, 0.5, both=False)
    if name in ("mid", "low", "high"):
        frac = {"mid": 0.5, "low": 0.01, "high": 0.99}[name]
        # (low / high: the run spans about a per cent of n; its length is taken at the
        # quantile of its inner end, 0.02 / 0.98, where the sample sigma is largest)
        cl = plateau_len(n, {"mid": 0.5, "low": 0.02, "high": 0.98}[name])
        c = PlateauCase(name, n, False, 0.5 if name == "mid" else frac - (cl / n if name == "high" else 0.0), [(0, cl)],
                        seed=1)
        _five(c)
    elif name == "floor":
        # c <= n / 1024: k = c and c + 1 take the tile-flag top-k on unaligned keys
        cl = n // 1024 - 96
        c = PlateauCase(name, n, False, "floor", [(0, cl)], seed=2)
        c.probe(1, "k=1", "lo", "first", "lo==hi", hi_on=0)
        c.probe(cl, "last", "lo", "last", lo_on=0)
        c.probe(cl + 1, "above", "cand", "first", lo_on=0)
        c.probe(n, "k=n", "cand", "last")
    elif name == "ceiling":
        cl = n // 1024 - 96
        c = PlateauCase(name, n, False, "ceil", [(0, cl)], seed=3)
        c.probe(1, "k=1", "cand", "first")
        c.probe(n - cl, "below", "cand", "last", hi_on=0)
        c.probe(n - cl + 1, "first", "hi", "first", hi_on=0)
        c.probe(n, "k=n", "lo", "last", "lo==hi", lo_on=0)
    elif name == "adjacent":
        c = PlateauCase(name, n, False, 0.5, [(0, c_edge), (1, c_edge)], seed=4)
        a = c.groups[0][2]
        c.probe(a, "last of P", "lo", "last", "hi==lo+1", lo_on=0, hi_on=1)
        c.probe(a + 1, "first of P+1", "hi", "first", "hi==lo+1", lo_on=0, hi_on=1)
    elif name in ("between_1", "between_40000"):
        m = int(name.split("_")[1])
        c = PlateauCase(name, n, False, 0.5, [(0, c_edge), (1, m), (2, c_edge)], seed=5)
        a = c.groups[0][2]
        c.probe(a, "last of P", "lo", "last", "W==0", lo_on=0, hi_on=2)
        if m == 1:
            c.probe(a + 1, "the one P+1", "cand", "only", "W==0", lo_on=0, hi_on=2)
        else:
            c.probe(a + 1, "first of P+1", "cand", "first", "W==0", lo_on=0, hi_on=2)
            c.probe(a + m // 2, "middle of P+1", "cand", "mid", "W==0", lo_on=0, hi_on=2)
            c.probe(a + m, "last of P+1", "cand", "last", "W==0", lo_on=0, hi_on=2)
        c.probe(a + m + 1, "first of P+2", "hi", "first", "W==0", lo_on=0, hi_on=2)
    elif name == "f32_zero_mid":
        c = PlateauCase(name, n, True, KEY_NEG0, [(0, c_mid)], seed=6, key_range=F32_FINITE)
        _five(c)
    elif name == "f32_zero_adjacent":
        c = PlateauCase(name, n, True, KEY_NEG0, [(0, c_edge), (1, c_edge)], seed=7, key_range=F32_FINITE)
        a = c.groups[0][2]
        c.probe(a, "last -0.0", "lo", "last", "hi==lo+1", lo_on=0, hi_on=1)
        c.probe(a + 1, "first +0.0", "hi", "first", "hi==lo+1", lo_on=0, hi_on=1)
    elif name == "f32_subnormal_mid":
        c = PlateauCase(name, n, True, KEY_SUB1, [(0, c_mid)], seed=8, key_range=F32_FINITE)
        _five(c)
    elif name == "f32_subnormal_adjacent":
        c = PlateauCase(name, n, True, KEY_SUB1, [(0, c_edge), (1, c_edge)], seed=9, key_range=F32_FINITE)
        a = c.groups[0][2]
        c.probe(a, "last 0x1", "lo", "last", "hi==lo+1", lo_on=0, hi_on=1)
        c.probe(a + 1, "first 0x2", "hi", "first", "hi==lo+1", lo_on=0, hi_on=1)
    elif name == "f32_nan_top":
        # the NaN run ends the array (the "mid" shape at the top: nothing sorts above a NaN)
        cl = plateau_len(n, 0.97)
        c = PlateauCase(name, n, True, "ceil", [(0, cl)], seed=10, key_range=F32_FINITE, top=NAN_KEY)
        c.probe(n - cl, "below", "cand", "last", hi_on=0)
        c.probe(n - cl + 1, "first NaN", "hi", "first", hi_on=0)
        c.probe(n - cl // 2, "middle NaN", "lo", "mid", "lo==hi", lo_on=0, hi_on=0)
        c.probe(n, "last NaN", "lo", "last", "lo==hi", lo_on=0)
    elif name == "f32_inf_nan":
        # +inf then NaN at the top: no key between them, though hi != lo + 1 in key space
        cl = plateau_len(n, 0.97, both=False)
        c = PlateauCase(name, n, True, "ceil", [(KEY_PINF - NAN_KEY, cl), (0, cl)], seed=11, key_range=F32_FINITE,
                        top=NAN_KEY)
        a = c.groups[0][2]
        c.probe(a, "last +inf", "lo", "last", "M==0", lo_on=0, hi_on=1)
        c.probe(a + 1, "first NaN", "hi", "first", "M==0", lo_on=0, hi_on=1)
        c.probe(n, "last NaN", "lo", "last", "lo==hi", lo_on=1)
    else:
        raise KeyError(name)
    if name == "f32_nan_top" or name == "f32_inf_nan":
        # the NaN run carries several payloads and both signs: all one key
        w = np.array(c.ref.words)
        nan = np.flatnonzero(c.ref.key == np.uint32(NAN_KEY))
        w[nan] = f32t.NAN_BITS[np.arange(nan.size) % f32t.NAN_BITS.size]
        c.ref = Ref(w, True)
    return c


I32_CASES = ("mid", "low", "high", "floor", "ceiling", "adjacent", "between_1", "between_40000")
F32_CASES = ("f32_zero_mid", "f32_zero_adjacent", "f32_subnormal_mid", "f32_subnormal_adjacent", "f32_nan_top",
             "f32_inf_nan")
PER_LEVEL_CASES = SHARDED_CASES = ("mid", "adjacent", "between_1", "between_40000")
# between_40000: 40000 keys are 625 sample keys, and the window is 2 * (5 sigma + 2) = 1284
# sample ranks at the median, so a window cannot hold them AND keep 4 sigmas (512) on both
# sides: its honest window ends inside the P+1 run for some of its probes.  Those probes are
# not asserted reached (NOT_BY_MARGIN); W == 0 over more than FIN_LDS_KEYS candidates is
# reached by construction in the planted variant "plus2" below.
NOT_BY_MARGIN = ("between_40000",)


# ------------------------------------------------------------- planted inputs
PLANTED_A = 1000  # the int32 value of band A


class PlantedCase:
    """The sampled chunks hold, sorted: low filler, a band of A, a band of B, high
    filler.  For every k in [k_lo, k_hi] the lower window rank falls in the A band and
    the upper one in the B band, BAND_MARGIN sample ranks from the band's ends.  The
    bands reach BAND_EXTRA sample ranks further out than that: together they then hold
    more than kth_window_slack64 / 64 = 1.5 times the window's sample keys, so the early
    window never stops at a coarser bin and lo = A, hi = B on a default ctx too.  The rest
    of the array makes L, E1, M, E2 exact."""

    VARIANTS = {"wide": 1000, "plus1": 1, "plus2": 2, "one_band": 0}  # B - A

    def __init__(self, variant, n=N_SMALL, seed=21):
        rng = np.random.default_rng([seed, n, self.VARIANTS[variant]])
        self.variant, self.n = variant, n
        s = self.s = sample_size(n)
        gap = self.VARIANTS[variant]
        A, B = PLANTED_A, PLANTED_A + gap
        # the counts: the eight boundaries L .. L+E1+M+E2+1 centred on n / 2
        E1 = 3000
        E2 = 3000 if gap else 0
        M = {0: 0, 1: 0, 2: 40000, 1000: 3000}[gap]  # plus2: more than the finisher's LDS holds
        L = n // 2 - (E1 + M + E2) // 2
        self.L, self.E1, self.M, self.E2, self.A, self.B = L, E1, M, E2, A, B
        self.k_lo, self.k_hi = L - 64, L + E1 + M + E2 + 1 + 64
        rl = [window_ranks(n, k, s) for k in (self.k_lo, self.k_hi)]
        # band A covers every lower window rank, band B every upper one, with the margin;
        # the bands meet at the sample's middle (one band: A covers both)
        self.a_first = rl[0][0] - BAND_MARGIN - BAND_EXTRA
        self.b_last = rl[1][1] + BAND_MARGIN + BAND_EXTRA
        self.split = s // 2 if gap else self.b_last
        nA, nB = self.split - self.a_first + 1, self.b_last - self.split
        assert nA <= E1 and nB <= E2
        below = np.sort(rng.integers(-(1 << 31), A - 1000, self.a_first - 1))
        above = np.sort(rng.integers(B + 1000, 1 << 31, s - self.b_last))
        sample = np.concatenate([below, np.full(nA, A), np.full(nB, B), above]).astype(np.int32)
        assert sample.size == s
        rest_n = n - s
        n_below = L - below.size
        n_above = rest_n - n_below - (E1 - nA) - M - (E2 - nB)
        assert n_below > 0 and n_above > 0
        inside = np.full(M, A + 1) if gap == 2 else rng.integers(A + 1, max(B, A + 2), M)
        rest = np.concatenate([rng.integers(-(1 << 31), A, n_below), np.full(E1 - nA, A), inside, np.full(E2 - nB, B),
                               rng.integers(B + 1, 1 << 31, n_above)]).astype(np.int32)
        words = np.empty(n, dtype=np.int32)
        idx = sample_indices(n)
        free = np.ones(n, dtype=bool)
        free[idx] = False
        words[idx] = sample  # sorted in sample order: the sample phase sorts it anyway
        words[free] = rest[rng.permutation(rest_n)]
        self.ref = Ref(words)
        self.lo_key, self.hi_key = int(i32_key([A])[0]), int(i32_key([B])[0])
        b = [L, L + 1, L + E1, L + E1 + 1, L + E1 + M, L + E1 + M + 1, L + E1 + M + E2, L + E1 + M + E2 + 1]
        names = ["miss below by one", "first of lo", "last of lo", "first past lo", "last before hi", "first past M",
                 "last of hi", "miss above by one"]
        self.bounds = list(zip(b, names))

    def expect(self, k):
        """(path, branch) for rank k."""
        br = self.ref.branch(k, self.lo_key, self.hi_key)[0]
        return (4 if br.startswith("miss") else 3), br

    def ks(self):
        return sorted({k for k, _ in self.bounds})


@functools.lru_cache(maxsize=None)
def planted_case(variant, n=N_SMALL):
    return PlantedCase(variant, n)


# ------------------------------------------------------------------ staircase
def staircase_values():
    """{-2^b - 1, -2^b, 2^b - 1, 2^b : b = 0..31} clipped to int32, with INT32_MIN and
    INT32_MAX: the distinct values, sorted (the 130 listed values hold a few twice).
    In order-key space (value + 2^31) every adjacent pair straddles a multiple of a
    power of two."""
    v = [-(1 << 31), (1 << 31) - 1]
    for b in range(32):
        v += [-(1 << b) - 1, -(1 << b), (1 << b) - 1, 1 << b]
    return np.unique(np.clip(np.array(v, dtype=np.int64), -(1 << 31), (1 << 31) - 1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def staircase(n):
    """(Ref, first ranks, last ranks) of a staircase of n keys: each value with a random
    multiplicity in [1, 2n/G] (n < G: n of the values, once each), in random positions."""
    vals = staircase_values()
    rng = np.random.default_rng([31, n])
    G = vals.size
    if n < G:
        vals = np.sort(rng.choice(vals, n, replace=False))
        mult = np.ones(n, dtype=np.int64)
    else:
        cap = 2 * n // G
        mult = np.ones(G, dtype=np.int64)
        left = n - G
        while left:
            add = rng.multinomial(left, np.full(G, 1.0 / G))
            add = np.minimum(add, cap - mult)
            mult += add
            left = n - int(mult.sum())
    w = np.repeat(vals, mult)[rng.permutation(n)]
    last = np.cumsum(mult)
    return Ref(w), last - mult + 1, last


@functools.lru_cache(maxsize=None)
def small_content(kind, n):
    """Contents of the every-rank sweep over the LDS and radix paths."""
    if kind == "random":
        rng = np.random.default_rng([41, n])
        return Ref(rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32))
    if kind == "f32_specials":
        return Ref(np.array(f32t.make("specials", n)), f32=True)
    if kind == "staircase":
        return staircase(n)[0]
    raise KeyError(kind)


# -------------------------------------------------------------------- 16-bit keys
K16_SIZES = (k16t.SMALL_N, k16t.SMALL_N + 1, (1 << 20) + 5)
K16_QUANTILES = (0.0, 0.01, 0.5, 0.99, 1.0)
K16_SPECIAL_KEYS = {"-0.0": 0x7FFF, "+0.0": 0x8000, "+inf": None, "NaN": 0xFFFF}


class K16Ref:
    """A 16-bit input: bits, order keys, their sort, and every tie group's edges from one bincount."""

    def __init__(self, bits, kind):
        self.kind = kind
        self.bits = np.ascontiguousarray(bits, dtype=np.uint16)
        self.n = self.bits.size
        self.key = k16t.order_key(self.bits, kind)
        self.sorted = np.sort(self.key)
        self.count = np.bincount(self.key, minlength=65536)
        self.last = np.cumsum(self.count)          # last rank of key v's group (where count[v] > 0)
        self.first = self.last - self.count + 1
        self.present = np.flatnonzero(self.count)

    def wants(self, ks):
        return k16t.of_order_key(self.sorted[np.asarray(ks, dtype=np.int64) - 1], self.kind)

    def group_of_rank(self, k):
        return int(self.sorted[k - 1])

    def probed_groups(self, quantiles=K16_QUANTILES):
        """Order keys of the tie groups nearest each quantile and their two neighbours; for
        the float kinds also the groups of -0.0, +0.0, +inf and NaN where present."""
        out = set()
        for q in quantiles:
            g = self.group_of_rank(min(max(int(math.ceil(q * self.n)), 1), self.n))
            i = int(np.searchsorted(self.present, g))
            out.update(int(self.present[j]) for j in (i - 1, i, i + 1) if 0 <= j < self.present.size)
        if self.kind in k16t.INF:
            for name, key in K16_SPECIAL_KEYS.items():
                key = 0x8000 | k16t.INF[self.kind] if key is None else key
                if self.count[key]:
                    out.add(key)
        return sorted(out)

    def edge_ranks(self, quantiles=K16_QUANTILES):
        """First and last rank of every probed group, ascending, without repeats."""
        ks = set()
        for g in self.probed_groups(quantiles):
            ks.update((int(self.first[g]), int(self.last[g])))
        return sorted(ks)

    def topk(self, k, largest):
        return topk_ref(self.key, self.sorted, k, largest)


@functools.lru_cache(maxsize=None)
def k16_input(kind, n):
    return K16Ref(k16t.family("specials", n, kind), kind)
