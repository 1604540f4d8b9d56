"""Inputs and references for the wide-rows edge tests (tests/test_gpu_wide_edges.py;
proved on the CPU by tests/test_wide_edges_inputs.py).  numpy only.

Three families, each built in order-key space and mapped back to words by the
documented rule (the inverse of V.Flavor.keys):

  Staircase  a row whose distinct values are the last key of one digit bin and the
             first key of the next, for the bins 1, half and last of every digit of
             the radix descent (11 + 11 + 10 bits of a 32-bit key, 11 + 5 of a 16-bit
             ord), under a first, a middle and a last populated prefix, plus the
             lowest and highest key of the type.  Probed at the first and last rank
             of every tie group.
  Fence      a row with one tie value T, b keys below it and the rest above, T
             placed on the columns around the boundaries of a forced plan's slices
             (or the fused walk's tiles).  Probed at k = b + j where the quota of
             ties runs out on, just before and just after each boundary.
  Mass       a float row of about a hundred weighted keys (the staircase's pairs
             within a few T of the row maximum, and one tie group across the slice
             boundaries) padded with keys of fixed-point weight 0.  Probed with the
             p and u that put p Z and u S(n) half a key's weight before S(j), for j
             the first and last rank of every tie group.

Every expected value comes from the plain references the other wide-rows tests use:
V.expect_select / V.expect_topk (one stable argsort of the order key) and
test_gpu_topp.RowRef (float64 cumulative weights).  Nothing here calls the library
except V.Flavor.slice_keys, which reads the plan's rounding from it.
"""
import collections
import os
import re

import numpy as np

import test_gpu_rows_var as V
import test_gpu_rows_wide16 as W16
import test_gpu_sample as S
import test_gpu_topp as T

FLAVORS = V.FLAVORS
FLOATS = T.NAMES
# (slices, group_rows): fused, 3 and 7 slices, 7 slices in groups of 5 rows
PLANS = ((1, 0), (3, 0), (7, 0), (7, 5))
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-k-selection_amd", "csrc")


# ------------------------------------------------------------------ the shape
def fused_block():
    """WD_FBLOCK, read from the kernel source."""
    if "fblock" not in _BUILT:
        with open(os.path.join(CSRC, "kth_rows_wide.hpp")) as f:
            m = re.search(r"constexpr\s+int\s+WD_FBLOCK\s*=\s*(\d+)\s*;", f.read())
        _BUILT["fblock"] = int(m.group(1))
    return _BUILT["fblock"]


def tile_of(fl):
    """The columns the fused walk takes a trip: one 16-byte load a thread."""
    return fused_block() * fl.align


def short_last(fl, cols, slices):
    sk = fl.slice_keys(cols, slices)
    return (slices - 1) * sk < cols < slices * sk


def cols_of(fl):
    """The smallest length with two whole tiles of the fused walk and a partial third, a partial
    (3-key) last vector, and a short last slice under the forced 3- and 7-slice plans."""
    if ("cols", fl.name) not in _BUILT:
        c = 2 * tile_of(fl) + 1
        while not (c % fl.align == 3 and short_last(fl, c, 3) and short_last(fl, c, 7)):
            c += 1
        _BUILT[("cols", fl.name)] = c
    return _BUILT[("cols", fl.name)]


def units_of(fl, cols, slices):
    """(begin, end) of every slice of a forced plan; slices == 1: of every tile of the fused walk."""
    size = tile_of(fl) if slices == 1 else fl.slice_keys(cols, slices)
    return [(b, min(b + size, cols)) for b in range(0, cols, size)]


# ------------------------------------------------------------------ keys and words
def nbits(fl):
    return 16 if fl.w16 else 32


def digits_of(fl):
    """(shift, bins) of every digit of the descent."""
    return ((5, 2048), (0, 32)) if fl.w16 else ((21, 2048), (10, 2048), (0, 1024))


def words_of(fl, keys):
    """The words whose order keys are `keys` (the documented rule, inverted)."""
    k = np.asarray(keys, dtype=np.uint64).astype(fl.np_t)
    top = fl.np_t(1 << (nbits(fl) - 1))
    if fl.name in ("i32", "i16"):
        return k ^ top
    if fl.name == "u16":
        return k
    return np.where(k & top, k & ~top, ~k).astype(fl.np_t)


def populated(fl, keys):
    """key(word(key)) == key: false in the NaN ranges of the float kinds but their canonical top."""
    k = np.asarray(keys, dtype=np.uint64).astype(fl.np_t)
    return fl.keys(words_of(fl, k)) == k


def value_key(fl, x):
    """The order key of the float x (float kinds; x representable in the kind)."""
    if fl.name == "f32":
        w = np.array([x], dtype=np.float32).view(np.uint32)
    else:
        w = W16.to_kind_bits(np.array([x], dtype=np.float32), fl.name)
        assert T.values(fl, w)[0] == x, (fl.name, x)
    return int(fl.keys(w)[0])


# ------------------------------------------------------------------ (a) the digit staircase
Pair = collections.namedtuple("Pair", "digit prefix want_b bin a b")  # a: last key of bin - 1, b: first key of bin


def _nearest(pool, x):
    return min(pool, key=lambda v: (abs(v - x), v))


def boundary_pairs(fl, lo=None, hi=None):
    """The pairs (last key of bin B - 1, first key of bin B) of every digit inside [lo, hi], and
    the substitutions made.  Digit 0: B = 1, half, last (full range) or nine boundaries spread over
    the range; where a wanted boundary has an unpopulable side, the nearest
    boundary with both sides populated stands in.  Lower digits: B = 1, half, last under a first,
    a middle and a last prefix, a prefix being usable when all three of its pairs are populated
    and in range; each lower digit refines the prefixes of the digit above it."""
    full = lo is None
    lo, hi = (0, (1 << nbits(fl)) - 1) if full else (lo, hi)
    digs = digits_of(fl)
    pairs, subs = [], []

    def ok(base, shift, bs):
        """Per base: every pair around base + (b << shift), b in bs, is in range and populated."""
        x = np.atleast_1d(np.asarray(base, dtype=np.int64))[:, None] + (np.asarray(bs, dtype=np.int64) << shift)[None, :]
        good = (x - 1 >= lo) & (x <= hi)
        x = np.where(good, x, 1)
        good &= populated(fl, (x - 1).ravel()).reshape(x.shape) & populated(fl, x.ravel()).reshape(x.shape)
        return good

    shift, bins = digs[0]
    good = [int(b) for b in np.nonzero(ok(0, shift, np.arange(1, bins))[0])[0] + 1]
    wanted = (1, bins // 2, bins - 1) if full else tuple(sorted(set(good[::max(1, len(good) // 8)]) | {good[-1]}))
    for w in wanted:
        b = _nearest(good, w)
        if b != w:
            subs.append((0, 0, w, b))
        pairs.append(Pair(0, 0, w, b, (b << shift) - 1, b << shift))
    prefixes = {"first": 0, "middle": 0, "last": 0}  # the prefix above digit d, right-aligned
    for d in range(1, len(digs)):
        shift, bins = digs[d]
        up_shift, up_bins = digs[d - 1]
        bs = (1, bins // 2, bins - 1)
        for tag in ("first", "middle", "last"):
            kids = (prefixes[tag] * up_bins if d > 1 else 0) + np.arange(up_bins)
            usable = [int(q) for q in kids[ok(kids.astype(np.int64) << up_shift, shift, bs).all(axis=1)]]
            assert usable, (fl.name, d, tag)
            q = {"first": usable[0], "last": usable[-1]}.get(tag, _nearest(usable, (usable[0] + usable[-1] + 1) // 2))
            wanted_q = {"first": int(kids[0]), "last": int(kids[-1])}.get(tag, int(kids[up_bins // 2]))
            if full and q != wanted_q:
                subs.append((d, tag, wanted_q, q))
            prefixes[tag] = q
            for b in bs:
                x = (q << up_shift) + (b << shift)
                pairs.append(Pair(d, q, b, b, x - 1, x))
    every = np.arange(lo, hi + 1, dtype=np.uint64) if hi - lo < (1 << 17) else None
    if every is not None:
        pop = every[populated(fl, every)]
        ends = (int(pop[0]), int(pop[-1]))
    elif fl.name == "i32":
        ends = (lo, hi)
    else:  # float32: -inf below, the canonical NaN above (full range), else the range's ends
        ends = (value_key(fl, -np.inf), 0xFFFFFFFF) if full else (lo, hi)
    assert populated(fl, list(ends)).all()
    return pairs, subs, ends


def fill_cycle(values, count, seed):
    """`count` keys (None: every value once round): the values in turn with multiplicities 1, 2, 3,
    1, ..., in a fixed-seed order."""
    out, i = [], 0
    while len(out) < count if count else i < len(values):
        out += [values[i % len(values)]] * (1 + i % 3)
        i += 1
    out = np.array(out[:count], dtype=np.uint64)
    return out[np.random.default_rng(seed).permutation(out.size)]


def group_edges(keys, largest):
    """[(rank, key, 'first' | 'last')] for every tie group of the row, in the direction's order."""
    vals, counts = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    if largest:
        vals, counts = vals[::-1], counts[::-1]
    ends = np.cumsum(counts)
    out = []
    for v, c, e in zip(vals, counts, ends):
        out.append((int(e - c + 1), int(v), "first"))
        out.append((int(e), int(v), "last"))
    return out


class Staircase:
    def __init__(self, name):
        self.fl = fl = V.Flavor(name)
        self.cols = cols = cols_of(fl)
        self.pairs, self.subs, self.ends = boundary_pairs(fl)
        self.values = sorted({k for p in self.pairs for k in (p.a, p.b)} | set(self.ends))
        self.keys = fill_cycle(self.values, cols, 20260 + FLAVORS.index(name))
        self.row = words_of(fl, self.keys)
        assert np.array_equal(fl.keys(self.row).astype(np.uint64), self.keys)
        self.row2 = self.row[np.random.default_rng(77).permutation(cols)]  # the same keys at other columns
        self.equal = np.full(cols, self.row[0], dtype=fl.np_t)
        self._cases = {}

    def probes(self, largest):
        return group_edges(self.keys, largest)

    def case(self, largest):
        """(words, ks): one row a probe, and an all-equal row at its median."""
        if largest not in self._cases:
            ks = [p[0] for p in self.probes(largest)] + [(self.cols + 1) // 2]
            words = np.vstack([np.tile(self.row, (len(ks) - 1, 1)), self.equal[None]])
            self._cases[largest] = (words, ks)
        return self._cases[largest]

    def pair_words(self):
        return np.vstack([self.row, self.row2])


def digits_picked(fl, keys, answer):
    """How many digits the descent picks before its early end for `answer`: 0 when the row holds
    one value, d when the keys sharing the answer's first d digits are one value, else all."""
    keys = np.asarray(keys, dtype=np.uint64)
    digs = digits_of(fl)
    if np.unique(keys).size == 1:
        return 0
    if fl.w16:  # the 16-bit descent ends early only on a one-valued row
        return len(digs)
    for d, (shift, _) in enumerate(digs[:-1], 1):
        if np.unique(keys[(keys >> np.uint64(shift)) == (np.uint64(answer) >> np.uint64(shift))]).size == 1:
            return d
    return len(digs)


# ------------------------------------------------------------------ (b) the tie fence
# what a unit (slice or tile) holds: T on its first / last column, T at columns inside, no key below T
SPECS = {3: ({"in": 2, "last": 1}, {"first": 1, "in": 1, "last": 1, "no_low": 1}, {"first": 1, "last": 1}),
         7: ({"in": 2, "last": 1}, {"first": 1, "in": 1, "last": 1, "no_low": 1}, {"first": 1}, {},
             {"in": 2, "last": 1}, {"first": 1, "in": 1}, {"first": 1, "last": 1})}


class Fence:
    def __init__(self, name, slices):
        self.fl = fl = V.Flavor(name)
        self.slices, self.cols = slices, cols_of(fl)
        self.units = units_of(fl, self.cols, slices)
        spec = SPECS[len(self.units)]
        mid = 1 << (nbits(fl) - 1)
        t = mid + (0x3F800000 if not fl.w16 else 0x3C00) + 5  # every digit non-zero, ~key populated too
        lows, highs = [t - 3, t - 2, t - 1], [t + 1, t + 2, t + 3]
        keys = np.zeros(self.cols, dtype=np.uint64)
        self.t_cols = []
        for (b, e), sp in zip(self.units, spec):
            c = np.arange(b, e)
            keys[b:e] = np.where(c % 2 == 0, np.array(lows)[(c // 2) % 3], np.array(highs)[(c // 2) % 3])
            if sp.get("no_low"):
                keys[b:e] = np.array(highs)[c % 3]
            elif e - b < 4:  # the fused walk's 3-key tail: T, a key below it, T
                keys[b + 1] = lows[0]
            at = ([b] if sp.get("first") else []) + ([e - 1] if sp.get("last") else [])
            at += [b + (i + 1) * (e - b) // (sp["in"] + 1) for i in range(sp.get("in", 0)) if e - b > 4]
            self.t_cols += sorted(set(at))
        keys[self.t_cols] = t
        self.t, self.keys = t, keys
        self.below = int((keys < t).sum())
        self.e = [sum(1 for c in self.t_cols if c < e) for _, e in self.units]  # E_s
        js = {1, len(self.t_cols)} | set(self.e) | {x + 1 for x in self.e}
        self.js = sorted(j for j in js if 1 <= j <= len(self.t_cols))
        self.ks = [self.below + j for j in self.js]
        mask = (1 << nbits(fl)) - 1
        self.rows = {False: words_of(fl, keys), True: words_of(fl, keys ^ np.uint64(mask))}
        for largest, row in self.rows.items():
            assert np.array_equal(fl.keys(row).astype(np.uint64), keys ^ np.uint64(mask if largest else 0))

    def case(self, largest):
        """(words, ks): one row a probe."""
        return np.tile(self.rows[largest], (len(self.ks), 1)), list(self.ks)

    def pair_words(self, largest):
        return np.vstack([self.rows[largest], self.rows[largest][::-1]])


def fences(name):
    """The fused-tile, 3-slice and 7-slice fences of a flavor."""
    return [fence(name, s) for s in (1, 3, 7)]


# ------------------------------------------------------------------ (c) the mass staircase
M_TOP = 4.0
REACH = 4.0  # the weighted keys lie within REACH * T of the row maximum (the margin proof sets it)
TIES = 12


class Mass:
    def __init__(self, name, temp):
        self.fl = fl = V.Flavor(name)
        self.temp, self.cols = temp, cols_of(fl)
        cols = self.cols
        lo, hi = value_key(fl, M_TOP - REACH * temp), value_key(fl, M_TOP)
        self.pairs, self.subs, _ = boundary_pairs(fl, lo, hi)
        values = sorted({k for p in self.pairs for k in (p.a, p.b)} | {lo, hi})
        tie = (lo + hi) // 2
        while tie in values or not populated(fl, [tie]).all():
            tie += 1
        assert lo < tie < hi
        weighted = fill_cycle(values, None, 311)
        # the tie group: around the boundaries of the 7-slice plan, the 3-slice plan and the fused tiles
        u7, u3, u1 = (units_of(fl, cols, s) for s in (7, 3, 1))
        at = [u7[0][1] - 1, u7[1][0], u7[2][1] - 1, u7[3][0], u7[6][0], cols - 1, u3[0][1] - 1, u3[1][0],
              u1[0][1] - 1, u1[1][0], u7[4][0] + 17, u7[5][0] + 33]
        assert len(set(at)) == TIES
        free = np.setdiff1d(np.arange(cols), at)
        free = free[np.random.default_rng(312).permutation(free.size)]
        keys = np.zeros(cols, dtype=np.uint64)
        keys[at] = tie
        keys[free[:weighted.size]] = weighted
        # weight 0 in fixed point: -inf, and values 40 T to 100 T below the maximum
        pad = free[weighted.size:]
        far = np.linspace(M_TOP - 100 * temp, M_TOP - 40 * temp, 97).astype(np.float32)
        far_w = far.view(np.uint32) if fl.name == "f32" else W16.to_kind_bits(far, fl.name)
        far_k = fl.keys(far_w).astype(np.uint64)
        n = np.arange(pad.size)
        keys[pad] = np.where(n % 3 == 0, np.uint64(value_key(fl, -np.inf)), far_k[n % 97])
        self.tie_cols, self.weighted = at, weighted.size + TIES
        self.row = words_of(fl, keys)
        assert np.array_equal(fl.keys(self.row).astype(np.uint64), keys)
        self.ref = T.RowRef(fl, self.row, 1.0, temp, cols)  # the order and S(j); p is set per probe
        s = self.ref.s
        okeys = keys[self.ref.order][:self.weighted]
        assert (okeys >= lo).all() and (keys[self.ref.order][self.weighted:] < lo).all()
        self.edges = [j for j, _, _ in group_edges(okeys, True)]
        self.edges = sorted(set(self.edges))
        self.z = float(self.ref.z)
        # nucleus: one probe an edge
        self.nuc = [(j, float(np.float32((s[j] - (s[j] - s[j - 1]) / 2) / self.z))) for j in self.edges]
        # top-p: every fourth probe under the caps j - 1, j, j + 1
        self.capped = [(j, p, cap) for j, p in self.nuc[::4] for cap in (j - 1, j, j + 1)]
        # sampling: (p, cap) configurations, then one probe an edge within the kept keys
        ja, pa = min(self.nuc, key=lambda t: abs(t[1] - 0.5))
        jb, pb = min(self.nuc, key=lambda t: abs(t[1] - 0.9))
        self.configs = [(1.0, 0, cols), (pa, 0, ja), (pb, 0, jb), (pa, ja - 1, ja), (pa, ja, ja), (pa, ja + 1, ja),
                        (1.0, ja, cols)]
        self.draws = []  # (p, cap, cnt, j, u)
        for p, cap, n in self.configs:
            cnt = min(n, cap) if cap > 0 else n
            assert 1 <= cnt
            for j in sorted({e for e in self.edges if e <= cnt} | ({cnt} if cnt <= self.weighted else set())):
                if j <= cnt:
                    self.draws.append((p, cap, cnt, j, float(np.float32((s[j] - (s[j] - s[j - 1]) / 2) / s[cnt]))))

    def words(self, rows):
        return np.tile(self.row, (rows, 1))

    def ref_at(self, p):
        return T.RowRef(self.fl, self.row, p, self.temp, self.cols)


def nucleus_margin(ref, p32):
    """min over j of |p Z - S(j)| / (eps p Z)."""
    pz = float(np.float32(p32)) * ref.z
    return float(np.abs(ref.s - pz).min() / (ref.eps * pz))


def draw_margin(ref, cnt, u32):
    """min over j <= cnt of |A - S(j)| / (e A), A = u S(cnt), e = 2 eps."""
    a = S.u_of(u32) * ref.s[cnt]
    return float(np.abs(ref.s[:cnt + 1] - a).min() / (2.0 * ref.eps * a))


# ------------------------------------------------------------------ built once
_BUILT = {}


def _once(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


def staircase(name):
    return _once(("a", name), lambda: Staircase(name))


def fence(name, slices):
    return _once(("b", name, slices), lambda: Fence(name, slices))


def mass(name, temp):
    return _once(("c", name, temp), lambda: Mass(name, temp))


def expected(tag, fn):
    """A reference result computed once and shared (never written to)."""
    return _once(("want",) + tag, fn)
