// kth_rows_topp.hpp -- top-p (nucleus) selection per row for wide float rows
// (include/kth.h "wide rows, top-p"): the size n_r of each row's nucleus and
// its smallest kept logit.  A nucleus is a weighted select: where the radix
// select of kth_rows_wide.hpp looks for the bin at which the *count* of the
// larger keys reaches k, this one looks for the bin at which their
// *probability mass* reaches p * Z.
//
// Keys are flipped order keys throughout (fk = ~key, the top-k largest
// convention: the smaller fk, the larger the logit), so "the first n keys" of
// the contract are the n smallest fk, ties by column.
//
// Weights are fixed point, w_fix = rint(w * 2^39) in a u64, w evaluated in
// float32 (tp_wfix, the one place that knows the weight rule).  Integer adds
// commute, so every sum -- a workgroup's LDS bin, a row's bin in scratch, Z --
// is the same number whatever the plan, the slice count, the load path or the
// order in which the adds land.  No float is ever accumulated.  With cols <=
// 2^24 and w <= 1 a sum stays below 2^63.
//
// Passes, per row:
//   M      the row's top and bottom order key (one read).  m, the top, is the
//          reference of every weight; the bottom is the threshold of a row
//          that keeps everything (p >= 1).
//   digit  K::PASSES weighted digit passes (11 + 11 + 10 bits of a 32-bit key,
//          11 + 5 of a 16-bit ord).  For the keys matching the prefix: a u32
//          count and a u64 mass per bin, and the min / max of those keys for
//          the early end of kth_rows_wide.hpp (one value fills the bin).
//   pick   Z = the first digit's total mass; target = max(1, ceil(p * Z)), by
//          one thread in double.  The first bin, in fk order, at which the
//          running mass reaches the remaining target is picked; the mass and
//          the count of the bins before it are subtracted / added up, the
//          prefix is extended.  At the end
//            n = count_better + clamp(ceil(remaining / w_fix(thr)), 1, count_equal).
//          Invariant: a bin is picked only when it moves the running mass past
//          the target (block_pick_vals: target > mass before, <= mass with it),
//          so the picked bin, and in the end the threshold value, always has
//          non-zero mass: the division above is never by zero, and keys of
//          weight 0 (-inf, or more than about 27 T below m) are never the
//          threshold of a filtered row.
//
// Rows settled by the first pick, whose later workgroups return at once:
//   len == 0            n = 0, the zero word;
//   p >= 1 or NaN       n = len, thr = the row's bottom key, no digit pass;
//   p <= 0              n = 1, thr = m, no digit pass;
//   m is +inf or NaN    the keys equal to m weigh 1 and all others 0, so the
//                       first digit's total mass is their count c << 39 and
//                       n = clamp(ceil(p * c), 1, c), thr = m: no exponential
//                       is evaluated for such a row.
//
// Two forms, by kth_rows_wide.hpp's plan.  Split: k_tp_max, then per digit
// k_tp_count (grid slices x group rows; LDS bins, non-empty ones added to the
// row's bins in scratch with agent-scope atomics) and k_tp_pick (one workgroup
// a row) after the kernel boundary: no cooperative launch, no grid barrier, no
// in-launch flag.  Fused: k_tp_fused, one 512-thread workgroup per row, M and
// every digit in one launch, bins in LDS only.
//
// Scratch (split form): per row 2048 u64 masses, 2048 u32 counts and a TpState,
// the top-p calls' own.  Every sequence leaves masses and counts zero (the pick
// clears what it reads) and the state's accumulating words (nmn, mx, m_top,
// m_bot) zero (the pick that settles a row clears them).
//
// The key type lives in a traits class K: TpF32 here, TpK16<BF> in
// kth_rows_topp16.hpp.  Included by kth_kernels.hip after kth_rows_wide16.hpp.
#pragma once

namespace kth {

constexpr int TP_FRAC = 39;
constexpr u64 TP_ONE = 1ull << TP_FRAC;  // the weight of a key equal to m

// The per-row arrays of a top-p call, advanced to the group's first row; each
// may be null (then the scalar beside it holds for every row).  k == 0: a
// nucleus call (no cap, ks unused).
struct TopP {
    const int32_t *lens;
    const float *ps, *temps;
    const int32_t *ks;
    float p, temp;
    int32_t k;
};

// A row's state between the kernels of the split form (scratch).
struct TpState {
    u64 target;       // the fixed-point mass still to reach among the keys matching `prefix`
    uint32_t better;  // keys before every key matching `prefix`
    uint32_t prefix;  // the digits picked so far, right-aligned
    uint32_t done;
    uint32_t eqn;     // keys matching `prefix`
    uint32_t nmn, mx;        // max(fk ^ MASK), max(fk) of the keys matching `prefix`
    uint32_t m_top, m_bot;   // pass M: max(fk ^ MASK), max(fk) of the row
};
constexpr int TP_STATE_BYTES = sizeof(TpState);

__device__ __forceinline__ uint32_t tp_row_len(const TopP &v, u64 r, uint32_t cols) {
    if (!v.lens) return cols;
    const int32_t n = v.lens[r];
    return n < 0 ? 0u : (uint32_t)n < cols ? (uint32_t)n : cols;
}
// p_r in [0, 1]: 1 stands for "no filter" (p >= 1 or NaN), below 0 counts as 0
__device__ __forceinline__ float tp_row_p(const TopP &v, u64 r) {
    const float p = v.ps ? v.ps[r] : v.p;
    return !(p < 1.0f) ? 1.0f : p < 0.0f ? 0.0f : p;
}
// 1 / T_r; a device T that is not finite or not > 0 counts as 1
__device__ __forceinline__ float tp_row_inv_temp(const TopP &v, u64 r) {
    float t = v.temps ? v.temps[r] : v.temp;
    if (!(t > 0.0f) || t == __builtin_inff()) t = 1.0f;
    return 1.0f / t;
}
__device__ __forceinline__ uint32_t tp_row_cap(const TopP &v, u64 r) {
    const int32_t q = v.ks ? v.ks[r] : v.k;
    return q < 0 ? 0u : q < v.k ? (uint32_t)q : (uint32_t)v.k;
}
// (workgroup-uniform) a row the first pick settles from pass M alone
__device__ __forceinline__ bool tp_row_trivial(uint32_t len, float p) { return len == 0u || p >= 1.0f || p <= 0.0f; }

// The weight of key fk (value x) of a row whose top key is fm (value m), as
// fixed point.  special: m is +inf or NaN.  The one definition every pass and
// every pick uses, so a key weighs the same wherever it is met.
__device__ __forceinline__ u64 tp_wfix(uint32_t fk, float x, uint32_t fm, float m, float inv_t, bool special) {
    if (fk == fm) return TP_ONE;
    if (special) return 0;
    const float d = x - m;  // <= 0; -inf for x = -inf
    const float w = d == 0.0f ? 1.0f : expf(d * inv_t);
    return (u64)rintf(w * (float)TP_ONE);  // (a power of two: the product is exact)
}

// target = max(1, ceil(p * Z)), at most Z
__device__ __forceinline__ u64 tp_target(float p, u64 z) {
    const double t = ceil((double)p * (double)z);
    const u64 q = t < 1.0 ? 1ull : (u64)t;
    return q < z ? q : z;
}
// n of the keys equal to the threshold: clamp(ceil(remaining / wf), 1, eq)
__device__ __forceinline__ uint32_t tp_ties(u64 remaining, u64 wf, uint32_t eq) {
    const u64 q = (remaining + wf - 1) / wf;
    return q < 1 ? 1u : q < eq ? (uint32_t)q : eq;
}

// float32 keys
struct TpF32 {
    using elem = uint32_t;  // an input element and the threshold's word
    static constexpr int PASSES = 3, PER = 4;
    static constexpr uint32_t MASK = 0xFFFFFFFFu;
    static __device__ __forceinline__ uint32_t dbits(int pass) { return pass == 2 ? 10u : 11u; }
    static __device__ __forceinline__ uint32_t shift(int pass) { return wd_shift(pass); }
    static __device__ __forceinline__ float val(uint32_t bits) { return __uint_as_float(bits); }
    static __device__ __forceinline__ uint32_t bits_of(uint32_t fk) { return WideKey<true>::bits(~fk); }
    static __device__ __forceinline__ bool special(uint32_t fk) { return ~fk >= key_of_f32(0x7F800000u); }
    template <bool VEC>
    static __device__ __forceinline__ uint4 load(const elem *__restrict__ row, uint32_t e, uint32_t end) {
        return wd_load4<VEC>(row, e, end);
    }
    // f(fk, value) for each of the loaded columns e .. e+3 below `end`
    template <class F>
    static __device__ __forceinline__ void each(const uint4 &x, uint32_t e, uint32_t end, F f) {
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + (uint32_t)j < end) f(~WideKey<true>::key(w[j]), __uint_as_float(w[j]));
    }
};

// f(fk, value) for every key of columns [begin, end) (begin % K::PER == 0),
// WD_U loads in flight per thread.
template <class K, bool VEC, int BLOCK, class F>
__device__ __forceinline__ void tp_walk(const typename K::elem *__restrict__ row, uint32_t begin, uint32_t end, F f) {
    for (uint32_t base = begin + threadIdx.x * (uint32_t)K::PER; base < end; base += (uint32_t)(BLOCK * K::PER * WD_U)) {
        uint4 x[WD_U];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) x[u] = K::template load<VEC>(row, base + (uint32_t)(u * BLOCK * K::PER), end);
#pragma unroll
        for (int u = 0; u < WD_U; ++u) K::each(x[u], base + (uint32_t)(u * BLOCK * K::PER), end, f);
    }
}

// smm[0 .. 1] take the wave-reduced maxima a and b (LDS, zeroed by the caller)
__device__ __forceinline__ void tp_max2(uint32_t a, uint32_t b, uint32_t *smm) {
    a = wd_wave_max(a);
    b = wd_wave_max(b);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        (void)__hip_atomic_fetch_max(smm, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_max(smm + 1, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Pass M over columns [begin, end): smm[0 .. 1] take max(fk ^ MASK), max(fk).
template <class K, bool VEC, int BLOCK>
__device__ __forceinline__ void tp_max_range(const typename K::elem *__restrict__ row, uint32_t begin, uint32_t end,
                                             uint32_t *smm) {
    uint32_t top = 0, bot = 0;
    tp_walk<K, VEC, BLOCK>(row, begin, end, [&](uint32_t fk, float) {
        top = (fk ^ K::MASK) > top ? (fk ^ K::MASK) : top;
        bot = fk > bot ? fk : bot;
    });
    tp_max2(top, bot, smm);
}

// Digit `pass` of the keys of columns [begin, end) that match `prefix`: count
// and mass per bin into the workgroup's LDS bins hc / hm, smm[0 .. 1] take
// max(fk ^ MASK), max(fk) of those keys.  The caller zeroes hc, hm and smm
// before and synchronises after.
template <class K, bool VEC, int BLOCK>
__device__ __forceinline__ void tp_count_range(const typename K::elem *__restrict__ row, uint32_t begin, uint32_t end,
                                               int pass, uint32_t prefix, uint32_t fm, float m, float inv_t,
                                               bool special, uint32_t *hc, u64 *hm, uint32_t *smm) {
    const uint32_t mshift = K::shift(pass > 0 ? pass - 1 : 0), dshift = K::shift(pass);
    const uint32_t dmask = (1u << K::dbits(pass)) - 1u;
    uint32_t nmn = 0, mx = 0;
    tp_walk<K, VEC, BLOCK>(row, begin, end, [&](uint32_t fk, float x) {
        if (pass == 0 || (fk >> mshift) == prefix) {
            const uint32_t bin = (fk >> dshift) & dmask;
            wd_add(hc, bin);
            const u64 w = tp_wfix(fk, x, fm, m, inv_t, special);
            if (w) (void)__hip_atomic_fetch_add(hm + bin, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            nmn = (fk ^ K::MASK) > nmn ? (fk ^ K::MASK) : nmn;
            mx = fk > mx ? fk : mx;
        }
    });
    tp_max2(nmn, mx, smm);
}

template <int BLOCK>
__device__ __forceinline__ void tp_zero_lds(uint32_t *hc, u64 *hm, uint32_t *smm) {
    for (int i = threadIdx.x; i < NBINS; i += BLOCK) hc[i] = 0u, hm[i] = 0ull;
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
}

// A row's selection in registers (workgroup-uniform).
struct TpRun {
    u64 target;
    uint32_t better, prefix, eqn;
    uint32_t done, answer, n;  // at the end: the threshold (fk) and the nucleus size
};

// One digit's pick.  Thread t holds bins [t * PER, t * PER + PER): masses hm,
// counts hc.  nmn / mx: the matching keys' max(fk ^ MASK) / max(fk).  pass 0
// derives the target from Z.  scratch: BLOCK / 64 + 3 words, sx: 2 words (LDS).
template <class K, int BLOCK, int PER>
__device__ __forceinline__ void tp_pick_digit(const u64 (&hm)[PER], const uint32_t (&hc)[PER], int pass, float p,
                                              uint32_t nmn, uint32_t mx, uint32_t fm, float inv_t, bool special,
                                              TpRun &s, u64 *scratch, u64 *sx) {
    const float m = K::val(K::bits_of(fm));
    if (pass == 0) {
        u64 sum = 0, z;
#pragma unroll
        for (int j = 0; j < PER; ++j) sum += hm[j];
        (void)block_exclusive_scan<BLOCK>(sum, scratch, &z);
        if (threadIdx.x == 0) sx[0] = tp_target(p, z);  // once per row, by one thread
        __syncthreads();
        s.target = sx[0];
        __syncthreads();
        if (special) {  // the keys equal to m weigh TP_ONE, every other key 0
            s.answer = fm;
            s.n = tp_ties(s.target, TP_ONE, (uint32_t)(z >> TP_FRAC));
            s.done = 1;
            return;
        }
    }
    if ((nmn ^ K::MASK) == mx) {  // one value fills the bin (or the row): the threshold
        s.answer = mx;
        s.n = s.better + tp_ties(s.target, tp_wfix(mx, K::val(K::bits_of(mx)), fm, m, inv_t, false), s.eqn);
        s.done = 1;
        return;
    }
    uint32_t bin = 0;
    u64 below = 0;
    (void)block_pick_vals<BLOCK, PER>(hm, s.target, &bin, &below, scratch);
    uint32_t csum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) csum += hc[j];
    const u64 cpre = block_exclusive_scan<BLOCK>((u64)csum, scratch, nullptr);
    if (bin / (uint32_t)PER == threadIdx.x) {
        uint32_t c = (uint32_t)cpre;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const uint32_t b = threadIdx.x * (uint32_t)PER + (uint32_t)j;
            if (b < bin) c += hc[j];
            if (b == bin) sx[1] = hc[j];
        }
        sx[0] = c;
    }
    __syncthreads();
    s.better += (uint32_t)sx[0];
    s.eqn = (uint32_t)sx[1];
    __syncthreads();
    s.target -= below;
    s.prefix = pass == 0 ? bin : (s.prefix << K::dbits(pass)) | bin;
    if (pass == K::PASSES - 1) {  // the bin is one value, of non-zero mass (see the file comment)
        s.answer = s.prefix;
        s.n = s.better + tp_ties(s.target, tp_wfix(s.answer, K::val(K::bits_of(s.answer)), fm, m, inv_t, false), s.eqn);
        s.done = 1;
    }
}

// A settled row's outputs (one thread): n, the threshold's word (a NaN
// canonical, the zero word for an empty row) and, for kth_topp_*, the rank the
// var top-k takes, min(n, cap).  d_n, d_thr, rank: the group's first row; each
// may be null.
template <class K>
__device__ __forceinline__ void tp_write_row(const TopP &v, u64 r, uint32_t len, uint32_t n, uint32_t answer,
                                             int32_t *__restrict__ d_n, typename K::elem *__restrict__ d_thr,
                                             int32_t *__restrict__ rank) {
    if (d_n) d_n[r] = (int32_t)n;
    if (d_thr) d_thr[r] = len ? (typename K::elem)K::bits_of(answer) : (typename K::elem)0;
    if (rank) {
        const uint32_t cap = tp_row_cap(v, r);
        rank[r] = (int32_t)(n < cap ? n : cap);
    }
}
// The rows the first pick settles from pass M: true, with n and the threshold.
__device__ __forceinline__ bool tp_settle_trivial(uint32_t len, float p, uint32_t fm, uint32_t bot, uint32_t *n,
                                                  uint32_t *answer) {
    if (!tp_row_trivial(len, p)) return false;
    *n = len == 0u ? 0u : p >= 1.0f ? len : 1u;
    *answer = p >= 1.0f ? bot : fm;
    return true;
}

// ---- split form: pass M of one slice
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_tp_max(const typename K::elem *__restrict__ keys, u64 ld, uint32_t cols,
                                                        uint32_t slice_keys, TpState *__restrict__ st_g, TopP v) {
    __shared__ uint32_t smm[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t len = tp_row_len(v, r, cols);
    if (s * slice_keys >= len) return;  // (workgroup-uniform) a slice past its row's end
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    tp_max_range<K, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, smm);
    __syncthreads();
    if (threadIdx.x == 0) {
        (void)__hip_atomic_fetch_max(&st_g[r].m_top, smm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(&st_g[r].m_bot, smm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- split form: one weighted digit of one slice
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_tp_count(const typename K::elem *__restrict__ keys, u64 ld,
                                                          uint32_t cols, uint32_t slice_keys, int pass,
                                                          u64 *__restrict__ mass_g, uint32_t *__restrict__ cnt_g,
                                                          TpState *__restrict__ st_g, TopP v) {
    __shared__ u64 hm[NBINS];
    __shared__ uint32_t hc[NBINS];
    __shared__ uint32_t smm[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    TpState *st = st_g + r;
    uint32_t prefix = 0;
    if (pass > 0) {
        if (st->done) return;  // (workgroup-uniform) settled by an earlier pick
        prefix = st->prefix;
    }
    const uint32_t len = tp_row_len(v, r, cols);
    if (s * slice_keys >= len || tp_row_trivial(len, tp_row_p(v, r))) return;  // (workgroup-uniform)
    const uint32_t fm = st->m_top ^ K::MASK;
    tp_zero_lds<WD_BLOCK>(hc, hm, smm);
    __syncthreads();
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    tp_count_range<K, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, pass, prefix, fm, K::val(K::bits_of(fm)),
                                     tp_row_inv_temp(v, r), K::special(fm), hc, hm, smm);
    __syncthreads();
    const uint32_t nb = 1u << K::dbits(pass);
    for (uint32_t b = threadIdx.x; b < nb; b += WD_BLOCK) {
        const uint32_t c = hc[b];
        const u64 w = hm[b];
        if (c) (void)__hip_atomic_fetch_add(cnt_g + (u64)r * NBINS + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w) (void)__hip_atomic_fetch_add(mass_g + (u64)r * NBINS + b, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0 && (smm[0] | smm[1])) {
        (void)__hip_atomic_fetch_max(&st->nmn, smm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(&st->mx, smm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- split form: pick digit `pass` of every row of the group, advance its
// state, clear its bins and min / max words; a row that settles writes its
// outputs and clears pass M's words.
template <class K>
__global__ __launch_bounds__(WD_BLOCK) void k_tp_pick(u64 *__restrict__ mass_g, uint32_t *__restrict__ cnt_g,
                                                      TpState *__restrict__ st_g, int pass, uint32_t cols, TopP v,
                                                      int32_t *__restrict__ d_n, typename K::elem *__restrict__ d_thr,
                                                      int32_t *__restrict__ rank) {
    constexpr int PER = NBINS / WD_BLOCK;
    __shared__ u64 scratch[WD_BLOCK / WAVE + 3];
    __shared__ u64 sx[2];
    const uint32_t r = blockIdx.x;
    TpState *st = st_g + r;
    const TpState s0 = *st;
    if (pass > 0 && s0.done) return;  // (workgroup-uniform)
    const uint32_t len = tp_row_len(v, r, cols);
    const float p = tp_row_p(v, r);
    const uint32_t fm = s0.m_top ^ K::MASK;
    TpRun s;
    s.target = s0.target, s.better = pass == 0 ? 0u : s0.better, s.prefix = pass == 0 ? 0u : s0.prefix;
    s.eqn = pass == 0 ? len : s0.eqn, s.done = 0, s.answer = 0, s.n = 0;
    const bool trivial = pass == 0 && tp_settle_trivial(len, p, fm, s0.m_bot, &s.n, &s.answer);
    if (trivial) {  // (workgroup-uniform) no workgroup has counted this row: its bins are zero
        s.done = 1;
    } else {
        u64 hm[PER];
        uint32_t hc[PER];
        uint4 *mq = reinterpret_cast<uint4 *>(mass_g + (u64)r * NBINS + threadIdx.x * PER);
        uint4 *cq = reinterpret_cast<uint4 *>(cnt_g + (u64)r * NBINS + threadIdx.x * PER);
#pragma unroll
        for (int q = 0; q < PER / 2; ++q) {
            const uint4 x = mq[q];
            hm[2 * q] = (u64)x.x | (u64)x.y << 32, hm[2 * q + 1] = (u64)x.z | (u64)x.w << 32;
            mq[q] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 x = cq[q];
            hc[4 * q] = x.x, hc[4 * q + 1] = x.y, hc[4 * q + 2] = x.z, hc[4 * q + 3] = x.w;
            cq[q] = make_uint4(0u, 0u, 0u, 0u);
        }
        tp_pick_digit<K, WD_BLOCK, PER>(hm, hc, pass, p, s0.nmn, s0.mx, fm, tp_row_inv_temp(v, r), K::special(fm), s,
                                        scratch, sx);
    }
    __syncthreads();  // every thread has read the state before thread 0 rewrites it
    if (threadIdx.x == 0) {
        TpState n;
        n.target = s.target, n.better = s.better, n.prefix = s.prefix, n.done = s.done, n.eqn = s.eqn;
        n.nmn = 0u, n.mx = 0u;
        n.m_top = s.done ? 0u : s0.m_top, n.m_bot = s.done ? 0u : s0.m_bot;
        *st = n;
        if (s.done) tp_write_row<K>(v, r, len, s.n, s.answer, d_n, d_thr, rank);
    }
}

// ---- fused form: one workgroup per row, pass M and every digit in this launch
template <class K, bool VEC>
__global__ __launch_bounds__(WD_FBLOCK, 2) void k_tp_fused(const typename K::elem *__restrict__ keys, u64 ld,
                                                           uint32_t cols, TopP v, int32_t *__restrict__ d_n,
                                                           typename K::elem *__restrict__ d_thr,
                                                           int32_t *__restrict__ rank) {
    constexpr int PER = NBINS / WD_FBLOCK;
    __shared__ u64 hm_s[NBINS];
    __shared__ uint32_t hc_s[NBINS];
    __shared__ uint32_t smm[2];
    __shared__ u64 scratch[WD_FBLOCK / WAVE + 3];
    __shared__ u64 sx[2];
    const u64 r = blockIdx.x;
    const typename K::elem *row = keys + r * ld;
    const uint32_t len = tp_row_len(v, r, cols);
    const float p = tp_row_p(v, r);
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
    __syncthreads();
    tp_max_range<K, VEC, WD_FBLOCK>(row, 0u, len, smm);
    __syncthreads();
    const uint32_t fm = smm[0] ^ K::MASK, bot = smm[1];
    TpRun s;
    s.target = 0, s.better = 0, s.prefix = 0, s.eqn = len, s.done = 0, s.answer = 0, s.n = 0;
    if (tp_settle_trivial(len, p, fm, bot, &s.n, &s.answer)) {  // (workgroup-uniform)
        if (threadIdx.x == 0) tp_write_row<K>(v, r, len, s.n, s.answer, d_n, d_thr, rank);
        return;
    }
    const float inv_t = tp_row_inv_temp(v, r), m = K::val(K::bits_of(fm));
    const bool special = K::special(fm);
    for (int pass = 0; pass < K::PASSES; ++pass) {
        __syncthreads();  // the reads of the bins and smm before they are zeroed
        tp_zero_lds<WD_FBLOCK>(hc_s, hm_s, smm);
        __syncthreads();
        tp_count_range<K, VEC, WD_FBLOCK>(row, 0u, len, pass, s.prefix, fm, m, inv_t, special, hc_s, hm_s, smm);
        __syncthreads();
        u64 hm[PER];
        uint32_t hc[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) hm[j] = hm_s[threadIdx.x * PER + j], hc[j] = hc_s[threadIdx.x * PER + j];
        tp_pick_digit<K, WD_FBLOCK, PER>(hm, hc, pass, p, smm[0], smm[1], fm, inv_t, special, s, scratch, sx);
        if (s.done) break;  // (workgroup-uniform)
    }
    if (threadIdx.x == 0) tp_write_row<K>(v, r, len, s.n, s.answer, d_n, d_thr, rank);
}

}  // namespace kth
