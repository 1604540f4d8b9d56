// kth_rows_sample.hpp -- one token per row drawn from the top-k / top-p
// filtered distribution (include/kth.h "wide rows, sampling").  Drawing is the
// weighted select the nucleus is: with the row ordered largest first, ties by
// column, the token for a uniform number u is the first key at which the
// running mass passes u * S(n), n the number of kept keys.
//
// Everything a key weighs comes from kth_rows_topp.hpp: the order keys (fk,
// flipped), tp_wfix (the one weight rule), tp_walk / tp_count_range (the
// weighted digit pass) and the fixed-point integer sums, so n is the nucleus's
// n bit for bit wherever the cap does not bind, and every result is the same
// number whatever the plan, the load path or the run.
//
// Per row, after pass M (the row's top and bottom key):
//   descent A  how many keys are kept, and their mass.  The nucleus's digit
//          passes with a pick that follows two targets at once, the remaining
//          mass (tp_target) and the remaining count (the cap): the first bin
//          at which either running sum reaches its target is picked, and both
//          targets are reduced by what lies before it.  Carried besides the
//          nucleus's state: `before`, the mass of the keys before every key
//          matching the prefix.  At the threshold value, of weight wf,
//            q = min(ceil(mass left / wf), count left, keys equal),
//            n = better + q,  S_fix(n) = before + q * wf.
//          A bin picked by the count alone may weigh nothing (wf == 0: the
//          mass is not reached inside it); then q = min(count left, equal).
//          Rows that need no descent A: len == 0 (n = 0); p <= 0 (n = 1,
//          S_fix = 2^39); p >= 1 with no binding cap (n = len, S_fix(n) = Z,
//          which descent B's first digit produces).  p >= 1 with a binding cap
//          follows the count alone (the mass target is never reached).
//   descent B  where u lands: t = min(S_fix(n), floor(u * S_fix(n)) + 1), one
//          thread in double, then the same passes by mass only to the least j
//          with S_fix(j) >= t.  It yields the threshold value and the ordinal
//          q_B = ceil(mass left / wf) among the keys equal to it.  t >= 1, so a
//          picked bin and the threshold always weigh something; t <= S_fix(n),
//          so j <= n by integer arithmetic.
//   locate     the column of the q_B-th key, by column, equal to the
//          threshold within len: counts of equal keys per tile (fused) or per
//          slice (split, plain stores to scratch, then after the kernel
//          boundary the slice whose range holds the ordinal), and an ordered
//          block scan.
// A row whose top key is +inf or NaN is settled by the first digit of each
// descent as in the nucleus: the keys equal to it weigh 2^39, all others 0.
//
// Two forms, by kth_rows_wide.hpp's plan.  Split: k_sm_max, per digit of each
// descent k_sm_count (grid slices x group rows) and k_sm_pick (one workgroup a
// row), then k_sm_loc_count and k_sm_loc_pick, each after a kernel boundary: no
// cooperative launch, no grid barrier, no in-launch flag.  Fused: k_sm_fused,
// one 512-thread workgroup a row, everything in one launch.
//
// Scratch (split form): the top-p calls' bins (2048 u64 masses and 2048 u32
// counts a row, left zero by every pick), and of its own a SmState a row and a
// u32 per row and slice.  A sequence leaves the state's accumulating words
// (nmn, mx, m_top, m_bot) zero; its other words are rewritten before they are
// read.
// Included by kth_kernels.hip after kth_rows_topp16.hpp.
#pragma once

namespace kth {

constexpr uint32_t SM_NO_CAP = 0xFFFFFFFFu;
constexpr u64 SM_NO_MASS = ~0ull;  // a mass target that no sum reaches (sums stay at or below 2^63)

// A row's selection in registers (workgroup-uniform), and, with the words the
// counting kernels accumulate into, its state between the kernels of the split
// form.
struct SmRun {
    u64 tm;       // the fixed-point mass still to reach among the keys matching `prefix`
    u64 before;   // the mass of the keys before every key matching `prefix`
    u64 sn;       // S_fix(n), once descent A is over; 0: Z, which descent B's first digit sets
    uint32_t tc;  // the count still to reach (descent A; SM_NO_CAP: none)
    uint32_t better, prefix, eqn;
    uint32_t done, answer;  // the descent is over: the threshold (fk)
    uint32_t q;             // ... and how many of the keys equal to it are taken
    uint32_t n;             // descent A: the number of kept keys
};
struct SmState {
    SmRun s;
    uint32_t nmn, mx;       // max(fk ^ MASK), max(fk) of the keys matching `prefix`
    uint32_t m_top, m_bot;  // pass M: max(fk ^ MASK), max(fk) of the row
};
constexpr int SM_STATE_BYTES = sizeof(SmState);

// c_r: <= 0 is "no cap" (the sampler's "top-k off")
__device__ __forceinline__ uint32_t sm_row_cap(const TopP &v, u64 r) {
    const int32_t q = v.ks ? v.ks[r] : v.k;
    return q <= 0 ? SM_NO_CAP : (uint32_t)q;
}
// u_r: NaN or a negative value counts as 0
__device__ __forceinline__ float sm_row_u(const float *__restrict__ us, u64 r) {
    const float u = us[r];
    return u > 0.0f ? u : 0.0f;
}
// (workgroup-uniform) a row that needs no descent A
__device__ __forceinline__ bool sm_skip_a(uint32_t len, float p, uint32_t cap) {
    return len == 0u || p <= 0.0f || (p >= 1.0f && cap >= len);
}
// t = min(S_fix(n), floor(u * S_fix(n)) + 1)
__device__ __forceinline__ u64 sm_target(float u, u64 sn) {
    if (u >= 1.0f) return sn;
    const u64 t = (u64)floor((double)u * (double)sn) + 1ull;
    return t < sn ? t : sn;
}
// tp_ties for a target that may be SM_NO_MASS and a weight that may be 0
__device__ __forceinline__ uint32_t sm_ties(u64 remaining, u64 wf, uint32_t eq) {
    if (!wf) return eq;
    const u64 q = remaining / wf + (remaining % wf ? 1ull : 0ull);
    return q < 1 ? 1u : q < eq ? (uint32_t)q : eq;
}

// The end of a descent at threshold `answer`, whose keys weigh wf each.
__device__ __forceinline__ void sm_finish(SmRun &s, int phase, uint32_t answer, u64 wf) {
    const uint32_t qm = sm_ties(s.tm, wf, s.eqn);
    s.answer = answer;
    s.q = qm < s.tc ? qm : s.tc;
    if (phase == 0) {
        s.n = s.better + s.q;
        s.sn = s.before + (u64)s.q * wf;
    }
    s.done = 1;
}

// One digit's pick of descent `phase` (0: A, 1: B).  Thread t holds bins [t *
// PER, t * PER + PER): masses hm, counts hc.  nmn / mx: the matching keys'
// max(fk ^ MASK) / max(fk).  Pass 0 derives the mass target from Z.  scratch:
// BLOCK / 64 words, sx: 4 words (LDS).
template <class K, int BLOCK, int PER>
__device__ __forceinline__ void sm_pick_digit(const u64 (&hm)[PER], const uint32_t (&hc)[PER], int pass, int phase,
                                              float p, float u, uint32_t nmn, uint32_t mx, uint32_t fm, float inv_t,
                                              bool special, SmRun &s, u64 *scratch, u64 *sx) {
    const float m = K::val(K::bits_of(fm));
    u64 msum = 0;
    uint32_t csum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) msum += hm[j], csum += hc[j];
    u64 z;
    const u64 mpre = block_exclusive_scan<BLOCK>(msum, scratch, &z);
    if (pass == 0) {
        if (threadIdx.x == 0)  // once per row and descent, by one thread
            sx[0] = phase == 0 ? (p >= 1.0f ? SM_NO_MASS : tp_target(p, z)) : sm_target(u, s.sn ? s.sn : z);
        __syncthreads();
        s.tm = sx[0];
        __syncthreads();
        if (phase == 1 && !s.sn) s.sn = z;
        if (special && s.tm != SM_NO_MASS) {  // the keys equal to m weigh TP_ONE, every other key 0
            s.eqn = (uint32_t)(z >> TP_FRAC);
            sm_finish(s, phase, fm, TP_ONE);
            return;
        }
    }
    if ((nmn ^ K::MASK) == mx) {  // one value fills the bin (or the row): the threshold
        sm_finish(s, phase, mx, tp_wfix(mx, K::val(K::bits_of(mx)), fm, m, inv_t, special));
        return;
    }
    const u64 cpre = block_exclusive_scan<BLOCK>((u64)csum, scratch, nullptr);
    if (threadIdx.x == 0) sx[0] = ~0ull;
    __syncthreads();
    // the first bin at which the running mass or the running count reaches its target
    u64 cm = mpre, mb = 0;
    uint32_t cc = (uint32_t)cpre, cb = 0, ce = 0, mine = ~0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        cm += hm[j], cc += hc[j];
        if (mine == ~0u && (cm >= s.tm || cc >= s.tc))
            mine = threadIdx.x * (uint32_t)PER + (uint32_t)j, mb = cm - hm[j], cb = cc - hc[j], ce = hc[j];
    }
    if (mine != ~0u) (void)__hip_atomic_fetch_min(sx, (u64)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const uint32_t bin = (uint32_t)sx[0];
    if (mine == bin) sx[1] = mb, sx[2] = cb, sx[3] = ce;
    __syncthreads();
    const u64 below = sx[1];
    const uint32_t cbelow = (uint32_t)sx[2];
    s.eqn = (uint32_t)sx[3];
    __syncthreads();
    s.better += cbelow;
    s.before += below;
    s.tm -= below;
    s.tc -= cbelow;
    s.prefix = pass == 0 ? bin : (s.prefix << K::dbits(pass)) | bin;
    if (pass == K::PASSES - 1)  // the bin is one value
        sm_finish(s, phase, s.prefix, tp_wfix(s.prefix, K::val(K::bits_of(s.prefix)), fm, m, inv_t, special));
}

// A descent's start.  Descent A of a row that needs none is over at once.
__device__ __forceinline__ void sm_begin(SmRun &s, int phase, uint32_t len, float p, uint32_t cap) {
    s.tm = 0, s.before = 0, s.better = 0, s.prefix = 0, s.eqn = len, s.done = 0, s.answer = 0, s.q = 0;
    if (phase == 0) {
        s.tc = cap, s.n = 0, s.sn = 0;
    } else {
        s.tc = SM_NO_CAP;
        if (sm_skip_a(len, p, cap)) {
            s.n = len == 0u ? 0u : p <= 0.0f ? 1u : len;
            s.sn = p <= 0.0f ? TP_ONE : 0;
        }
    }
}

// The column of the ord-th (1-based) key equal to `thr` among columns [begin,
// end) (begin % K::PER == 0), by column; stored by the one thread that holds it.
// wsum: BLOCK / 64 words of LDS.
template <class K, bool VEC, int BLOCK>
__device__ __forceinline__ void sm_locate(const typename K::elem *__restrict__ row, uint32_t begin, uint32_t end,
                                          uint32_t thr, uint32_t ord, int32_t *__restrict__ tok, u64 *wsum) {
    uint32_t run = 0;  // workgroup-uniform: equal keys before this tile
    for (uint32_t cb = begin; cb < end; cb += (uint32_t)(BLOCK * K::PER)) {
        const uint32_t e = cb + threadIdx.x * (uint32_t)K::PER;
        const uint4 x = K::template load<VEC>(row, e, end);
        uint32_t cnt = 0;
        K::each(x, e, end, [&](uint32_t fk, float) { cnt += fk == thr ? 1u : 0u; });
        u64 total;
        const uint32_t pre = run + (uint32_t)block_exclusive_scan<BLOCK>((u64)cnt, wsum, &total);
        if (cnt && pre < ord && ord <= pre + cnt) {
            uint32_t c = pre, j = 0;
            K::each(x, e, end, [&](uint32_t fk, float) {
                if (fk == thr && ++c == ord) *tok = (int32_t)(e + j);
                ++j;
            });
        }
        run += (uint32_t)total;
        if (run >= ord) break;
    }
}

// ---- split form: pass M of one slice
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_sm_max(const typename K::elem *__restrict__ keys, u64 ld, uint32_t cols,
                                                        uint32_t slice_keys, SmState *__restrict__ st_g, TopP v) {
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

// ---- split form: one weighted digit of one slice, descent `phase`
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_sm_count(const typename K::elem *__restrict__ keys, u64 ld,
                                                          uint32_t cols, uint32_t slice_keys, int phase, int pass,
                                                          u64 *__restrict__ mass_g, uint32_t *__restrict__ cnt_g,
                                                          SmState *__restrict__ st_g, TopP v) {
    __shared__ u64 hm[NBINS];
    __shared__ uint32_t hc[NBINS];
    __shared__ uint32_t smm[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    SmState *st = st_g + r;
    const uint32_t len = tp_row_len(v, r, cols);
    if (s * slice_keys >= len) return;  // (workgroup-uniform)
    if (phase == 0 && sm_skip_a(len, tp_row_p(v, r), sm_row_cap(v, r))) return;  // (workgroup-uniform)
    uint32_t prefix = 0;
    if (pass > 0) {
        if (st->s.done) return;  // (workgroup-uniform) this descent was over at an earlier pick
        prefix = st->s.prefix;
    }
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

// ---- split form: pick digit `pass` of descent `phase` for every row of the
// group, advance its state, clear its bins and min / max words.  The pick that
// ends descent B clears pass M's words.
template <class K>
__global__ __launch_bounds__(WD_BLOCK) void k_sm_pick(u64 *__restrict__ mass_g, uint32_t *__restrict__ cnt_g,
                                                      SmState *__restrict__ st_g, int phase, int pass, uint32_t cols,
                                                      TopP v, const float *__restrict__ us) {
    constexpr int PER = NBINS / WD_BLOCK;
    __shared__ u64 scratch[WD_BLOCK / WAVE];
    __shared__ u64 sx[4];
    const uint32_t r = blockIdx.x;
    SmState *st = st_g + r;
    const SmState s0 = *st;
    const uint32_t len = tp_row_len(v, r, cols);
    const float p = tp_row_p(v, r);
    const uint32_t cap = sm_row_cap(v, r);
    const bool skip_a = sm_skip_a(len, p, cap);
    if (phase == 0 && skip_a) return;          // (workgroup-uniform) nothing was counted, nothing is kept
    if (pass > 0 && s0.s.done) return;         // (workgroup-uniform)
    const uint32_t fm = s0.m_top ^ K::MASK;
    SmRun s = s0.s;
    if (pass == 0) {
        const SmRun a = s;
        sm_begin(s, phase, len, p, cap);
        if (phase == 1 && !skip_a) s.n = a.n, s.sn = a.sn;
    }
    if (len == 0u) {  // (workgroup-uniform; descent B's first pick) no workgroup has counted this row
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
        sm_pick_digit<K, WD_BLOCK, PER>(hm, hc, pass, phase, p, phase ? sm_row_u(us, r) : 0.0f, s0.nmn, s0.mx, fm,
                                        tp_row_inv_temp(v, r), K::special(fm), s, scratch, sx);
    }
    __syncthreads();  // every thread has read the state before thread 0 rewrites it
    if (threadIdx.x == 0) {
        SmState n;
        n.s = s;
        n.nmn = 0u, n.mx = 0u;
        const bool over = phase == 1 && s.done;
        n.m_top = over ? 0u : s0.m_top, n.m_bot = over ? 0u : s0.m_bot;
        *st = n;
    }
}

// ---- split form: the keys of one slice equal to the threshold (plain stores;
// every slice of every row stores, a slice past its row's end stores 0)
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_sm_loc_count(const typename K::elem *__restrict__ keys, u64 ld,
                                                              uint32_t cols, uint32_t slice_keys,
                                                              const SmState *__restrict__ st_g,
                                                              uint32_t *__restrict__ loc_g, TopP v) {
    __shared__ uint32_t tot;
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t len = tp_row_len(v, r, cols);
    const uint32_t thr = st_g[r].s.answer;
    if (threadIdx.x == 0) tot = 0u;
    __syncthreads();
    const uint32_t begin = s * slice_keys;
    if (begin < len) {  // (workgroup-uniform)
        const uint32_t end = begin + slice_keys < len ? begin + slice_keys : len;
        uint32_t cnt = 0;
        tp_walk<K, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, [&](uint32_t fk, float) { cnt += fk == thr ? 1u : 0u; });
        cnt = wd_wave_sum(cnt);
        if ((threadIdx.x & (WAVE - 1)) == 0 && cnt)
            (void)__hip_atomic_fetch_add(&tot, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (threadIdx.x == 0) loc_g[(u64)r * gridDim.x + s] = tot;
}

// ---- split form: the slice whose range of equal keys holds the ordinal finds
// the column; slice 0 writes d_cnt and an empty row's token.  d_tok, d_cnt: the
// group's first row.
template <class K, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void k_sm_loc_pick(const typename K::elem *__restrict__ keys, u64 ld,
                                                             uint32_t cols, uint32_t slice_keys,
                                                             const SmState *__restrict__ st_g,
                                                             const uint32_t *__restrict__ loc_g, TopP v,
                                                             int32_t *__restrict__ d_tok, int32_t *__restrict__ d_cnt) {
    __shared__ u64 wsum[WD_BLOCK / WAVE];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t len = tp_row_len(v, r, cols);
    const uint32_t thr = st_g[r].s.answer, ord = st_g[r].s.q;
    if (s == 0u && threadIdx.x == 0) {
        if (d_cnt) d_cnt[r] = (int32_t)st_g[r].s.n;
        if (len == 0u) d_tok[r] = -1;
    }
    const uint32_t begin = s * slice_keys;
    if (begin >= len) return;  // (workgroup-uniform)
    uint32_t pre = 0;
    for (uint32_t i = 0; i < s; ++i) pre += loc_g[(u64)r * gridDim.x + i];
    const uint32_t mine = loc_g[(u64)r * gridDim.x + s];
    if (ord <= pre || ord > pre + mine) return;  // (workgroup-uniform)
    const uint32_t end = begin + slice_keys < len ? begin + slice_keys : len;
    sm_locate<K, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, thr, ord - pre, d_tok + r, wsum);
}

// ---- fused form: one workgroup per row, everything in this launch
template <class K, bool VEC>
__global__ __launch_bounds__(WD_FBLOCK, 2) void k_sm_fused(const typename K::elem *__restrict__ keys, u64 ld,
                                                           uint32_t cols, TopP v, const float *__restrict__ us,
                                                           int32_t *__restrict__ d_tok, int32_t *__restrict__ d_cnt) {
    constexpr int PER = NBINS / WD_FBLOCK;
    __shared__ u64 hm_s[NBINS];
    __shared__ uint32_t hc_s[NBINS];
    __shared__ uint32_t smm[2];
    __shared__ u64 scratch[WD_FBLOCK / WAVE];
    __shared__ u64 sx[4];
    const u64 r = blockIdx.x;
    const typename K::elem *row = keys + r * ld;
    const uint32_t len = tp_row_len(v, r, cols);
    if (len == 0u) {  // (workgroup-uniform)
        if (threadIdx.x == 0) {
            d_tok[r] = -1;
            if (d_cnt) d_cnt[r] = 0;
        }
        return;
    }
    const float p = tp_row_p(v, r), u = sm_row_u(us, r);
    const uint32_t cap = sm_row_cap(v, r);
    if (threadIdx.x < 2) smm[threadIdx.x] = 0u;
    __syncthreads();
    tp_max_range<K, VEC, WD_FBLOCK>(row, 0u, len, smm);
    __syncthreads();
    const uint32_t fm = smm[0] ^ K::MASK;
    const float inv_t = tp_row_inv_temp(v, r), m = K::val(K::bits_of(fm));
    const bool special = K::special(fm);
    SmRun s;
    s.n = 0, s.sn = 0;
    for (int phase = sm_skip_a(len, p, cap) ? 1 : 0; phase < 2; ++phase) {
        const uint32_t n = s.n;
        const u64 sn = s.sn;
        sm_begin(s, phase, len, p, cap);
        if (phase == 1 && !sm_skip_a(len, p, cap)) s.n = n, s.sn = sn;
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
            sm_pick_digit<K, WD_FBLOCK, PER>(hm, hc, pass, phase, p, u, smm[0], smm[1], fm, inv_t, special, s, scratch,
                                             sx);
            if (s.done) break;  // (workgroup-uniform)
        }
    }
    if (threadIdx.x == 0 && d_cnt) d_cnt[r] = (int32_t)s.n;
    sm_locate<K, VEC, WD_FBLOCK>(row, 0u, len, s.answer, s.q, d_tok + r, scratch);
}

}  // namespace kth
