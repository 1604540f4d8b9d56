// kth_rows_wide16_kernels.hpp -- the text of kth_rows_wide16.hpp's kernels.  No
// include guard: kth_rows_wide16.hpp includes it twice, with WD_VAR 0 for the
// uniform kernels (k_wide16_count, ...) and with WD_VAR 1 for their var twins
// (k_wide16_count_var, ...: one more argument, the WideVar), for the reason
// written in kth_rows_wide_kernels.hpp.  WD_LEN / WD_RANK: row r's length and
// rank, `cols` and `k` in the uniform kernels.
#if WD_VAR
#define WD_K(name) name##_var
#define WD_VAR_PARAM , WideVar v
#define WD_LEN(r) wd_row_len(v, r, cols)
#define WD_RANK(r, len, topk) wd_row_rank(v, r, k, len, topk)
#else
#define WD_K(name) name
#define WD_VAR_PARAM
#define WD_LEN(r) cols
#define WD_RANK(r, len, topk) k
#endif

// ---- split form: one digit of one slice
template <int CV, bool VEC, int PASS>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide16_count)(const uint16_t *__restrict__ keys, u64 ld,
                                                                    uint32_t cols, uint32_t slice_keys, uint32_t flip2,
                                                                    uint32_t nl2, uint32_t top2,
                                                                    uint32_t *__restrict__ hist_g,
                                                                    WideState *__restrict__ st_g WD_VAR_PARAM) {
    __shared__ uint32_t hist[PASS == 0 ? NBINS : (int)W16_D1_BINS];
    __shared__ uint32_t smm[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    WideState *st = st_g + r;
    uint32_t prefix = 0;
    if (PASS > 0) {
        if (st->done) return;  // (workgroup-uniform) settled by the first digit
        prefix = st->prefix;
    }
    const uint32_t len = WD_LEN(r);
    if (WD_VAR && s * slice_keys >= len) return;  // (workgroup-uniform) a slice past its row's end
    w16_zero_lds<WD_BLOCK, PASS>(hist, smm);
    __syncthreads();
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    w16_count_range<CV, VEC, WD_BLOCK, PASS>(keys + (u64)r * ld, begin, end, flip2, nl2, top2, prefix, hist, smm);
    __syncthreads();
    uint32_t *row_hist = hist_g + (u64)r * NBINS;
    for (uint32_t b = threadIdx.x; b < (PASS == 0 ? (uint32_t)NBINS : W16_D1_BINS); b += WD_BLOCK) {
        const uint32_t c = hist[b];
        if (c) (void)__hip_atomic_fetch_add(row_hist + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (PASS == 0 && threadIdx.x == 0 && (smm[0] | smm[1])) {
        (void)__hip_atomic_fetch_max(&st->nmn, smm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(&st->mx, smm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- split form: pick digit `pass` of every row of the group from its
// histogram (pass 1: its first 32 words), advance its state, clear what it
// read and the min / max words.  out (null for the top-k): the group's first
// row of the select's output.
__global__ __launch_bounds__(WD_BLOCK) void WD_K(k_wide16_pick)(uint32_t *__restrict__ hist_g,
                                                                WideState *__restrict__ st_g, int pass, uint32_t cols,
                                                                uint32_t k, uint32_t flip2, int kind,
                                                                uint16_t *__restrict__ out WD_VAR_PARAM) {
    constexpr int PER = NBINS / WD_BLOCK;
    static_assert(PER % 4 == 0 && W16_D1_BINS % PER == 0, "whole threads own the second digit's bins");
    __shared__ u64 scratch[WD_BLOCK / WAVE + 3];
    __shared__ uint32_t s_cnt;
    const uint32_t r = blockIdx.x;
    WideState *st = st_g + r;
    const WideState s = *st;
    if (pass > 0 && s.done) return;  // (workgroup-uniform)
    uint32_t kk = pass == 0 ? k : s.kk, prefix = pass == 0 ? 0u : s.prefix;
    const uint32_t cnt_prev = pass == 0 ? WD_LEN(r) : s.eqn;
    if (WD_VAR && pass == 0) kk = WD_RANK(r, cnt_prev, out == nullptr);
    const bool empty = WD_VAR && pass == 0 && kk == 0u;  // (workgroup-uniform) a var row with nothing to select
    uint4 *hq = reinterpret_cast<uint4 *>(hist_g + (u64)r * NBINS + threadIdx.x * PER);
    u64 hv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) hv[j] = 0;
    if (pass == 0 || threadIdx.x * PER < W16_D1_BINS) {
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 v = hq[q];
            hv[4 * q] = v.x, hv[4 * q + 1] = v.y, hv[4 * q + 2] = v.z, hv[4 * q + 3] = v.w;
            hq[q] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    __syncthreads();  // every thread has read the state before thread 0 rewrites it
    uint32_t done = 0, answer = 0, eqn = cnt_prev;
    if (WD_VAR && empty) {  // settled: quota 0 of the keys equal to the least ord
        done = 1;
    } else if (pass == 0 && (s.nmn ^ 0xFFFFu) == s.mx) {  // one value fills the row
        done = 1;
        answer = s.mx;
    } else {
        uint32_t bin = 0;
        u64 below = 0;
        (void)block_pick_vals<WD_BLOCK, PER>(hv, (u64)kk, &bin, &below, scratch);
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (threadIdx.x * PER + j == bin) s_cnt = (uint32_t)hv[j];
        __syncthreads();
        eqn = s_cnt;
        kk -= (uint32_t)below;
        prefix = pass == 0 ? bin : (prefix << W16_D1_BITS) | bin;
        if (pass == 1) {
            done = 1;
            answer = prefix;
        }
    }
    if (threadIdx.x == 0) {
        WideState n;
        n.kk = kk, n.prefix = prefix, n.done = done, n.answer = answer, n.eqn = eqn, n.nmn = 0u, n.mx = 0u, n.pad = 0u;
        *st = n;
        if (done && out) out[r] = (WD_VAR && empty) ? (uint16_t)0 : k16_bits_of_ord((answer ^ flip2) & 0xFFFFu, kind);
    }
}

// ---- top-k, split form: (better, equal) of every slice -> cnt_g[row][slice][2]
template <int CV, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide16_tk_count)(const uint16_t *__restrict__ keys, u64 ld,
                                                                       uint32_t cols, uint32_t slice_keys,
                                                                       uint32_t flip2, uint32_t nl2, uint32_t top2,
                                                                       const WideState *__restrict__ st_g,
                                                                       uint32_t *__restrict__ cnt_g WD_VAR_PARAM) {
    __shared__ uint32_t sc[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t answer = st_g[r].answer;
    if (threadIdx.x < 2) sc[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t len = WD_LEN(r);  // (a slice past its row's end: end <= begin, no key is loaded)
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    const uint16_t *row = keys + (u64)r * ld;
    uint32_t lt = 0, eq = 0;
    for (uint32_t base = begin + threadIdx.x * 8u; base < end; base += (uint32_t)(WD_BLOCK * 8 * WD_U)) {
        uint4 x[WD_U];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) x[u] = w16_load8<VEC>(row, base + (uint32_t)(u * WD_BLOCK * 8), end);
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const uint4 o = k16_ord8<CV>(x[u], nl2, top2);
            const uint32_t w[4] = {o.x ^ flip2, o.y ^ flip2, o.z ^ flip2, o.w ^ flip2};
            w16_cmp8(w, base + (uint32_t)(u * WD_BLOCK * 8), end, answer, lt, eq);
        }
    }
    lt = wd_wave_sum(lt);
    eq = wd_wave_sum(eq);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        (void)__hip_atomic_fetch_add(sc, lt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_add(sc + 1, eq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (threadIdx.x < 2) cnt_g[((u64)r * gridDim.x + s) * 2u + threadIdx.x] = sc[threadIdx.x];
}

// ---- top-k, split form: each slice's offset and quota share from the slices
// before it, then the ordered compaction of the slice.  vals / idx: the group's
// first row of the outputs (rows x k), either may be null.  A var call's slice
// 0 also writes the row's padding and its d_cnt, before anything can end the
// workgroup.
template <int CV, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide16_tk_write)(const uint16_t *__restrict__ keys, u64 ld,
                                                                       uint32_t cols, uint32_t slice_keys,
                                                                       uint32_t flip2, uint32_t nl2, uint32_t top2,
                                                                       int kind, uint32_t k,
                                                                       const WideState *__restrict__ st_g,
                                                                       const uint32_t *__restrict__ cnt_g,
                                                                       uint16_t *__restrict__ vals,
                                                                       int32_t *__restrict__ idx WD_VAR_PARAM) {
    __shared__ u64 wsum[WD_BLOCK / WAVE];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t len = WD_LEN(r);
#if WD_VAR
    if (s == 0)
        wd_pad_row<WD_BLOCK>(v, r, WD_RANK(r, len, true), k, vals ? vals + (u64)r * k : nullptr,
                             idx ? idx + (u64)r * k : nullptr);
#endif
    const uint32_t answer = st_g[r].answer, kk = st_g[r].kk;
    const uint32_t *cnt = cnt_g + (u64)r * gridDim.x * 2u;
    u64 mine = 0;
    if (threadIdx.x < s) mine = (u64)cnt[2u * threadIdx.x] | (u64)cnt[2u * threadIdx.x + 1u] << 32;
    u64 before;
    (void)block_exclusive_scan<WD_BLOCK>(mine, wsum, &before);
    const uint32_t lt_before = (uint32_t)before, eq_before = (uint32_t)(before >> 32);
    const uint32_t taken = eq_before < kk ? eq_before : kk, quota = kk - taken;
    const uint32_t my_lt = cnt[2u * s], my_eq = cnt[2u * s + 1u];
    const uint32_t want = my_lt + (my_eq < quota ? my_eq : quota);
    if (want == 0) return;  // (workgroup-uniform) nothing of this slice is kept
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    w16_write_range<CV, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, flip2, nl2, top2, kind, answer, quota,
                                       lt_before + taken, want, k, vals ? vals + (u64)r * k : nullptr,
                                       idx ? idx + (u64)r * k : nullptr, wsum);
}

// ---- fused form: one workgroup per row, both digits in this launch.  A var
// row with nothing to select ends before the digits; the row's workgroup
// writes its padding and d_cnt after its compaction.
template <int CV, bool VEC, bool TOPK>
__global__ __launch_bounds__(WD_FBLOCK, 4) void WD_K(k_wide16_fused)(const uint16_t *__restrict__ keys, u64 ld,
                                                                     uint32_t cols, uint32_t k, uint32_t flip2,
                                                                     uint32_t nl2, uint32_t top2, int kind,
                                                                     uint16_t *__restrict__ out,
                                                                     uint16_t *__restrict__ vals,
                                                                     int32_t *__restrict__ idx WD_VAR_PARAM) {
    constexpr int PER = NBINS / WD_FBLOCK;
    static_assert(W16_D1_BINS % PER == 0, "whole threads own the second digit's bins");
    __shared__ uint32_t hist[NBINS];
    __shared__ uint32_t smm[2];
    __shared__ u64 scratch[WD_FBLOCK / WAVE + 3];
    const u64 r = blockIdx.x;
    const uint16_t *row = keys + r * ld;
    const uint32_t len = WD_LEN(r), kr = WD_RANK(r, len, TOPK);
#if WD_VAR
    if (kr == 0u) {  // (workgroup-uniform) nothing to select
        if (TOPK) wd_pad_row<WD_FBLOCK>(v, r, 0u, k, vals ? vals + r * k : nullptr, idx ? idx + r * k : nullptr);
        else if (threadIdx.x == 0) out[r] = (uint16_t)0;
        return;
    }
#endif
    uint32_t kk = kr, answer = 0;
    w16_zero_lds<WD_FBLOCK, 0>(hist, smm);
    __syncthreads();
    w16_count_range<CV, VEC, WD_FBLOCK, 0>(row, 0u, len, flip2, nl2, top2, 0u, hist, smm);
    __syncthreads();
    if ((smm[0] ^ 0xFFFFu) == smm[1]) {  // (workgroup-uniform) one value fills the row: the answer
        answer = smm[1];
    } else {
        u64 hv[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) hv[j] = hist[threadIdx.x * PER + j];
        uint32_t bin = 0;
        u64 below = 0;
        (void)block_pick_vals<WD_FBLOCK, PER>(hv, (u64)kk, &bin, &below, scratch);
        kk -= (uint32_t)below;
        const uint32_t prefix = bin;
        __syncthreads();  // the reads of hist before the second digit zeroes it
        w16_zero_lds<WD_FBLOCK, 1>(hist, smm);
        __syncthreads();
        w16_count_range<CV, VEC, WD_FBLOCK, 1>(row, 0u, len, flip2, nl2, top2, prefix, hist, smm);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j)
            hv[j] = threadIdx.x * PER + j < W16_D1_BINS ? hist[threadIdx.x * PER + j] : 0u;
        (void)block_pick_vals<WD_FBLOCK, PER>(hv, (u64)kk, &bin, &below, scratch);
        kk -= (uint32_t)below;
        answer = (prefix << W16_D1_BITS) | bin;
    }
    if (!TOPK) {
        if (threadIdx.x == 0) out[r] = k16_bits_of_ord((answer ^ flip2) & 0xFFFFu, kind);
        return;
    }
    __syncthreads();
    w16_write_range<CV, VEC, WD_FBLOCK>(row, 0u, len, flip2, nl2, top2, kind, answer, kk, 0u, kr, k,
                                        vals ? vals + r * k : nullptr, idx ? idx + r * k : nullptr, scratch);
#if WD_VAR
    wd_pad_row<WD_FBLOCK>(v, r, kr, k, vals ? vals + r * k : nullptr, idx ? idx + r * k : nullptr);
#endif
}

#undef WD_K
#undef WD_VAR_PARAM
#undef WD_LEN
#undef WD_RANK
