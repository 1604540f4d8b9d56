// kth_rows_wide_kernels.hpp -- the text of kth_rows_wide.hpp's kernels.  No
// include guard: kth_rows_wide.hpp includes it twice, with WD_VAR 0 for the
// uniform kernels (k_wide_count, ...) and with WD_VAR 1 for their var twins
// (k_wide_count_var, ...: one more argument, the WideVar).  As with
// kth_k16_main_body.hpp, a template parameter would change the uniform
// kernels' mangled names and a shared __device__ body changed their register
// allocation; the preprocessor leaves them the code they had
// (profiles/rows_var_device_code.txt).  WD_LEN / WD_RANK: row r's length and
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
template <bool F32, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide_count)(const uint32_t *__restrict__ keys, u64 ld,
                                                                  uint32_t cols, uint32_t slice_keys, uint32_t flip,
                                                                  int pass, uint32_t *__restrict__ hist_g,
                                                                  WideState *__restrict__ st_g WD_VAR_PARAM) {
    __shared__ uint32_t hist[NBINS];
    __shared__ uint32_t smm[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    WideState *st = st_g + r;
    uint32_t prefix = 0;
    if (pass > 0) {
        if (st->done) return;  // (workgroup-uniform) settled by an earlier digit
        prefix = st->prefix;
    }
    const uint32_t len = WD_LEN(r);
    if (WD_VAR && s * slice_keys >= len) return;  // (workgroup-uniform) a slice past its row's end
    wd_zero_lds<WD_BLOCK>(hist, smm);
    __syncthreads();
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    wd_count_range<F32, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, flip, pass, prefix, hist, smm);
    __syncthreads();
    uint32_t *row_hist = hist_g + (u64)r * NBINS;
    for (uint32_t b = threadIdx.x; b < wd_bins(pass); b += WD_BLOCK) {
        const uint32_t c = hist[b];
        if (c) (void)__hip_atomic_fetch_add(row_hist + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0 && (smm[0] | smm[1])) {
        (void)__hip_atomic_fetch_max(&st->nmn, smm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(&st->mx, smm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- split form: pick digit `pass` of every row of the group from its
// histogram, advance its state, clear the histogram and the min / max words.
// out (null for the top-k): the group's first row of the select's output.
template <bool F32>
__global__ __launch_bounds__(WD_BLOCK) void WD_K(k_wide_pick)(uint32_t *__restrict__ hist_g,
                                                              WideState *__restrict__ st_g, int pass, uint32_t cols,
                                                              uint32_t k, uint32_t flip,
                                                              uint32_t *__restrict__ out WD_VAR_PARAM) {
    constexpr int PER = NBINS / WD_BLOCK;
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
    for (int q = 0; q < PER / 4; ++q) {
        const uint4 v = hq[q];
        hv[4 * q] = v.x, hv[4 * q + 1] = v.y, hv[4 * q + 2] = v.z, hv[4 * q + 3] = v.w;
        hq[q] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();  // every thread has read the state before thread 0 rewrites it
    uint32_t done = 0, answer = 0, eqn = cnt_prev;
    if (WD_VAR && empty) {  // settled: quota 0 of the keys equal to the least order key
        done = 1;
    } else if (~s.nmn == s.mx) {  // one value fills the bin (or the row)
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
        prefix = pass == 0 ? bin : (prefix << (pass == 1 ? 11 : 10)) | bin;
        if (pass == 2) {
            done = 1;
            answer = prefix;
        }
    }
    if (threadIdx.x == 0) {
        WideState n;
        n.kk = kk, n.prefix = prefix, n.done = done, n.answer = answer, n.eqn = eqn, n.nmn = 0u, n.mx = 0u, n.pad = 0u;
        *st = n;
        if (done && out) out[r] = (WD_VAR && empty) ? 0u : WideKey<F32>::bits(answer ^ flip);
    }
}

// ---- top-k, split form: (better, equal) of every slice -> cnt_g[row][slice][2]
template <bool F32, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide_tk_count)(const uint32_t *__restrict__ keys, u64 ld,
                                                                     uint32_t cols, uint32_t slice_keys, uint32_t flip,
                                                                     const WideState *__restrict__ st_g,
                                                                     uint32_t *__restrict__ cnt_g WD_VAR_PARAM) {
    __shared__ uint32_t sc[2];
    const uint32_t r = blockIdx.y, s = blockIdx.x;
    const uint32_t answer = st_g[r].answer;
    if (threadIdx.x < 2) sc[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t len = WD_LEN(r);  // (a slice past its row's end: end <= begin, no key is loaded)
    const uint32_t begin = s * slice_keys, end = begin + slice_keys < len ? begin + slice_keys : len;
    const uint32_t *row = keys + (u64)r * ld;
    uint32_t lt = 0, eq = 0;
    for (uint32_t base = begin + threadIdx.x * 4u; base < end; base += (uint32_t)(WD_BLOCK * 4 * WD_U)) {
        uint4 x[WD_U];
#pragma unroll
        for (int u = 0; u < WD_U; ++u) x[u] = wd_load4<VEC>(row, base + (uint32_t)(u * WD_BLOCK * 4), end);
#pragma unroll
        for (int u = 0; u < WD_U; ++u) {
            const uint32_t e = base + (uint32_t)(u * WD_BLOCK * 4);
            const uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t kx = WideKey<F32>::key(w[j]) ^ flip;
                const bool in = e + (uint32_t)j < end;
                lt += (in && kx < answer) ? 1u : 0u;
                eq += (in && kx == answer) ? 1u : 0u;
            }
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
template <bool F32, bool VEC>
__global__ __launch_bounds__(WD_BLOCK, 4) void WD_K(k_wide_tk_write)(const uint32_t *__restrict__ keys, u64 ld,
                                                                     uint32_t cols, uint32_t slice_keys, uint32_t flip,
                                                                     uint32_t k, const WideState *__restrict__ st_g,
                                                                     const uint32_t *__restrict__ cnt_g,
                                                                     uint32_t *__restrict__ vals,
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
    wd_write_range<F32, VEC, WD_BLOCK>(keys + (u64)r * ld, begin, end, flip, answer, quota, lt_before + taken, want, k,
                                       vals ? vals + (u64)r * k : nullptr, idx ? idx + (u64)r * k : nullptr, wsum);
}

// ---- fused form: one workgroup per row, every digit in this launch.  A var
// row with nothing to select ends before the digits; the row's workgroup
// writes its padding and d_cnt after its compaction.
template <bool F32, bool VEC, bool TOPK>
__global__ __launch_bounds__(WD_FBLOCK, 4) void WD_K(k_wide_fused)(const uint32_t *__restrict__ keys, u64 ld,
                                                                   uint32_t cols, uint32_t k, uint32_t flip,
                                                                   uint32_t *__restrict__ out,
                                                                   uint32_t *__restrict__ vals,
                                                                   int32_t *__restrict__ idx WD_VAR_PARAM) {
    constexpr int PER = NBINS / WD_FBLOCK;
    __shared__ uint32_t hist[NBINS];
    __shared__ uint32_t smm[2];
    __shared__ u64 scratch[WD_FBLOCK / WAVE + 3];
    const u64 r = blockIdx.x;
    const uint32_t *row = keys + r * ld;
    const uint32_t len = WD_LEN(r), kr = WD_RANK(r, len, TOPK);
#if WD_VAR
    if (kr == 0u) {  // (workgroup-uniform) nothing to select
        if (TOPK) wd_pad_row<WD_FBLOCK>(v, r, 0u, k, vals ? vals + r * k : nullptr, idx ? idx + r * k : nullptr);
        else if (threadIdx.x == 0) out[r] = 0u;
        return;
    }
#endif
    uint32_t kk = kr, prefix = 0, answer = 0;
    for (int pass = 0; pass < 3; ++pass) {
        wd_zero_lds<WD_FBLOCK>(hist, smm);
        __syncthreads();
        wd_count_range<F32, VEC, WD_FBLOCK>(row, 0u, len, flip, pass, prefix, hist, smm);
        __syncthreads();
        if (~smm[0] == smm[1]) {  // (workgroup-uniform) one value fills the bin: the answer
            answer = smm[1];
            break;
        }
        u64 hv[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) hv[j] = hist[threadIdx.x * PER + j];
        uint32_t bin = 0;
        u64 below = 0;
        (void)block_pick_vals<WD_FBLOCK, PER>(hv, (u64)kk, &bin, &below, scratch);
        kk -= (uint32_t)below;
        prefix = pass == 0 ? bin : (prefix << (pass == 1 ? 11 : 10)) | bin;
        answer = prefix;
        __syncthreads();  // the reads of hist and smm before the next digit zeroes them
    }
    if (!TOPK) {
        if (threadIdx.x == 0) out[r] = WideKey<F32>::bits(answer ^ flip);
        return;
    }
    __syncthreads();
    wd_write_range<F32, VEC, WD_FBLOCK>(row, 0u, len, flip, answer, kk, 0u, kr, k, vals ? vals + r * k : nullptr,
                                        idx ? idx + r * k : nullptr, scratch);
#if WD_VAR
    wd_pad_row<WD_FBLOCK>(v, r, kr, k, vals ? vals + r * k : nullptr, idx ? idx + r * k : nullptr);
#endif
}

#undef WD_K
#undef WD_VAR_PARAM
#undef WD_LEN
#undef WD_RANK
