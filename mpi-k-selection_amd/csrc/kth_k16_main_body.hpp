// kth_k16_main_body.hpp -- the text of kth_k16.hpp's streaming kernel.  No
// include guard: kth_k16.hpp includes it twice, with K16_MAIN_TF 0 for
// k16_main<CV> and with K16_MAIN_TF 1 for k16_main_tf<CV>, the flag-recording
// pass 0 of kth_topk_k16.  (A template parameter with a default would change
// k16_main<CV>'s mangled name, and a shared __device__ body changed its
// register allocation; the preprocessor leaves k16_main<CV> the tokens it had,
// so its device code is the merged one: profiles/topk16_device_code.txt.)
template <int CV>
#if K16_MAIN_TF
__global__ __launch_bounds__(BLK) void k16_main_tf(K16Args a, K16Flags f) {
#else
__global__ __launch_bounds__(BLK) void k16_main(K16Args a) {
#endif
    constexpr int U = K16_UNROLL, NW = BLK / WAVE;
    __shared__ uint32_t lh[K16_LDS_WORDS];
    __shared__ K16Win win[MULTI_MAX];
    // a wave's words per window: keys below it; keys added since its last flush, their first and last field
    __shared__ uint32_t wst[NW][MULTI_MAX][4];
    static_assert(U * 8 * WAVE + K16_WAVE_BUDGET <= 0xFFFFu / NW, "a field holds what NW waves add between flushes");
    const int D = a.D < MULTI_MAX ? a.D : MULTI_MAX;
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    if ((int)threadIdx.x < D) {
        const K16State s = a.st[threadIdx.x];
        K16Win w;
        w.lay = k16_layout(s.lo, s.hi, s.C);
        w.active = s.mode == K16_ACTIVE ? 1u : 0u;
        w.base = (uint32_t)threadIdx.x * (s.C + (uint32_t)K16_COARSE / 2u);
        if (w.base + (w.lay.nb + 1u) / 2u > (uint32_t)K16_LDS_WORDS) w.active = 0u;  // (cannot happen: k16_finish reports the rank)
        win[threadIdx.x] = w;
    }
    for (int i = threadIdx.x; i < K16_LDS_WORDS; i += BLK) lh[i] = 0u;
    if (threadIdx.x < NW * MULTI_MAX * 4) (&wst[0][0][0])[threadIdx.x] = (threadIdx.x & 3) == 2 ? ~0u : 0u;
    __syncthreads();
    bool any = false;
    for (int j = 0; j < D; ++j) any |= win[j].active != 0u;
#if K16_MAIN_TF
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the window this pass uses, and whether it runs
        f.hdr[0] = win[0].lay.lo;
        f.hdr[1] = win[0].lay.hi;
        f.hdr[2] = any ? 1u : 0u;
    }
#endif
    if (!any) return;  // block-uniform: every rank is settled

    const uint16_t *p = a.keys;
    const u64 n = a.n;
    u64 head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 1;
    if (head > n) head = n;
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(p + head);
    const u64 nv = (n - head) >> 3, tail0 = head + (nv << 3);
    const u64 tile = (u64)BLK * U, nfull = nv / tile;
    const uint32_t nl2 = a.nl2, top2 = a.top2;

    // One window's state while a wave scans keys: wave-uniform.
    struct WaveWin {
        uint32_t lo, hi, lt;
        uint32_t in, fmin, fmax;  // since the wave's last flush: keys added, the fields they may lie in
        K16Lay lay;               // (in SGPRs: the bin of a key costs no LDS read)
        uint32_t base;
    };
    // a key slot some lane's key of which lies in the window (mask N)
    auto near_slot = [&](int j, WaveWin &s, uint32_t x, unsigned long long N) __attribute__((always_inline)) {
        uint32_t *h = lh + s.base;
        const uint32_t f = s.lay.narrow ? x - s.lo : k16_bin(s.lay, x);  // (wave-uniform choice)
        const uint32_t c = (uint32_t)__popcll(N);
        s.in += c;
        if (c >= 8u) {  // keys that share a bin: one add of their count
#pragma unroll 1
            for (int r = 0; r < K16_LEADER_ROUNDS && N; ++r) {
                const int src = __builtin_ctzll(N);
                const uint32_t f0 = (uint32_t)__builtin_amdgcn_readlane((int)f, src);
                const unsigned long long eq = __builtin_amdgcn_ballot_w64(f == f0) & N;
                if (lane == src) k16_add_field(h, f0, (uint32_t)__popcll(eq));
                s.fmin = f0 < s.fmin ? f0 : s.fmin;
                s.fmax = f0 > s.fmax ? f0 : s.fmax;
                N &= ~eq;
            }
        }
        if (N) {  // wave-uniform
            if ((N >> lane) & 1ull) k16_add_field(h, f, 1u);
            s.fmin = 0u;
            s.fmax = s.lay.nb - 1u;
        }
    };
    // the wave swaps the fields [fmin, fmax] of window j out, into the global bins
    auto wave_flush = [&](int j, WaveWin &s) __attribute__((always_inline)) {
        u64 *gb = a.bins + (size_t)j * K16_RANK_WORDS;
        for (uint32_t i = (s.fmin >> 1) + lane; i <= (s.fmax >> 1); i += WAVE) {
            const uint32_t t = atomicExch(&lh[s.base + i], 0u);
            if (t) k16_flush_word(gb, 2u * i, t);
        }
        s.in = 0u;
        s.fmin = ~0u;
        s.fmax = 0u;
    };
    // (ballots are taken of plain compares only and combined as scalar masks)
    // one key a lane; a lane without a key passes ~0u, which no window counts
    auto key_slot = [&](int j, WaveWin &s, uint32_t x) __attribute__((always_inline)) {
        const unsigned long long LT = __builtin_amdgcn_ballot_w64(x < s.lo);
        const unsigned long long N = __builtin_amdgcn_ballot_w64(x <= s.hi) & ~LT;
        s.lt += (uint32_t)__popcll(LT);
        if (__builtin_expect(N != 0, 0)) near_slot(j, s, x, N);
    };
    // Four keys (two packed words) of the lanes in okm: the eight compares
    // first, then the scalar work (as k_main_multi's key_group; eight keys'
    // masks at once do not fit the SGPRs).
    auto key_group = [&](int j, WaveWin &s, uint32_t w0, uint32_t w1, unsigned long long okm) __attribute__((always_inline)) {
        const uint32_t k[4] = {w0 & 0xFFFFu, w0 >> 16, w1 & 0xFFFFu, w1 >> 16};
        unsigned long long LT[4], N[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            LT[i] = __builtin_amdgcn_ballot_w64(k[i] < s.lo);
            N[i] = __builtin_amdgcn_ballot_w64(k[i] <= s.hi);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s.lt += (uint32_t)__popcll(LT[i] & okm);
            const unsigned long long nn = N[i] & ~LT[i] & okm;
            if (__builtin_expect(nn != 0, 0)) near_slot(j, s, k[i], nn);
        }
    };
    auto scan_windows = [&](auto &&keys_of_window) __attribute__((always_inline)) {
        for (int j = 0; j < D; ++j) {  // wave-uniform
            const K16Win &w = win[j];
            if (!w.active) continue;
            WaveWin s;
            s.lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.lo);
            s.hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.hi);
            s.lt = 0u;
            s.lay.lo = s.lo;
            s.lay.hi = s.hi;
            s.lay.C = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.C);
            s.lay.shift = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.shift);
            s.lay.narrow = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.narrow);
            s.lay.nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.lay.nb);
            s.base = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.base);
            uint32_t *wv = wst[wid][j];
            s.in = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv[1]);
            s.fmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv[2]);
            s.fmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv[3]);
            keys_of_window(j, s);  // (at most U * 8 * WAVE = 4096 keys)
            if (s.in >= K16_WAVE_BUDGET) wave_flush(j, s);  // wave-uniform
            if (lane == 0) {
                wv[0] += s.lt;
                wv[1] = s.in;
                wv[2] = s.fmin;
                wv[3] = s.fmax;
            }
            __builtin_amdgcn_wave_barrier();  // (a wave's LDS accesses are in order)
        }
    };

    for (u64 t = blockIdx.x; t < nfull; t += gridDim.x) {
        uint4 x[U];
        const uint4 *src = v + t * tile + threadIdx.x;
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = load_nt(src + u * BLK);
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = k16_ord8<CV>(x[u], nl2, top2);
        scan_windows([&](int j, WaveWin &s) {
#if K16_MAIN_TF
            uint32_t rows = 0;  // bit u: load u may hold output (wave-uniform)
#endif
#pragma unroll
            for (int u = 0; u < U; ++u) {
#if K16_MAIN_TF
                const uint32_t m0 = f.largest ? s.lt : s.lt + s.in;
#endif
                key_group(j, s, x[u].x, x[u].y, ~0ull);
                key_group(j, s, x[u].z, x[u].w, ~0ull);
#if K16_MAIN_TF
                const uint32_t m1 = f.largest ? s.lt : s.lt + s.in;
                rows |= (f.largest ? m1 - m0 < 8u * WAVE : m1 != m0) ? 1u << u : 0u;
#endif
            }
#if K16_MAIN_TF
            if (j == 0 && lane == 0) reinterpret_cast<uint8_t *>(f.hdr + 4)[t * NW + wid] = (uint8_t)rows;
#endif
        });
    }
    // the 16-byte words after the full tiles, one a thread and round, masked
    for (u64 b = nfull * tile + (u64)blockIdx.x * BLK; b < nv; b += (u64)gridDim.x * BLK) {
        const u64 i = b + threadIdx.x;
        const bool in = i < nv;
        const uint4 q = k16_ord8<CV>(in ? load_nt(v + i) : make_uint4(0, 0, 0, 0), nl2, top2);
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(in);
        scan_windows([&](int j, WaveWin &s) {
            key_group(j, s, q.x, q.y, okm);
            key_group(j, s, q.z, q.w, okm);
        });
    }
    if (blockIdx.x == 0) {  // the < 8-key unaligned head and tail
        const bool okh = threadIdx.x < head, okt = threadIdx.x < n - tail0;
        const uint32_t kh = okh ? k16_ord1<CV>(p[threadIdx.x], nl2, top2) : ~0u;
        const uint32_t kt = okt ? k16_ord1<CV>(p[tail0 + threadIdx.x], nl2, top2) : ~0u;
        scan_windows([&](int j, WaveWin &s) {
            key_slot(j, s, kh);
            key_slot(j, s, kt);
        });
    }
    __syncthreads();
    for (int j = 0; j < D; ++j) {
        const K16Win &w = win[j];
        if (!w.active) continue;
        u64 *gb = a.bins + (size_t)j * K16_RANK_WORDS;
        const uint32_t words = (w.lay.nb + 1u) / 2u;
        for (uint32_t i = threadIdx.x; i < words; i += BLK) {
            const uint32_t t = lh[w.base + i];
            if (t) k16_flush_word(gb, 2u * i, t);
        }
        if ((int)threadIdx.x == 0) {
            u64 lt = 0;
            for (int q = 0; q < NW; ++q) lt += wst[q][j][0];
            if (lt) atomicAdd(&gb[K16_BINS_MAX], lt);
        }
    }
}
